"""the reference's OWN test programs (/root/reference/test/*.cpp with its Catch2 header), compiled
UNMODIFIED against include/Spectra — tests/cpp/eigen_lite stands in for Eigen, which this image does not have — and linked with
libmispec.so (oracle/build_ref_programs.sh, run by __graft_entry__.build() where the reference is present).  The binaries
are built in the container that holds /root/reference and travel to the GPU box; nothing here reads the reference at run time.

Elsewhere: Givens / QR / Eigen / Schur / Orthogonalization.cpp test host-side classes and run without a GPU
(tests/test_cpp_reference_programs_host.py).  Programs that cannot be built against this repository and why:
HermEigs.cpp, ComplexEigs.cpp, BKLDLT.cpp instantiate the complex SOLVERS / a complex LDL' (the device solvers are fp64 real),
SymGEigsShift.cpp passes a dense B to SymShiftInvert (sparse only here), JDSym*.cpp / RitzPairs / SearchSpace test internals of
the Davidson solver that live in libmispec.so here."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["onesweep", "reference"], autouse=True)
def orth_env(request, monkeypatch):
    """Every test of this module runs under both defaults of the orthogonalisation scheme (MISPEC_ORTH: the library default
    `onesweep` and the reference's two-pass control flow); solvers that set a mode themselves are run once."""
    params = getattr(getattr(request.node, "callspec", None), "params", {})
    if "orth" in params and request.param == "reference":
        pytest.skip("this test selects its modes itself")
    monkeypatch.setenv("MISPEC_ORTH", request.param)
    return request.param

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "programs")
PROGRAMS = ["SymEigs", "SymEigsShift", "GenEigs", "GenEigsRealShift", "GenEigsComplexShift", "SymGEigsCholesky", "SymGEigsRegInv",
            "SVD", "DavidsonSymEigs", "Example1", "Example2", "Example3", "Example4",
            # built with oracle/eigen_shim in Eigen's place (complex and float instantiations, oracle/build_ref_programs.sh)
            "Arnoldi", "SparseSymMatProd", "SparseGenMatProd", "DenseSymMatProd", "DenseGenMatProd"]


@pytest.mark.parametrize("name", PROGRAMS)
def test_reference_test_program(name):
    exe = os.path.join(REF, name + ".bin")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/programs/%s.bin not built (needs the reference's sources at build time)" % name)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    out = r.stdout
    # Example1 (20, 5, 12) exhausts its Krylov space after 10 steps; whether the surviving 1e-15 of noise trips the breakdown clamp
    # (Lanczos.h:163-168) at a step where the solver can still recover depends on the summation order of A x.  The dense product
    # operators therefore sum small matrices row by row in storage order (dense.hip k_row_gemv_serial) — the order of a CPU
    # row-dot, of the sparse kernels and of the oracle, all of which pass this case; no outcome is whitelisted any more.
    assert r.returncode == 0 and "All tests passed" in out, out[-3000:]
