"""The reference's own test/HermEigs.cpp (HermEigsSolver over DenseHermMatProd<complex> and SparseHermMatProd<complex>, five rules,
||AU - UD|| <= 1e-9), compiled unmodified against include/Spectra with tests/cpp/eigen_lite in Eigen's place (tests/cpp/eigen_lite_herm in front of it
for the Hermitian meaning of complex sparse selfadjointView products) by oracle/build_ref_programs.sh HermEigs (run by
__graft_entry__.build() where the reference is present).  The binary travels with the
tree; nothing here reads the reference."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "oracle", "_ref", "programs", "HermEigs.bin")


def test_reference_hermeigs_program():
    if not os.path.exists(EXE):
        pytest.skip("oracle/_ref/programs/HermEigs.bin not built (needs the reference's sources at build time)")
    r = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and "All tests passed" in r.stdout, r.stdout[-3000:]
