"""Block shift solve, the parts that need no GPU: the host-only plan that cuts k columns into panels (mispec_symshift_block_plan),
option `shift_block`, the NULL-handle refusals of the new entry points, and — on the host backend of the LOBPCG control flow — the
fixture and the iteration cap that tests/test_gpu_lobpcg_solver_pre.py uses for the factorisation preconditioner."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import lobpcg_checks as L
import shift_block_checks as SB
import spectra_amd as sa
from spectra_amd import _capi


@pytest.mark.parametrize("panel", SB.PLAN_PANELS)
@pytest.mark.parametrize("k", SB.COLUMN_COUNTS)
def test_plan_under_the_option(k, panel):
    try:
        sa.set_option("shift_block", panel)
        widths = sa.shift_block_plan(k)
    finally:
        sa.set_option("shift_block", None)
    cap = max(int(panel), 1)
    assert sum(widths) == k and all(w in (1, 2, 4) and w <= cap for w in widths)
    assert widths == sorted(widths, reverse=True)  # widest first
    if panel == "0":
        assert widths == [1] * k
    else:
        # as many of the widest panels as fit, then the next width: at most one panel of 2 under 4, at most one single column
        assert widths.count(cap) == k // cap and widths.count(1) == k % 2
    assert sa.shift_block_plan(k, int(panel) or 1) == widths  # the forced plan does not read the option


def test_plan_auto_and_forced():
    sa.set_option("shift_block", None)
    for k in SB.COLUMN_COUNTS:
        auto = sa.shift_block_plan(k)
        assert sum(auto) == k and auto == sorted(auto, reverse=True) and set(auto) <= {1, 2, 4}
        assert sa.shift_block_plan(k, 1) == [1] * k
    assert sa.shift_block_plan(21, 4) == [4] * 5 + [1]
    assert sa.shift_block_plan(21, 2) == [2] * 10 + [1]
    assert sa.shift_block_plan(3, 4) == [2, 1]


def test_plan_refusals():
    lib = sa.lib()
    out, count = (C.c_int * 8)(), C.c_int(0)
    for k in (0, -1):
        assert lib.mispec_symshift_block_plan(k, 0, out, 8, C.byref(count)) == _capi.MISPEC_EINVAL
    assert lib.mispec_symshift_block_plan(4, 0, None, 8, C.byref(count)) == _capi.MISPEC_EINVAL
    assert lib.mispec_symshift_block_plan(4, 0, out, 8, None) == _capi.MISPEC_EINVAL
    assert lib.mispec_symshift_block_plan(4, 3, out, 8, C.byref(count)) == _capi.MISPEC_EINVAL
    assert lib.mispec_symshift_block_plan(8, 1, out, 7, C.byref(count)) == _capi.MISPEC_EINVAL  # eight single columns do not fit
    assert lib.mispec_symshift_block_plan(8, 1, out, 8, C.byref(count)) == _capi.MISPEC_OK and count.value == 8


def test_option_values():
    try:
        for v in ("auto", "0", "2", "4"):
            sa.set_option("shift_block", v)
            assert sa.get_option("shift_block") == v
        for v in ("1", "8", "wide"):
            with pytest.raises(Exception) as e:
                sa.set_option("shift_block", v)
            assert "auto | 0 | 2 | 4" in str(e.value) and "shift_block" in str(e.value)
            assert sa.get_option("shift_block") == "4"  # a refused value changes nothing
    finally:
        sa.set_option("shift_block", None)


def test_null_handles_are_refused_without_a_device():
    lib = sa.lib()
    x = np.zeros(4)
    p = x.ctypes.data_as(C.POINTER(C.c_double))
    ms = C.c_float(0)
    assert lib.mispec_symshift_solve_block(None, None, 4, 1, None, 4) == _capi.MISPEC_EINVAL
    assert lib.mispec_symshift_solve_block_host(None, p, 4, 1, p, 4) == _capi.MISPEC_EINVAL
    assert lib.mispec_symshift_solve_block_time(None, None, 4, 1, None, 4, 1, C.byref(ms)) == _capi.MISPEC_EINVAL
    assert lib.mispec_lobpcg_set_preconditioner_solver(None, None) == _capi.MISPEC_EINVAL


def test_symbols_and_documents():
    names = ("mispec_symshift_solve_block", "mispec_symshift_solve_block_host", "mispec_symshift_block_plan",
             "mispec_symshift_solve_block_time", "mispec_lobpcg_set_preconditioner_solver")
    root = os.path.dirname(os.path.dirname(os.path.abspath(_capi.__file__)))
    with open(os.path.join(root, "include", "mispec.h")) as f:
        header = f.read()
    with open(os.path.join(root, "include", "mispec_lobpcg_pre.h")) as f:
        header += f.read()
    for name in names:
        assert (name in _capi.SIGNATURES or name in _capi.LOBPCG_PRE_SIGNATURES) and name + "(" in header
        assert getattr(sa.lib(), name) is not None
    assert "shift_block " in header
    with open(os.path.join(root, "README.md")) as f:
        assert "MISPEC_SHIFT_BLOCK" in f.read()


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    return L.build_host_library(tmp_path_factory.mktemp("lobpcg"))


def test_the_fixture_needs_the_factorisation_preconditioner(hostlib):
    """Passes without the block solve: the control flow on the host backend, A = K + E at (n, m) = (1000, 4), reaches Success within
    the cap of the GPU test with T = K^{-1} given as a matrix (measured: 20 iterations), and does not converge in 300 with Jacobi."""
    n, m = SB.PRE_CASES[0]
    A = SB.Amat(n)
    T = sp.csr_matrix(np.linalg.inv(SB.Kmat(n).toarray()))
    s = L.HostSolver(hostlib, A, L.X0(n, m), preconditioner=T)
    nconv = s.compute(L.SMALLEST, SB.PRE_MAXIT, L.TOL)
    print("host backend, T = K^-1: %d iterations (recorded %d), %d retries" % (s.num_iterations(), SB.PRE_HOST_ITERATIONS[(n, m)],
                                                                                  s.num_retries()))
    assert s.info() == L.SUCCESS and nconv == m and s.num_iterations() <= SB.PRE_MAXIT
    assert np.abs(np.sort(s.eigenvalues()) - np.linalg.eigvalsh(A.toarray())[:m]).max() <= 2 * L.TOL
    j = L.HostSolver(hostlib, A, L.X0(n, m), preconditioner="jacobi")
    j.compute(L.SMALLEST, SB.PRE_MAXIT_JACOBI, L.TOL)
    print("host backend, Jacobi: residuals", j.residual_norms())
    assert j.info() == L.NO_CONVERGENCE
