"""CPU-side checks of the LOBPCG solver: the new C-ABI symbols, and the control flow of spectra_amd/csrc/lobpcg_flow.hpp on a plain host
backend (tests/cpp/lobpcg_host_capi.cpp) against numpy / scipy on the fixtures of tests/lobpcg_checks.py.  The GPU runs the same
solver-level checks through the library in tests/test_gpu_lobpcg.py.

Iteration counts at tol = 1e-8: the caps of lobpcg_checks are the conditions.  Every solve prints its own count next to the one recorded
in lobpcg_checks.RECORDED_ITERATIONS (this flow on the host backend, g++ -O2, x86-64).  The recorded counts are not asserted: a count
can move by one with the summation order.  A float64 numpy restatement of the flow needed the same counts except 36 instead of 37 on
B plus Jacobi (4099, 16), where this flow repeats one Rayleigh-Ritz step without P (its Cholesky rejects pivots below 1e-8, see
lobpcg_flow.hpp)."""
import ctypes as C
import re
import os

import numpy as np
import pytest
import scipy.sparse as sp

import lobpcg_checks as L
from spectra_amd import _capi

NEW_SYMBOLS = ["mispec_lobpcg_create", "mispec_lobpcg_destroy", "mispec_lobpcg_set_B", "mispec_lobpcg_set_preconditioner",
               "mispec_lobpcg_set_jacobi", "mispec_lobpcg_set_constraints", "mispec_lobpcg_set_initial", "mispec_lobpcg_compute",
               "mispec_lobpcg_info", "mispec_lobpcg_num_iterations", "mispec_lobpcg_num_operations", "mispec_lobpcg_num_retries",
               "mispec_lobpcg_eigenvalues", "mispec_lobpcg_eigenvectors", "mispec_lobpcg_residuals", "mispec_lobpcg_residual_norms",
               "mispec_lobpcg_gram", "mispec_lobpcg_resid", "mispec_lobpcg_block_sub", "mispec_lobpcg_kernel_time"]


def test_new_symbols_resolve_in_the_extras_library():
    import spectra_amd as sa

    lib = sa.lib()
    extras = C.CDLL(_capi.EXTRAS_LIB_PATH)
    core = C.CDLL(_capi.LIB_PATH)
    assert "mispec_lobpcg_" in _capi.EXTRAS_PREFIXES
    for nm in NEW_SYMBOLS:
        assert hasattr(lib, nm) and hasattr(extras, nm), nm
        assert not hasattr(core, nm), nm
        assert nm.startswith("mispec_lobpcg_") and nm in _capi.SIGNATURES, nm
    hdr = open(os.path.join(L.ROOT, "include", "mispec_extras.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mispec_lobpcg_[A-Za-z0-9_]+)\s*\(", hdr))
    assert declared == set(NEW_SYMBOLS)
    core_hdr = open(os.path.join(L.ROOT, "include", "mispec.h")).read()
    assert "lobpcg" not in core_hdr.lower()
    import test_capi_load

    assert test_capi_load.header_symbols() == set(_capi.SIGNATURES)


def test_null_arguments_are_invalid():
    import spectra_amd as sa

    lib = sa.lib()
    h = C.c_void_p()
    n64 = C.c_int64()
    out = np.zeros(4)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.mispec_lobpcg_create(None, None, 3, C.byref(h)) == _capi.MISPEC_EINVAL
    assert b"NULL" in lib.mispec_last_error()
    assert lib.mispec_lobpcg_set_B(None, None) == _capi.MISPEC_EINVAL
    assert lib.mispec_lobpcg_set_preconditioner(None, None) == _capi.MISPEC_EINVAL
    assert lib.mispec_lobpcg_set_jacobi(None, 1) == _capi.MISPEC_EINVAL
    assert lib.mispec_lobpcg_set_constraints(None, dp, 4, 1) == _capi.MISPEC_EINVAL
    assert lib.mispec_lobpcg_set_initial(None, dp, 4) == _capi.MISPEC_EINVAL
    assert lib.mispec_lobpcg_compute(None, L.SMALLEST, 10, 1e-8, C.byref(n64)) == _capi.MISPEC_EINVAL
    assert lib.mispec_lobpcg_eigenvalues(None, dp) == _capi.MISPEC_EINVAL
    assert lib.mispec_lobpcg_eigenvectors(None, dp, 4) == _capi.MISPEC_EINVAL
    assert lib.mispec_lobpcg_residuals(None, dp, 4) == _capi.MISPEC_EINVAL
    assert lib.mispec_lobpcg_residual_norms(None, dp) == _capi.MISPEC_EINVAL
    assert lib.mispec_lobpcg_gram(None, None, 4, 1, None, 4, 1, 4, 0, dp) == _capi.MISPEC_EINVAL
    assert lib.mispec_lobpcg_resid(None, None, None, 4, 1, 4, dp, None, 0, None, None, 4, dp) == _capi.MISPEC_EINVAL
    assert lib.mispec_lobpcg_block_sub(None, None, 4, 1, None, 4, 1, dp, 4) == _capi.MISPEC_EINVAL
    assert lib.mispec_lobpcg_info(None) == L.INVALID_INPUT
    assert lib.mispec_lobpcg_num_iterations(None) == 0 and lib.mispec_lobpcg_num_operations(None) == 0
    assert lib.mispec_lobpcg_destroy(None) == _capi.MISPEC_OK


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    return L.build_host_library(tmp_path_factory.mktemp("lobpcg"))


def solve(hostlib, n, m, with_B=False, pre="jacobi", selection=L.SMALLEST, maxit=L.MAXIT_JACOBI):
    s = L.HostSolver(hostlib, L.band(n), L.X0(n, m), B=L.Bmat(n) if with_B else None, preconditioner=pre)
    nconv = s.compute(selection, maxit, L.TOL)
    msg = "n=%d m=%d B=%s pre=%s: info %d after %d iterations (recorded %s, cap %d), %d retries without P, residual norms %s" % (
        n, m, with_B, pre, s.info(), s.num_iterations(), L.RECORDED_ITERATIONS.get((pre, with_B, selection, n, m)), maxit, s.num_retries(),
        s.residual_norms())
    print(msg)
    assert s.info() == L.SUCCESS and nconv == m and s.num_iterations() <= maxit, msg
    res = L.check_solution(n, m, s.eigenvalues(), s.eigenvectors(), with_B=with_B, largest=selection == L.LARGEST, msg=msg)
    assert np.abs(res - s.residual_norms()).max() < 1e-10, msg  # the reported norms are those of the fresh products
    assert s.num_operations() == m + s.active_column_sum() + m, msg
    return s


@pytest.mark.parametrize("n,m", L.JACOBI_CASES)
def test_jacobi_smallest(hostlib, n, m):
    solve(hostlib, n, m)


@pytest.mark.parametrize("n,m", L.B_JACOBI_CASES)
def test_pencil_with_jacobi(hostlib, n, m):
    solve(hostlib, n, m, with_B=True)


@pytest.mark.parametrize("selection", [L.SMALLEST, L.LARGEST])
def test_unpreconditioned(hostlib, selection):
    solve(hostlib, 300, 3, pre=None, selection=selection, maxit=L.MAXIT_PLAIN)


def test_sparse_preconditioner_equals_jacobi(hostlib):
    """T = diag(1 / diag A) as a matrix takes the other path (resid into the scratch block, then R = T W) to the same iterates."""
    n, m = 300, 3
    T = sp.diags(1.0 / L.band(n).diagonal()).tocsr()
    s = L.HostSolver(hostlib, L.band(n), L.X0(n, m), preconditioner=T)
    assert s.compute(L.SMALLEST, L.MAXIT_JACOBI, L.TOL) == m and s.info() == L.SUCCESS
    j = solve(hostlib, n, m)
    assert s.num_iterations() == j.num_iterations()
    assert np.abs(s.eigenvalues() - j.eigenvalues()).max() < 1e-12
    L.check_solution(n, m, s.eigenvalues(), s.eigenvectors())


def test_random_start(hostlib):
    n, m = 300, 3
    s = L.HostSolver(hostlib, L.band(n), None, nev=m, preconditioner="jacobi")
    assert s.compute(L.SMALLEST, L.MAXIT_JACOBI, L.TOL) == m and s.info() == L.SUCCESS
    L.check_solution(n, m, s.eigenvalues(), s.eigenvectors())


@pytest.mark.parametrize("with_B", [False, True])
def test_constraints_deflate_known_eigenvectors(hostlib, with_B):
    import scipy.linalg as sla

    n, m, c = 300, 3, 3
    A, B = L.band(n), L.Bmat(n)
    w, V = sla.eigh(A.toarray(), B.toarray() if with_B else None)
    Y = V[:, :c]
    s = L.HostSolver(hostlib, A, L.X0(n, m), B=B if with_B else None, preconditioner="jacobi", constraints=Y)
    assert s.compute(L.SMALLEST, L.MAXIT_JACOBI, L.TOL) == m and s.info() == L.SUCCESS
    X = s.eigenvectors()
    L.check_solution(n, m, s.eigenvalues(), X, with_B=with_B, skip=c)  # eigenvalues 4 to 6
    assert np.abs(Y.T @ (B @ X if with_B else X)).max() < 1e-10


def test_soft_locking_saves_products(hostlib):
    """Columns of (1000, 8) converge at different iterations: the products with A are m at the start, the active widths, and m for the
    fresh products of the end — strictly fewer than m per iteration."""
    n, m = 1000, 8
    s = solve(hostlib, n, m)
    assert s.num_operations() == m + s.active_column_sum() + m
    assert s.active_column_sum() < m * s.num_iterations()
    assert s.num_operations() < m * (s.num_iterations() + 2)


def test_limits(hostlib):
    n = 50
    for m in (0, 22, n):
        with pytest.raises(ValueError):
            L.HostSolver(hostlib, L.band(n), None, nev=m)
    with pytest.raises(ValueError):
        L.HostSolver(hostlib, L.band(n), None, nev=3, constraints=np.ones((n, 22)))
    with pytest.raises(ValueError):
        L.HostSolver(hostlib, L.band(24), None, nev=12, constraints=np.eye(24)[:, :12])  # m + c = n
    s = L.HostSolver(hostlib, L.band(n), None, nev=3)
    assert s.info() == L.INVALID_INPUT  # before compute
    with pytest.raises(ValueError):
        s.compute(0, 10, L.TOL)  # LargestMagn


def test_equal_start_columns_are_a_numerical_issue(hostlib):
    n, m = 300, 3
    X = L.X0(n, m).copy()
    X[:, 1] = X[:, 0]
    s = L.HostSolver(hostlib, L.band(n), X, preconditioner="jacobi")
    assert s.compute() == 0
    assert s.info() == L.NUMERICAL_ISSUE and s.num_iterations() == 0
    # no iteration was completed: the Rayleigh quotients of the start vectors are reported
    A = L.band(n)
    want = [X[:, j] @ (A @ X[:, j]) / (X[:, j] @ X[:, j]) for j in range(m)]
    assert np.abs(s.eigenvalues() - want).max() < 1e-9 * np.abs(want).max()


def test_exact_eigenvector_with_an_unreachable_threshold(hostlib):
    """A start block whose first column is an exact eigenvector, with a threshold no residual can reach (1e-300): that column's
    residual is rounding noise, and the CholQR of R meets a Gram matrix that is not numerically positive definite.  The run ends with
    NumericalIssue from THAT branch (the flow's counter: no retry without P was made), and X, lambda of the last completed iteration
    are still there: the exact pair is returned to rounding."""
    n, m = 300, 3
    A = L.band(n)
    w, V = np.linalg.eigh(A.toarray())
    X = L.X0(n, m).copy()
    X[:, 0] = V[:, 0]
    s = L.HostSolver(hostlib, A, X, preconditioner="jacobi")
    assert s.compute(L.SMALLEST, 100, 1e-300) == 0
    assert s.info() == L.NUMERICAL_ISSUE and s.num_retries() == 0 and s.num_iterations() < 100
    assert abs(s.eigenvalues()[0] - w[0]) < 1e-12
    Xr = s.eigenvectors()
    assert np.linalg.norm(A @ Xr[:, 0] - w[0] * Xr[:, 0]) < 1e-12


def test_retry_without_p_on_a_block_that_loses_rank(hostlib):
    """The retry, on a constructed input: a preconditioner of rank m, T = U V' (see lobpcg_checks.rank_loss_case).  Every preconditioned
    residual block and every P then lie in span(U), m dimensions: from the second iteration on [R | P] has 2m columns of rank m, the
    Cholesky of gramB must fail whatever the rounding, and each step is repeated on [X | R].  After three iterations: two retries (the
    flow's counter), NoConvergence — the iterates cannot leave span[X0, U] — and the eigenvalues are the Ritz values of A on that
    subspace, which numpy computes independently."""
    A, X, T, ritz = L.rank_loss_case()
    s = L.HostSolver(hostlib, A, X, preconditioner=T)
    assert s.compute(L.SMALLEST, 3, L.TOL) == 0
    assert s.info() == L.NO_CONVERGENCE and s.num_iterations() == 3 and s.num_retries() == 2
    assert np.abs(s.eigenvalues() - ritz).max() < 1e-10
    assert np.abs(s.eigenvectors().T @ s.eigenvectors() - np.eye(X.shape[1])).max() < 1e-10
