"""LOBPCG with a factorisation as the preconditioner (mispec_lobpcg_set_preconditioner_solver): A = K + E with K = tridiag(-1, 2, -1)
and a weak far coupling E, T = K^{-1} held by a SparseSymShiftSolve / SymShiftInvert and applied to the active columns by the block
shift solve.  Jacobi does not converge on this matrix in 300 iterations (tests/test_host_shift_block.py)."""
import functools

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import lobpcg_checks as L
import shift_block_checks as SB
import spectra_amd as sa

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    return L.build_host_library(tmp_path_factory.mktemp("lobpcg"))


@functools.lru_cache(maxsize=None)
def reference_eigenvalues(n, with_B):
    Ad = SB.Amat(n).toarray()
    return sla.eigh(Ad, L.Bmat(n).toarray(), eigvals_only=True) if with_B else np.linalg.eigvalsh(Ad)


def factorisation_of_K(ctx, n, B=None, sigma=0.0):
    K = sp.tril(SB.Kmat(n)).tocsc()
    T = sa.SparseSymShiftSolve(K, ctx=ctx) if B is None else sa.SymShiftInvert(K, sp.tril(B).tocsc(), ctx=ctx)
    T.set_shift(sigma)
    return T


def solve(ctx, n, m, with_B=False, host=None):
    A, B = SB.Amat(n), L.Bmat(n) if with_B else None
    op = sa.SparseSymMatProd(A, ctx=ctx)
    Bop = sa.SparseSymMatProd(B, ctx=ctx) if with_B else None
    s = sa.LOBPCGSolver(op, L.X0(n, m), B=Bop, preconditioner=factorisation_of_K(ctx, n, B))
    assert s.T is not None  # the solver keeps the factorisation alive
    nconv = s.compute(sa.SortRule.SmallestAlge, SB.PRE_MAXIT, L.TOL)
    msg = "n=%d m=%d B=%s: info %s after %d iterations on the device, %s on the host backend (cap %d), %d retries, norms %s" % (
        n, m, with_B, s.info().name, s.num_iterations(), host, SB.PRE_MAXIT, s.num_retries(), s.residual_norms())
    print(msg)
    assert s.info() == sa.LOBPCGInfo.Success and nconv == m and s.num_iterations() <= SB.PRE_MAXIT, msg
    lam, X = s.eigenvalues(), s.eigenvectors()
    ref = reference_eigenvalues(n, with_B)[:m]
    assert np.abs(np.sort(lam) - ref).max() <= 2 * L.TOL, (msg, lam, ref)
    BX = B @ X if with_B else X
    res = np.linalg.norm(A @ X - BX * lam, axis=0)
    assert res.max() < 2 * L.TOL, (msg, res)
    assert np.abs(X.T @ BX - np.eye(m)).max() < 1e-10, msg
    assert np.abs(res - s.residual_norms()).max() < 1e-10, msg
    return s


def test_dense_last_level(ctx, hostlib):
    n, m = SB.PRE_CASES[0]
    h = L.HostSolver(hostlib, SB.Amat(n), L.X0(n, m), preconditioner=sp.csr_matrix(np.linalg.inv(SB.Kmat(n).toarray())))
    h.compute(L.SMALLEST, SB.PRE_MAXIT, L.TOL)
    solve(ctx, n, m, host=str(h.num_iterations()))


def test_banded_path(ctx):
    n, m = SB.PRE_CASES[1]
    solve(ctx, n, m, host="%d (recorded)" % SB.PRE_HOST_ITERATIONS[(n, m)])


def test_pencil(ctx):
    solve(ctx, 1000, 4, with_B=True, host="(not run)")


def test_column_loop_gives_the_same_solve(ctx):
    """shift_block=0 against auto: the block solve is bit-identical to the column loop, so eigenvalues and counts agree to the bit"""
    n, m = SB.PRE_CASES[1]

    def run(opt):
        sa.set_option("shift_block", opt)
        try:
            op = sa.SparseSymMatProd(SB.Amat(n), ctx=ctx)
            s = sa.LOBPCGSolver(op, L.X0(n, m), preconditioner=factorisation_of_K(ctx, n))
            s.compute(sa.SortRule.SmallestAlge, SB.PRE_MAXIT, L.TOL)
            return s.eigenvalues(), s.num_iterations(), s.eigenvectors()
        finally:
            sa.set_option("shift_block", None)

    results = [run(opt) for opt in ("0", None, "4", "2")]
    for lam, its, X in results[1:]:
        assert np.array_equal(lam, results[0][0]) and its == results[0][1] and np.array_equal(X, results[0][2])


def test_refusals(ctx):
    n, m = 4500, 4
    op = sa.SparseSymMatProd(SB.Amat(n), ctx=ctx)
    with pytest.raises(ValueError, match="positive definite"):
        sa.LOBPCGSolver(op, L.X0(n, m), preconditioner=factorisation_of_K(ctx, n, sigma=0.9))  # sigma inside the spectrum of K
    with pytest.raises(ValueError):
        sa.LOBPCGSolver(op, L.X0(n, m), preconditioner=factorisation_of_K(ctx, n - 1))
    G = sa.SparseGenRealShiftSolve(SB.Kmat(100).tocsc(), ctx=ctx)
    G.set_shift(0.0)
    with pytest.raises(ValueError):
        sa.LOBPCGSolver(sa.SparseSymMatProd(SB.Amat(100), ctx=ctx), L.X0(100, 2), preconditioner=G)
    never = sa.SparseSymShiftSolve(sp.tril(SB.Kmat(n)).tocsc(), ctx=ctx)
    s = sa.LOBPCGSolver(op, L.X0(n, m), preconditioner=never)
    with pytest.raises(AssertionError):  # std::logic_error: set_shift() has not been called
        s.compute(sa.SortRule.SmallestAlge, 10, L.TOL)
    never.set_shift(0.9)  # factored between two compute() calls, but indefinite
    with pytest.raises(ValueError, match="positive definite"):
        s.compute(sa.SortRule.SmallestAlge, 10, L.TOL)
    never.set_shift(0.0)
    assert s.compute(sa.SortRule.SmallestAlge, SB.PRE_MAXIT, L.TOL) == m
    # replaced by Jacobi: a solver that was never factored is no longer consulted
    unused = sa.SparseSymShiftSolve(sp.tril(SB.Kmat(n)).tocsc(), ctx=ctx)
    s2 = sa.LOBPCGSolver(op, L.X0(n, m), preconditioner=unused)
    sa.check(sa.lib().mispec_lobpcg_set_jacobi(s2.h, 1))
    s2.compute(sa.SortRule.SmallestAlge, 3, L.TOL)
    assert s2.info() == sa.LOBPCGInfo.NoConvergence
    # "ilu" and a matrix of the wrong shape stay ValueError
    with pytest.raises(ValueError):
        sa.LOBPCGSolver(op, L.X0(n, m), preconditioner="ilu")
    with pytest.raises(ValueError):
        sa.LOBPCGSolver(op, L.X0(n, m), preconditioner=sa.SparseSymMatProd(SB.Kmat(n - 1), ctx=ctx))
