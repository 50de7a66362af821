"""spectra_amd.LOBPCGSolver on the device: the solver-level checks of tests/test_host_lobpcg.py (fixtures and bars of
tests/lobpcg_checks.py) through the library.  The device's iteration count is reported next to the host backend's (the same control flow
over plain loops, compiled here) and must be within the cap; equality is not required, the summation orders differ."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import lobpcg_checks as L
import spectra_amd as sa
from spectra_amd import _capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    return L.build_host_library(tmp_path_factory.mktemp("lobpcg"))


def host_iterations(hostlib, n, m, with_B=False, pre="jacobi", selection=L.SMALLEST, maxit=L.MAXIT_JACOBI, constraints=None, random=False):
    pre_h = sp.diags(1.0 / L.band(n).diagonal()).tocsr() if pre == "matrix" else pre
    s = L.HostSolver(hostlib, L.band(n), None if random else L.X0(n, m), nev=m, B=L.Bmat(n) if with_B else None, preconditioner=pre_h,
                     constraints=constraints)
    s.compute(selection, maxit, L.TOL)
    return s.num_iterations()


def device_solve(ctx, hostlib, n, m, with_B=False, pre="jacobi", selection=sa.SortRule.SmallestAlge, maxit=L.MAXIT_JACOBI, reorder=None,
                 constraints=None, random=False, skip=0):
    op = sa.SparseSymMatProd(L.band(n), ctx=ctx, reorder=reorder)
    Bop = sa.SparseSymMatProd(L.Bmat(n), ctx=ctx) if with_B else None
    T = sa.SparseSymMatProd(sp.diags(1.0 / L.band(n).diagonal()).tocsc(), ctx=ctx) if pre == "matrix" else pre
    s = sa.LOBPCGSolver(op, None if random else L.X0(n, m), nev=m, B=Bop, preconditioner=T, constraints=constraints)
    assert s.info() == sa.LOBPCGInfo.InvalidInput
    nconv = s.compute(selection, maxit, L.TOL)
    host = host_iterations(hostlib, n, m, with_B, pre, int(selection), maxit, constraints, random)
    msg = "n=%d m=%d B=%s pre=%s reorder=%s: info %s after %d iterations on the device, %d on the host backend (cap %d), %d retries, norms %s" % (
        n, m, with_B, pre, reorder, s.info().name, s.num_iterations(), host, maxit, s.num_retries(), s.residual_norms())
    print(msg)
    assert s.info() == sa.LOBPCGInfo.Success and nconv == m and s.num_iterations() <= maxit, msg
    lam, X = s.eigenvalues(), s.eigenvectors()
    res = L.check_solution(n, m, lam, X, with_B=with_B, largest=selection == sa.SortRule.LargestAlge, skip=skip, msg=msg)
    assert np.abs(res - s.residual_norms()).max() < 1e-10, msg
    Rdev = s.residuals()
    BX = L.Bmat(n) @ X if with_B else X
    assert np.abs(Rdev - (L.band(n) @ X - BX * lam)).max() < 1e-10, msg
    assert s.num_operations() <= m * (s.num_iterations() + 2), msg
    return s


@pytest.mark.parametrize("n,m", L.JACOBI_CASES + [(20011, 8)])
def test_jacobi_smallest(ctx, hostlib, n, m):
    device_solve(ctx, hostlib, n, m)


def test_pencil(ctx, hostlib):
    device_solve(ctx, hostlib, 1000, 8, with_B=True)


def test_sparse_preconditioner(ctx, hostlib):
    device_solve(ctx, hostlib, 1000, 4, pre="matrix")


def test_constraints(ctx, hostlib):
    n, m, c = 300, 3, 3
    w, V = np.linalg.eigh(L.band(n).toarray())
    Y = V[:, :c]
    s = device_solve(ctx, hostlib, n, m, constraints=Y, skip=c)  # eigenvalues 4 to 6
    assert np.abs(Y.T @ s.eigenvectors()).max() < 1e-10


def test_largest_unpreconditioned(ctx, hostlib):
    device_solve(ctx, hostlib, 300, 3, pre=None, selection=sa.SortRule.LargestAlge, maxit=L.MAXIT_PLAIN)


def test_reordered_operator(ctx, hostlib):
    s = device_solve(ctx, hostlib, 1000, 4, reorder="rcm")
    assert s.op.reordering() == "rcm"


def test_random_start(ctx, hostlib):
    device_solve(ctx, hostlib, 1000, 4, random=True)


def test_block_product_leaves_the_solve_unchanged(ctx):
    """Option spmm=0 (one SpMV per column) against auto (panels of 8 / 4 / 2): the block product is bit-identical to the column loop, so
    eigenvalues, vectors and counts agree to the bit (as tests/test_gpu_davidson_block.py shows for the Davidson solver)."""
    n, m = 1000, 8

    def solve(spmm):
        sa.set_option("spmm", spmm)
        try:
            s = sa.LOBPCGSolver(sa.SparseSymMatProd(L.band(n), ctx=ctx), L.X0(n, m), B=sa.SparseSymMatProd(L.Bmat(n), ctx=ctx),
                                preconditioner="jacobi")
            nconv = s.compute()
            return nconv, s.eigenvalues(), s.eigenvectors(), s.num_iterations(), s.num_operations(), int(s.info())
        finally:
            sa.set_option("spmm", None)

    assert max(sa.spmm_plan(m)) > 1
    old, new = solve("0"), solve("auto")
    assert old[0] == m and old[5] == int(sa.LOBPCGInfo.Success)
    assert np.array_equal(new[1], old[1]) and np.array_equal(new[2], old[2])
    assert (new[0],) + new[3:] == (old[0],) + old[3:]


def test_failure_keeps_the_last_iterate(ctx):
    n, m = 300, 3
    X = L.X0(n, m).copy()
    X[:, 1] = X[:, 0]
    s = sa.LOBPCGSolver(sa.SparseSymMatProd(L.band(n), ctx=ctx), X, preconditioner="jacobi")
    assert s.compute() == 0 and s.info() == sa.LOBPCGInfo.NumericalIssue and s.num_iterations() == 0
    # no iteration was completed: the Rayleigh quotients of the start vectors are reported
    A = L.band(n)
    want = np.array([X[:, j] @ (A @ X[:, j]) / (X[:, j] @ X[:, j]) for j in range(m)])
    assert np.abs(s.eigenvalues() - want).max() < 1e-9 * np.abs(want).max()
    assert np.all(np.isfinite(s.eigenvectors()))


def test_retry_without_p_on_a_block_that_loses_rank(ctx):
    """tests/test_host_lobpcg.py's constructed input on the device: a preconditioner of rank m keeps R and P in one m-dimensional
    space, so the Cholesky of gramB fails from the second iteration on and every step is repeated on [X | R]."""
    A, X, T, ritz = L.rank_loss_case()
    s = sa.LOBPCGSolver(sa.SparseSymMatProd(A, ctx=ctx), X, preconditioner=sa.SparseGenMatProd(T, ctx=ctx))
    assert s.compute(sa.SortRule.SmallestAlge, 3, L.TOL) == 0
    assert s.info() == sa.LOBPCGInfo.NoConvergence and s.num_iterations() == 3 and s.num_retries() == 2
    assert np.abs(s.eigenvalues() - ritz).max() < 1e-10
    Xd = s.eigenvectors()
    assert np.abs(Xd.T @ Xd - np.eye(X.shape[1])).max() < 1e-10


def test_constraints_set_right_after_creation(ctx):
    """The constraint block is filled by a copy that is not ordered against the context's stream; the zero fill of the new block must
    not land after it.  Twenty fresh solvers in a row each see their constraints: a zeroed block would be refused as linearly dependent
    at compute()."""
    n, m, c = 300, 3, 3
    w, V = np.linalg.eigh(L.band(n).toarray())
    op = sa.SparseSymMatProd(L.band(n), ctx=ctx)
    for _ in range(20):
        s = sa.LOBPCGSolver(op, L.X0(n, m), preconditioner="jacobi", constraints=V[:, :c])
        s.compute(sa.SortRule.SmallestAlge, 2, L.TOL)
        assert s.num_iterations() == 2
        assert np.abs(V[:, :c].T @ s.eigenvectors()).max() < 1e-10


def test_argument_limits(ctx):
    n = 300
    op = sa.SparseSymMatProd(L.band(n), ctx=ctx)
    with pytest.raises(ValueError):
        sa.LOBPCGSolver(op, nev=22)
    with pytest.raises(ValueError):
        sa.LOBPCGSolver(op, nev=0)
    small = sa.SparseSymMatProd(L.band(12), ctx=ctx)
    with pytest.raises(ValueError):
        sa.LOBPCGSolver(small, nev=12)                                  # m = n
    with pytest.raises(ValueError):
        sa.LOBPCGSolver(small, nev=6, constraints=np.eye(12)[:, :6])    # m + c = n
    with pytest.raises(ValueError):
        sa.LOBPCGSolver(op, nev=3, constraints=np.ones((n, 22)))
    with pytest.raises(ValueError):
        sa.LOBPCGSolver(op, nev=3, B=sa.SparseSymMatProd(L.Bmat(n + 1), ctx=ctx))
    with pytest.raises(ValueError):
        sa.LOBPCGSolver(op, nev=3, preconditioner=sa.SparseSymMatProd(L.Bmat(n + 1), ctx=ctx))
    with pytest.raises(ValueError):
        sa.LOBPCGSolver(op, nev=3, preconditioner="ilu")
    with pytest.raises(ValueError):
        sa.LOBPCGSolver(op, nev=3).compute(sa.SortRule.LargestMagn)
    with pytest.raises(ValueError):
        sa.LOBPCGSolver(op, nev=3).eigenvalues()                         # before compute
    neg = L.band(n).tolil()
    neg[5, 5] = -1.0
    with pytest.raises(ValueError, match="positive diagonal"):
        sa.LOBPCGSolver(sa.SparseSymMatProd(neg.tocsc(), ctx=ctx), nev=3, preconditioner="jacobi")
    # a row-sharded operator
    lib = sa.lib()
    grp = C.c_void_p()
    _capi.check(lib.mispec_loopback_create(2, C.byref(grp)))
    try:
        sctx = sa.Context(0)
        _capi.check(lib.mispec_loopback_attach(grp, sctx.h, 0))
        sctx.rank, sctx.world = 0, 2
        shard = sa.SparseSymMatProd(L.band(n), ctx=sctx)
        assert shard.local_rows() < n
        with pytest.raises(ValueError, match="unsharded"):
            sa.LOBPCGSolver(shard, nev=3)
        del shard, sctx
    finally:
        _capi.check(lib.mispec_loopback_destroy(grp))
