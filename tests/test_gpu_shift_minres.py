"""The iterative path of the shift-and-invert operators (csrc/shift_minres.hip): Jacobi-preconditioned MINRES on the SpMV's own
operators, for matrices no direct path takes.  Opt-in (option shift_solver, the solver argument), so every test names its solver kind.
The bars against SuperLU are those of tests/test_gpu_shift_wide.py (relative residual and error <= 1e-12); the eigenproblem bars are
DESIGN.md section 5's."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

import lobpcg_checks as L
import shift_minres_checks as K
import spectra_amd as sa
from spectra_amd import _capi

pytestmark = pytest.mark.gpu

BIG = (26, 28, 30)


def assert_info(info, max_iterations=20000):
    assert info["last_backward_error"] <= 1e-13 and 0 <= info["last_iterations"] <= max_iterations, info


# ---- 1. against SuperLU --------------------------------------------------------------------------------------------------------
def test_expander_under_auto(ctx):
    A, _ = K.expander()
    n = A.shape[0]
    op = sa.SparseSymShiftSolve(K.lower(A), ctx=ctx, solver="auto")
    assert op.path_info() == {"path": 3, "block_rows": 0, "blocks": 0, "factor_bytes": 0}, op.path_info()
    direct = sa.SparseSymShiftSolve(K.lower(A), ctx=ctx, solver="direct")
    assert direct.path_info()["path"] == -1
    with pytest.raises(ValueError, match="only banded"):
        direct.set_shift(0.0)
    x = np.random.default_rng(1).uniform(-1, 1, n)
    for sigma in (0.0, -1.5):
        op.set_shift(sigma)
        ref = op.refinement_info()
        assert ref["refine_steps"] == 0 and ref["boosted_pivots"] == 0 and 0 < ref["probe_backward_error"] <= 1e-13, ref
        assert op.iterative_info()["probe_iterations"] > 0
        _, info = K.check_solve(op, A - sigma * sp.identity(n), x)
        assert_info(info)


@pytest.mark.parametrize("sigma", [0.0, 0.7])
def test_laplacian_forced_iterative(ctx, sigma):
    A, _ = K.lap3(17, 17, 17)
    n = A.shape[0]
    op = sa.SparseSymShiftSolve(K.lower(A), ctx=ctx, solver="iterative")
    assert op.path_info()["path"] == 3
    op.set_shift(sigma)
    x = np.random.default_rng(2).uniform(-1, 1, n)
    _, info = K.check_solve(op, A - sigma * sp.identity(n), x)
    assert_info(info)


def test_direct_and_iterative_agree(ctx):
    A, _ = K.lap3(17, 17, 17)
    n = A.shape[0]
    direct = sa.SparseSymShiftSolve(K.lower(A), ctx=ctx, solver="direct")
    auto = sa.SparseSymShiftSolve(K.lower(A), ctx=ctx, solver="auto")  # a direct path exists: auto keeps it
    it = sa.SparseSymShiftSolve(K.lower(A), ctx=ctx, solver="iterative")
    assert direct.path_info()["path"] == 2 and auto.path_info() == direct.path_info() and it.path_info()["path"] == 3
    assert direct.iterative_info() == {"last_iterations": 0, "total_iterations": 0, "solves": 0, "last_passes": 0,
                                       "last_backward_error": 0.0, "probe_iterations": 0}
    x = np.random.default_rng(3).uniform(-1, 1, n)
    for op in (direct, it):
        op.set_shift(0.0)
    yd, yi = direct.perform_op(x), it.perform_op(x)
    print("direct against iterative: %.2e" % (np.abs(yd - yi).max() / np.abs(yd).max()))
    assert np.abs(yd - yi).max() <= 1e-12 * max(1.0, np.abs(yd).max())
    assert_info(it.iterative_info())


def test_pencil(ctx):
    A, B = K.expander_pencil()
    n, sigma = A.shape[0], -0.5
    op = sa.SymShiftInvert(K.lower(A), K.lower(B), ctx=ctx, solver="auto")
    assert op.path_info()["path"] == 3
    op.set_shift(sigma)
    x = np.random.default_rng(4).uniform(-1, 1, n)
    _, info = K.check_solve(op, A - sigma * B, x)
    assert_info(info)


# ---- 2. kernel shapes: one row, the pair loop's tail, one and several workgroups -----------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 1023, 1025, 4097])
def test_kernel_shapes(ctx, n):
    A = K.random_sym(n, seed=n)
    op = sa.SparseSymShiftSolve(K.lower(A), ctx=ctx, solver="iterative")
    assert op.path_info()["path"] == 3
    x = np.random.default_rng(n).uniform(-1, 1, n)
    for sigma in (0.0, 0.25):
        op.set_shift(sigma)
        M = (A - sigma * sp.identity(n)).toarray()
        ref = np.linalg.solve(M, x)
        # the solve is accepted at a backward error of 4e-15 and these matrices are diagonally dominant (condition number below
        # 100): the bars of the SuperLU comparisons hold against the dense solve too
        _, info = K.check_solve(op, sp.csc_matrix(M), x, ref=ref)
        assert_info(info)
        assert np.array_equal(op.perform_op(np.zeros(n)), np.zeros(n))  # x = 0 gives y = 0 exactly, without iterating
        assert op.iterative_info()["last_iterations"] == 0


def test_multiple_of_identity(ctx):
    n = 257
    op = sa.SparseSymShiftSolve(sp.identity(n, format="csc") * 4.0, ctx=ctx, solver="iterative")
    op.set_shift(2.0)
    x = np.random.default_rng(5).uniform(-1, 1, n)
    y = op.perform_op(x)
    info = op.iterative_info()
    print(info)
    assert info["last_iterations"] == 1 and info["last_passes"] == 1, info  # the Krylov space is exhausted after one step
    assert np.abs(y - x / 2.0).max() <= 4 * np.finfo(float).eps


def test_solve_into_a_pointer_that_is_only_8_byte_aligned(ctx):
    n = 1025
    A = K.random_sym(n, seed=77)
    op = sa.SparseSymShiftSolve(K.lower(A), ctx=ctx, solver="iterative")
    op.set_shift(0.0)
    x = np.random.default_rng(6).uniform(-1, 1, n)
    want = op.perform_op(x)
    xd = torch.zeros(n + 3, dtype=torch.float64, device="cuda")
    yd = torch.full((n + 3,), -123.5, dtype=torch.float64, device="cuda")
    xd[1:n + 1] = torch.from_numpy(x).cuda()
    assert (xd.data_ptr() + 8) % 16 == 8 and (yd.data_ptr() + 8) % 16 == 8
    torch.cuda.synchronize()
    op.solve_device(xd.data_ptr() + 8, yd.data_ptr() + 8)
    torch.cuda.synchronize()
    got = yd.cpu().numpy()
    assert np.array_equal(got[1:n + 1], want)
    assert got[0] == -123.5 and np.all(got[n + 1:] == -123.5)


# ---- 3. same bits ------------------------------------------------------------------------------------------------------------
def test_bits(ctx):
    A, _ = K.lap3(17, 17, 17)
    n, kmax = A.shape[0], 5
    op = sa.SparseSymShiftSolve(K.lower(A), ctx=ctx, solver="iterative")
    op.set_shift(0.0)
    rng = np.random.default_rng(7)
    x = rng.uniform(-1, 1, n)
    y = op.perform_op(x)
    assert np.array_equal(y, op.perform_op(x))  # two solves of one right-hand side
    iters = op.iterative_info()["last_iterations"]
    try:
        for check in (1, 16):
            sa.set_option("shift", "minres_check=%d" % check)
            assert np.array_equal(y, op.perform_op(x)), check
            assert op.iterative_info()["last_iterations"] == iters
    finally:
        sa.set_option("shift", None)
    op.set_shift(0.0)  # a second set_shift at the same sigma
    assert np.array_equal(y, op.perform_op(x))
    ld = n + 3
    host = np.full((kmax, ld), 7.25)
    host[:, :n] = rng.uniform(-1, 1, (kmax, n))
    Xd = torch.from_numpy(host).cuda()  # (kmax, ld) row-major = ld x kmax column-major
    Yd = torch.full((kmax, ld), -123.5, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    op.solve_block_device(Xd.data_ptr(), ld, kmax, Yd.data_ptr(), ld)
    torch.cuda.synchronize()
    Y = Yd.cpu().numpy()
    for c in range(kmax):
        assert np.array_equal(Y[c, :n], op.perform_op(host[c, :n])), c
    assert np.all(Y[:, n:] == -123.5)
    Yh = op.perform_op_block(host[:, :n].T)
    assert np.array_equal(Yh, Y[:, :n].T)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    A, _ = K.expander()
    n = A.shape[0]
    op = sa.SparseSymShiftSolve(K.lower(A), ctx=ctx, solver="auto")
    with pytest.raises(AssertionError, match="set_shift"):  # std::logic_error: solve before set_shift, as on the other paths
        op.perform_op(np.ones(n))
    bulk = A.diagonal().mean() / 2  # inside the bulk of the spectrum: Jacobi-preconditioned MINRES does not get there
    op.set_iterative(max_iterations=200)
    with pytest.raises(ValueError, match="did not converge in 200 iterations"):
        op.set_shift(bulk)
    with pytest.raises(AssertionError, match="set_shift"):  # the refused shift is not used
        op.perform_op(np.ones(n))
    op.set_iterative()  # the defaults again
    op.set_shift(0.0)  # the handle recovers
    x = np.random.default_rng(2).uniform(-1, 1, n)
    assert np.linalg.norm(A @ op.perform_op(x) - x) <= 1e-12 * np.linalg.norm(x)
    with pytest.raises(ValueError, match="unknown shift solver"):
        sa.SparseSymShiftSolve(K.lower(A), ctx=ctx, solver="minres")


def test_lobpcg_refuses_the_iterative_path(ctx):
    A, _ = K.lap3(17, 17, 17)
    T = sa.SparseSymShiftSolve(K.lower(A), ctx=ctx, solver="iterative")
    T.set_shift(0.0)
    with pytest.raises(ValueError, match="iterative shift-solve path"):
        sa.LOBPCGSolver(sa.SparseSymMatProd(A.tocsr(), ctx=ctx), L.X0(A.shape[0], 4), preconditioner=T)


def test_a_sharded_context_is_refused(ctx):
    A, _ = K.lap3(17, 17, 17)
    lib = sa.lib()
    grp = C.c_void_p()
    _capi.check(lib.mispec_loopback_create(2, C.byref(grp)))
    try:
        sctx = sa.Context(0)
        _capi.check(lib.mispec_loopback_attach(grp, sctx.h, 0))
        sctx.rank, sctx.world = 0, 2
        for solver in ("auto", "iterative"):
            with pytest.raises(ValueError, match="cannot be row-sharded"):
                sa.SparseSymShiftSolve(K.lower(A), ctx=sctx, solver=solver)
        del sctx
    finally:
        _capi.check(lib.mispec_loopback_destroy(grp))


# ---- 5. eigenproblems ------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["onesweep", "reference"])
def orth_env(request, monkeypatch):
    """both defaults of the orthogonalisation scheme, as tests/test_gpu_shift.py runs its solvers"""
    monkeypatch.setenv("MISPEC_ORTH", request.param)
    return request.param


def check_eigenpairs(ev, X, want, A, B=None):
    order = np.argsort(ev)
    ev, X = ev[order], X[:, order]
    BX = X if B is None else B @ X
    assert np.abs(ev - want).max() <= 1e-9, (ev, want)
    assert np.abs(A @ X - BX * ev).max() <= 1e-10
    assert np.abs(X.T @ BX - np.eye(len(ev))).max() <= 1e-10


def test_eigenpairs_of_a_3d_laplacian(ctx, orth_env):
    A, lam = K.lap3(*BIG)
    k, m = 4, 20
    op = sa.SparseSymShiftSolve(K.lower(A), ctx=ctx, solver="auto")
    assert op.path_info()["path"] == 3 and op.bandwidth_info()["as_given"] == BIG[0] * BIG[1]
    eigs = sa.SymEigsShiftSolver(op, k, m, 0.0)
    eigs.init()
    assert eigs.compute(sa.SortRule.LargestMagn, 1000, 1e-11) == k
    assert eigs.orth_info()["mode"] == "reference", eigs.orth_info()  # host-driven steps on this path, whatever MISPEC_ORTH says
    info = op.iterative_info()
    print(orth_env, info)
    assert_info(info)
    check_eigenpairs(eigs.eigenvalues(), eigs.eigenvectors(), lam[:k], A)


@functools.lru_cache(maxsize=None)
def generalized_reference(k):
    A, _ = K.lap3(*BIG)
    B = sp.diags(np.random.default_rng(8).uniform(1.0, 2.0, A.shape[0])).tocsc()
    return A, B, np.sort(spla.eigsh(A, k=k, M=B, sigma=0.0, which="LM", tol=1e-13, return_eigenvectors=False))


def test_generalized_eigenpairs(ctx, orth_env):
    k, m = 4, 20
    A, B, want = generalized_reference(k)
    op = sa.SymShiftInvert(K.lower(A), B, ctx=ctx, solver="auto")
    assert op.path_info()["path"] == 3
    eigs = sa.SymGEigsShiftSolver(op, sa.SparseSymMatProd(B, ctx=ctx), k, m, 0.0, "ShiftInvert")
    eigs.init()
    assert eigs.compute(sa.SortRule.LargestMagn, 1000, 1e-11) == k
    assert_info(op.iterative_info())
    check_eigenpairs(eigs.eigenvalues(), eigs.eigenvectors(), want, A, B)
