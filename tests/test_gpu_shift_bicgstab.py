"""The iterative path of the general shift-and-invert operator (csrc/shift_bicgstab.hip): Jacobi-preconditioned BiCGStab on the
SpMV's own operator, for non-symmetric matrices beyond the dense path's n = 4096.  Opt-in (option shift_solver, the solver
argument), so every test names its solver kind.  The bars against SuperLU are shift_minres_checks.check_solve's (relative residual
and error <= 1e-12); the iteration-count caps come from the numpy restatement in shift_gen_checks (twice its count plus 10: a
condition on the recurrence, not a measurement); the eigenproblem bars are DESIGN.md section 5's."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import shift_gen_checks as G
import spectra_amd as sa

pytestmark = pytest.mark.gpu

BIG = (26, 28, 30)
SHAPES = [1, 2, 3, 255, 256, 257, 1023, 1025, 4097]


def assert_info(info, reference_iterations=None):
    assert info["last_backward_error"] <= 1e-13 and info["last_iterations"] >= 0, info
    if reference_iterations is not None:  # test 9 of the issue: the recurrence is the restatement's
        assert info["last_iterations"] <= 2 * reference_iterations + 10, (info, reference_iterations)


def solve_and_check(op, A, sigma, name=None, args=None, ref=None):
    n = A.shape[0]
    op.set_shift(sigma)
    _, info = G.check_solve(op, A - sigma * sp.identity(n), G.solve_rhs(n), ref=ref)
    assert_info(info, None if name is None else G.reference_count(name, args, sigma))
    return info


# ---- 1. against SuperLU --------------------------------------------------------------------------------------------------------
def test_digraph_under_auto(ctx):
    A = G.digraph()
    op = sa.SparseGenRealShiftSolve(A, ctx=ctx, solver="auto")
    assert op.path_info() == {"path": 3, "block_rows": 0, "blocks": 0, "factor_bytes": 0}, op.path_info()
    with pytest.raises(ValueError, match="only n <= 4096"):
        sa.SparseGenRealShiftSolve(A, ctx=ctx, solver="direct")
    for sigma in (0.0, -1.5):
        solve_and_check(op, A, sigma, "digraph", ())
        ref = op.refinement_info()
        assert ref["refine_steps"] == 0 and ref["boosted_pivots"] == 0 and 0 < ref["probe_backward_error"] <= 1e-13, ref
        assert op.iterative_info()["probe_iterations"] > 0


@pytest.mark.parametrize("sigma", [0.0, -1.0])
def test_convection_diffusion_forced_iterative(ctx, sigma):
    A, _ = G.cd3(17, 17, 17, 0.4)
    op = sa.SparseGenRealShiftSolve(A, ctx=ctx, solver="iterative")
    assert op.path_info()["path"] == 3
    solve_and_check(op, A, sigma, "cd3", (17, 17, 17, 0.4))


# ---- 2. transposition ----------------------------------------------------------------------------------------------------------
def test_both_storage_orders_give_one_operator(ctx):
    A = G.digraph()
    n = A.shape[0]
    x = G.solve_rhs(n)
    ys = []
    for mat in (A.tocsc(), A.tocsr()):
        op = sa.SparseGenRealShiftSolve(mat, ctx=ctx, solver="auto")
        op.set_shift(0.0)
        y, info = G.check_solve(op, A, x)  # a transposed operator misses these bars by orders of magnitude
        assert_info(info)
        ys.append(y)
    assert np.array_equal(ys[0], ys[1])


# ---- 3. direct and iterative agree ---------------------------------------------------------------------------------------------
def test_direct_and_iterative_agree(ctx):
    A, _ = G.cd3(12, 13, 14, 0.4)
    n = A.shape[0]
    direct = sa.SparseGenRealShiftSolve(A, ctx=ctx, solver="direct")
    auto = sa.SparseGenRealShiftSolve(A, ctx=ctx, solver="auto")  # the dense path exists: auto keeps it
    it = sa.SparseGenRealShiftSolve(A, ctx=ctx, solver="iterative")
    assert direct.path_info()["path"] == 0 and auto.path_info() == direct.path_info() and it.path_info()["path"] == 3
    assert direct.iterative_info() == {"last_iterations": 0, "total_iterations": 0, "solves": 0, "last_passes": 0,
                                       "last_backward_error": 0.0, "probe_iterations": 0}
    x = G.solve_rhs(n)
    for op in (direct, it):
        op.set_shift(0.0)
    yd, yi = direct.perform_op(x), it.perform_op(x)
    print("direct against iterative: %.2e" % (np.abs(yd - yi).max() / np.abs(yd).max()))
    assert np.abs(yd - yi).max() <= 1e-12 * np.abs(yd).max()
    assert_info(it.iterative_info())


# ---- 4. kernel shapes: one row, the pair loop's tail, one and several workgroups -----------------------------------------------
@pytest.mark.parametrize("n", SHAPES)
def test_kernel_shapes(ctx, n):
    A = G.random_gen(n, n)
    op = sa.SparseGenRealShiftSolve(A, ctx=ctx, solver="iterative")
    assert op.path_info()["path"] == 3
    for sigma in (0.0, 0.25):
        ref = np.linalg.solve((A - sigma * sp.identity(n)).toarray(), G.solve_rhs(n))
        solve_and_check(op, A, sigma, "random_gen", (n, n), ref=ref)
        assert np.array_equal(op.perform_op(np.zeros(n)), np.zeros(n))  # x = 0 gives y = 0 exactly, without iterating
        assert op.iterative_info()["last_iterations"] == 0


# ---- 5. exhausted Krylov space -------------------------------------------------------------------------------------------------
def test_multiple_of_identity(ctx):
    n = 257
    op = sa.SparseGenRealShiftSolve(sp.identity(n, format="csc") * 4.0, ctx=ctx, solver="iterative")
    op.set_shift(2.0)
    x = G.solve_rhs(n)
    y = op.perform_op(x)
    info = op.iterative_info()
    print(info)
    assert info["last_iterations"] == 1 and info["last_passes"] == 1, info
    assert np.all(np.abs(y - x / 2.0) <= 4 * np.spacing(np.abs(x / 2.0)))  # 4 ulp of x / 2, entry by entry


# ---- 6. 8-byte alignment -------------------------------------------------------------------------------------------------------
def test_solve_into_a_pointer_that_is_only_8_byte_aligned(ctx):
    n = 1025
    op = sa.SparseGenRealShiftSolve(G.random_gen(n, 77), ctx=ctx, solver="iterative")
    op.set_shift(0.0)
    x = G.solve_rhs(n)
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


# ---- 7. same bits for every check ----------------------------------------------------------------------------------------------
def test_bits(ctx):
    n, kmax = 1025, 3
    op = sa.SparseGenRealShiftSolve(G.random_gen(n, n), ctx=ctx, solver="iterative")
    op.set_shift(0.0)
    x = G.solve_rhs(n)
    y = op.perform_op(x)
    assert np.array_equal(y, op.perform_op(x))  # two consecutive calls
    iters = op.iterative_info()["last_iterations"]
    try:
        for check in (1, 16, 64):
            sa.set_option("shift", "minres_check=%d" % check)
            assert np.array_equal(y, op.perform_op(x)), check
            assert op.iterative_info()["last_iterations"] == iters
    finally:
        sa.set_option("shift", None)
    X = np.asfortranarray(np.random.default_rng(7).uniform(-1, 1, (n, kmax)))  # block solves run the column loop
    Y = op.perform_op_block(X)
    for c in range(kmax):
        assert np.array_equal(Y[:, c], op.perform_op(X[:, c])), c


# ---- 8. refusal ----------------------------------------------------------------------------------------------------------------
def test_a_singular_shift_is_refused_and_the_handle_recovers(ctx):
    n = 257
    A = G.upper_bidiagonal(n)
    op = sa.SparseGenRealShiftSolve(A, ctx=ctx, solver="iterative")
    with pytest.raises(AssertionError, match="set_shift"):  # std::logic_error: solve before set_shift, as on the other paths
        op.perform_op(np.ones(n))
    op.set_iterative(max_iterations=200)
    with pytest.raises(ValueError, match="did not converge"):
        op.set_shift(3.0)  # A - 3 I is exactly singular: a convergence failure, no device fault
    print(sa.lib().mispec_last_error().decode())
    with pytest.raises(AssertionError, match="set_shift"):  # the refused shift is not used
        op.perform_op(np.ones(n))
    solve_and_check(op, A, 0.5)  # the handle recovers
    with pytest.raises(ValueError, match="unknown shift solver"):
        sa.SparseGenRealShiftSolve(A, ctx=ctx, solver="bicgstab")


def test_a_complex_shift_is_refused_on_the_iterative_path(ctx):
    import ctypes as C

    A = G.random_gen(64, 64)
    op = sa.SparseGenRealShiftSolve(A, ctx=ctx, solver="iterative")
    rc = sa.lib().mispec_symshift_set_shift_complex(op.h, C.c_double(0.5), C.c_double(0.25))
    assert rc == sa._capi.MISPEC_EINVAL and "real shifts only" in sa.lib().mispec_last_error().decode()


def test_a_sharded_context_is_refused(ctx):
    import ctypes as C

    from spectra_amd import _capi

    A = G.random_gen(64, 64)
    lib = sa.lib()
    grp = C.c_void_p()
    _capi.check(lib.mispec_loopback_create(2, C.byref(grp)))
    try:
        sctx = sa.Context(0)
        _capi.check(lib.mispec_loopback_attach(grp, sctx.h, 0))
        sctx.rank, sctx.world = 0, 2
        for solver in ("auto", "iterative"):
            with pytest.raises(ValueError, match="cannot be row-sharded"):
                sa.SparseGenRealShiftSolve(A, ctx=sctx, solver=solver)
        del sctx
    finally:
        _capi.check(lib.mispec_loopback_destroy(grp))


# ---- 10. eigenproblems ---------------------------------------------------------------------------------------------------------
def gen_eigs(op, k, m):
    eigs = sa.GenEigsRealShiftSolver(op, k, m, 0.0)
    eigs.init()
    assert eigs.compute(sa.SortRule.LargestMagn, 1000, 1e-11) == k
    ev, X = eigs.eigenvalues(), eigs.eigenvectors()
    order = np.argsort(ev.real)
    return eigs, ev[order], X[:, order]


def test_eigenvalues_of_convection_diffusion(ctx):
    A, lam = G.cd3(*BIG, 0.1)
    k, m = 4, 20
    op = sa.SparseGenRealShiftSolve(A, ctx=ctx, solver="auto")
    assert op.path_info()["path"] == 3 and A.shape[0] == 21840
    eigs, ev, X = gen_eigs(op, k, m)
    info = op.iterative_info()
    print(info, ev)
    assert_info(info)
    assert np.abs(ev.imag).max() == 0.0 and np.all(np.abs(ev.real - lam[:k]) <= 1e-9 * lam[:k]), (ev, lam[:k])
    assert np.abs(A @ X - X * ev).max() <= 1e-10
    # the factorisation under the solver takes host-driven steps on this path (csrc/fac.hip), in the reference's control flow
    assert sa.Factorization(op, m, symmetric=False).orth_info()["mode"] == "reference"


def test_eigenvalues_through_the_dense_and_the_iterative_operator(ctx):
    A, lam = G.cd3(12, 13, 14, 0.1)
    k, m = 4, 20
    got = []
    for solver, path in (("direct", 0), ("iterative", 3)):
        op = sa.SparseGenRealShiftSolve(A, ctx=ctx, solver=solver)
        assert op.path_info()["path"] == path
        got.append(gen_eigs(op, k, m)[1])
    print(got)
    assert np.abs(got[0] - got[1]).max() <= 1e-10
    assert np.all(np.abs(got[1].real - lam[:k]) <= 1e-9 * lam[:k])
