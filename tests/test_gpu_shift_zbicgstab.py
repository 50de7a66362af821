"""Complex shifts on the iterative path of the general shift-and-invert operator (csrc/shift_zbicgstab.hip): Jacobi-preconditioned
BiCGStab in complex arithmetic on the SpMV's own operator, y = Re((A - sigma I)^{-1} x) beyond the dense path's n = 4096.  Opt-in
(complex_solver=), so every test names its solver kind.  The bars against SuperLU on the complex matrix are
shift_cplx_checks.check_solve's (error <= 1e-12 max(1, max |ref|), backward error <= 1e-13); the iteration-count caps come from
the numpy restatement in shift_cplx_checks (twice its count plus 10: a condition on the recurrence, not a measurement); the
eigenproblem bars are DESIGN.md section 5's."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import shift_cplx_checks as Z
import spectra_amd as sa

pytestmark = pytest.mark.gpu

BIG = (20, 21, 22, 0.5)  # n = 9240
SMALL = (12, 13, 14, 0.5)  # n = 2184: the dense path exists
SHIFT = (1.5, 1.0)


def solve_and_check(op, A, sigma, name=None, args=None, ref=None):
    n = A.shape[0]
    op.set_shift(sigma.real, sigma.imag)
    y, info = Z.check_solve(op, A, sigma, Z.solve_rhs(n), ref=ref)
    if name is not None:  # the recurrence is the restatement's
        count = Z.reference_count(name, args, sigma)
        assert info["last_iterations"] <= 2 * count + 10, (info, count)
    return y, info


# ---- 1. against SuperLU --------------------------------------------------------------------------------------------------------
def test_rotating_flow_under_auto(ctx):
    A, _ = Z.rot3(*BIG)
    assert A.shape[0] == 9240
    op = sa.SparseGenComplexShiftSolve(A, ctx=ctx, complex_solver="auto")
    assert op.path_info() == {"path": 3, "block_rows": 0, "blocks": 0, "factor_bytes": 0}, op.path_info()
    with pytest.raises(ValueError, match="only n <= 4096"):
        sa.SparseGenComplexShiftSolve(A, ctx=ctx, complex_solver="direct")
    for sigma in (1.5 + 1j, 0.5j):
        solve_and_check(op, A, sigma, "rot3", BIG)
        ref = op.refinement_info()
        assert ref["refine_steps"] == 0 and ref["boosted_pivots"] == 0 and 0 < ref["probe_backward_error"] <= 1e-13, ref
        assert op.iterative_info()["probe_iterations"] > 0


# ---- 2. transposition ----------------------------------------------------------------------------------------------------------
def test_both_storage_orders_give_one_operator(ctx):
    A, _ = Z.rot3(*BIG)
    x = Z.solve_rhs(A.shape[0])
    ys = []
    for mat in (A.tocsc(), A.tocsr()):
        op = sa.SparseGenComplexShiftSolve(mat, ctx=ctx, complex_solver="auto")
        op.set_shift(*SHIFT)
        ys.append(Z.check_solve(op, A, complex(*SHIFT), x)[0])  # a transposed operator (the shift's conjugate) misses these bars
    assert np.array_equal(ys[0], ys[1])


# ---- 3. direct and iterative agree ---------------------------------------------------------------------------------------------
def test_direct_and_iterative_agree(ctx):
    A, _ = Z.rot3(*SMALL)
    n = A.shape[0]
    direct = sa.SparseGenComplexShiftSolve(A, ctx=ctx, complex_solver="direct")
    auto = sa.SparseGenComplexShiftSolve(A, ctx=ctx, complex_solver="auto")  # the dense path exists: auto keeps it
    it = sa.SparseGenComplexShiftSolve(A, ctx=ctx, complex_solver="iterative")
    assert direct.path_info()["path"] == 0 and auto.path_info() == direct.path_info() and it.path_info()["path"] == 3
    x = Z.solve_rhs(n)
    for op in (direct, it):
        op.set_shift(*SHIFT)
    yd, yi = direct.perform_op(x), it.perform_op(x)
    print("direct against iterative: %.2e" % (np.abs(yd - yi).max() / np.abs(yd).max()))
    assert np.abs(yd - yi).max() <= 1e-12 * np.abs(yd).max()
    assert it.iterative_info()["last_backward_error"] <= 1e-13 and direct.iterative_info()["solves"] == 0


# ---- 4. kernel shapes: one row, the pair loop's tail, one and several workgroups -----------------------------------------------
@pytest.mark.parametrize("n", Z.SHAPES)
def test_kernel_shapes(ctx, n):
    A = Z.random_gen(n, n)
    op = sa.SparseGenComplexShiftSolve(A, ctx=ctx, complex_solver="iterative")
    assert op.path_info()["path"] == 3
    x = Z.solve_rhs(n)
    for sigma in (0.25 + 0.5j, -1j):
        ref = None if n > 4096 else np.linalg.solve(A.toarray() - sigma * np.eye(n), x.astype(complex)).real
        solve_and_check(op, A, sigma, "random_gen", (n, n), ref=ref)
        assert np.array_equal(op.perform_op(np.zeros(n)), np.zeros(n))  # x = 0 gives y = 0 exactly, without iterating
        assert op.iterative_info()["last_iterations"] == 0


# ---- 5. exhausted Krylov space -------------------------------------------------------------------------------------------------
def test_multiple_of_identity(ctx):
    n = 257
    op = sa.SparseGenComplexShiftSolve(sp.identity(n, format="csc") * 4.0, ctx=ctx, complex_solver="iterative")
    op.set_shift(2.0, 1.0)
    x = Z.solve_rhs(n)
    y = op.perform_op(x)
    info = op.iterative_info()
    print(info)
    assert info["last_iterations"] == 1 and info["last_passes"] == 1, info
    want = (x / (2 - 1j)).real
    assert np.all(np.abs(y - want) <= 4 * np.spacing(np.abs(want)))  # 4 ulp, entry by entry


# ---- 6. 8-byte alignment -------------------------------------------------------------------------------------------------------
def test_solve_into_a_pointer_that_is_only_8_byte_aligned(ctx):
    n = 1025
    op = sa.SparseGenComplexShiftSolve(Z.random_gen(n, 77), ctx=ctx, complex_solver="iterative")
    op.set_shift(0.25, 0.5)
    x = Z.solve_rhs(n)
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
    op = sa.SparseGenComplexShiftSolve(Z.random_gen(n, n), ctx=ctx, complex_solver="iterative")
    op.set_shift(0.25, 0.5)
    x = Z.solve_rhs(n)
    y = op.perform_op(x)
    assert np.array_equal(y, op.perform_op(x))  # two consecutive calls
    iters = op.iterative_info()["last_iterations"]
    assert iters > 0
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


# ---- 8. real and complex shifts on one handle ----------------------------------------------------------------------------------
def test_real_and_complex_shifts_on_one_handle(ctx):
    n = 1025
    A = Z.random_gen(n, n)
    x = Z.solve_rhs(n)
    op = sa.SparseGenComplexShiftSolve(A, ctx=ctx, complex_solver="iterative")
    real = sa.SparseGenRealShiftSolve(A, ctx=ctx, solver="iterative")
    real.set_shift(0.3)
    want_real = real.perform_op(x)
    op.set_shift(0.3, 0.7)
    y1 = Z.check_solve(op, A, 0.3 + 0.7j, x)[0]
    op.set_shift(0.3, 0.0)
    y2 = op.perform_op(x)
    op.set_shift(0.3, 0.7)
    y3 = op.perform_op(x)
    assert np.array_equal(y1, y3) and np.array_equal(y2, want_real)
    assert np.abs(y1 - y2).max() > 1e-3  # (two different operators)
    sa.lib().mispec_symshift_set_shift(op.h, C.c_double(0.3))  # the real entry point on the same handle
    assert np.array_equal(op.perform_op(x), want_real)


# ---- 9. refusal ----------------------------------------------------------------------------------------------------------------
def test_a_shift_that_does_not_converge_is_refused_and_the_handle_recovers(ctx):
    A, _ = Z.rot3(8, 9, 10, 0.5)
    n = A.shape[0]
    op = sa.SparseGenComplexShiftSolve(A, ctx=ctx, complex_solver="iterative")
    with pytest.raises(AssertionError, match="set_shift"):  # std::logic_error: solve before set_shift, as on the other paths
        op.perform_op(np.ones(n))
    op.set_iterative(max_iterations=200)
    with pytest.raises(ValueError, match="did not converge"):
        op.set_shift(6.0, 0.3)  # inside the spectrum's hull: a convergence failure, no device fault
    print(sa.lib().mispec_last_error().decode())
    with pytest.raises(AssertionError, match="set_shift"):  # the refused shift is not used
        op.perform_op(np.ones(n))
    solve_and_check(op, A, 1.5 + 1j, "rot3", (8, 9, 10, 0.5))  # the handle recovers


def test_a_sharded_context_is_refused(ctx):
    from spectra_amd import _capi

    A = Z.random_gen(64, 64)
    lib = sa.lib()
    grp = C.c_void_p()
    _capi.check(lib.mispec_loopback_create(2, C.byref(grp)))
    try:
        sctx = sa.Context(0)
        _capi.check(lib.mispec_loopback_attach(grp, sctx.h, 0))
        sctx.rank, sctx.world = 0, 2
        for solver in ("auto", "iterative"):
            with pytest.raises(ValueError, match="cannot be row-sharded"):
                sa.SparseGenComplexShiftSolve(A, ctx=sctx, complex_solver=solver)
        del sctx
    finally:
        _capi.check(lib.mispec_loopback_destroy(grp))


# ---- 10. eigenproblems ---------------------------------------------------------------------------------------------------------
def gen_eigs(op, k, m):
    eigs = sa.GenEigsComplexShiftSolver(op, k, m, *SHIFT)
    eigs.init()
    assert eigs.compute(sa.SortRule.LargestMagn, 1000, 1e-11) == k
    return eigs.eigenvalues(), eigs.eigenvectors()


def test_eigenvalues_of_the_rotating_flow(ctx):
    A, lam = Z.rot3(*BIG)
    k, m = 4, 20
    op = sa.SparseGenComplexShiftSolve(A, ctx=ctx, complex_solver="auto")
    assert op.path_info()["path"] == 3
    ev, X = gen_eigs(op, k, m)
    info = op.iterative_info()
    print(info, ev)
    assert info["last_backward_error"] <= 1e-13
    assert len(ev) == k and max(np.abs(lam - e).min() / abs(e) for e in ev) <= 1e-9, ev
    want = np.array([2.04269546 + 0.99068595j, 2.04269546 - 0.99068595j, 2.04269546 + 0.96291729j, 2.04269546 - 0.96291729j])
    assert all(np.abs(want - e).min() <= 1e-7 for e in ev) and all(np.abs(ev - w).min() <= 1e-7 for w in want), ev
    assert np.abs(A @ X - X * ev).max() <= 1e-10
    # the factorisation under the solver takes host-driven steps on this path (csrc/fac.hip), in the reference's control flow
    assert sa.Factorization(op, m, symmetric=False).orth_info()["mode"] == "reference"


def test_eigenvalues_through_the_dense_and_the_iterative_operator(ctx):
    A, lam = Z.rot3(*SMALL)
    k, m = 4, 20
    got = []
    for solver, path in (("direct", 0), ("iterative", 3)):
        op = sa.SparseGenComplexShiftSolve(A, ctx=ctx, complex_solver=solver)
        assert op.path_info()["path"] == path
        got.append(gen_eigs(op, k, m)[0])
    print(got)
    # a conjugate pair may be represented by either member: compare up to conjugation
    assert max(Z.match_up_to_conjugation(got[0], got[1], False), Z.match_up_to_conjugation(got[1], got[0], False)) <= 1e-10
    assert max(np.abs(lam - e).min() / abs(e) for e in got[1]) <= 1e-9
