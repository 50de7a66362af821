"""The block-tridiagonal path of the shift-and-invert operators (csrc/shift_blocktri.hip): symmetric bands of half-bandwidth
65 ... 512 beyond n = 4096, cut into dense s x s blocks (s = the half-bandwidth), factored on the device at set_shift() and solved by a
chain of one launch per block.  Shapes are chosen for the block layout (a short last block, exact multiples, odd s, the cap 512);
the bars are those of tests/test_gpu_shift.py for the chunk path."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

import lobpcg_checks as L
import spectra_amd as sa
from spectra_amd import _capi

pytestmark = pytest.mark.gpu


def banded_spd(n, b, seed=0):
    rng = np.random.default_rng(seed)
    diags = [rng.uniform(-0.5, 0.5, n - d) for d in range(1, b + 1)]
    A = sp.diags([rng.uniform(-0.5, 0.5, n) + b + 0.5] + diags + diags, [0] + list(range(1, b + 1)) + [-d for d in range(1, b + 1)],
                 format="csc")
    return A


def banded_indef(n, b, seed=0):
    rng = np.random.default_rng(seed)
    diags = [rng.uniform(-0.5, 0.5, n - d) for d in range(1, b + 1)]
    return sp.diags([rng.uniform(-0.5, 0.5, n)] + diags + diags, [0] + list(range(1, b + 1)) + [-d for d in range(1, b + 1)], format="csc")


GRID = (66, 75)  # short side first: n = 4950, half-bandwidth 66


@functools.lru_cache(maxsize=None)
def grid_laplacian(p=GRID[0], q=GRID[1]):
    """the 5-point Laplacian of a p x q grid numbered along the short side p, and its eigenvalues (closed form), ascending"""
    T = lambda m: sp.diags([2 * np.ones(m), -np.ones(m - 1), -np.ones(m - 1)], [0, 1, -1])  # noqa: E731
    A = (sp.kron(T(q), sp.identity(p)) + sp.kron(sp.identity(q), T(p))).tocsc()
    lam = (2 - 2 * np.cos(np.arange(1, p + 1) * np.pi / (p + 1)))[:, None] + (2 - 2 * np.cos(np.arange(1, q + 1) * np.pi / (q + 1)))[None, :]
    return A, np.sort(lam, axis=None)


def is_block_path(op, n, b):
    info = op.path_info()
    return info == {"path": 2, "block_rows": b, "blocks": -(-n // b), "factor_bytes": 16 * -(-n // b) * b * b}, info


def check_solve(op, M, x, res_tol, err_tol, ref=None):
    y = op.perform_op(x)
    ref = spla.splu(M.tocsc()).solve(x) if ref is None else ref
    res, err = np.linalg.norm(M @ y - x) / np.linalg.norm(x), np.abs(y - ref).max() / max(1.0, np.abs(ref).max())
    print("relative residual %.2e, error against SuperLU %.2e, refinement %s" % (res, err, getattr(op, "refinement_info", dict)()))
    assert res <= res_tol and err <= err_tol, (res, err)
    return y


# ---- 1. the operator against SuperLU ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,b", [(4097, 65), (4160, 65), (4200, 100), (4608, 128), (6000, 257), (8229, 512)])
def test_block_solve_matches_sparse_lu(ctx, n, b):
    A = banded_spd(n, b, seed=n)
    op = sa.SparseSymShiftSolve(sp.tril(A).tocsc(), ctx=ctx)
    ok, info = is_block_path(op, n, b)
    assert ok, info
    x = np.random.default_rng(1).uniform(-1, 1, n)
    for sigma in (0.0, -1.5):
        op.set_shift(sigma)
        check_solve(op, A - sigma * sp.identity(n), x, 1e-12, 1e-12)
        assert op.refinement_info()["refine_steps"] == 0 and op.refinement_info()["boosted_pivots"] == 0, op.refinement_info()


# ---- 2. interior shift: no pivoting across blocks, the calibrated refinement wins the digits back ---------------------------------
@pytest.mark.parametrize("n,b", [(4500, 65), (6000, 129)])
def test_interior_shift(ctx, n, b):
    sigma = 0.3
    A = banded_indef(n, b, seed=n)
    op = sa.SparseSymShiftSolve(sp.tril(A).tocsc(), ctx=ctx)
    assert is_block_path(op, n, b)[0]
    op.set_shift(sigma)
    info = op.refinement_info()
    print(info)
    assert info["refine_steps"] <= 12 and info["probe_backward_error"] <= 1e-13 and info["boosted_pivots"] == 0, info
    x = np.random.default_rng(4).uniform(-1, 1, n)
    check_solve(op, A - sigma * sp.identity(n), x, 1e-10, 1e-8)


# ---- 3. pencil: B is subtracted at assembly, its band is narrower than A's ---------------------------------------------------
@pytest.mark.parametrize("sigma,res_tol,err_tol", [(0.0, 1e-12, 1e-12), (0.7, 1e-10, 1e-8)])
def test_pencil(ctx, sigma, res_tol, err_tol):
    n = 4300
    A, B = banded_spd(n, 80, 1), banded_spd(n, 3, 2)
    op = sa.SymShiftInvert(sp.tril(A).tocsc(), sp.tril(B).tocsc(), ctx=ctx)
    assert is_block_path(op, n, 80)[0]
    op.set_shift(sigma)
    x = np.random.default_rng(3).uniform(-1, 1, n)
    check_solve(op, A - sigma * B, x, res_tol, err_tol)


# ---- 4. reordering -----------------------------------------------------------------------------------------------------------
def test_reordered_wide_band(ctx):
    n, b = 6000, 100
    rng = np.random.default_rng(11)
    q = rng.permutation(n)
    A = banded_spd(n, b, seed=7)[q][:, q].tocsc()
    op = sa.SparseSymShiftSolve(sp.tril(A).tocsc(), ctx=ctx)
    info = op.bandwidth_info()
    print(info, op.path_info())
    assert info["reordered"] and info["as_given"] >= 1000 and 64 < info["stored"] <= 512, info
    assert is_block_path(op, n, info["stored"])[0], op.path_info()
    for sigma in (0.0, -1.0):
        op.set_shift(sigma)
        check_solve(op, A - sigma * sp.identity(n), rng.uniform(-1, 1, n), 1e-12, 1e-11)


def test_reordering_still_prefers_the_chunk_path(ctx):
    """the scrambled half-bandwidth 20 case of tests/test_gpu_shift.py: the ordering brings it under 64, which keeps priority"""
    n, b = 30_000, 20
    q = np.random.default_rng(11).permutation(n)
    op = sa.SparseSymShiftSolve(sp.tril(banded_spd(n, b, seed=7)[q][:, q]).tocsc(), ctx=ctx)
    info = op.bandwidth_info()
    assert info["reordered"] and info["stored"] <= 64, info
    assert op.path_info() == {"path": 1, "block_rows": 0, "blocks": 0, "factor_bytes": 0}


def test_grid_in_natural_order(ctx):
    A, _ = grid_laplacian()
    op = sa.SparseSymShiftSolve(sp.tril(A).tocsc(), ctx=ctx)
    info, path = op.bandwidth_info(), op.path_info()
    assert info["as_given"] == GRID[0] and info["stored"] <= info["as_given"] and info["reordered"] == (info["stored"] < info["as_given"]), info
    assert path["path"] == 2 and path["block_rows"] == info["stored"], path


# ---- 5. eigenpairs with a closed form -----------------------------------------------------------------------------------------
@pytest.fixture(params=["onesweep", "reference"])
def orth_env(request, monkeypatch):
    """both defaults of the orthogonalisation scheme, as tests/test_gpu_shift.py runs its solvers"""
    monkeypatch.setenv("MISPEC_ORTH", request.param)
    return request.param


@pytest.mark.parametrize("sigma", [0.0, 1.0])
def test_grid_eigenpairs(ctx, orth_env, sigma):
    A, lam = grid_laplacian()
    k, m = 6, 20
    op = sa.SparseSymShiftSolve(sp.tril(A).tocsc(), ctx=ctx)
    eigs = sa.SymEigsShiftSolver(op, k, m, sigma)
    eigs.init()
    assert eigs.compute(sa.SortRule.LargestMagn, 1000, 1e-11) == k
    assert op.path_info()["path"] == 2
    print(sigma, op.refinement_info())
    ev, X = eigs.eigenvalues(), eigs.eigenvectors()
    near = np.sort(lam[np.argsort(np.abs(lam - sigma))[:k]])
    assert np.abs(np.sort(ev) - near).max() <= 1e-10, (np.sort(ev), near)
    assert np.abs(A @ X - X * ev).max() <= 1e-9 and np.abs(X.T @ X - np.eye(k)).max() <= 1e-10


# ---- 6. same bits -----------------------------------------------------------------------------------------------------------
def test_block_solve_has_the_bits_of_the_single_solve(ctx):
    n, b, kmax = 4160, 65, 5
    op = sa.SparseSymShiftSolve(sp.tril(banded_spd(n, b, seed=n)).tocsc(), ctx=ctx)
    op.set_shift(-1.5)
    rng = np.random.default_rng(6)
    for ld in (n, n + 3):
        host = np.full((kmax, ld), 7.25)
        host[:, :n] = rng.uniform(-1, 1, (kmax, n))
        Xd = torch.from_numpy(host).cuda()  # (kmax, ld) row-major = ld x kmax column-major
        single = torch.empty((kmax, n), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for c in range(kmax):
            op.solve_device(Xd.data_ptr() + 8 * c * ld, single.data_ptr() + 8 * c * n)
        torch.cuda.synchronize()
        try:
            for opt in (None, "0", "4"):
                sa.set_option("shift_block", opt)
                for k in (1, 2, 5):
                    Yd = torch.full((kmax, ld), -123.5, dtype=torch.float64, device="cuda")
                    torch.cuda.synchronize()
                    op.solve_block_device(Xd.data_ptr(), ld, k, Yd.data_ptr(), ld)
                    torch.cuda.synchronize()
                    assert np.array_equal(Yd[:k, :n].cpu().numpy(), single[:k].cpu().numpy()), (ld, opt, k)
                    assert bool((Yd[k:] == -123.5).all()) and bool((Yd[:, n:] == -123.5).all()), (ld, opt, k)
                    if ld == n:  # the host entry: perform_op_block against perform_op
                        Y = op.perform_op_block(host[:k, :n].T)
                        for c in range(k):
                            assert np.array_equal(Y[:, c], op.perform_op(host[c, :n])), (opt, k, c)
                            assert np.array_equal(Y[:, c], single[c].cpu().numpy()), (opt, k, c)
        finally:
            sa.set_option("shift_block", None)


def test_two_factorisations_give_the_same_bits(ctx):
    n, b = 4160, 65
    op = sa.SparseSymShiftSolve(sp.tril(banded_spd(n, b, seed=n)).tocsc(), ctx=ctx)
    x = np.random.default_rng(7).uniform(-1, 1, n)
    ys = []
    for _ in range(2):
        op.set_shift(-1.5)
        ys.append(op.perform_op(x))
    assert np.array_equal(ys[0], ys[1])
    assert np.array_equal(ys[0], op.perform_op(x))  # and two solves of one factorisation


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    n = 4200
    A = banded_spd(n, 70, 3).tolil()
    A[0, :] = 0.0
    A[:, 0] = 0.0
    A[0, 0] = 2.0
    op = sa.SparseSymShiftSolve(sp.tril(A.tocsc()).tocsc(), ctx=ctx)
    assert op.path_info()["path"] == 2
    with pytest.raises(AssertionError, match="set_shift"):  # std::logic_error: solve before set_shift, as on the other paths
        op.perform_op(np.ones(n))
    with pytest.raises(ValueError, match="factorization failed"):  # column 0 of block 0 is exactly zero
        op.set_shift(2.0)
    with pytest.raises(AssertionError, match="set_shift"):  # the failed factorisation is not used
        op.perform_op(np.ones(n))
    op.set_shift(0.0)  # the handle recovers
    x = np.random.default_rng(2).uniform(-1, 1, n)
    assert np.linalg.norm(A.tocsc() @ op.perform_op(x) - x) <= 1e-12 * np.linalg.norm(x)
    wide = sa.SparseSymShiftSolve(sp.tril(banded_spd(6000, 513, 1)).tocsc(), ctx=ctx)  # a full band cannot be reordered below its width
    assert wide.path_info()["path"] == -1 and sa.lib().mispec_symshift_path(6000, 513) == _capi.MISPEC_EINVAL
    with pytest.raises(ValueError, match="only banded"):
        wide.set_shift(1.0)


# ---- 8. LOBPCG with this factorisation as its preconditioner -------------------------------------------------------------------
def test_lobpcg_preconditioner(ctx):
    A, lam = grid_laplacian()
    n, m = A.shape[0], 4
    T = sa.SparseSymShiftSolve(sp.tril(A).tocsc(), ctx=ctx)
    T.set_shift(0.0)
    assert T.path_info()["path"] == 2
    s = sa.LOBPCGSolver(sa.SparseSymMatProd(A.tocsr(), ctx=ctx), L.X0(n, m), preconditioner=T)
    nconv = s.compute(sa.SortRule.SmallestAlge, 40, L.TOL)
    print("info %s after %d iterations, norms %s" % (s.info().name, s.num_iterations(), s.residual_norms()))
    assert s.info() == sa.LOBPCGInfo.Success and nconv == m
    ev, X = s.eigenvalues(), s.eigenvectors()
    assert np.abs(np.sort(ev) - lam[:m]).max() <= 2 * L.TOL, (ev, lam[:m])
    assert np.linalg.norm(A @ X - X * ev, axis=0).max() < 2 * L.TOL and np.abs(X.T @ X - np.eye(m)).max() < 1e-10
