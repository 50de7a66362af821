"""Block shift solve (mispec_symshift_solve_block): every column of the result has exactly the bits of mispec_symshift_solve on that
column alone — on the panel kernels of the narrow-band levels (sweeps and explicit chunk inverses, separator right-hand sides, back
substitution), the dense inverses, and on every path that loops over the columns — under every value of option `shift_block`."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

import shift_block_checks as SB
import spectra_amd as sa
from spectra_amd import _capi

pytestmark = [pytest.mark.gpu, pytest.mark.operator_only]

SENTINEL = -123.5
KMAX = max(SB.COLUMN_COUNTS)


def bits(t):
    return t.contiguous().view(torch.int64)


def check_device_block(op, n, lds=None, options=("4", "2", "0", None)):
    """Block solves of k = 1 ... 21 columns against single solves on the same pointers, compared bit for bit on the device; rows
    beyond n and columns beyond k of Y keep their sentinel.  Returns the first five columns of the result (host, n x 5)."""
    first = None
    for ld in lds or (n, n + 3):
        Xd = torch.from_numpy(np.ascontiguousarray(SB.rhs_block(n, KMAX, ld).T)).cuda()  # (KMAX, ld) row-major = ld x KMAX column-major
        single = torch.empty((KMAX, n), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for c in range(KMAX):
            op.solve_device(Xd.data_ptr() + 8 * c * ld, single.data_ptr() + 8 * c * n)
        try:
            for opt in options:
                sa.set_option("shift_block", opt)
                for k in (SB.COLUMN_COUNTS if opt in ("4", "2") else (5, KMAX)):
                    Yd = torch.full((KMAX, ld), SENTINEL, dtype=torch.float64, device="cuda")
                    torch.cuda.synchronize()
                    op.solve_block_device(Xd.data_ptr(), ld, k, Yd.data_ptr(), ld)
                    torch.cuda.synchronize()
                    same = (bits(Yd[:k, :n]) == bits(single[:k])).all(dim=1).cpu().numpy()
                    assert same.all(), ("columns that differ from the single solve", n, ld, opt, k, np.nonzero(~same)[0])
                    assert bool((Yd[k:] == SENTINEL).all()) and bool((Yd[:, n:] == SENTINEL).all()), (n, ld, opt, k)
        finally:
            sa.set_option("shift_block", None)
        if first is None:
            first = single[:5].cpu().numpy().T
    return first


def check_against_splu(A, sigma, n, Y, B=None, X=None):
    """the bars of test_banded_solve_matches_sparse_lu, per column; X: the right-hand sides of Y (default: check_device_block's)"""
    M = (A - sigma * (sp.identity(n) if B is None else B)).tocsc()
    X = SB.rhs_block(n, KMAX)[:n, :5] if X is None else X
    ref = spla.splu(M).solve(X)
    for c in range(5):
        assert np.abs(Y[:, c] - ref[:, c]).max() <= 1e-12 * max(1.0, np.abs(ref[:, c]).max()), c
        assert np.linalg.norm(M @ Y[:, c] - X[:, c]) <= 1e-12 * np.linalg.norm(X[:, c]), c


@pytest.mark.parametrize("mode", ["sweeps", "chunk_inverses"])
@pytest.mark.parametrize("n,b", SB.NARROW_SHAPES + SB.DEEP_SHAPES)
def test_narrow_band_levels(ctx, n, b, mode):
    A = SB.banded_spd(n, b, seed=n)
    op = sa.SparseSymShiftSolve(sp.tril(A).tocsc(), ctx=ctx)
    try:
        if mode == "sweeps":
            sa.set_option("shift", "block_inverse=0")  # read when the levels are factored
        op.set_shift(-1.5)
    finally:
        sa.set_option("shift", None)
    Y = check_device_block(op, n)
    check_against_splu(A, -1.5, n, Y)


@pytest.mark.parametrize("n,b", [(50, 16), (51, 16), (1500, 3), (3000, 16), (6000, 16)])
def test_dense_inverse_and_wide_top_level(ctx, n, b):
    # n <= 4096 with a band wider than 8 (an odd n: the kernel without 16-byte loads) and a narrow band of one chunk: the dense inverse (ld = n + 3 mixes 16- and 8-byte aligned columns: single products
    # there); n = 6000: a wide top level, the column loop
    A = SB.banded_spd(n, b, seed=n)
    op = sa.SparseSymShiftSolve(sp.tril(A).tocsc(), ctx=ctx)
    op.set_shift(0.0)
    Y = check_device_block(op, n, lds=(n, n + 3, n + 4))
    check_against_splu(A, 0.0, n, Y)


def check_host_block(op, n, k=5):
    X = SB.rhs_block(n, k)
    for opt in ("4", "2", "0", None):
        try:
            sa.set_option("shift_block", opt)
            Y = op.perform_op_block(X)
        finally:
            sa.set_option("shift_block", None)
        assert Y.flags.f_contiguous and Y.shape == (n, k)
        for c in range(k):
            assert np.array_equal(Y[:, c], op.perform_op(X[:, c])), (opt, c)
    return X, Y


def test_pencil(ctx):
    n = 20_000
    A = SB.banded_spd(n, 3, seed=5)
    B = sp.diags([np.full(n - 1, 0.3), np.full(n, 2.0), np.full(n - 1, 0.3)], [-1, 0, 1], format="csc")
    op = sa.SymShiftInvert(sp.tril(A).tocsc(), sp.tril(B).tocsc(), ctx=ctx)
    op.set_shift(-0.7)
    X, Y = check_host_block(op, n)
    check_against_splu(A, -0.7, n, Y, B=B, X=X)


def test_reordered_band(ctx):
    n = 50_000
    q = np.random.default_rng(11).permutation(n)
    A = SB.banded_spd(n, 3, seed=7)[q][:, q].tocsc()
    op = sa.SparseSymShiftSolve(sp.tril(A).tocsc(), ctx=ctx)
    assert op.bandwidth_info()["reordered"]
    op.set_shift(-1.0)
    Y = check_device_block(op, n)
    check_host_block(op, n)
    X = SB.rhs_block(n, KMAX)[:, :5]
    M = (A + sp.identity(n)).tocsc()
    for c in range(5):
        assert np.linalg.norm(M @ Y[:, c] - X[:, c]) <= 1e-12 * np.linalg.norm(X[:, c])


def test_indefinite_shifts_refine_every_column(ctx):
    # the matrices of test_banded_solve_with_interior_shift_matches_sparse_lu: every column gets the calibrated number of steps
    steps = []
    for n, b, sigma in [(3000, 2, 0.3), (5000, 3, 1.0), (100_000, 3, 0.1234)]:
        A = SB.banded_indefinite(n, b, seed=n + b)
        op = sa.SparseSymShiftSolve(sp.tril(A).tocsc(), ctx=ctx)
        op.set_shift(sigma)
        steps.append(op.refinement_info()["refine_steps"])
        check_device_block(op, n)
    print("refinement steps:", steps)
    assert max(steps) > 0, steps


def test_general_operator(ctx):
    n = 100
    rng = np.random.default_rng(3)
    G = (sp.random(n, n, 0.1, random_state=rng, format="csc") + sp.diags(rng.uniform(3.0, 4.0, n))).tocsc()
    op = sa.SparseGenRealShiftSolve(G, ctx=ctx)
    op.set_shift(0.5)
    X, Y = check_host_block(op, n)
    assert np.abs((G - 0.5 * sp.identity(n)) @ Y - X).max() <= 1e-12


def test_argument_errors(ctx):
    n = 3000
    op = sa.SparseSymShiftSolve(sp.tril(SB.banded_spd(n, 2)).tocsc(), ctx=ctx)
    lib = sa.lib()
    Xd = torch.zeros((4, n + 2), dtype=torch.float64, device="cuda")
    Yd = torch.zeros((4, n + 2), dtype=torch.float64, device="cuda")
    x, y = C.c_void_p(Xd.data_ptr()), C.c_void_p(Yd.data_ptr())
    assert lib.mispec_symshift_solve_block(op.h, x, n, 2, y, n) == _capi.MISPEC_ELOGIC  # before set_shift, as the single solve
    ms = C.c_float(0)
    assert lib.mispec_symshift_solve_block_time(op.h, x, n, 2, y, n, 1, C.byref(ms)) == _capi.MISPEC_ELOGIC
    with pytest.raises(AssertionError):
        op.perform_op_block(np.zeros((n, 2)))
    op.set_shift(-1.0)
    assert lib.mispec_symshift_solve_block(op.h, x, n + 2, 4, y, n + 2) == _capi.MISPEC_OK
    assert lib.mispec_symshift_solve_block(op.h, None, n, 2, y, n) == _capi.MISPEC_EINVAL
    assert lib.mispec_symshift_solve_block(op.h, x, n, 2, None, n) == _capi.MISPEC_EINVAL
    assert lib.mispec_symshift_solve_block(op.h, x, n, 0, y, n) == _capi.MISPEC_EINVAL
    assert lib.mispec_symshift_solve_block(op.h, x, n - 1, 2, y, n) == _capi.MISPEC_EINVAL
    assert lib.mispec_symshift_solve_block(op.h, x, n, 2, y, n - 1) == _capi.MISPEC_EINVAL
    assert lib.mispec_symshift_solve_block_time(op.h, x, n, 2, y, n, 0, C.byref(ms)) == _capi.MISPEC_EINVAL
    assert lib.mispec_symshift_solve_block_time(op.h, x, n, 2, y, n, 2, C.byref(ms)) == _capi.MISPEC_OK and ms.value > 0
    with pytest.raises(ValueError):
        op.perform_op_block(np.zeros((n + 1, 2)))
    with pytest.raises(ValueError):
        op.perform_op_block(np.zeros((n, 0)))
    torch.cuda.synchronize()
