"""The block product Y = A X on the device (mispec_spmm / launch_spmm, spectra_amd/csrc/spmm.hip): A is read once per panel of
8 / 4 / 2 columns instead of once per column.

Its contract is the arithmetic of the single product — one accumulator per (row, column) from 0.0, entries added in storage
order, every product rounded before it is added — so EVERY comparison here is np.array_equal, against
  * op.perform_op(X[:, c]) of the same operator (the SpMV in whatever format the matrix uses), and
  * oracle.Op.csr(...).perform_op (the CPU row-dot) for matrices in the caller's order.
X is uniform(-1, 1) with another seed per column: a swapped or repeated column, or a product contracted into an fma, moves bits.
The block kernel's LDS chunk holds 2032 entries (spmm.hip kSpmmCap), fewer than the stream kernel's 4080, so the n = 6000 matrix
of test_gpu_spmv.py::test_rows_longer_than_the_lds_chunk has rows that cross this kernel's chunk boundaries too."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import oracle as O
import spectra_amd as sa

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
LADDER = [1, 2, 255, 256, 257, 511, 1000, 4097]
KS = [1, 2, 3, 4, 5, 7, 8, 9, 13, 16, 17]


def block(rows, k, seed=100):
    """rows x k, column c drawn with its own seed"""
    return np.asfortranarray(np.stack([np.random.default_rng(seed + c).uniform(-1, 1, rows) for c in range(k)], axis=1))


@functools.lru_cache(maxsize=None)
def ragged(n):
    """the ragged ladder of test_gpu_spmv.py: about 8 entries per row, rows 0 and n // 2 emptied"""
    rng = np.random.default_rng(n)
    A = sp.random(n, n, density=min(1.0, 8.0 / n), random_state=n, format="csr")
    A.data[:] = rng.uniform(-1, 1, A.nnz)
    if n > 4:
        A = A.tolil()
        A[n // 2, :] = 0
        A[0, :] = 0
        A = A.tocsr()
        A.eliminate_zeros()
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def oracle_block(key, k):
    """columns 0 .. k-1 of the CPU row-dot reference of a cached matrix (computed once per matrix for the widest k asked: the
    tests slice it)"""
    A = MATRICES[key]()
    X = block(A.shape[1], k)
    op = O.Op.csr(A.shape[0], A.shape[1], A.indptr, A.indices, A.data)
    Y = np.asfortranarray(np.stack([op.perform_op(np.ascontiguousarray(X[:, c])) for c in range(k)], axis=1))
    Y.setflags(write=False)
    return Y


@functools.lru_cache(maxsize=None)
def long_rows():
    n = 6000
    rng = np.random.default_rng(7)
    rows = [np.full(n, 3), np.full(5000, 700), rng.integers(0, n, 20000)]
    cols = [np.arange(n), rng.choice(n, 5000, replace=False), rng.integers(0, n, 20000)]
    r, c = np.concatenate(rows), np.concatenate(cols)
    A = sp.coo_matrix((rng.uniform(-1, 1, len(r)), (r, c)), shape=(n, n)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def boundary():
    """n = 257 (one row past a 256-row block) with a last row that is certainly not empty"""
    A = ragged(257).tolil()
    A[256, [0, 100, 255, 256]] = [0.5, -0.25, 0.75, 0.625]
    A = A.tocsr()
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def rect(rows, cols):
    A = sp.random(rows, cols, density=0.05, random_state=rows, format="csr")
    A.data[:] = np.random.default_rng(cols).uniform(-1, 1, A.nnz)
    A.sort_indices()
    return A


MATRICES = {("ragged", n): functools.partial(ragged, n) for n in LADDER}
MATRICES["long"] = long_rows
MATRICES["boundary"] = boundary
MATRICES[("rect", 300, 500)] = functools.partial(rect, 300, 500)
MATRICES[("rect", 500, 300)] = functools.partial(rect, 500, 300)
KMAX = 17


def reference(key, k):
    return oracle_block(key, KMAX)[:, :k]


def device_spmm(op, X, k=None, ldx_pad=3, ldy_pad=5, extra_cols=2):
    """mispec_spmm through spmm_device with torch tensors for the device memory: ldx = cols + ldx_pad, ldy = rows + ldy_pad, Y
    with extra_cols more columns than k, all of Y pre-filled with a sentinel.  Returns Y[:rows, :k] after checking that every
    padding entry and every column >= k still holds the sentinel."""
    rows, cols = op.rows(), op.cols()
    k = X.shape[1] if k is None else k
    ldx, ldy = cols + ldx_pad, rows + ldy_pad
    Xh = np.full((max(k, 1), ldx), 0.125)            # row c of this array is column c of the column-major block
    Xh[:k, :cols] = X[:, :k].T
    Xd = torch.from_numpy(Xh).cuda()
    Yd = torch.full((k + extra_cols, ldy), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    op.spmm_device(Xd.data_ptr(), ldx, k, Yd.data_ptr(), ldy)
    op.ctx.sync()
    Yh = Yd.cpu().numpy()
    assert np.all(Yh[:, rows:] == SENTINEL), "padding rows of Y were written"
    assert np.all(Yh[k:, :] == SENTINEL), "columns >= k of Y were written"
    return np.asfortranarray(Yh[:k, :rows].T)


def per_column(op, X):
    return np.asfortranarray(np.stack([op.perform_op(np.ascontiguousarray(X[:, c])) for c in range(X.shape[1])], axis=1))


class spmm_option:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        sa.set_option("spmm", self.value)

    def __exit__(self, *exc):
        sa.set_option("spmm", None)


_ops = {}


def gen_op(ctx, key):
    if key not in _ops:
        _ops[key] = sa.SparseGenMatProd(MATRICES[key](), ctx=ctx)
    return _ops[key]


def check_against_both_references(ctx, key, k):
    op = gen_op(ctx, key)
    X = block(op.cols(), KMAX)[:, :k]
    Y = device_spmm(op, X)
    assert Y.shape == (op.rows(), k)
    assert np.array_equal(Y, reference(key, k))
    assert np.array_equal(Y, per_column(op, X))


@pytest.mark.parametrize("n", LADDER)
def test_ragged_ladder_at_k_5(ctx, n):
    check_against_both_references(ctx, ("ragged", n), 5)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", [257, 1000])
def test_every_k(ctx, n, k):
    check_against_both_references(ctx, ("ragged", n), k)


@pytest.mark.parametrize("value", ["auto", "0", "2", "4", "8"])
@pytest.mark.parametrize("n,k", [(257, 13), (1000, 17), (4097, 7)])
def test_each_forced_panel_width(ctx, n, k, value):
    with spmm_option(value):
        check_against_both_references(ctx, ("ragged", n), k)


@pytest.mark.parametrize("k", [3, 8])
def test_rows_longer_than_the_lds_chunk(ctx, k):
    A = long_rows()
    assert np.diff(A.indptr).max() > 2 * 2032  # rows 3 and 700 span several chunks of the block kernel
    check_against_both_references(ctx, "long", k)


@pytest.mark.parametrize("shape", [(300, 500), (500, 300)])
def test_rectangular(ctx, shape):
    check_against_both_references(ctx, ("rect",) + shape, 7)


def test_tight_and_padded_leading_dimensions(ctx):
    key = ("ragged", 1000)
    op = gen_op(ctx, key)
    X = block(1000, KMAX)[:, :6]
    ref = reference(key, 6)
    assert np.array_equal(device_spmm(op, X, ldx_pad=0, ldy_pad=0, extra_cols=0), ref)
    assert np.array_equal(device_spmm(op, X, ldx_pad=3, ldy_pad=5), ref)
    assert np.array_equal(device_spmm(op, X, ldx_pad=0, ldy_pad=5), ref)
    assert np.array_equal(device_spmm(op, X, ldx_pad=3, ldy_pad=0), ref)
    # fewer columns than the block holds: k = 4 of the 6
    assert np.array_equal(device_spmm(op, X, k=4), ref[:, :4])


def test_last_row_of_a_block_and_last_column_of_a_panel(ctx):
    # n = 257: row 256 is the only row of the second 256-row block; k = 9: column 8 is the single column after a panel of 8.
    # Neither may be zero in the reference, or a kernel that dropped them would pass.
    ref = reference("boundary", 9)
    assert ref.shape == (257, 9)
    assert np.all(ref[256, :] != 0.0) and np.count_nonzero(ref[:, 8]) > 200 and ref[256, 8] != 0.0
    assert np.all(ref[255, :] != 0.0) and np.count_nonzero(ref[:, 7]) > 200
    check_against_both_references(ctx, "boundary", 9)
    with spmm_option("4"):   # 4 + 4 + 1: column 3 and column 7 end panels
        check_against_both_references(ctx, "boundary", 9)


def test_the_spmv_format_of_the_matrix_does_not_matter(ctx):
    n, offsets = 3000, (1, 2, 50)
    op = sa.SparseSymMatProd.synth_band(n, offsets=offsets, ctx=ctx)
    assert op.spmv_format() == 2  # diagonal storage is the automatic choice
    rp, ci, v = O.synth_band_csr(n, offsets=offsets)
    X = block(n, 5, seed=40)
    cpu = O.Op.csr(n, n, rp, ci, v)
    ref = np.stack([cpu.perform_op(np.ascontiguousarray(X[:, c])) for c in range(5)], axis=1)
    for fmt in (-1, 0, 1, 2):
        op.set_spmv_format(fmt)
        assert fmt < 0 or op.spmv_format() == fmt
        Y = device_spmm(op, X)
        assert np.array_equal(Y, ref), fmt
        assert np.array_equal(Y, per_column(op, X)), fmt
    op.set_spmv_format(-1)


def scrambled(n, offsets, seed):
    """a symmetric band on the diagonals +-offsets (no main diagonal unless 0 is listed) under a random symmetric permutation"""
    rng = np.random.default_rng(seed)
    L = sp.diags([rng.uniform(-1, 1, n - o) for o in offsets], [-o for o in offsets], format="csr")
    S = (L + sp.tril(L, -1).T).tocsr()
    p = rng.permutation(n)
    B = S[p][:, p].tocsr()
    B.sort_indices()
    return B


def test_reordered_matrix_keeps_the_callers_order(ctx):
    """Two scrambled bands at k = 5, before and after op.reorder("rcm").

    Rows of at most two entries (offsets +-1): a sum of two products does not depend on their order, so Y after the
    reordering equals Y before it bit for bit, in the caller's order.  Rows of up to seven entries: the stored rows of P A P'
    are sorted by their new columns, so the summation order — of the SpMV as of the block product — is another one and Y moves
    by rounding (m = 7 products of magnitude < 1, each of the two sums within (m - 1) (eps / 2) m of the exact one, so they differ
    by m (m - 1) eps at the most); there the bit-for-bit references are the reordered
    operator's own perform_op and the CPU row-dot on the permuted CSR."""
    n, k = 1500, 5
    X = block(n, k, seed=60)
    B2 = scrambled(n, (1,), 5)
    assert np.diff(B2.indptr).max() == 2
    op = sa.SparseGenMatProd(B2, ctx=ctx, reorder="none")
    before = device_spmm(op, X)
    cpu = O.Op.csr(n, n, B2.indptr, B2.indices, B2.data)
    assert np.array_equal(before, np.stack([cpu.perform_op(np.ascontiguousarray(X[:, c])) for c in range(k)], axis=1))
    assert op.reorder("rcm") and op.reordering() == "rcm"
    perm = op.permutation()
    assert not np.array_equal(perm, np.arange(n))
    after = device_spmm(op, X)
    assert np.array_equal(after, before)
    assert np.array_equal(after, per_column(op, X))

    B7 = scrambled(n, (0, 1, 2, 40), 6)
    op = sa.SparseGenMatProd(B7, ctx=ctx, reorder="none")
    before = device_spmm(op, X)
    assert op.reorder("rcm")
    perm = op.permutation()
    after = device_spmm(op, X)
    assert np.array_equal(after, per_column(op, X))
    Bp = B7[perm][:, perm].tocsr()
    Bp.sort_indices()
    cpu = O.Op.csr(n, n, Bp.indptr, Bp.indices, Bp.data)
    for c in range(k):
        assert np.array_equal(after[perm, c], cpu.perform_op(np.ascontiguousarray(X[perm, c])))
    assert np.abs(after - before).max() <= 7 * 6 * np.finfo(float).eps
    with spmm_option("0"):
        assert np.array_equal(device_spmm(op, X), after)


def test_matmul_runs_in_slabs_of_32_columns(ctx):
    key = ("ragged", 1000)
    op = gen_op(ctx, key)
    A = MATRICES[key]()
    X = block(1000, 40, seed=7)
    Y = op @ X
    assert Y.shape == (1000, 40)
    assert np.array_equal(Y, per_column(op, X))
    cpu = O.Op.csr(1000, 1000, A.indptr, A.indices, A.data)
    for c in (0, 31, 32, 39):
        assert np.array_equal(Y[:, c], cpu.perform_op(np.ascontiguousarray(X[:, c])))
    # a leading dimension of the host block that is larger than the row count (a view of a taller array)
    tall = np.asfortranarray(np.random.default_rng(3).uniform(-1, 1, (1007, 40)))
    assert np.array_equal(op @ tall[:1000, :], per_column(op, np.asfortranarray(tall[:1000, :])))
    empty = op @ np.empty((1000, 0))
    assert empty.shape == (1000, 0)


def test_refusals_name_the_entry_point(ctx):
    op = gen_op(ctx, ("rect", 300, 500))
    Xd = torch.zeros((4, 510), dtype=torch.float64, device="cuda")
    Yd = torch.zeros((4, 310), dtype=torch.float64, device="cuda")
    x, y = Xd.data_ptr(), Yd.data_ptr()
    for args in [(0, 510, 4, y, 310), (x, 510, 4, 0, 310), (x, 510, -1, y, 310), (x, 499, 4, y, 310), (x, 510, 4, y, 299)]:
        with pytest.raises(ValueError, match="mispec_spmm"):
            op.spmm_device(*args)
        with pytest.raises(ValueError, match="mispec_spmm"):
            op.spmm_time(*args, 1)
    op.spmm_device(x, 510, 0, y, 310)  # k = 0: nothing to do, no launch
    op.spmm_device(x, 500, 4, y, 300)  # the smallest leading dimensions
    op.ctx.sync()
    assert op.spmm_time(x, 510, 4, y, 310, 2) > 0.0


@pytest.mark.parametrize("key,k", [(("ragged", 4097), 17), ("long", 13), (("rect", 500, 300), 16)])
def test_option_0_and_auto_give_equal_bits(ctx, key, k):
    # spmm=0 is one launch_spmv per column, the path every block product took before: this ties the block kernel to it
    op = gen_op(ctx, key)
    X = block(op.cols(), k, seed=11)
    with spmm_option("0"):
        assert sa.spmm_plan(k) == [1] * k
        old = device_spmm(op, X)
    with spmm_option("auto"):
        assert max(sa.spmm_plan(k)) > 1
        new = device_spmm(op, X)
    assert np.array_equal(old, new)
    assert np.array_equal(old, per_column(op, X))
