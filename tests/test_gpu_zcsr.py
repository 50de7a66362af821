"""The complex Hermitian sparse operator on the device (csrc/zcsr.hip, mispec_zcsr: one triangle mirrored conjugated into full int32
CSR, k_zspmv_csr) and the restart primitives of the complex factorisation over it (k_zvq in place and into a buffer, the new
residual; tests/herm_checks.py, also run on a host backend by tests/test_host_hermeigs.py).  Below the first tests, which compare with
scipy at one tolerance per matrix: k_zvq at each of its seven tile heights, and the three instantiations of k_zspmv_csr row by row
against long-double row sums with a bound counted from the kernel (an arrowhead of 10^5 entries over rows of 0 ... 18 entries;
the complex M-band at n = 10^7)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import spectra_amd as sa
from spectra_amd import workloads

import herm_checks as HC
import zfac_checks as Z
import zprim_checks as P

pytestmark = pytest.mark.gpu


def random_lower(n, density, seed, empty_rows=()):
    """Lower triangle (with a real diagonal) of a random complex Hermitian sparse matrix, and the full matrix it stands for."""
    rng = np.random.default_rng(seed)
    M = sp.random(n, n, density=density, format="coo", random_state=rng, data_rvs=lambda k: rng.uniform(-0.5, 0.5, k))
    M = M + 1j * sp.random(n, n, density=density, format="coo", random_state=rng, data_rvs=lambda k: rng.uniform(-0.5, 0.5, k))
    L = sp.tril(M, -1) + sp.diags(rng.uniform(-0.5, 0.5, n))
    L = L.tocsr()
    for r in empty_rows:
        L[r, :] = 0
        L[:, r] = 0
    L.eliminate_zeros()
    full = (L + sp.tril(L, -1).conj().T).tocsr()
    return L, full


def x_for(n, seed=3):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)


def rel_err(y, ref, full, x):
    bound = np.abs(full) @ np.abs(x)
    return np.abs(y - ref).max() / max(bound.max(), 1e-300)


@pytest.mark.parametrize("n,density", [(1, 1.0), (10, 0.5), (1001, 0.01), (4099, 0.002)])
def test_spmv_matches_scipy(ctx, n, density):
    L, full = random_lower(n, density, seed=n)
    op = sa.SparseHermMatProd(L.tocsc(), "L", ctx)
    assert op.rows() == n and op.cols() == n and op.nnz() == full.nnz
    x = x_for(n)
    assert rel_err(op.perform_op(x), full @ x, full, x) <= 1e-14


def test_spmv_bit_identical_runs_and_layouts(ctx):
    n = 3000
    L, full = random_lower(n, 0.003, seed=11)
    x = x_for(n)
    a = sa.SparseHermMatProd(L.tocsc(), "L", ctx)
    y1, y2 = a.perform_op(x), a.perform_op(x)
    assert np.array_equal(y1, y2)
    U = L.conj().T  # the same operator stored as its upper triangle
    for mat, uplo in ((L.tocsr(), "L"), (U.tocsr(), "U"), (U.tocsc(), "U")):
        assert np.array_equal(sa.SparseHermMatProd(mat, uplo, ctx).perform_op(x), y1)
    # garbage in the triangle that is not read changes nothing
    G = (L + sp.triu(sp.random(n, n, density=0.003, random_state=5), 1) * (3 + 2j)).tocsc()
    assert np.array_equal(sa.SparseHermMatProd(G, "L", ctx).perform_op(x), y1)
    # and the diagonal's imaginary part is dropped
    D = (L + sp.diags(np.full(n, 0.25j))).tocsc()
    assert np.array_equal(sa.SparseHermMatProd(D, "L", ctx).perform_op(x), y1)
    assert a(5, 5).imag == 0.0 and a(0, 1) == np.conj(a(1, 0))


def test_spmv_empty_rows_int64_indices_and_zero_matrix(ctx):
    n = 777  # not a multiple of any tile size
    L, full = random_lower(n, 0.01, seed=2, empty_rows=(0, 13, 776))
    x = x_for(n)
    y = sa.SparseHermMatProd(L.tocsc(), "L", ctx).perform_op(x)
    assert y[0] == 0 and y[13] == 0 and y[776] == 0
    assert rel_err(y, full @ x, full, x) <= 1e-14
    L64 = L.tocsc()
    L64.indptr, L64.indices = L64.indptr.astype(np.int64), L64.indices.astype(np.int64)
    assert np.array_equal(sa.SparseHermMatProd(L64, "L", ctx).perform_op(x), y)
    Zm = sp.csc_matrix((n, n), dtype=np.complex128)
    z = sa.SparseHermMatProd(Zm, "L", ctx)
    assert z.nnz() == 0 and np.array_equal(z.perform_op(x), np.zeros(n, dtype=np.complex128))


def test_spmv_rejects_bad_input(ctx):
    with pytest.raises(ValueError):
        sa.SparseHermMatProd(sp.csc_matrix((3, 4), dtype=np.complex128), "L", ctx)
    with pytest.raises(ValueError):
        sa.SparseHermMatProd(sp.identity(4, dtype=np.complex128, format="csc"), "X", ctx)


@pytest.mark.parametrize("n,m,k", [(300, 20, 8), (5000, 40, 20)])
def test_restart_primitives_on_the_device_csr_operator(ctx, n, m, k):
    L, full = random_lower(n, 8.0 / n, seed=n)
    op = sa.SparseHermMatProd(L.tocsc(), "L", ctx)
    lib = sa.lib()
    fac = C.c_void_p()
    Z.ok(lib.mispec_zfac_create_csr(ctx.h, op.h, m, 1, C.byref(fac)))
    try:
        HC.restart_checks(lib, fac, full.toarray() if n <= 300 else full, m, k)
    finally:
        lib.mispec_zfac_destroy(fac)


# ---------------------------------------------------------------------------------------------------------------------------
# k_zvq at every tile height (tests/herm_checks.py tile_height_checks)
# ---------------------------------------------------------------------------------------------------------------------------
def vq_case_rows(m):
    """n for the width m: odd primes, so no tile height R > 1 divides n and the last tile is partial.  The m-step factorisation
    in front of the check costs m^2 n / 2 column reads; from m = 2048 on n shrinks (m stays) to keep the file's run time down."""
    return 6007 if m <= 1025 else 3001 if m <= 2049 else 4099


@pytest.mark.parametrize("m", HC.VQ_WIDTHS)
def test_vq_at_every_tile_height(ctx, m):
    n = vq_case_rows(m)
    assert n >= m and all(n % R for R in (2, 4, 8, 16, 32, 64))
    L, full = random_lower(n, 8.0 / n, seed=n + m)
    op = sa.SparseHermMatProd(L.tocsc(), "L", ctx)
    lib = sa.lib()
    fac = C.c_void_p()
    Z.ok(lib.mispec_zfac_create_csr(ctx.h, op.h, m, 1, C.byref(fac)))
    try:
        HC.tile_height_checks(lib, fac, n, m, HC.hip_vq_roundings, P.hip_dot_roundings)
    finally:
        lib.mispec_zfac_destroy(fac)


# ---------------------------------------------------------------------------------------------------------------------------
# k_zspmv_csr<4 | 8 | 16> row by row
# ---------------------------------------------------------------------------------------------------------------------------
# Bound of one row of L stored entries with LPR lanes per row, per real component: a lane takes ceil(L / LPR) entries at 2 fma each
# (k_zspmv_csr: re = fma(a.x, v.x, re); re = fma(-a.y, v.y, re)), then log2(LPR) additions of the xor butterfly:
#   k = 2 ceil(L / LPR) + log2(LPR),   |y_r - ref_r| <= gamma_k * sum_e (|a.x v.x| + |a.y v.y|)   (re; |a.x v.y| + |a.y v.x| for im)
# An empty row must give exactly 0.  Sensitivity: the last stored entry of every row, left out, moves the row's reference by at
# least 100 bounds in one of its two components.
LANES = (4, 8, 16)


def row_bounds(lengths, lanes):
    k = 2 * -(-lengths // lanes) + int(np.log2(lanes))
    return P.gamma(k.astype(np.float64))


def rows_reference(full, x):
    """Row sums of the CSR matrix `full` times x in long double: (re, im), the per-component sums of absolute terms, the last
    entry's contribution, the row lengths."""
    P.assert_long_double()
    LD = P.LD
    ar, ai = P.parts(full.data)
    xr, xi = P.parts(x[full.indices])
    lengths = np.diff(full.indptr)
    rows = np.nonzero(lengths)[0]
    starts = full.indptr[:-1][rows]
    n = full.shape[0]

    def rowsum(t):
        out = np.zeros(n, dtype=LD)
        out[rows] = np.add.reduceat(t, starts)
        return out

    t1, t2, t3, t4 = ar * xr, ai * xi, ar * xi, ai * xr
    re, im = rowsum(t1 - t2), rowsum(t3 + t4)
    Tre, Tim = rowsum(np.abs(t1) + np.abs(t2)), rowsum(np.abs(t3) + np.abs(t4))
    last = full.indptr[1:][rows] - 1
    last_re, last_im = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    last_re[rows], last_im[rows] = (t1 - t2)[last], (t3 + t4)[last]
    return (re, im), (Tre, Tim), (last_re, last_im), lengths


def check_rows(op, x, ref, T, last, lengths, what):
    (re, im), (Tre, Tim), (lre, lim) = ref, T, last
    empty = lengths == 0
    ys = {}
    for lanes in LANES:
        y = op.perform_op_lanes(lanes, x)
        ys[lanes] = y
        g = row_bounds(lengths, lanes)
        er, ei = np.abs(y.real - re), np.abs(y.imag - im)
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(float(np.nanmax(er / (g * Tre))), float(np.nanmax(ei / (g * Tim))))
        print(f"{what}, {lanes} lanes per row: worst error / bound over {lengths.size} rows = {worst:.3e}")
        assert not y[empty].any()
        assert np.all(er <= g * Tre) and np.all(ei <= g * Tim), (what, lanes)
        seen = np.maximum(np.abs(lre)[~empty] / (g * Tre)[~empty], np.abs(lim)[~empty] / (g * Tim)[~empty])
        assert float(seen.min()) >= 100.0, (what, lanes, "a row's last entry would not be missed: change the data")
    assert np.array_equal(op.perform_op(x), ys[8])  # perform_op (and the solver) run the 8-lane kernel


def away_from_zero(rng, size):
    return rng.uniform(0.25, 1.0, size) * rng.choice([-1.0, 1.0], size)


def arrowhead_band(n, rng):
    """Lower triangle of: a band whose half-width w = (i // 64) % 9 changes every 64 rows, a diagonal present where i % 3 != 0, an
    arrowhead column 0 present where i % 5 != 0.  Full row lengths are 2 w + {0, 1, 2} inside a block — every length 0 ... 18 —
    and row 0 holds more than 10^5 entries.  No value is near zero."""
    i = np.arange(n)
    w = (i // 64) % 9
    rows, cols = [], []
    for d in range(1, 9):
        r = i[(w >= d) & (i - d >= 1)]
        rows.append(r)
        cols.append(r - d)
    dg = i[i % 3 != 0]
    rows.append(dg)
    cols.append(dg)
    ar = i[(i % 5 != 0) & (i > 0)]
    rows.append(ar)
    cols.append(np.zeros_like(ar))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = away_from_zero(rng, rows.size) + 1j * np.where(rows == cols, 0.0, away_from_zero(rng, rows.size))
    L = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    full = (L + sp.tril(L, -1).conj().T).tocsr()
    full.sort_indices()
    return L, full


def test_spmv_row_by_row_arrowhead_and_varying_band(ctx):
    n = 130_003
    rng = np.random.default_rng(77)
    L, full = arrowhead_band(n, rng)
    lengths = np.diff(full.indptr)
    assert set(range(18)) <= set(lengths.tolist()) and lengths.max() >= 100_000 and lengths[0] == lengths.max()
    op = sa.SparseHermMatProd(L, "L", ctx)
    assert op.nnz() == full.nnz
    x = away_from_zero(rng, n) + 1j * away_from_zero(rng, n)
    ref, T, last, lengths = rows_reference(full, x)
    check_rows(op, x, ref, T, last, lengths, f"arrowhead + band, n={n}")
    with pytest.raises(ValueError):
        op.perform_op_lanes(5, x)
    with pytest.raises(ValueError):
        op.perform_op_lanes(0, x)


def band_reference(n, x, seed=20240607, offsets=workloads.BAND_OFFSETS):
    """workloads.herm_band(n) times x as a long-double sum of shifted diagonals, from the hash that defines the matrix (not from
    the CSR arrays the library was given): the same quantities as rows_reference.  Entries are visited in the order of their
    columns (lower offsets far to near, the diagonal, upper offsets near to far) so that `last` ends as the last stored entry."""
    P.assert_long_double()
    LD = P.LD
    xr, xi = P.parts(x)
    re, im, Tre, Tim, lre, lim = (np.zeros(n, dtype=LD) for _ in range(6))
    lengths = np.zeros(n, dtype=np.int64)
    r_all = np.arange(n, dtype=np.uint64)

    def add(rows, ar, ai, src):
        """y[rows] += (ar + i ai) * x[src]"""
        vr, vi = xr[src], xi[src]
        t1, t2, t3, t4 = ar * vr, ai * vi, ar * vi, ai * vr
        re[rows] += t1 - t2
        im[rows] += t3 + t4
        Tre[rows] += np.abs(t1) + np.abs(t2)
        Tim[rows] += np.abs(t3) + np.abs(t4)
        lre[rows], lim[rows] = t1 - t2, t3 + t4
        lengths[rows] += 1

    offs = [o for o in offsets if o < n]
    for off in sorted(offs, reverse=True):   # entry (r, r - off), r >= off
        r = r_all[off:]
        c = r - np.uint64(off)
        add(slice(off, n), workloads.hash_value(seed, c, r).astype(LD), workloads.hash_value(seed + 1, c, r).astype(LD), slice(0, n - off))
    add(slice(0, n), workloads.hash_value(seed, r_all, r_all).astype(LD), np.zeros(n, dtype=LD), slice(0, n))
    for off in sorted(offs):                 # entry (r - off, r) = conj of (r, r - off)
        r = r_all[off:]
        c = r - np.uint64(off)
        add(slice(0, n - off), workloads.hash_value(seed, c, r).astype(LD), -workloads.hash_value(seed + 1, c, r).astype(LD), slice(off, n))
    return (re, im), (Tre, Tim), (lre, lim), lengths


def test_band_reference_equals_the_csr_reference():
    """The two long-double references of this file agree where both apply (CPU only; it runs with the GPU tests because the module
    needs the library's workloads)."""
    n = 5003
    L = workloads.herm_band(n, offsets=(1, 2, 3, 1000, 1001))
    full = (L + sp.tril(L, -1).conj().T).tocsr()
    full.sort_indices()
    rng = np.random.default_rng(3)
    x = away_from_zero(rng, n) + 1j * away_from_zero(rng, n)
    a = rows_reference(full, x)
    b = band_reference(n, x, offsets=(1, 2, 3, 1000, 1001))
    assert np.array_equal(a[3], b[3])
    for (p, q), (r, s) in zip(a[:3], b[:3]):
        assert np.abs(p - r).max() <= 1e-17 and np.abs(q - s).max() <= 1e-17
    assert np.array_equal(a[2][0], b[2][0]) and np.array_equal(a[2][1], b[2][1])


def test_spmv_row_by_row_band_of_ten_million_rows(ctx):
    n = 10**7
    L = workloads.herm_band(n)
    op = sa.SparseHermMatProd(L, "L", ctx)
    assert op.nnz() == 2 * L.nnz - n
    del L
    rng = np.random.default_rng(78)
    x = away_from_zero(rng, n) + 1j * away_from_zero(rng, n)
    ref, T, last, lengths = band_reference(n, x)
    assert lengths.sum() == op.nnz() and lengths.max() == 15 and lengths.min() == 8
    check_rows(op, x, ref, T, last, lengths, f"complex M-band, n={n}")
