"""Ingest from device memory (spectra_amd/csrc/ingest_dev.hip): operators built from torch sparse tensors on the GPU must be the
operators the host path builds from the same arrays — the mirrored matrix byte for byte, every format decision, every product and
a whole solve bit for bit.  The yardstick is always the host path (mispec_mirror_triangle_host, the scipy constructors)."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import spectra_amd as sa
from spectra_amd import _capi

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:Sparse CS[RC] tensor support is in beta")]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- matrices: raw compressed arrays (outer, inner, val); the same arrays are read as CSR or as CSC -----------------------------
def raw_of(M):
    M = M.tocsr()
    M.sort_indices()
    return M.shape[0], M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data.astype(np.float64)


def band(n, offsets, seed):
    """Entries on +-offsets (and the diagonal when 0 is among them), different values in the two triangles."""
    rng = np.random.default_rng(seed)
    diags, offs = [], []
    for o in sorted(set(offsets) | {-k for k in offsets}):
        offs.append(o)
        diags.append(rng.uniform(-1.0, 1.0, n - abs(o)))
    return sp.diags(diags, offs, shape=(n, n), format="csr")


@functools.lru_cache(maxsize=None)
def matrix(name):
    rng = np.random.default_rng(11)
    if name == "one":
        return 1, np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int64), np.array([2.5])
    if name == "empty5":
        return 5, np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0)
    if name == "tridiag257":
        return raw_of(band(257, (0, 1), 1))
    if name == "band70000":  # crosses the host routine's 32768-row bucket and 65536
        return raw_of(band(70000, (0, 1, 2, 300, 40000), 2))
    if name in ("arrow70000", "arrow1100000"):  # a full first row and column: one mirrored row of n entries
        n = int(name[5:])
        r = np.concatenate([np.arange(n), np.zeros(n - 1, dtype=np.int64), np.arange(1, n)])
        c = np.concatenate([np.arange(n), np.arange(1, n), np.zeros(n - 1, dtype=np.int64)])
        return raw_of(sp.coo_matrix((rng.uniform(-1.0, 1.0, r.size), (r, c)), shape=(n, n)))
    if name == "special":  # -0.0, a NaN with a payload, a denormal, an infinity
        v = np.array([0x8000000000000000, 0x7FF8DEAD00000001, 0x0000000000000001, 0x3FF0000000000000, 0xFFF0000000000000,
                      0x7FF0000000000000, 0x800000000000000F], dtype=np.uint64).view(np.float64)
        outer = np.array([0, 2, 3, 5, 7], dtype=np.int64)
        inner = np.array([0, 2, 1, 0, 3, 2, 3], dtype=np.int64)
        return 4, outer, inner, v
    if name == "random1000":  # NOT canonical: shuffled inner indices, ~5 % duplicated positions, both triangles, empty outers
        n = 1000
        M = sp.random(n, n, density=0.01, format="csr", random_state=5)
        outer, inner, val = [0], [], []
        for i in range(n):
            cols = M.indices[M.indptr[i]:M.indptr[i + 1]]
            if i % 37 == 0:
                cols = cols[:0]
            dup = cols[rng.random(cols.size) < 0.05]
            cols = np.concatenate([cols, dup, dup[:1]])
            rng.shuffle(cols)
            inner.extend(cols.tolist())
            val.extend(rng.uniform(-1.0, 1.0, cols.size).tolist())
            outer.append(len(inner))
        return n, np.array(outer, dtype=np.int64), np.array(inner, dtype=np.int64), np.array(val)
    raise KeyError(name)


MIRROR_MATRICES = ["one", "empty5", "tridiag257", "random1000", "band70000", "arrow70000", "special"]


def host_mirror(name, uplo, row_major):
    """mispec_mirror_triangle_host on the raw arrays (sa.mirror_triangle_host would canonicalise a scipy matrix first)."""
    return _host_mirror(name, uplo, bool(row_major))


@functools.lru_cache(maxsize=None)
def _host_mirror(name, uplo, row_major):
    n, outer, inner, val = matrix(name)
    o32, i32 = outer.astype(np.int32), inner.astype(np.int32)
    cap = 2 * val.size + 1
    rp, ci, v = np.zeros(n + 1, dtype=np.int32), np.zeros(cap, dtype=np.int32), np.zeros(cap)
    nnz = C.c_int64(0)
    _capi.check(sa.lib().mispec_mirror_triangle_host(n, sa._ip(o32), sa._ip(i32), sa._dp(val), uplo.encode(), int(row_major), sa._ip(rp),
                                                     sa._ip(ci), sa._dp(v), cap, C.byref(nnz)))
    return rp, ci[:nnz.value].copy(), v[:nnz.value].copy()


def torch_compressed(n_rows, n_cols, outer, inner, val, row_major, idx):
    import torch

    dt = {32: torch.int32, 64: torch.int64}[idx]
    o = torch.from_numpy(np.ascontiguousarray(outer)).to(device="cuda", dtype=dt)
    i = torch.from_numpy(np.ascontiguousarray(inner)).to(device="cuda", dtype=dt)
    v = torch.from_numpy(np.ascontiguousarray(val)).cuda()
    make = torch.sparse_csr_tensor if row_major else torch.sparse_csc_tensor
    return make(o, i, v, size=(n_rows, n_cols), check_invariants=False)


# ---- the mirror against mispec_mirror_triangle_host ----------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [32, 64])
@pytest.mark.parametrize("layout", ["csr", "csc"])
@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("name", MIRROR_MATRICES)
def test_mirror_equals_the_host_routine_byte_for_byte(ctx, name, uplo, layout, idx):
    n, outer, inner, val = matrix(name)
    row_major = layout == "csr"
    rp, ci, v = host_mirror(name, uplo, row_major)
    t = torch_compressed(n, n, outer, inner, val, row_major, idx)
    drp, dci, dv = sa.mirror_triangle_device(t, uplo, ctx=ctx)
    assert drp.dtype == np.int32 and dci.dtype == np.int32 and dv.dtype == np.float64
    assert np.array_equal(drp, rp)
    assert np.array_equal(dci, ci)
    assert np.array_equal(bits(dv), bits(v))
    if name == "arrow70000":
        assert np.diff(rp).max() == 70000
    if name == "random1000":  # the input really is what the case is about
        assert any(np.any(np.diff(inner[outer[i]:outer[i + 1]]) < 0) for i in range(n)) and np.any(np.diff(rp) == 0)
        assert any(np.unique(inner[outer[i]:outer[i + 1]]).size < outer[i + 1] - outer[i] for i in range(n))


@pytest.mark.parametrize("uplo,layout,idx", [("L", "csc", 64), ("U", "csr", 32), ("L", "csr", 32)])
def test_a_row_beyond_the_device_ranking_limit_is_mirrored_by_the_host_routine(ctx, uplo, layout, idx):
    # one row of 1 100 000 entries, more than kLongRow = 2^20 of ingest_dev.hip: found after the scan, handed to the host routine
    name, n = "arrow1100000", 1100000
    _, outer, inner, val = matrix(name)
    rp, ci, v = host_mirror(name, uplo, layout == "csr")
    assert np.diff(rp).max() == n > 2 ** 20
    t = torch_compressed(n, n, outer, inner, val, layout == "csr", idx)
    drp, dci, dv = sa.mirror_triangle_device(t, uplo, ctx=ctx)
    assert np.array_equal(drp, rp) and np.array_equal(dci, ci) and np.array_equal(bits(dv), bits(v))
    if layout == "csc":  # whole operators once: the symmetric one, and the general transpose (row 0 of the matrix holds n entries)
        M = sp.csc_matrix((val, inner, outer), shape=(n, n))
        dev, host = sa.SparseSymMatProd.from_torch(t, uplo=uplo, ctx=ctx, reorder="none"), sa.SparseSymMatProd(M, uplo=uplo, ctx=ctx, reorder="none")
        same_products(dev, host)
        assert dev.reordering_info() == host.reordering_info() and dev.tiles_info() == host.tiles_info()
        same_products(sa.SparseGenMatProd.from_torch(t, ctx=ctx, reorder="none"), sa.SparseGenMatProd(M, ctx=ctx, reorder="none"))


# ---- whole operators: from_torch against the scipy constructor -----------------------------------------------------------------
SCALED_HEADLINE = (1, 2, 3, 30, 31, 300, 301)  # the 15-entry M-band offsets scaled to n = 3000: diagonal storage, dia_sym


@functools.lru_cache(maxsize=None)
def canonical(name):
    if name == "band3000":
        return band(3000, (0,) + SCALED_HEADLINE, 3)
    if name == "rect300x500":
        M = sp.random(300, 500, density=0.03, format="csr", random_state=9)
        M.sort_indices()
        return M
    n, outer, inner, val = matrix(name)
    M = sp.csr_matrix((val, inner, outer), shape=(n, n))
    M.sum_duplicates()
    M.sort_indices()
    return M


def windows_table(op):
    try:
        return op.windows_table()
    except ValueError:
        return None


def assert_same_operator(dev, host, seed=3):
    for a, b in zip(dev.to_host_csr(), host.to_host_csr()):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                                     b.view(np.uint64) if b.dtype == np.float64 else b)
    assert dev.rows() == host.rows() and dev.cols() == host.cols() and dev.nnz() == host.nnz()
    assert dev.spmv_format() == host.spmv_format()
    assert dev.offset_codes() == host.offset_codes()
    assert dev.dia_info() == host.dia_info()
    assert dev.windows_info() == host.windows_info()
    wd, wh = windows_table(dev), windows_table(host)
    assert (wd is None) == (wh is None) and (wd is None or np.array_equal(wd, wh))
    assert dev.reordering_info() == host.reordering_info()
    assert dev.staged_info() == host.staged_info() and dev.tiles_info() == host.tiles_info()
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, host.cols())
    X = rng.uniform(-1.0, 1.0, (host.cols(), 5))
    for fmt in (-1, 0, 1, 2):
        dev.set_spmv_format(fmt)
        host.set_spmv_format(fmt)
        assert dev.spmv_format() == host.spmv_format(), fmt
        assert np.array_equal(bits(dev.perform_op(x)), bits(host.perform_op(x))), fmt
    dev.set_spmv_format(-1)
    host.set_spmv_format(-1)
    assert np.array_equal(bits(dev @ X), bits(host @ X))


def as_layout(M, layout):
    M = M.tocsr() if layout == "csr" else M.tocsc()
    M.sort_indices()
    return M


def torch_of(M, idx):
    return torch_compressed(M.shape[0], M.shape[1], M.indptr, M.indices, M.data, M.format == "csr", idx)


@pytest.mark.parametrize("layout,idx", [("csr", 64), ("csc", 32)])
@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("name", ["band70000", "random1000", "band3000"])
def test_symmetric_operator_equals_the_host_built_one(ctx, name, uplo, layout, idx):
    M = as_layout(canonical(name), layout)
    host = sa.SparseSymMatProd(M, uplo=uplo, ctx=ctx)
    dev = sa.SparseSymMatProd.from_torch(torch_of(M, idx), uplo=uplo, ctx=ctx)
    assert_same_operator(dev, host)
    if name == "band3000":  # the formats the case is about
        assert host.spmv_format() == 2 and host.dia_info()["nmirrored"] > 0
    if name == "random1000":
        assert host.offset_codes() == 0


@pytest.mark.parametrize("layout,idx", [("csr", 32), ("csc", 64)])
@pytest.mark.parametrize("name", ["band70000", "random1000", "band3000", "rect300x500"])
def test_general_operator_equals_the_host_built_one(ctx, name, layout, idx):
    M = as_layout(canonical(name), layout)
    host = sa.SparseGenMatProd(M, ctx=ctx)
    dev = sa.SparseGenMatProd.from_torch(torch_of(M, idx), ctx=ctx)
    assert_same_operator(dev, host)


def raw_general_on_host(ctx, n, outer, inner, val, row_major):
    """mispec_csr_upload / mispec_csr_from_csc on raw arrays (the scipy constructor would canonicalise them first)."""
    o32, i32, h = outer.astype(np.int32), inner.astype(np.int32), C.c_void_p()
    fn = sa.lib().mispec_csr_upload if row_major else sa.lib().mispec_csr_from_csc
    _capi.check(fn(ctx.h, n, n, sa._ip(o32), sa._ip(i32), sa._dp(val), C.byref(h)))
    op = sa.SparseGenMatProd.__new__(sa.SparseGenMatProd)
    sa._DeviceMatrix.__init__(op, ctx, h)
    return op


@pytest.mark.parametrize("layout,idx", [("csr", 64), ("csr", 32), ("csc", 64), ("csc", 32)])
def test_general_operator_from_arrays_that_are_not_canonical(ctx, layout, idx):
    # unsorted inner indices and duplicates: CSR is taken as it is (no sorting, no merging), CSC comes out in column order and
    # stable within equal columns — whatever mispec_csr_upload / mispec_csr_from_csc make of the same arrays
    n, outer, inner, val = matrix("random1000")
    host = raw_general_on_host(ctx, n, outer, inner, val, layout == "csr")
    dev = sa.SparseGenMatProd.from_torch(torch_compressed(n, n, outer, inner, val, layout == "csr", idx), ctx=ctx)
    assert_same_operator(dev, host)
    rp, ci, v = host.to_host_csr()
    assert v.size == val.size  # duplicates are kept
    if layout == "csr":
        assert np.array_equal(ci, inner) and np.array_equal(bits(v), bits(val))
    else:
        assert all(np.all(np.diff(ci[rp[i]:rp[i + 1]]) >= 0) for i in range(n))


@pytest.mark.parametrize("offsets,downloads", [((0, 1, 2, 3, 4, 5, 140000), False), ((0, 1, 140000, 150000), True)])
def test_the_far_statistic_and_the_automatic_host_branch(ctx, offsets, downloads):
    # n >= 2 kFarWindow = 262144 with entries further than kFarWindow from the diagonal: a non-zero far count, and with more
    # than a quarter of them the branch that downloads on its own (reordering attempt, staged image), no option set
    n = 300000
    M = as_layout(sp.tril(band(n, offsets, 12)), "csc")
    host = sa.SparseSymMatProd(M, ctx=ctx)
    dev = sa.SparseSymMatProd.from_torch(torch_of(M, 64), ctx=ctx)
    info = host.reordering_info()
    far_entries = sum(2 * (n - k) for k in offsets if k > 131072)
    assert info["far_fraction_before"] == far_entries / host.nnz() and (info["far_fraction_before"] > 0.25) == downloads
    assert dev.reordering_info() == info
    assert dev.staged_info() == host.staged_info() and dev.tiles_info() == host.tiles_info()
    assert (host.staged_info()["bins"] > 0 or host.tiles_info()["segments"] > 0 or host.reordering() == "rcm") == downloads
    assert np.array_equal(dev.permutation(), host.permutation())
    assert dev.dia_info() == host.dia_info() and dev.offset_codes() == host.offset_codes() and dev.windows_info() == host.windows_info()
    same_products(dev, host)


def test_stage_timers_are_filled_and_reset(ctx):
    M = as_layout(canonical("band70000"), "csc")
    sa.SparseSymMatProd.from_torch(torch_of(M, 64), ctx=ctx)
    t = sa.last_ingest_info()
    assert t["mirror_triangle"] > 0 and t["index_formats_and_h2d"] > 0 and t["validate"] == 0
    assert t["total"] >= t["mirror_triangle"] + t["index_formats_and_h2d"]
    assert t["tiles_build"] == 0 and t["staged_build"] == 0 and t["far_statistics_and_reordering"] == 0
    sa.SparseGenMatProd.from_torch(torch_of(as_layout(M, "csr"), 32), ctx=ctx)
    t = sa.last_ingest_info()
    assert t["mirror_triangle"] == 0 and t["validate"] > 0 and t["index_formats_and_h2d"] > 0 and t["total"] >= t["validate"]


def test_float32_values_are_widened(ctx):
    M = as_layout(canonical("band3000"), "csc")
    M32 = M.astype(np.float32)
    host = sa.SparseSymMatProd(M32.astype(np.float64), ctx=ctx)
    import torch

    t = torch.sparse_csc_tensor(torch.from_numpy(M32.indptr).cuda(), torch.from_numpy(M32.indices).cuda(), torch.from_numpy(M32.data).cuda(),
                                size=M32.shape)
    assert t.values().dtype == torch.float32
    assert_same_operator(sa.SparseSymMatProd.from_torch(t, ctx=ctx), host)


# ---- the branch that downloads: structures built by host code ------------------------------------------------------------------
def with_option(name, value, make):
    sa.set_option(name, value)
    try:
        return make()
    finally:
        sa.set_option(name, None)


def same_products(dev, host, seed=4):
    rng = np.random.default_rng(seed)
    x, X = rng.uniform(-1.0, 1.0, host.cols()), rng.uniform(-1.0, 1.0, (host.cols(), 5))
    assert dev.spmv_format() == host.spmv_format()
    assert np.array_equal(bits(dev.perform_op(x)), bits(host.perform_op(x)))
    assert np.array_equal(bits(dev @ X), bits(host @ X))
    for a, b in zip(dev.to_host_csr(), host.to_host_csr()):
        assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b)


def test_forced_reordering_takes_the_host_path(ctx):
    M = as_layout(canonical("random1000"), "csc")
    host = sa.SparseSymMatProd(M, ctx=ctx, reorder="rcm")
    dev = sa.SparseSymMatProd.from_torch(torch_of(M, 64), ctx=ctx, reorder="rcm")
    assert host.reordering() == "rcm" and dev.reordering() == "rcm"
    assert np.array_equal(dev.permutation(), host.permutation()) and not np.array_equal(host.permutation(), np.arange(1000))
    assert dev.reordering_info() == host.reordering_info()
    same_products(dev, host)


@pytest.mark.parametrize("option,info", [("spmv_staged", "staged_info"), ("spmv_tiles", "tiles_info")])
def test_forced_scatter_formats_take_the_host_path(ctx, option, info):
    M = as_layout(canonical("random1000"), "csr")
    host = with_option(option, "1", lambda: sa.SparseGenMatProd(M, ctx=ctx))
    dev = with_option(option, "1", lambda: sa.SparseGenMatProd.from_torch(torch_of(M, 32), ctx=ctx))
    assert getattr(dev, info)() == getattr(host, info)()
    assert list(getattr(host, info)().values())[0] > 0 and host.spmv_format() in (3, 4)
    same_products(dev, host)
    hs = with_option(option, "1", lambda: sa.SparseSymMatProd(M.tocsc(), ctx=ctx))
    ds = with_option(option, "1", lambda: sa.SparseSymMatProd.from_torch(torch_of(M.tocsc(), 64), ctx=ctx))
    assert getattr(ds, info)() == getattr(hs, info)() and list(getattr(hs, info)().values())[0] > 0
    same_products(ds, hs)


# ---- one solve ------------------------------------------------------------------------------------------------------------------
def test_a_solve_is_the_same_bit_for_bit(ctx):
    M = as_layout(canonical("band3000"), "csc")
    runs = []
    for op in (sa.SparseSymMatProd(M, ctx=ctx), sa.SparseSymMatProd.from_torch(torch_of(M, 64), ctx=ctx)):
        eigs = sa.SymEigsSolver(op, 4, 12)
        eigs.init()
        nconv = eigs.compute(sa.SortRule.LargestMagn)
        assert eigs.info() == sa.CompInfo.Successful
        runs.append((nconv, eigs.num_iterations(), eigs.num_operations(), bits(eigs.eigenvalues()).tolist()))
    assert runs[0][0] == 4
    assert runs[0] == runs[1]


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def tri_arrays(idx_dtype):
    """The lower triangle (CSC) of a 300-row band as torch DEVICE tensors (outer, inner, values) plus the scipy matrix."""
    import torch

    M = sp.tril(band(300, (0, 1, 7), 6)).tocsc()
    M.sort_indices()
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dt)
    return M, dev(M.indptr, idx_dtype), dev(M.indices, idx_dtype), dev(M.data, torch.float64)


def from_pointers(ctx, n, outer, inner, val, index_bytes=None):
    import torch

    torch.cuda.synchronize()
    return sa.SparseSymMatProd.from_device_pointers(n, outer.data_ptr(), inner.data_ptr(), index_bytes or outer.element_size(),
                                                    val.data_ptr(), False, uplo="L", ctx=ctx)


def assert_a_valid_ingest_follows(ctx):
    import torch

    M, outer, inner, val = tri_arrays(torch.int64)
    dev, host = from_pointers(ctx, 300, outer, inner, val), sa.SparseSymMatProd(M, ctx=ctx)
    x = np.random.default_rng(8).uniform(-1.0, 1.0, 300)
    assert np.array_equal(bits(dev.perform_op(x)), bits(host.perform_op(x)))


@pytest.mark.parametrize("case", ["inner -1", "inner n", "int64 2^31", "decreasing outer", "index_bytes 2"])
def test_bad_arrays_are_refused_with_the_host_message(ctx, case):
    import torch

    M, outer, inner, val = tri_arrays(torch.int64 if case == "int64 2^31" else torch.int32)
    index_bytes, message = None, "index out of range"
    if case == "inner -1":
        inner[5] = -1
    elif case == "inner n":
        inner[inner.numel() - 1] = 300
    elif case == "int64 2^31":
        inner[17] = 2 ** 31
    elif case == "decreasing outer":
        outer[100] = outer[99] - 1
        message = "row pointers must be non-decreasing"
    else:
        index_bytes, message = 2, "index_bytes must be 4"
    with pytest.raises(ValueError, match=message):
        from_pointers(ctx, 300, outer, inner, val, index_bytes)
    if case in ("inner -1", "inner n"):  # the host path's message for the same arrays
        with pytest.raises(ValueError, match=message):
            _capi.check(sa.lib().mispec_csr_from_triangle(ctx.h, 300, sa._ip(outer.cpu().numpy()), sa._ip(inner.cpu().numpy()),
                                                          sa._dp(val.cpu().numpy()), b"L", 0, C.byref(C.c_void_p())))
    assert_a_valid_ingest_follows(ctx)


def test_general_arrays_are_checked_too(ctx):
    import torch

    M = canonical("rect300x500")
    for layout, message in (("csr", "column index out of range"), ("csc", "row index out of range")):
        A = as_layout(M, layout)
        t = torch_of(A, 64)
        inner = t.col_indices() if layout == "csr" else t.row_indices()
        inner[3] = 500 if layout == "csr" else 300
        with pytest.raises(ValueError, match=message):
            sa.SparseGenMatProd.from_torch(t, ctx=ctx)
    assert_a_valid_ingest_follows(ctx)


def test_a_sharded_context_is_refused(ctx):
    import torch

    M, outer, inner, val = tri_arrays(torch.int32)
    lib = sa.lib()
    grp = C.c_void_p()
    _capi.check(lib.mispec_loopback_create(2, C.byref(grp)))
    try:
        sctx = sa.Context(0)
        _capi.check(lib.mispec_loopback_attach(grp, sctx.h, 0))
        sctx.rank, sctx.world = 0, 2
        with pytest.raises(ValueError, match="sharded context"):
            from_pointers(sctx, 300, outer, inner, val)
        t = torch.sparse_csc_tensor(outer, inner, val, size=(300, 300))
        with pytest.raises(ValueError, match="sharded context"):
            sa.SparseGenMatProd.from_torch(t, ctx=sctx)
        with pytest.raises(ValueError, match="sharded context"):
            sa.mirror_triangle_device(t, "L", ctx=sctx)
        del sctx
    finally:
        _capi.check(lib.mispec_loopback_destroy(grp))
    assert_a_valid_ingest_follows(ctx)


def test_tensors_of_the_wrong_kind_are_refused(ctx):
    import torch

    M, outer, inner, val = tri_arrays(torch.int64)
    t = torch.sparse_csc_tensor(outer, inner, val, size=(300, 300))
    with pytest.raises(ValueError, match="got a tensor on cpu"):
        sa.SparseSymMatProd.from_torch(t.cpu(), ctx=ctx)
    with pytest.raises(ValueError, match="got layout torch.sparse_coo"):
        sa.SparseSymMatProd.from_torch(t.to_sparse_coo(), ctx=ctx)
    with pytest.raises(ValueError, match="got a batched tensor"):
        sa.SparseGenMatProd.from_torch(torch.stack([t.to_dense(), t.to_dense()]).to_sparse_csr(), ctx=ctx)
    with pytest.raises(ValueError, match="must be square"):
        sa.SparseSymMatProd.from_torch(torch_of(canonical("rect300x500"), 32), ctx=ctx)
    assert_a_valid_ingest_follows(ctx)


# ---- the inputs are copied ------------------------------------------------------------------------------------------------------
def test_the_inputs_may_be_overwritten_afterwards(ctx):
    import torch

    M = as_layout(canonical("band3000"), "csr")
    x = np.random.default_rng(9).uniform(-1.0, 1.0, 3000)
    for make in (sa.SparseSymMatProd.from_torch, sa.SparseGenMatProd.from_torch):
        t = torch_of(M, 64)
        op = make(t, ctx=ctx)
        before = op.perform_op(x).copy()
        t.values().fill_(float("nan"))
        t.crow_indices().fill_(-3)
        t.col_indices().fill_(2 ** 40)
        torch.cuda.synchronize()
        assert np.array_equal(bits(op.perform_op(x)), bits(before))
        del t
        torch.cuda.empty_cache()
        assert np.array_equal(bits(op.perform_op(x)), bits(before)) and not np.isnan(before).any()
