"""Mirrored diagonals of the diagonal SpMV format (option `dia_sym`): a lower diagonal whose bits equal its upper partner's is not
stored and is read from the partner's array k rows higher.  Products, solver runs and epilogue records must not change by a bit,
whichever diagonals are mirrored; a diagonal that differs anywhere stays stored."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import spectra_amd as sa
from spectra_amd import _capi

pytestmark = pytest.mark.gpu

SETTINGS = ("0", "auto", "all")
HEADLINE = (1, 2, 3, 1000, 1001, 100000, 100001)
N_HEADLINE = 131072 + 256 * 5 + 3
REACH = 131072  # kDiaSymReach of csr_dia.hip: dia_sym = auto mirrors the eligible diagonals up to it
SHAPES = [
    (200, (1, 2, 3)),                                   # one partial block; the lead is all zeros
    (256 * 3 + 37, (1, 2, 3, 255, 256, 257)),           # odd and even k, the source crosses one block edge, ragged last block
    (256 * 9 + 1, (1, 300, 513, 1000, 1001)),           # the source 2-4 blocks back
    (1500, (1, 1400, 1499)),                            # k almost n; its diagonals are under 3/4 full, so diagonal storage is
                                                        # declined at ingest and forced format 2 runs the offset codes
    (1500, (1, 2, 3, 1499)),                            # k almost n WITH diagonal storage (9 diagonals, 0.78 full): nearly every
                                                        # row of the mirrored -1499 reads the zero lead
    (N_HEADLINE, HEADLINE),                             # the headline pattern, far diagonals included
    (256 * 8 + 37, (1, 300, 600, 900)),                 # 9 diagonals in 7 clusters: 8 registers of window entries (NCW = 8), even
                                                        # and odd shifts
    (256 * 40 + 37, (1, 2, 3, 500, 501, 502, 503, 2000, 2001, 2002)),  # 21 diagonals, 5 clusters: one row per thread, 3 groups,
                                                        # plain (setting 0) and mirrored
    (1000, tuple(range(1, 16))),                        # 31 diagonals in one cluster: 4 groups, plain and mirrored
]
SEVEN_CLUSTERS, THREE_GROUPS = SHAPES[6], SHAPES[7]


def build(make, setting):
    """An operator built under dia_sym = setting (the option is read when the diagonal storage is built)."""
    sa.set_option("dia_sym", setting)
    try:
        return make()
    finally:
        sa.set_option("dia_sym", None)


def seeded(n, seed=7):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def products(op, x):
    """(format-0 product, format-2 product) of one operator; the second must really run diagonal storage."""
    op.set_spmv_format(0)
    assert op.spmv_format() == 0
    ref = op.perform_op(x).copy()
    op.set_spmv_format(2)
    assert op.spmv_format() == 2
    return ref, op.perform_op(x).copy()


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("n,offsets", SHAPES, ids=[f"n{n}-{len(o)}" for n, o in SHAPES])
def test_product_bit_for_bit(ctx, n, offsets, setting):
    op = build(lambda: sa.SparseSymMatProd.synth_band(n, offsets=offsets, ctx=ctx), setting)
    info = op.dia_info()
    if offsets == (1, 1400, 1499):  # no diagonal storage (see SHAPES): the forced format falls back, the product still has to agree
        assert info == {"ndia": 0, "nstored": 0, "nmirrored": 0, "lead_blocks": 0}
        op.set_spmv_format(0)
        ref = op.perform_op(seeded(n)).copy()
        op.set_spmv_format(2)
        assert op.spmv_format() == 1
        assert np.array_equal(bits(op.perform_op(seeded(n))), bits(ref))
        return
    assert info["ndia"] == 2 * len(offsets) + 1 and info["nstored"] + info["nmirrored"] == info["ndia"]
    want = {"0": [], "all": list(offsets), "auto": [k for k in offsets if k <= REACH]}[setting]
    assert info["nmirrored"] == len(want) and info["lead_blocks"] == (max(want, default=0) + 255) // 256
    ref, got = products(op, seeded(n))
    assert np.array_equal(bits(got), bits(ref))
    assert np.abs(ref).max() > 0.0


def test_counts_through_dia_info(ctx):
    n, offsets = SHAPES[1]
    by = {s: build(lambda: sa.SparseSymMatProd.synth_band(n, offsets=offsets, ctx=ctx), s).dia_info() for s in SETTINGS}
    assert by["all"]["nmirrored"] == 6 and by["0"]["nmirrored"] == 0
    for info in by.values():
        assert info["nstored"] + info["nmirrored"] == info["ndia"] == 13
    assert by["0"]["lead_blocks"] == 0 and by["all"]["lead_blocks"] == 2


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("n,offsets", [SHAPES[2], SEVEN_CLUSTERS], ids=["5clusters", "7clusters"])
def test_unaligned_operands(ctx, n, offsets, setting):
    """y eight bytes off a 16-byte boundary: the one-row-per-thread kernel k_spmv_dia_win runs (NCW = 6 and 8)."""
    import torch

    op = build(lambda: sa.SparseSymMatProd.synth_band(n, offsets=offsets, ctx=ctx), setting)
    xh = seeded(n)
    ref, aligned = products(op, xh)
    x = torch.from_numpy(xh).cuda()
    buf = torch.zeros(n + 3, dtype=torch.float64, device="cuda")
    y = buf[1:n + 1]
    assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 8
    torch.cuda.synchronize()
    op.spmv_device(x.data_ptr(), y.data_ptr())
    ctx.sync()
    out = buf.cpu().numpy()
    assert out[0] == 0.0 and out[n + 1] == 0.0 and out[n + 2] == 0.0
    assert np.array_equal(bits(out[1:n + 1]), bits(ref))
    assert np.array_equal(bits(aligned), bits(ref))


def test_falling_back(ctx):
    import scipy.sparse as sp

    n, offsets = SHAPES[1]
    rp, ci, v = O.synth_band_csr(n, offsets=offsets)
    A = sp.csr_matrix((v.copy(), ci.copy(), rp.copy()), shape=(n, n))
    A.sort_indices()
    assert (A != A.T).nnz == 0

    def entry(M, r, c):
        p = M.indptr[r] + int(np.searchsorted(M.indices[M.indptr[r]:M.indptr[r + 1]], c))
        assert M.indices[p] == c
        return p

    same = build(lambda: sa.SparseGenMatProd(A, ctx=ctx), "all")
    assert same.dia_info()["nmirrored"] == 6  # handed over as a full matrix and found symmetric by the comparison alone
    x = seeded(n)
    ref, got = products(same, x)
    assert np.array_equal(bits(got), bits(ref))

    B = A.copy()
    p = entry(B, 600, 600 - 255)
    B.data[p] = np.nextafter(B.data[p], np.inf)  # one ulp, in one row of diagonal -255
    B.data[entry(B, 300, 298)] = -0.0            # (+0.0, -0.0) stored explicitly on diagonals -2 / +2
    B.data[entry(B, 298, 300)] = 0.0
    assert B.nnz == A.nnz
    for setting, mirrored in (("all", 4), ("auto", 4), ("0", 0)):
        pert = build(lambda: sa.SparseGenMatProd(B, ctx=ctx), setting)
        info = pert.dia_info()
        assert info["ndia"] == 13 and info["nmirrored"] == mirrored and info["nstored"] == 13 - mirrored  # -255 and -2 stay stored
        ref, got = products(pert, x)
        assert np.array_equal(bits(got), bits(ref))
        assert np.allclose(ref, B @ x, rtol=0, atol=1e-12)

    # which two stay stored: each change alone takes exactly one diagonal out of the six, and with -255 mirrored the product of
    # row 600 would be off by an ulp (the sign of a zero is invisible in a product, hence the count for -2)
    for change in ("ulp", "zero"):
        B1 = A.copy()
        if change == "ulp":
            p = entry(B1, 600, 600 - 255)
            B1.data[p] = np.nextafter(B1.data[p], np.inf)
        else:
            B1.data[entry(B1, 300, 298)] = -0.0
            B1.data[entry(B1, 298, 300)] = 0.0
        one = build(lambda: sa.SparseGenMatProd(B1, ctx=ctx), "all")
        assert one.dia_info()["nmirrored"] == 5, change
        ref, got = products(one, x)
        assert np.array_equal(bits(got), bits(ref)), change

    gen = build(lambda: sa.SparseGenMatProd.synth_band(4096, ctx=ctx), "all")
    assert gen.dia_info()["nmirrored"] == 0  # the non-symmetric band (at this size its far diagonals rule diagonal storage out)
    gen = build(lambda: sa.SparseGenMatProd.synth_band(4096, offsets=(1, 2, 3, 100), ctx=ctx), "all")
    info = gen.dia_info()
    assert info["ndia"] == 9 and info["nmirrored"] == 0 and info["lead_blocks"] == 0  # ... and one that has it: nothing is equal
    ref, got = products(gen, seeded(4096))
    assert np.array_equal(bits(got), bits(ref))


@pytest.mark.parametrize("orth", ["onesweep", "reference", "onesweep-twored"])
@pytest.mark.parametrize("n,offsets", [(N_HEADLINE, HEADLINE), THREE_GROUPS], ids=["headline", "21diagonals"])
def test_in_the_solver(ctx, n, offsets, orth):
    """Both fused instantiations (the post-scaled one of the one-sweep steps — with onesweep-twored on every step, not only the
    first of a run — and the plain one of the reference flow) and their epilogue records, two rows per thread (headline) and one
    row per thread with three groups (21 diagonals): a solve does not change by a bit."""
    runs = {}
    for setting in ("0", "all"):
        op = build(lambda: sa.SparseSymMatProd.synth_band(n, offsets=offsets, ctx=ctx), setting)
        assert op.spmv_format() == 2 and op.dia_info()["nmirrored"] == (len(offsets) if setting == "all" else 0)
        eigs = sa.SymEigsSolver(op, 6, 16)
        eigs.set_orth_mode(orth)
        eigs.init()
        nconv = eigs.compute(sa.SortRule.LargestMagn, 1000, 1e-10)
        runs[setting] = (nconv, eigs.eigenvalues().copy(), eigs.num_operations(), eigs.num_iterations(), eigs.residuals().copy())
    a, b = runs["0"], runs["all"]
    assert a[0] == b[0] == 6
    assert np.array_equal(bits(a[1]), bits(b[1]))
    assert a[2] == b[2] and a[3] == b[3]
    assert np.array_equal(bits(a[4]), bits(b[4]))


@pytest.fixture(scope="module")
def headline_reference(ctx):
    op = build(lambda: sa.SparseSymMatProd.synth_band(N_HEADLINE, offsets=HEADLINE, ctx=ctx), "0")
    x = seeded(N_HEADLINE, 11)
    op.set_spmv_format(0)
    y = op.perform_op(x).copy()
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@pytest.mark.parametrize("world", [2, 3])
def test_row_shards(headline_reference, world):
    """The shards of a row partition (loopback communicator, as in test_gpu_sharded.py): with row_begin > 0 the lead holds what the
    first local rows read above the shard, taken from their own lower entries."""
    import torch

    xh, ref = headline_reference
    lib = sa.lib()
    grp = C.c_void_p()
    _capi.check(lib.mispec_loopback_create(world, C.byref(grp)))
    try:
        x = torch.from_numpy(np.array(xh)).cuda()
        for rank in range(world):
            sctx = sa.Context(0)
            _capi.check(lib.mispec_loopback_attach(grp, sctx.h, rank))
            sctx.rank, sctx.world = rank, world
            op = build(lambda: sa.SparseSymMatProd.synth_band(N_HEADLINE, offsets=HEADLINE, ctx=sctx), "all")
            b, e = sa.shard_range(N_HEADLINE, world, rank)
            assert op.local_rows() == e - b
            op.set_spmv_format(2)
            info = op.dia_info()
            if rank in (0, world - 1):
                assert op.spmv_format() == 2 and info["nmirrored"] == 7 and info["lead_blocks"] == 391
            else:  # the middle shard of three holds no entry of the diagonals +-100000 / 100001: under 3/4 full, no diagonal storage
                assert op.spmv_format() == 1 and info["ndia"] == 0
            y = torch.zeros(e - b + 2, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            op.spmv_device(x.data_ptr(), y.data_ptr())
            sctx.sync()
            out = y.cpu().numpy()
            assert np.array_equal(bits(out[:e - b]), bits(ref[b:e])), rank
            assert out[e - b] == 0.0 and out[e - b + 1] == 0.0
            del op
    finally:
        _capi.check(lib.mispec_loopback_destroy(grp))
