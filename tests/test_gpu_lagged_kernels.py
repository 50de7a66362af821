"""The one-sweep Lanczos kernels one pass at a time (tests/lagged_checks.py: the hooks sa.lagged_pass / sa.fused_restart_pass,
long-double references, bounds counted from the kernels' source) at the smallest shapes at which each branch of
csrc/krylov.hip (k_orth_lagged, k_reduce_partials and its tails, k_vq_fused), csrc/orth_dma.hip and csrc/orth_wide.hip exists.
Sizes that depend on the device are derived from its CU count; the figures in the comments are for 256 CUs.
tests/test_host_lagged_checks.py shows, without a GPU, that an honest float64 implementation meets these bounds and that each
targeted defect exceeds them at least 100 times."""
import functools
import itertools

import numpy as np
import pytest
import torch

import lagged_checks as L
import spectra_amd as sa
from krylov_checks import Ratios

pytestmark = pytest.mark.gpu
FORMS = list(itertools.product((0, 1), (0, 1)))  # (pending, onered)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=2)
def device_basis(n, ncols, seed=11):
    """(host basis, the same on the device as a (columns, ld) tensor), shared by the cases of one shape and never written."""
    V = L.basis(n, ncols, seed)
    return V, torch.from_numpy(np.ascontiguousarray(V.T)).to("cuda")


def up(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda")


def run_lagged(ctx, case, Vd=None, pstride=0):
    Vd = up(case.V.T) if Vd is None else Vd
    f, src, vout = up(case.f), up(case.src), up(case.vout_in)
    res = sa.lagged_pass(Vd[: case.i], case.i, case.n, f, src, vout, case.c_in, case.alpha, case.beta, pending=case.pending,
                         onered=case.onered, diag=case.diag, subd=case.subd, status=case.status, lag_last=case.lag_last,
                         lag_chk_max=case.lag_chk_max, lag_rel_c_max=case.lag_rel_c_max, lag_limit=case.lag_limit, n_op=case.n_op,
                         lag_steps=case.lag_steps, onered_steps=case.onered_steps, alpha_parts=case.alpha_parts, pstride=pstride,
                         red=case.red_in, ctx=ctx)
    res["vout"], res["f"] = vout.cpu().numpy(), f.cpu().numpy()
    return res


def generic_steps(ctx, n, steps, model, out, kernel, forms=FORMS, ncols=None):
    """Step i on the first i columns of one shared basis, generic data, every form; returns the launch parameters seen."""
    V, Vd = device_basis(n, ncols or max(steps))
    seen = set()
    for i in steps:
        launch = model.lagged(n, i)
        assert launch["kernel"] == kernel, (n, i, launch)
        seen.add((launch["MAXS"], launch["R"], launch["NW"], launch["depth"], launch["T"]))
        for pending, onered in forms:
            case = L.lagged_case(V[:, :i], n, i, pending, onered, seed=1000 * i + 2 * pending + onered)
            res = run_lagged(ctx, case, Vd)
            L.check_lagged_pass(case, res, model, out)
            L.check_lagged_tail(case, res, model, out)
    return seen


# ---- k_orth_lagged<MAXS, R, NW, ONERED> -------------------------------------------------------------------------------------
# every i = 1 ... 127 at 1000 rows: every MAXS = 1 ... 16 of NW = 4 with the tile height switching at 40 | 41 columns, the switch
# to NW = 8 at 64 and its MAXS = 8 ... 16; in the one-reduction form every owner wavefront and slot of column i - 1
@pytest.mark.parametrize("lo,hi", [(1, 24), (25, 44), (45, 63), (64, 84), (85, 106), (107, 127)])
def test_register_kernel_every_column_count(ctx, lo, hi):
    model, out = L.LaggedModel(cus()), Ratios()
    seen = generic_steps(ctx, 1000, range(lo, hi + 1), model, out, "k_orth_lagged", ncols=127)
    want = {(L.cdiv(i, 4), 2 if i <= 40 else 1, 4) if i < 64 else (min(max(L.cdiv(i, 8), 8), 16), 1, 8) for i in range(lo, hi + 1)}
    assert {s[:3] for s in seen} == want
    out.assert_ok(f"k_orth_lagged 1000 rows, i = {lo} ... {hi}")


# one row pair and the zero-padded odd row, one tile and its edges at R = 1 and R = 2
@pytest.mark.parametrize("n", [1, 2, 3, 127, 128, 129, 255, 256, 257])
def test_register_kernel_row_edges(ctx, n):
    model, out = L.LaggedModel(cus()), Ratios()
    generic_steps(ctx, n, (1, 5, 41, 70), model, out, "k_orth_lagged")
    out.assert_ok(f"k_orth_lagged {n} rows")


# several tiles per workgroup (psum[buf] and vprev_s[buf] alternate): more than 2 x 4 CUs tiles of 256 rows under
# orth_kernel=reg — three tiles at R = 2 (40 columns), five at R = 1 (41); NW = 8: more than 2 x 2 CUs tiles of 128 rows (70)
@pytest.mark.parametrize("pending,onered", FORMS)
@pytest.mark.parametrize("i", [40, 41, 70])
def test_register_kernel_several_tiles_per_workgroup(ctx, i, pending, onered):
    n = 2 * (4 * cus() * 256) + 259 if i < 64 else 2 * (2 * cus() * 128) + 259  # 524 547 | 131 331
    model, out = L.LaggedModel(cus(), "reg"), Ratios()
    assert model.lagged(n, i)["T"] == {40: 3, 41: 5, 70: 3}[i]
    try:
        sa.set_option("orth_kernel", "reg")
        generic_steps(ctx, n, (i,), model, out, "k_orth_lagged", forms=[(pending, onered)], ncols=41 if i < 64 else 70)
    finally:
        sa.set_option("orth_kernel", None)
    out.assert_ok(f"k_orth_lagged {n} rows, i = {i}")


# ---- k_orth_lagged_dma<MAXS, DEPTH, ONERED> ---------------------------------------------------------------------------------
# the switch at 1024 tiles of 128 rows: the last size of the register kernel, exactly 1024 full tiles, and 1025 tiles, ragged and
# odd (four or five tiles per workgroup: the ring wraps); MAXS = 1, 2, 10, 11 with three ring slots, 12 and 16 with two
@pytest.mark.parametrize("i", [1, 4, 5, 40, 41, 44, 45, 63])
@pytest.mark.parametrize("n", [131_071, 131_072, 131_075])
def test_across_the_switch_to_the_lds_dma_kernel(ctx, n, i):
    model, out = L.LaggedModel(cus()), Ratios()
    kernel = "k_orth_lagged" if n < 131_072 else "k_orth_lagged_dma"
    seen = generic_steps(ctx, n, (i,), model, out, kernel, ncols=63)
    if n >= 131_072:
        assert {s[3] for s in seen} == {3 if i <= 44 else 2}
    out.assert_ok(f"{kernel} {n} rows, i = {i}")


def test_lds_dma_kernel_with_two_ring_slots_forced(ctx):
    model, out = L.LaggedModel(cus(), "dma2"), Ratios()
    try:
        sa.set_option("orth_kernel", "dma2")
        seen = generic_steps(ctx, 131_075, (44,), model, out, "k_orth_lagged_dma", ncols=63)
    finally:
        sa.set_option("orth_kernel", None)
    assert {s[3] for s in seen} == {2}
    out.assert_ok("k_orth_lagged_dma<11, 2> 131 075 rows")


# one tile per workgroup: the ring never wraps
def test_lds_dma_kernel_on_one_tile_per_workgroup(ctx):
    model, out = L.LaggedModel(cus(), "dma"), Ratios()
    try:
        sa.set_option("orth_kernel", "dma")
        seen = generic_steps(ctx, 1000, (1, 5, 41, 45, 63), model, out, "k_orth_lagged_dma", ncols=127)
    finally:
        sa.set_option("orth_kernel", None)
    assert {s[4] for s in seen} == {1}
    out.assert_ok("k_orth_lagged_dma 1000 rows")


# ---- panelled steps: CORRECT_ONLY panels, k_lagged_last_panel, k_lagged_dots -----------------------------------------------
# two to eight panels, the last one of 1, 2, 63 and 64 columns; every c_in entry differs, so coefficients of the wrong panel fail
@pytest.mark.parametrize("i", [128, 129, 191, 192, 193, 255, 256, 257, 320, 511])
@pytest.mark.parametrize("n", [1000, 30_001])
def test_panelled_steps(ctx, n, i):
    model, out = L.LaggedModel(cus()), Ratios()
    generic_steps(ctx, n, (i,), model, out, "panels", ncols=511)
    out.assert_ok(f"panelled step {n} rows, i = {i}: {model.describe(n, i)}")


# ---- k_reduce_partials ------------------------------------------------------------------------------------------------------
# one record count on each side of every switch: one round with RPL = 1 | 2 | 4 records per lane (64 | 65, 128 | 129, 256 records)
# against the passes of 48 columns (257 records; 97 slots at 256 records), the scalar slots riding in the last pass (45 slots) or
# in one of their own (47), and 3 and 1023 slots
def test_reduction_forms(ctx):
    c = cus()
    model, out = L.LaggedModel(c), Ratios()
    forms = set()
    for i, nrec, form in [(1, 64, "round1"), (1, 65, "round2"), (1, 128, "round2"), (1, 129, "round4"), (1, 256, "round4"),
                          (1, 257, "passes"), (22, 257, "passes"), (23, 257, "passes"), (46, 256, "round4"), (47, 256, "passes"),
                          (511, 65, "passes")]:
        if nrec > 4 * c:
            continue
        launch = model.lagged(1, i)
        n = nrec * (256 if i >= 128 else 128 * launch["R"])
        launch = model.lagged(n, i)
        assert launch["nrec"] == nrec and model.reduce_form(nrec, 2 * i + 1) == form, (i, nrec, launch)
        forms.add(form)
        for pending, onered in [(0, 0), (1, 1)]:
            V, Vd = device_basis(n, i, seed=7)
            case = L.lagged_case(V, n, i, pending, onered, seed=i + nrec, alpha_count=300 if i != 23 else 9000)
            res = run_lagged(ctx, case, Vd)
            L.check_lagged_pass(case, res, model, out)
            L.check_lagged_tail(case, res, model, out)
    assert forms == {"round1", "round2", "round4", "passes"}
    out.assert_ok("k_reduce_partials")


# ---- the tail: every branch of finish_lagged and start_next_onered on constructed data --------------------------------------
def tail_of(ctx, case, model, out):
    res = run_lagged(ctx, case)
    L.check_lagged_pass(case, res, model, out)
    return L.check_lagged_tail(case, res, model, out), res


@pytest.mark.parametrize("pending", [0, 1])
def test_tail_branches(ctx, pending):
    model, out = L.LaggedModel(cus()), Ratios()
    n, i = 200, 6
    s, _ = tail_of(ctx, L.unit_case(n, i, pending, 1, "none"), model, out)
    assert (s["status"], s["lag_pending"], s["count"], s["need_corr"]) == (L.OK, 0, 0, 0) and s["written"]
    s, res = tail_of(ctx, L.unit_case(n, i, pending, 2, "lag"), model, out)
    assert (s["status"], s["lag_pending"], s["count"]) == (L.OK, 1, 1) and s["carried"] and res["beta"] < res["red"][L.SLOT_BETA]
    s, _ = tail_of(ctx, L.unit_case(n, i, pending, 3, "more"), model, out)
    assert (s["status"], s["stop_step"], s["stop_count"], s["lag_pending"]) == (L.MORE_CORR, i, 0, 0)
    s, _ = tail_of(ctx, L.unit_case(n, i, pending, 4, "tiny"), model, out)
    assert (s["status"], s["stop_step"], s["stop_count"]) == (L.TINY_F, i, 0)
    case = L.unit_case(n, i, pending, 5, "lag")
    case.lag_last = 1
    s, res = tail_of(ctx, case, model, out)
    assert (s["status"], s["need_corr"], s["lag_pending"], s["count"]) == (L.OK, 1, 0, 0) and res["beta"] == res["red"][L.SLOT_BETA]
    if pending:
        s, _ = tail_of(ctx, L.unit_case(n, i, 1, 6, "check"), model, out)
        assert (s["status"], s["stop_step"], s["stop_count"]) == (L.LAG_CHECK, i, 1) and not s["written"]
    # the one-reduction tail behind the step: alpha~ for the next one, or its small-beta stop
    s, _ = tail_of(ctx, L.unit_case(n, i, pending, 7, "lag", parts=300), model, out)
    assert s["status"] == L.OK and s["onered_steps"] == 4
    s, _ = tail_of(ctx, L.unit_case(n, i, pending, 8, "small", parts=9000), model, out)
    assert (s["status"], s["stop_step"], s["stop_count"], s["onered_steps"]) == (L.SMALL_BETA, i + 1, 0, 3)
    s, _ = tail_of(ctx, L.unit_case(n, i, pending, 9, "more", parts=300), model, out)
    assert s["status"] == L.MORE_CORR and s["onered_steps"] == 3
    # i = 1 and 2: no subd[i - 2], one coefficient
    for i_small in (1, 2):
        s, _ = tail_of(ctx, L.unit_case(n, i_small, pending, 10 + i_small, "lag"), model, out)
        assert s["carried"]
    out.assert_ok(f"tail of the lagged step, pending = {pending}")


def test_tail_on_realistic_data(ctx):
    model, out = L.LaggedModel(cus()), Ratios()
    s, _ = tail_of(ctx, L.qr_case(300, 20, 21), model, out)
    assert s["carried"] and s["status"] == L.OK
    out.assert_ok("lagged correction on a QR basis")


@pytest.mark.parametrize("status", [L.SMALL_BETA, L.MORE_CORR, L.TINY_F, L.LAG_CHECK, L.RESTART_CHECK])
def test_a_stopped_run_leaves_everything_as_it_was(ctx, status):
    model, out = L.LaggedModel(cus()), Ratios()
    for n, i, onered in [(1000, 5, 1), (1000, 70, 0), (1000, 130, 1)]:
        V, Vd = device_basis(n, 130)
        case = L.lagged_case(V[:, :i], n, i, 1, onered, seed=i)
        case.status = status
        res = run_lagged(ctx, case, Vd)
        s = L.check_lagged_tail(case, res, model, out)
        assert not s["live"] and res["status"] == status


# ---- k_vq_fused<S, J> ---------------------------------------------------------------------------------------------------------
def run_fused(ctx, case, pstride=0):
    Vd, ft, fnew = up(case.V.T), up(case.ftilde), up(case.fnew_in)
    res = sa.fused_restart_pass(Vd, case.m, case.n, case.Q, case.c, ft, fnew, case.q_last, case.h_sub, case.kcol, status=case.status,
                                force_check=case.force_check, pstride=pstride, red=case.red_in, ctx=ctx)
    res["V"], res["fnew"] = np.asfortranarray(Vd.cpu().numpy().T), fnew.cpu().numpy()
    assert np.array_equal(ft.cpu().numpy().view(np.int64), case.ftilde.view(np.int64))  # ftilde is read only
    return res


def n_prefetch():
    return 3 * cus() * 128 + 1699  # 100 003: more tiles of 128 rows than 3 CUs workgroups — some prefetch a second tile


SHAPES = [(m, p) for m in (1, 20, 40, 41, 64) for p in (1, 16, 17, 32, 33, 48, 49, 64) if p <= m]


# every instantiation — <4,16> (p <= 16), <8,10> (17 ... 32, m <= 40), <8,16> (m >= 41), <12,16>, <16,16> — at its first and last
# output-column count, the new residual from the first and the last output column
@pytest.mark.parametrize("n", [1, 2, 3, 127, 128, 129, 1000])
def test_fused_restart_pass(ctx, n):
    model, out = L.LaggedModel(cus()), Ratios()
    kernels = set()
    for m, p in SHAPES:
        V = L.basis(n, m, seed=m)
        kernels.add(model.vq_fused(n, m, p)["kernel"])
        for kcol in sorted({0, p - 1}):
            case = L.fused_case(V, n, m, p, kcol, seed=100 * m + p + kcol)
            L.check_fused_pass(case, run_fused(ctx, case), model, out)
    assert kernels == {"k_vq_fused<4,16>", "k_vq_fused<8,10>", "k_vq_fused<8,16>", "k_vq_fused<12,16>", "k_vq_fused<16,16>"}
    out.assert_ok(f"k_vq_fused {n} rows")


@pytest.mark.parametrize("m,p", [(20, 16), (40, 32), (41, 17), (41, 33), (64, 64)])
def test_fused_restart_pass_with_the_prefetch_of_a_second_tile(ctx, m, p):
    n = n_prefetch()
    model, out = L.LaggedModel(cus()), Ratios()
    assert model.vq_fused(n, m, p)["T"] == 2
    V = L.basis(n, m, seed=m)
    for kcol in (0, p - 1):
        case = L.fused_case(V, n, m, p, kcol, seed=100 * m + p + kcol)
        L.check_fused_pass(case, run_fused(ctx, case), model, out)
    out.assert_ok(f"k_vq_fused {n} rows, {m} -> {p}")


def test_fused_restart_tail_both_ways(ctx):
    model, out = L.LaggedModel(cus()), Ratios()
    case = L.fused_case(L.basis(1000, 20, 3), 1000, 20, 9, 8, seed=1)  # V'f_corr of order one: the restart's test fails
    res = run_fused(ctx, case)
    L.check_fused_pass(case, res, model, out)
    assert (res["status"], res["stop_step"], res["stop_count"]) == (L.RESTART_CHECK, 8, 1)
    case = L.unit_fused_case(200, 20, 9, 8, seed=2)  # V'f_corr = 0 exactly: it passes
    res = run_fused(ctx, case)
    L.check_fused_pass(case, res, model, out)
    assert res["status"] == L.OK and res["rst_err"] == 0.0 and res["beta"] > 0.0
    case = L.unit_fused_case(200, 20, 9, 8, seed=2)  # ... unless the factorisation's test switch forces the stop
    case.force_check = 1
    res = run_fused(ctx, case)
    L.check_fused_pass(case, res, model, out)
    assert res["status"] == L.RESTART_CHECK
    case = L.fused_case(L.basis(1000, 20, 3), 1000, 20, 9, 8, seed=1, status=L.MORE_CORR)  # a stopped run: record and state stay
    res = run_fused(ctx, case)
    L.check_fused_tail(case, res, out, "stopped")
    assert res["status"] == L.MORE_CORR
    out.assert_ok("tail of the fused restart")


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_the_hooks_refuse_bad_arguments(ctx):
    n = 1000
    V, Vd = device_basis(n, 130)
    wide = torch.zeros((512, 8), dtype=torch.float64, device="cuda")
    vec = lambda: torch.zeros(V.shape[0], dtype=torch.float64, device="cuda")
    kw = dict(pending=0, onered=0, diag=np.zeros(600), subd=np.zeros(600), ctx=ctx)
    with pytest.raises(ValueError):  # i < 1
        sa.lagged_pass(Vd, 0, n, vec(), vec(), vec(), np.zeros(0), 1.0, 1.0, **kw)
    with pytest.raises(ValueError):  # 2 i + 1 > 1024
        sa.lagged_pass(wide, 512, 6, vec(), vec(), vec(), np.zeros(512), 1.0, 1.0, **kw)
    with pytest.raises(ValueError):  # ld < n
        sa.lagged_pass(Vd, 5, V.shape[0] + 2, vec(), vec(), vec(), np.zeros(5), 1.0, 1.0, **kw)
    with pytest.raises(ValueError):  # columns that are not 16-byte aligned
        sa.lagged_pass(Vd[:, 1:], 5, n, vec(), vec(), vec(), np.zeros(5), 1.0, 1.0, **kw)
    for i in (5, 70, 130):  # a record stride smaller than the grid: register kernel (4 and 8 wavefronts), panels
        with pytest.raises(ValueError, match="stride"):
            sa.lagged_pass(Vd, i, n, vec(), vec(), vec(), np.zeros(i), 1.0, 1.0, pstride=L.LaggedModel(cus()).lagged(n, i)["grid"] - 1, **kw)
    try:
        sa.set_option("orth_kernel", "dma")
        with pytest.raises(ValueError, match="stride"):
            sa.lagged_pass(Vd, 5, n, vec(), vec(), vec(), np.zeros(5), 1.0, 1.0, pstride=7, **kw)
    finally:
        sa.set_option("orth_kernel", None)
    Q, c = np.zeros((20, 9)), np.zeros(20)
    with pytest.raises(ValueError):  # p > m
        sa.fused_restart_pass(Vd, 8, n, np.zeros((8, 9)), np.zeros(8), vec(), vec(), 1.0, 1.0, 0, ctx=ctx)
    with pytest.raises(ValueError):  # m > 64
        sa.fused_restart_pass(Vd, 65, n, np.zeros((65, 9)), np.zeros(65), vec(), vec(), 1.0, 1.0, 0, ctx=ctx)
    with pytest.raises(ValueError):  # kcol outside the output columns
        sa.fused_restart_pass(Vd, 20, n, Q, c, vec(), vec(), 1.0, 1.0, 9, ctx=ctx)
    with pytest.raises(ValueError):  # ld < n
        sa.fused_restart_pass(Vd, 20, V.shape[0] + 2, Q, c, vec(), vec(), 1.0, 1.0, 0, ctx=ctx)
    with pytest.raises(ValueError):  # the new residual in the buffer of the old one
        f = vec()
        sa.fused_restart_pass(Vd, 20, n, Q, c, f, f, 1.0, 1.0, 0, ctx=ctx)
    with pytest.raises(ValueError, match="stride"):
        sa.fused_restart_pass(Vd, 20, n, Q, c, vec(), vec(), 1.0, 1.0, 0, pstride=7, ctx=ctx)
    assert np.array_equal(Vd.cpu().numpy().T.view(np.int64), V.view(np.int64))  # nothing was launched
