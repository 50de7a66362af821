"""tests/lagged_checks.py without a GPU: a float64 numpy stand-in of both passes of the one-sweep path and of their tails
(lagged_checks.host_lagged_pass / host_fused_pass) meets every bound at host-sized shapes, and each targeted defect, built into
the stand-in, exceeds the bound of the check aimed at it at least 100 times; the launch model is compared with the figures the
kernels' source gives for 256 CUs.

The tail restatement (lagged_checks.tail_lagged) against oracle/onesweep_variant.hpp: the oracle bindings expose that code only
through whole solves (oracle.SymEigsSolver.set_onesweep / onesweep_stats: counts of lagged steps and fallbacks, the largest
accepted |c| / |f| and the largest |V'v_i| of a solve) — no step takes a record in or hands its state out, so none of the
per-step quantities checked here (status, stop_step, H entries, beta, alpha~) can be compared through them.  What the two share
is checked on a whole solve: the thresholds (a correction is carried while |c|^2 <= 1e-6 |f|^2, so the largest accepted ratio
stays below 1e-3; a column is accepted while chk <= eps) bound the statistics the oracle reports."""
import numpy as np
import pytest

import krylov_checks as K
import lagged_checks as L

MODEL = L.HostLaggedModel()
FORMS = [(0, 0), (0, 1), (1, 0), (1, 1)]


def honest(case, out):
    res = L.host_lagged_pass(case)
    L.check_lagged_pass(case, res, MODEL, out)
    return L.check_lagged_tail(case, res, MODEL, out), res


@pytest.mark.parametrize("n,i", [(1, 1), (2, 1), (3, 2), (129, 5), (257, 41), (1000, 70), (1000, 127), (1000, 130), (601, 320),
                                 (5003, 44)])
def test_honest_stand_in_meets_every_bound_of_the_pass(n, i):
    out = K.Ratios()
    V = L.basis(n, i, seed=n + i)
    for pending, onered in FORMS:
        honest(L.lagged_case(V, n, i, pending, onered, seed=3 * i + pending), out)
    out.assert_ok(f"stand-in, {n} x {i}")


def test_honest_stand_in_takes_every_branch_of_the_tail():
    out = K.Ratios()
    n, i = 200, 6
    want = {"none": L.OK, "lag": L.OK, "more": L.MORE_CORR, "tiny": L.TINY_F, "check": L.LAG_CHECK, "small": L.SMALL_BETA}
    for kind, status in want.items():
        for pending in (0, 1):
            if kind == "check" and not pending:
                continue
            s, res = honest(L.unit_case(n, i, pending, 5, kind, parts=300), out)
            assert s["status"] == status and res["status"] == status, (kind, pending, s["status"])
            assert s["carried"] == (kind == "lag") and s["written"] == (kind != "check")
    case = L.unit_case(n, i, 1, 5, "lag")
    case.lag_last = 1
    s, _ = honest(case, out)
    assert s["need_corr"] == 1 and not s["carried"] and s["lag_pending"] == 0
    s, _ = honest(L.qr_case(300, 20, 4), out)
    assert s["carried"]
    case = L.lagged_case(L.basis(100, 5, 1), 100, 5, 1, 1, seed=2)
    case.status = L.MORE_CORR
    s, res = honest_stopped(case, out)
    assert not s["live"] and res["status"] == L.MORE_CORR
    out.assert_ok("stand-in, tail")


def honest_stopped(case, out):
    res = L.host_lagged_pass(case)
    return L.check_lagged_tail(case, res, MODEL, out), res


def defect_ratio(case, defect, col, key):
    out = K.Ratios()
    L.check_lagged_pass(case, L.host_lagged_pass(case, defect, col), MODEL, out, strict=False)
    return out[key][0]


# each defect against the check aimed at it: (defect, column, (pending, onered), the check that must exceed its bound 100 times)
DEFECTS = [("c_last_row", 3, (1, 1), "c"), ("c_last_row", 69, (0, 0), "c"), ("chk_last_row", 3, (1, 1), "chk"),
           ("chk_last_row", 0, (1, 0), "chk"), ("last_tile", 0, (1, 1), "c"), ("last_tile", 0, (1, 1), "chk"),
           ("last_tile", 0, (0, 0), "sum_f2"), ("last_tile", 0, (0, 0), "slot_i"), ("skip_column", 0, (1, 0), "v_i"),
           ("skip_column", 48, (1, 1), "v_i"), ("prev_column", 0, (0, 1), "dst"), ("prev_column", 0, (1, 1), "dst"),
           ("swap_slots", 7, (1, 1), "c"), ("swap_slots", 7, (1, 1), "chk"), ("no_division", 0, (0, 0), "v_i"),
           ("no_division", 0, (0, 1), "v_i")]


@pytest.mark.parametrize("defect,col,form,key", DEFECTS)
def test_defects_of_the_pass_exceed_their_bound(defect, col, form, key):
    n, i = 1000, 70
    case = L.lagged_case(L.basis(n, i, seed=9), n, i, form[0], form[1], seed=17)
    clean = defect_ratio(case, None, 0, key)
    bad = defect_ratio(case, defect, col, key)
    print(f"{defect} (column {col}, pending = {form[0]}, onered = {form[1]}): {key} at {bad:.3e} of its bound (honest: {clean:.3e})")
    assert clean <= 1.0 and bad >= 100.0, (defect, key, clean, bad)


@pytest.mark.parametrize("i,col", [(130, 64), (130, 129), (320, 200), (511, 448)])
def test_coefficients_of_panel_0_in_another_panel_exceed_the_bound(i, col):
    n = 601
    case = L.lagged_case(L.basis(n, i, seed=9), n, i, 1, 1, seed=17)
    bad = defect_ratio(case, "panel0", col, "v_i")
    print(f"panel0 (panel {col // 64} of step {i}): v_i at {bad:.3e} of its bound")
    assert defect_ratio(case, None, 0, "v_i") <= 1.0 and bad >= 100.0


@pytest.mark.parametrize("n,m,p,kcol", [(1, 1, 1, 0), (3, 2, 2, 1), (129, 20, 17, 0), (1000, 40, 32, 31), (1000, 41, 33, 32),
                                        (1000, 64, 64, 63), (5003, 64, 49, 0)])
def test_honest_stand_in_meets_every_bound_of_the_fused_restart(n, m, p, kcol):
    out = K.Ratios()
    case = L.fused_case(L.basis(n, m, seed=m), n, m, p, kcol, seed=p)
    res = L.host_fused_pass(case)
    L.check_fused_pass(case, res, MODEL, out)
    assert res["status"] == L.RESTART_CHECK  # V'f_corr of order one
    case = L.unit_fused_case(max(n, m + 2), m, p, kcol, seed=p)
    res = L.host_fused_pass(case)
    L.check_fused_pass(case, res, MODEL, out)
    assert res["status"] == L.OK and res["rst_err"] == 0.0
    case.status = L.TINY_F
    L.check_fused_tail(case, dict(L.host_fused_pass(case), red=case.red_in), out, "stopped")
    out.assert_ok(f"stand-in, fused restart {n} x {m} -> {p}")


@pytest.mark.parametrize("defect,col,kcol,key", [("kcol", 0, 0, "fnew"), ("kcol", 0, 16, "fnew"), ("zero_q", 5, 16, "X"),
                                                 ("zero_q", 16, 16, "X"), ("zero_q", 16, 16, "fnew")])
def test_defects_of_the_fused_restart_exceed_their_bound(defect, col, kcol, key):
    n, m, p = 1000, 40, 17
    case = L.fused_case(L.basis(n, m, seed=4), n, m, p, kcol, seed=8)
    ratios = []
    for d in (None, defect):
        out = K.Ratios()
        res = L.host_fused_pass(case, d, col)
        if d == "zero_q":  # (the stand-in forms fnew from its own X: refer it to the X a correct Q gives, as the check's data does)
            res_ok = L.host_fused_pass(case)
            if key == "fnew":
                res["V"] = res_ok["V"]
        L.check_fused_pass(case, res, MODEL, out, strict=False)
        ratios.append(out[key][0])
    print(f"{defect} (column {col}, kcol = {kcol}): {key} at {ratios[1]:.3e} of its bound (honest: {ratios[0]:.3e})")
    assert ratios[0] <= 1.0 and ratios[1] >= 100.0, ratios


def test_launch_model_at_256_cus():
    """The figures the kernels' source gives (csrc/krylov.hip launch_orth_lagged, orth_dma.hip, orth_wide.hip, launch_vq_fused)."""
    M = L.LaggedModel(256)
    g = lambda n, i, *keys: tuple(M.lagged(n, i)[k] for k in keys)
    assert g(1000, 40, "kernel", "MAXS", "R", "NW", "grid", "T") == ("k_orth_lagged", 10, 2, 4, 4, 1)
    assert g(1000, 41, "MAXS", "R", "grid") == (11, 1, 8)
    assert g(1000, 63, "MAXS", "NW") == (16, 4) and g(1000, 64, "MAXS", "NW", "R") == (8, 8, 1) and g(1000, 127, "MAXS", "NW") == (16, 8)
    assert g(131_071, 5, "kernel", "grid") == ("k_orth_lagged", 512)
    assert g(131_072, 5, "kernel", "MAXS", "depth", "grid", "T") == ("k_orth_lagged_dma", 2, 3, 256, 4)
    assert g(131_075, 44, "depth", "T") == (3, 5) and g(131_075, 45, "depth") == (2,) and g(131_075, 64, "kernel") == ("k_orth_lagged",)
    assert L.LaggedModel(256, "reg").lagged(524_547, 40)["T"] == 3 and L.LaggedModel(256, "reg").lagged(524_547, 41)["T"] == 5
    assert L.LaggedModel(256, "reg").lagged(131_331, 70)["T"] == 3 and L.LaggedModel(256, "reg").lagged(131_331, 70)["grid"] == 512
    assert L.LaggedModel(256, "dma").lagged(1000, 63)["kernel"] == "k_orth_lagged_dma" and L.LaggedModel(256, "dma2").lagged(1000, 5)["depth"] == 2
    assert g(1000, 128, "kernel", "npan", "MAXS", "grid") == ("panels", 2, 16, 4) and g(30_001, 129, "npan", "MAXS", "grid", "T") == (3, 1, 118, 2)
    assert g(30_001, 511, "npan", "MAXS") == (8, 16)
    assert M.k_vi(1000, 5) == 7 and M.k_vi(1000, 70) == 15 and M.k_vi(1000, 129) == 23 and M.k_vi(1000, 511) == 28
    assert M.k_dot(1000, 5) == 2 + 2 + 6 + 1 + 6 and M.k_dot(131_075, 44) == 2 + 5 + 6 + 4 + 6
    f = lambda m, p: M.vq_fused(1000, m, p)["kernel"]
    assert (f(20, 16), f(40, 17), f(40, 32), f(41, 17), f(64, 33), f(64, 49)) == (
        "k_vq_fused<4,16>", "k_vq_fused<8,10>", "k_vq_fused<8,10>", "k_vq_fused<8,16>", "k_vq_fused<12,16>", "k_vq_fused<16,16>")
    assert M.vq_fused(100_003, 64, 64)["T"] == 2 and M.vq_fused(100_003, 64, 64)["grid"] == 768
    assert [M.reduce_form(r, c) for r, c in [(64, 3), (65, 3), (129, 3), (256, 93), (257, 3), (256, 95)]] == [
        "round1", "round2", "round4", "round4", "passes", "passes"]


def test_the_oracle_reports_statistics_inside_the_thresholds_the_restatement_uses():
    """The only quantities of the tail the oracle bindings hand out (see the module text)."""
    import scipy.sparse as sp

    import oracle

    n, k, m = 400, 6, 24
    r, c, v = oracle.gen_sparse_data(n, 0.05)
    A = sp.coo_matrix((v, (r, c)), shape=(n, n)).tocsc()
    for one_reduction in (False, True):
        ref = oracle.SymEigsSolver(oracle.Op.csc_sym(n, A.indptr, A.indices, A.data, True), k, m)
        ref.set_onesweep(True, fused=True, one_reduction=one_reduction)
        ref.init()
        ref.compute(oracle.LargestAlge)
        stats = ref.onesweep_stats()
        assert stats["lagged_steps"] > 0
        assert stats["max_rel_c"] <= np.sqrt(1e-6) * (1.0 + 1e-12)  # lag_limit of tail_lagged: |c|^2 <= 1e-6 |f|^2
        if one_reduction:
            assert stats["one_reduction_steps"] > 0
