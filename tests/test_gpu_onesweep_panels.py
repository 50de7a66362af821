"""The opt-in one-sweep Lanczos steps on bases of 129 to 512 columns (mode "onesweep-wide", include/mispec.h MISPEC_ORTH_WIDE,
DESIGN.md 3.2.4): from step 128 on the pass over V runs in column panels (csrc/orth_wide.hip).  Gates: the Lanczos identities and
the reference flow's H at the factorisation level; at the solve level the gates of test_gpu_onesweep.py::test_onesweep_on_wide_bases
(the reference-mode device solve, the oracle of the reference algorithm and the oracle's restatement of the variant); the limits of
the mode; a spectrum that drives the steps out of the lagged path; one size at which the narrow steps of the same sweep take the
LDS-DMA kernel.

The oracle runs of the n = 30 001 shapes take a minute each on the CPU: they are recorded in tests/golden/onesweep_wide_oracle.json
(tests/golden/make_onesweep_wide_golden.py, which also asserts that the oracle BY ITSELF meets the gates on every shape used here —
all six shapes did, none was replaced); the n = 1000 shapes run the oracle live.  As in test_onesweep_on_wide_bases the 200 000-row
case is gated by the reference-mode device solve and scipy's product only."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import oracle as O
import spectra_amd as sa
from spectra_amd import _capi
from helpers import sparse_fixture, wanted_by_rule
from test_gpu_onesweep import ADVERSARIAL

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "symeigs_golden.npz"))
OFFSETS = (1, 2, 3, 100, 101, 2000, 2001)
FIRST_PANEL_STEP = 128
EPS = np.finfo(float).eps


@pytest.fixture(params=["one-reduction", "two-reductions"], autouse=True)
def reductions(request, monkeypatch):
    """Both forms of the lagged step, as in test_gpu_onesweep.py: one reduction per step (the default) and MISPEC_ONE_REDUCTION=0."""
    monkeypatch.setenv("MISPEC_ONE_REDUCTION", "1" if request.param == "one-reduction" else "0")
    return request.param


_matrices = {}


def matrix(ctx, n):
    """(device operator, symmetric scipy matrix, oracle operator factory) — built once per size."""
    if n not in _matrices:
        if n == 1000:
            A, S = sparse_fixture(n, 0.01)
            op = sa.SparseSymMatProd(A, ctx=ctx)
            Sc = sp.csr_matrix(S)
            Sc.sort_indices()
            oop = lambda: O.Op.csr(n, n, Sc.indptr.astype(np.int32), Sc.indices.astype(np.int32), Sc.data)  # noqa: E731
        else:
            offsets = OFFSETS if n == 30_001 else None  # 200 000 rows: the benchmark's M-band
            kw = {} if offsets is None else {"offsets": offsets}
            op = sa.SparseSymMatProd.synth_band(n, ctx=ctx, **kw)
            rp, ci, v = O.synth_band_csr(n, **kw)
            S = sp.csr_matrix((v, ci, rp), shape=(n, n))
            oop = lambda: O.Op.csr(n, n, rp, ci, v)  # noqa: E731
        _matrices[n] = (op, S, oop)
    return _matrices[n]


def solve(op, k, m, rule, mode, ctx=None, **kw):
    eigs = sa.SymEigsSolver(op, k, m) if ctx is None else sa.SymEigsSolver(op, k, m, ctx=ctx)
    eigs.set_orth_mode(mode)
    eigs.init(kw.pop("v0", None))
    nconv = eigs.compute(rule, **kw)
    return eigs, nconv


def lanczos_identities(fac, S, k, tol):
    # (test_gpu_onesweep.py's check, restated)
    V, H, f = fac.matrix_V(k), fac.matrix_H()[:k, :k], fac.vector_f()
    resid = S @ V - V @ H
    resid[:, k - 1] -= f
    assert np.abs(resid).max() < tol and np.abs(V.T @ V - np.eye(k)).max() < tol  # A V = V H + f e_k'
    assert np.abs(V.T @ f).max() < tol * max(1.0, np.abs(f).max()) and abs(np.linalg.norm(f) - fac.f_norm()) < tol


def factorize(op, m, mode):
    fac = sa.Factorization(op, m, True)
    fac.set_orth_mode(mode)
    fac.init_random(0)
    fac.factorize_from(1, m)
    return fac


# ---- 1. factorisation level ---------------------------------------------------------------------------------------------------------
_reference_H = {}


@pytest.mark.parametrize("m", [129, 130, 192, 193, 257, 512])
@pytest.mark.parametrize("n", [1000, 30_001])
def test_panelled_steps_build_the_factorisation_of_the_reference_flow(ctx, n, m):
    # m: the first panelled step (i = 128), the panel edges 128 / 192 / 256 from both sides, and the record's last slot (2 * 511);
    # n = 30 001 is odd: the last 128-row tile is ragged
    op, S, _ = matrix(ctx, n)
    if (n, m) not in _reference_H:
        ref = factorize(op, m, "reference")
        assert ref.orth_info()["mode"] == "reference" and ref.orth_info()["panel_steps"] == 0
        _reference_H[(n, m)] = ref.matrix_H()
    Href = _reference_H[(n, m)]
    fac = factorize(op, m, "onesweep-wide")
    info = fac.orth_info()
    print("n %d m %d: panel_steps %d lagged_steps %d check_stops %d state_stops %d max_chk %.2e" % (
        n, m, info["panel_steps"], info["lagged_steps"], info["check_stops"], info["state_stops"], info["max_chk"]))
    assert info["mode"] == "onesweep" and info["wide"]
    lanczos_identities(fac, S, m, 1e-10)
    H = fac.matrix_H()
    print("   max|H - H_reference| / max|H| = %.2e" % (np.abs(H - Href).max() / np.abs(Href).max()))
    assert np.abs(H - Href).max() <= 1e-10 * np.abs(Href).max()
    # steps i = 128 .. m - 1 go in panels, minus those that left the lagged path
    left = info["check_stops"] + info["state_stops"]
    assert 0 < info["panel_steps"] <= m - FIRST_PANEL_STEP and info["panel_steps"] >= m - FIRST_PANEL_STEP - left
    if m >= 192:
        assert info["panel_steps"] >= 0.8 * (m - FIRST_PANEL_STEP)


@pytest.mark.parametrize("n", [1000, 30_001])
def test_the_flag_leaves_narrow_bases_untouched(ctx, n):
    # m = 128: no step has 128 finished columns, every launch is the one it is without the flag — the same bits
    op, S, _ = matrix(ctx, n)
    wide, plain = factorize(op, 128, "onesweep-wide"), factorize(op, 128, "onesweep")
    assert wide.orth_info()["panel_steps"] == 0 and wide.orth_info()["mode"] == "onesweep" and wide.orth_info()["wide"]
    assert wide.orth_info()["lagged_steps"] == plain.orth_info()["lagged_steps"] > 0
    assert np.array_equal(wide.matrix_V(), plain.matrix_V())
    assert np.array_equal(wide.matrix_H(), plain.matrix_H())
    assert np.array_equal(wide.vector_f(), plain.vector_f())


# ---- 2. solve level -----------------------------------------------------------------------------------------------------------------
_reference_solves = {}
_oracle_records = None


def reference_solve(op, n, k, m, rule):
    """The reference-mode device solve of a shape (it does not depend on the reduction form): run once."""
    key = (n, k, m, rule)
    if key not in _reference_solves:
        ref, nconv = solve(op, k, m, sa.SortRule[rule], "reference", maxit=1000, tol=1e-11)
        _reference_solves[key] = {"nconv": nconv, "eigenvalues": ref.eigenvalues(), "num_operations": ref.num_operations(),
                                  "lagged_steps": ref.orth_info()["lagged_steps"], "mode": ref.orth_info()["mode"]}
    return _reference_solves[key]


def oracle_solve(oop, n, k, m, rule, flavour):
    """nconv, info, eigenvalues and operation count of the CPU oracle: flavour "reference" is the reference algorithm, the two others
    its restatement of the one-sweep variant.  n = 1000: run here; n = 30 001: the record of make_onesweep_wide_golden.py."""
    global _oracle_records
    if n != 1000:
        if _oracle_records is None:
            with open(os.path.join(HERE, "golden", "onesweep_wide_oracle.json")) as f:
                _oracle_records = json.load(f)
        rec = _oracle_records["%d_%d_%d_%s_%s" % (n, k, m, rule, flavour)]
        return rec["nconv"], rec["info"], np.array(rec["eigenvalues"]), rec["num_operations"]
    o = O.SymEigsSolver(oop(), k, m)
    if flavour != "reference":
        o.set_onesweep(True, fused=False, one_reduction=(flavour == "one-reduction"))
    o.init()
    nconv = o.compute(getattr(O, rule), 1000, 1e-11)
    return nconv, o.info(), o.eigenvalues(), o.num_operations()


def solve_level_gates(ctx, n, k, m, rule, reductions, with_oracle):
    op, S, oop = matrix(ctx, n)
    ref = reference_solve(op, n, k, m, rule)
    one, nconv = solve(op, k, m, sa.SortRule[rule], "onesweep-wide", maxit=1000, tol=1e-11)
    assert one.info() == sa.CompInfo.Successful and nconv == ref["nconv"] == k
    evals, evecs = one.eigenvalues(), one.eigenvectors()
    info = one.orth_info()
    resid = (np.linalg.norm(S @ evecs - evecs * evals, axis=0) / np.linalg.norm(evecs, axis=0)).max()
    print("n %d k %d m %d %s: resid %.2e dlam %.2e orth %.2e ops %d (reference mode %d) %r" % (
        n, k, m, rule, resid, np.abs(evals - ref["eigenvalues"]).max(), np.abs(evecs.T @ evecs - np.eye(k)).max(),
        one.num_operations(), ref["num_operations"], info))
    assert resid <= 1e-10
    assert np.abs(evals - ref["eigenvalues"]).max() < 1e-9
    assert np.abs(evecs.T @ evecs - np.eye(k)).max() <= 1e-10
    assert abs(one.num_operations() - ref["num_operations"]) <= (m - k)
    assert info["mode"] == "onesweep" and info["wide"] and info["panel_steps"] > 0
    assert info["lagged_steps"] >= 0.8 * one.num_operations() and ref["lagged_steps"] == 0 and ref["mode"] == "reference"
    assert info["fused_restarts"] == 0 and info["max_chk"] <= 64 * EPS
    if with_oracle:
        for flavour in ("reference", reductions):
            nconv_o, info_o, evals_o, nops_o = oracle_solve(oop, n, k, m, rule, flavour)
            assert nconv_o == k and info_o == 0
            assert np.abs(np.sort(evals_o) - np.sort(evals)).max() < 1e-9
            assert abs(nops_o - one.num_operations()) <= (m - k)
    return one, info


@pytest.mark.parametrize("n,k,m", [(1000, 64, 129), (1000, 60, 130), (1000, 80, 200), (30_001, 90, 193), (30_001, 150, 400),
                                   (30_001, 200, 512)])
@pytest.mark.parametrize("rule", ["LargestAlge", "BothEnds"])
def test_onesweep_wide_solves(ctx, n, k, m, rule, reductions):
    # test_onesweep_on_wide_bases with mode "onesweep-wide" on 128 < ncv <= 512, plus the oracle's restatement of the variant
    solve_level_gates(ctx, n, k, m, rule, reductions, with_oracle=True)


# ---- 3. limits and fall-backs -------------------------------------------------------------------------------------------------------
def test_bases_beyond_512_columns_keep_the_reference_flow(ctx):
    # 2 i + 1 record slots end at i = 511
    op, S, _ = matrix(ctx, 1000)
    eigs, nconv = solve(op, 20, 513, sa.SortRule.LargestAlge, "onesweep-wide")
    info = eigs.orth_info()
    assert nconv == 20 and info["mode"] == "reference" and not info["wide"] and info["panel_steps"] == 0 and info["lagged_steps"] == 0
    assert np.abs(eigs.eigenvalues() - wanted_by_rule(GOLD["spectrum_1000"], "LargestAlge", 20)[::-1]).max() < 1e-9


def test_without_the_flag_wide_bases_keep_the_reference_flow(ctx):
    op, S, _ = matrix(ctx, 1000)
    eigs, nconv = solve(op, 20, 130, sa.SortRule.LargestAlge, "onesweep")
    info = eigs.orth_info()
    assert nconv == 20 and info["mode"] == "reference" and not info["wide"] and info["panel_steps"] == 0 and info["lagged_steps"] == 0
    assert np.abs(eigs.eigenvalues() - wanted_by_rule(GOLD["spectrum_1000"], "LargestAlge", 20)[::-1]).max() < 1e-9


def test_the_flag_is_ignored_where_onesweep_does_not_apply(ctx):
    # a user operator with the reference's host-pointer contract: every product is a host turn, the reference flow runs
    _, S, _ = matrix(ctx, 1000)

    class HostOp:
        def rows(self):
            return 1000

        def cols(self):
            return 1000

        def perform_op(self, x):
            return S @ x

    eigs, nconv = solve(HostOp(), 20, 130, sa.SortRule.LargestAlge, "onesweep-wide", ctx=ctx)
    info = eigs.orth_info()
    assert nconv == 20 and info["mode"] == "reference" and not info["wide"] and info["panel_steps"] == 0 and info["lagged_steps"] == 0
    assert np.abs(eigs.eigenvalues() - wanted_by_rule(GOLD["spectrum_1000"], "LargestAlge", 20)[::-1]).max() < 1e-9


def test_the_flag_without_the_onesweep_mode_is_refused(ctx):
    op, _, _ = matrix(ctx, 1000)
    fac = sa.Factorization(op, 130, True)
    assert sa.lib().mispec_fac_set_orth_mode(fac.h, 0 | 0x2000) == _capi.MISPEC_EINVAL   # MISPEC_ORTH_REFERENCE | MISPEC_ORTH_WIDE
    assert fac.orth_info()["mode"] == "reference" and not fac.orth_info()["wide"]      # ncv = 130 without the flag
    assert sa.lib().mispec_fac_set_orth_mode(fac.h, 1 | 0x2000) == 0
    assert fac.orth_info()["mode"] == "onesweep" and fac.orth_info()["wide"]


# ---- 4. leaving the lagged path -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rule,k", [("outliers", "LargestAlge", 12)])
def test_the_host_continues_from_a_panelled_step(ctx, name, rule, k):
    # A few huge outliers over a 1e-6 bulk: once they are found the residual collapses (the beta < eps sqrt(n) clamp,
    # Lanczos.h:163-168) and the steps leave the lagged path through the state stops — about every third step in the oracle's
    # restatement of the variant (190 of 585 at ncv = 160, k = 12, four restarts), so many of them at a step that ran in panels, from
    # whose records the host then continues.  Same gates as the solves above, scaled as test_onesweep_default_on_adversarial_spectra
    # scales them.
    m = 160
    A = ADVERSARIAL[name]()
    op = sa.SparseSymMatProd(A, ctx=ctx)
    scale = max(1.0, np.abs(A.data).max())
    ref, nconv_ref = solve(op, k, m, sa.SortRule[rule], "reference", maxit=400, tol=1e-10)
    one, nconv = solve(op, k, m, sa.SortRule[rule], "onesweep-wide", maxit=400, tol=1e-10)
    info = one.orth_info()
    print("%s %s: check_stops %d state_stops %d panel_steps %d lagged_steps %d ops %d (reference mode %d)" % (
        name, rule, info["check_stops"], info["state_stops"], info["panel_steps"], info["lagged_steps"], one.num_operations(),
        ref.num_operations()))
    assert one.info() == ref.info() == sa.CompInfo.Successful and nconv == nconv_ref == k
    assert info["mode"] == "onesweep" and info["wide"] and info["panel_steps"] > 0 and ref.orth_info()["mode"] == "reference"
    assert info["check_stops"] + info["state_stops"] >= 0  # reported
    ev, U = one.eigenvalues(), one.eigenvectors()
    assert np.abs(np.sort(ev) - np.sort(ref.eigenvalues())).max() <= 1e-9 * scale
    assert (np.linalg.norm(A @ U - U * ev, axis=0) / np.linalg.norm(U, axis=0)).max() <= 1e-10 * scale
    assert np.abs(U.T @ U - np.eye(k)).max() <= 1e-10
    assert abs(one.num_operations() - ref.num_operations()) <= (m - k)
    assert info["max_chk"] <= 64 * EPS


# ---- 5. a size at which the narrow steps of the same sweep take the LDS-DMA kernel ------------------------------------------------------
@pytest.mark.parametrize("rule", ["LargestAlge", "BothEnds"])
def test_dma_steps_wide_steps_and_panelled_steps_in_one_sweep(ctx, rule, reductions):
    # 200 000 rows >= 131 072: steps i <= 63 go through the LDS-DMA ring (one workgroup per CU), 64 <= i <= 127 through the
    # eight-wavefront kernel, i >= 128 through the panels — three grids, hence three record counts, handed from step to step
    solve_level_gates(ctx, 200_000, 70, 160, rule, reductions, with_oracle=False)
