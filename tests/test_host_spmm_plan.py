"""The cut of a block product's k columns into panels (mispec_spmm_plan, spectra_amd/csrc/spmm.hip) and the option `spmm`
that caps the panel width — host arithmetic only, no device.  The block product itself runs the widths this function
returns, in this order (tests/test_gpu_spmm.py)."""
import ctypes as C

import pytest

import spectra_amd as sa
from spectra_amd import _capi

KS = range(0, 41)


# the widths `auto` keeps: those at which one panel measured faster than as many single products on both benchmark matrices
# (width 2 lost on M-band and is left to the forced values)
AUTO_WIDTHS = (8, 4)


def check_plan(widths, k, allowed):
    assert sum(widths) == k
    assert all(w in (8, 4, 2, 1) for w in widths)
    assert all(w in allowed or w == 1 for w in widths)
    assert widths == sorted(widths, reverse=True)            # non-increasing, so single columns come last
    # single columns are only what no allowed panel fits into any more: at most one when width 2 is allowed
    assert widths.count(1) < min(allowed)
    assert widths.count(1) <= 1 or 2 not in allowed


@pytest.mark.parametrize("k", KS)
def test_automatic_plan(k):
    assert sa.get_option("spmm") in (None, "auto")
    widths = sa.spmm_plan(k)
    check_plan(widths, k, AUTO_WIDTHS)
    assert widths == sa.spmm_plan(k, 0)
    assert widths.count(8) == k // 8 and widths.count(4) == (k % 8) // 4


@pytest.mark.parametrize("forced", [8, 4, 2])
@pytest.mark.parametrize("k", KS)
def test_forced_width_caps_the_panels(k, forced):
    widths = sa.spmm_plan(k, forced)
    check_plan(widths, k, [w for w in (8, 4, 2) if w <= forced])
    assert widths.count(1) <= 1                              # forced 8 / 4 / 2 all end in width 2: one single column at the most
    # greedy: as many panels of the cap as fit, then each narrower width at most once
    assert widths.count(forced) == k // forced
    assert all(widths.count(w) <= 1 for w in (8, 4, 2) if w < forced)


def test_the_cut_of_the_issue_examples():
    assert sa.spmm_plan(1, 8) == [1]
    assert sa.spmm_plan(13, 8) == [8, 4, 1]
    assert sa.spmm_plan(0, 8) == []
    assert sa.spmm_plan(23, 8) == [8, 8, 4, 2, 1]
    assert sa.spmm_plan(7, 4) == [4, 2, 1]
    assert sa.spmm_plan(7, 2) == [2, 2, 2, 1]


@pytest.mark.parametrize("k", KS)
def test_option_value_0_and_forced_single_columns_yield_k_ones(k):
    assert sa.spmm_plan(k, 1) == [1] * k
    try:
        sa.set_option("spmm", "0")
        assert sa.spmm_plan(k) == [1] * k
    finally:
        sa.set_option("spmm", None)


def test_the_option_is_what_an_unforced_plan_follows():
    try:
        for v in ("2", "4", "8"):
            sa.set_option("spmm", v)
            for k in KS:
                assert sa.spmm_plan(k) == sa.spmm_plan(k, int(v))
        sa.set_option("spmm", "auto")
        auto = [sa.spmm_plan(k) for k in KS]
    finally:
        sa.set_option("spmm", None)
    assert auto == [sa.spmm_plan(k) for k in KS]


@pytest.mark.parametrize("forced", [-1, 3, 5, 6, 7, 16])
def test_a_bad_forced_width_is_refused(forced):
    with pytest.raises(ValueError, match="mispec_spmm_plan"):
        sa.spmm_plan(5, forced)


def test_negative_k_and_a_too_small_capacity_are_refused():
    with pytest.raises(ValueError, match="mispec_spmm_plan"):
        sa.spmm_plan(-1)
    out = (C.c_int * 4)()
    count = C.c_int(-7)
    lib = sa.lib()
    assert lib.mispec_spmm_plan(13, 8, out, 2, C.byref(count)) == _capi.MISPEC_EINVAL   # 8 + 4 + 1: three panels
    assert b"mispec_spmm_plan" in lib.mispec_last_error() and count.value == -7
    assert lib.mispec_spmm_plan(13, 8, out, 3, C.byref(count)) == 0 and count.value == 3 and list(out)[:3] == [8, 4, 1]
    assert lib.mispec_spmm_plan(0, 8, None, 0, C.byref(count)) == 0 and count.value == 0
    assert lib.mispec_spmm_plan(3, 8, out, 4, None) == _capi.MISPEC_EINVAL


def test_option_spmm_round_trips_and_refuses_other_values():
    before = sa.get_option("spmm")
    try:
        for v in ("auto", "0", "2", "4", "8"):
            sa.set_option("spmm", v)
            assert sa.get_option("spmm") == v
        for bad in ("3", "on"):
            with pytest.raises(ValueError, match=r"is not a value of option spmm .*; accepted: auto \| 0 \| 2 \| 4 \| 8"):
                sa.set_option("spmm", bad)
            assert sa.get_option("spmm") == "8"
    finally:
        sa.set_option("spmm", None)
    assert sa.get_option("spmm") == before
