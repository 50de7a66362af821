"""Option `dia_sym` of the diagonal SpMV format, the parts that need no GPU: the host-only rule that says which diagonals may be
mirrored (mispec_dia_sym_plan), the option's accepted values, and the new symbols of the C API."""
import os

import pytest

import spectra_amd as sa
from spectra_amd import _capi

M_BAND = (1, 2, 3, 1000, 1001, 100000, 100001)
OFFSETS = sorted([0] + [s * k for k in M_BAND for s in (1, -1)])


def mirrored(offsets, reach):
    flags, lead = sa.dia_sym_plan(offsets, reach)
    return sorted(o for o, f in zip(offsets, flags) if f), lead


def test_plan_near_diagonals_within_reach():
    for reach in (1001, 2048, 99999):
        offs, lead = mirrored(OFFSETS, reach)
        assert offs == [-1001, -1000, -3, -2, -1]
        assert lead == -(-1001 // 256) == 4


def test_plan_all():
    offs, lead = mirrored(OFFSETS, -1)
    assert offs == sorted(-k for k in M_BAND)
    assert lead == -(-100001 // 256) == 391
    assert mirrored(OFFSETS, 100001) == (offs, lead)  # the reach is inclusive
    assert mirrored(OFFSETS, 100000)[0] == sorted(-k for k in M_BAND if k <= 100000)


def test_plan_needs_the_partner_and_never_takes_the_main_diagonal():
    offs, lead = mirrored([-700, -5, -1, 0, 1, 7, 700], -1)
    assert offs == [-700, -1]  # -5 has no +5
    assert lead == 3
    assert mirrored([0], -1) == ([], 0)
    assert mirrored([-2, 0], -1) == ([], 0)
    assert mirrored([0, 1, 2], -1) == ([], 0)  # upper diagonals are the ones that stay
    assert mirrored(OFFSETS, 0) == ([], 0)


@pytest.mark.parametrize("kmax", [1, 255, 256, 257, 512, 513])
def test_plan_lead_blocks(kmax):
    flags, lead = sa.dia_sym_plan([-kmax, -1, 0, 1, kmax], -1)
    assert flags == [True, True, False, False, False]
    assert lead == (kmax + 255) // 256


def test_option_values():
    try:
        for v in ("auto", "0", "all"):
            sa.set_option("dia_sym", v)
            assert sa.get_option("dia_sym") == v
        for v in ("1", "near"):
            with pytest.raises(Exception) as e:
                sa.set_option("dia_sym", v)
            assert "auto | 0 | all" in str(e.value) and "dia_sym" in str(e.value)
            assert sa.get_option("dia_sym") == "all"  # a refused value changes nothing
    finally:
        sa.set_option("dia_sym", None)


def test_symbols():
    lib = sa.lib()
    for name in ("mispec_dia_sym_plan", "mispec_csr_dia_info"):
        assert name in _capi.SIGNATURES
        assert getattr(lib, name) is not None
    root = os.path.dirname(os.path.dirname(os.path.abspath(_capi.__file__)))
    with open(os.path.join(root, "include", "mispec.h")) as f:
        header = f.read()
    assert "mispec_dia_sym_plan(" in header and "mispec_csr_dia_info(" in header and "dia_sym " in header
