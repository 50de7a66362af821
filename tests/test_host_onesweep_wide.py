"""The opt-in one-sweep steps on wide bases (MISPEC_ORTH_WIDE, include/mispec.h), the parts that need no GPU: the option value,
the Python names of the mode and the declared symbols."""
import os
import re

import pytest

import spectra_amd as sa
from spectra_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = 0x2000


def test_the_option_value_is_accepted_and_read_back():
    try:
        sa.set_option("orth", "onesweep-wide")
        assert sa.get_option("orth") == "onesweep-wide"
    finally:
        sa.set_option("orth", None)
    assert sa.get_option("orth") == os.environ.get("MISPEC_ORTH")
    with pytest.raises(ValueError, match="accepted: .*onesweep-wide"):  # the refusal lists the accepted values, the new one among them
        sa.set_option("orth", "onesweep-wider")


def test_the_mode_names_carry_the_flag():
    assert sa.ORTH_MODES["onesweep-wide"] == 1 | WIDE
    assert sa.ORTH_MODES["onesweep-wide-onered"] == 1 | WIDE | 0x800
    assert sa.ORTH_MODES["onesweep-wide-twored"] == 1 | WIDE | 0x1000
    # no other name carries it, and the flag collides with none of the others
    for name, value in sa.ORTH_MODES.items():
        assert bool(value & WIDE) == name.startswith("onesweep-wide"), name
    assert not any(WIDE & f for f in (0xFF, 0x100, 0x200, 0x400, 0x800, 0x1000))


def test_the_mode_value_round_trips():
    for name in ("onesweep-wide", "onesweep-wide-onered", "onesweep-wide-twored"):
        value = sa._orth_mode_value(name)
        assert value == sa.ORTH_MODES[name] and sa._orth_mode_value(value) == value
    with pytest.raises(ValueError, match="onesweep-wide"):
        sa._orth_mode_value("onesweep-widest")
    with pytest.raises(ValueError):
        sa._orth_mode_value(WIDE)  # the flag without the one-sweep mode is no mode


def test_the_header_declares_the_flag_and_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "mispec.h")).read()
    assert re.search(r"\bMISPEC_ORTH_WIDE\s*=\s*0x2000\b", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym, handle in (("mispec_fac_panel_steps", "mispec_fac"), ("mispec_symeigs_panel_steps", "mispec_symeigs")):
        assert re.search(r"\bint\s+%s\s*\(\s*const\s+%s\s*\*\s*\w+\s*,\s*int64_t\s*\*\s*steps\s*\)\s*;" % (sym, handle), code), sym
        assert sym in _capi.SIGNATURES and hasattr(sa.lib(), sym)
    # the comment that said "wider bases" are ignored now names the flag
    assert "ignored otherwise" in hdr and "unless MISPEC_ORTH_WIDE is set" in hdr
    cpp = open(os.path.join(ROOT, "include", "Spectra", "HermEigsBase.h")).read()
    assert "MISPEC_ORTH_WIDE" in cpp


def test_the_new_entry_points_refuse_null_arguments():
    # (that MISPEC_ORTH_REFERENCE | MISPEC_ORTH_WIDE is refused on a live factorisation needs a GPU: test_gpu_onesweep_panels.py)
    assert sa.lib().mispec_fac_panel_steps(None, None) == _capi.MISPEC_EINVAL
    assert sa.lib().mispec_symeigs_panel_steps(None, None) == _capi.MISPEC_EINVAL
