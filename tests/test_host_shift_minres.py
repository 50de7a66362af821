"""Host side of the iterative shift-solve path (no GPU): option shift_solver, the path a solver kind selects, the NULL-handle
refusals of the new entry points."""
import pytest

import spectra_amd as sa
from spectra_amd import _capi

DIRECT, AUTO, ITERATIVE = 0, 1, 2


@pytest.fixture
def restore_options():
    yield
    sa.set_option("shift_solver", None)
    sa.set_option("shift", None)


def test_option_shift_solver(restore_options, monkeypatch):
    monkeypatch.delenv("MISPEC_SHIFT_SOLVER", raising=False)
    assert sa.get_option("shift_solver") is None
    for value in ("direct", "auto", "iterative"):
        sa.set_option("shift_solver", value)
        assert sa.get_option("shift_solver") == value
    for bad in ("minres", "Direct", "1", ""):
        with pytest.raises(ValueError, match=r"accepted: direct \| auto \| iterative"):
            sa.set_option("shift_solver", bad)
    assert sa.get_option("shift_solver") == "iterative"  # a refused value changes nothing
    sa.set_option("shift_solver", None)
    assert sa.get_option("shift_solver") is None


def test_option_selects_the_default_kind(restore_options, monkeypatch):
    monkeypatch.delenv("MISPEC_SHIFT_SOLVER", raising=False)
    lib = sa.lib()
    assert lib.mispec_symshift_solver_path(6000, 513, -1) == _capi.MISPEC_EINVAL  # unset: direct
    sa.set_option("shift_solver", "auto")
    assert lib.mispec_symshift_solver_path(6000, 513, -1) == 3 and lib.mispec_symshift_solver_path(5000, 512, -1) == 2
    assert lib.mispec_symshift_solver_path(6000, 513, DIRECT) == _capi.MISPEC_EINVAL  # the argument overrides the option
    sa.set_option("shift_solver", None)
    monkeypatch.setenv("MISPEC_SHIFT_SOLVER", "iterative")
    assert lib.mispec_symshift_solver_path(5000, 512, -1) == 3
    assert sa.shift_solver_path(5000, 512) == 3 and sa.shift_solver_path(5000, 512, "direct") == 2


@pytest.mark.parametrize("n,b,direct", [(4097, 513, None), (6000, 513, None), (5000, 512, 2), (4096, 4000, 0), (1, 0, 1)])
def test_solver_path(n, b, direct):
    lib = sa.lib()
    refused = _capi.MISPEC_EINVAL
    assert lib.mispec_symshift_solver_path(n, b, DIRECT) == (refused if direct is None else direct)
    assert lib.mispec_symshift_solver_path(n, b, DIRECT) == lib.mispec_symshift_path(n, b)
    assert lib.mispec_symshift_solver_path(n, b, AUTO) == (3 if direct is None else direct)
    assert lib.mispec_symshift_solver_path(n, b, ITERATIVE) == 3
    if direct is None:
        with pytest.raises(ValueError, match="only banded"):
            sa.shift_solver_path(n, b, "direct")


def test_the_pure_path_is_unchanged():
    lib = sa.lib()
    assert lib.mispec_symshift_path(4097, 513) == _capi.MISPEC_EINVAL
    assert "only banded" in lib.mispec_last_error().decode()
    assert lib.mispec_symshift_path(5000, 512) == 2


def test_bad_arguments():
    lib = sa.lib()
    for n, b, solver in [(0, 0, AUTO), (10, -1, AUTO), (10, 1, 3), (10, 1, -2)]:
        assert lib.mispec_symshift_solver_path(n, b, solver) == _capi.MISPEC_EINVAL
    with pytest.raises(ValueError, match="unknown shift solver"):
        sa.shift_solver_path(10, 1, "minres")


def test_null_handles_are_refused():
    lib = sa.lib()
    assert lib.mispec_symshift_iterative_info(None, None, None, None, None, None, None) == _capi.MISPEC_EINVAL
    assert "NULL" in lib.mispec_last_error().decode()
    assert lib.mispec_symshift_set_iterative(None, 0.0, 0) == _capi.MISPEC_EINVAL
    assert "NULL" in lib.mispec_last_error().decode()


def test_minres_check_key(restore_options):
    for value in ("minres_check=1", "minres_check=16", "minres_check=64", "lds=0,minres_check=8"):
        sa.set_option("shift", value)
        assert sa.get_option("shift") == value
    for bad in ("minres_check=0", "minres_check=65", "minres_check=x", "minres_check=1,minres_check=2"):
        with pytest.raises(ValueError, match="minres_check=<integer from 1 to 64>"):
            sa.set_option("shift", bad)
