"""Path selection of the shift-and-invert operators, the part that needs no GPU: mispec_symshift_path names the path of (n,
half-bandwidth) — 0 the explicit inverse, 1 the partitioned chunk path, 2 the block-tridiagonal path (csrc/shiftsolve.hpp shift_path,
csrc/shift_blocktri.hip) — and mispec_symshift_path_info refuses a NULL handle without touching a device."""
import ctypes as C

import pytest

import spectra_amd as sa
from spectra_amd import _capi


@pytest.mark.parametrize("n,b,path", [(4096, 65, 0), (100, 99, 0), (3000, 8, 1), (4097, 64, 1), (4097, 65, 2), (1_000_000, 512, 2),
                                      (4097, 513, _capi.MISPEC_EINVAL)])
def test_path_of_a_shape(n, b, path):
    assert sa.lib().mispec_symshift_path(n, b) == path


def test_the_refusal_names_both_limits():
    assert sa.lib().mispec_symshift_path(4097, 513) == _capi.MISPEC_EINVAL
    msg = sa.lib().mispec_last_error().decode()
    assert "only banded" in msg and "64" in msg and "512" in msg, msg


def test_paths_agree_with_the_level_plan():
    """the chunk path is exactly where the level plan has levels; the level plan describes that path only"""
    lib = sa.lib()
    for n, b in [(50, 1), (3000, 8), (4097, 9), (4097, 64), (100_000, 64), (5000, 65), (4096, 65), (100, 99), (5000, 512), (5000, 513)]:
        path = lib.mispec_symshift_path(n, b)
        levels = lib.mispec_symshift_level_plan(n, b, 0, None, None, None, None)
        assert (path == 1) == (levels >= 1), (n, b, path, levels)
        assert (path == 0) == (levels == 0), (n, b, path, levels)
        if path in (2, _capi.MISPEC_EINVAL):
            assert levels == _capi.MISPEC_EINVAL, (n, b, path, levels)


@pytest.mark.parametrize("n,b", [(0, 3), (-5, 3), (100, -1)])
def test_bad_arguments(n, b):
    assert sa.lib().mispec_symshift_path(n, b) == _capi.MISPEC_EINVAL


def test_symbols_and_null_handle():
    lib = sa.lib()
    assert lib.mispec_symshift_path is not None and lib.mispec_symshift_path_info is not None
    path, rows, blocks, nbytes = C.c_int(7), C.c_int64(7), C.c_int64(7), C.c_int64(7)
    rc = lib.mispec_symshift_path_info(None, C.byref(path), C.byref(rows), C.byref(blocks), C.byref(nbytes))
    assert rc == _capi.MISPEC_EINVAL
    assert (path.value, rows.value, blocks.value, nbytes.value) == (7, 7, 7, 7)  # nothing is written
