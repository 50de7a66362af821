"""CPU-only checks of the drop-in boundary: the C-ABI library loads, exports every symbol the header
declares, fails loudly without a GPU, and its pure host logic (row partition, error classes) works."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import spectra_amd as sa
from spectra_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols(which=("mispec.h", "mispec_extras.h")):
    names = set()
    for h in which:
        hdr = open(os.path.join(ROOT, "include", h)).read()
        hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
        names |= set(re.findall(r"\b(mispec_[A-Za-z0-9_]+)\s*\(", hdr))
    return names - {"mispec_op_fn"}


def test_library_exports_every_declared_symbol():
    lib = sa.lib()
    names = header_symbols()
    assert len(names) >= 60
    # two libraries (round 6): the Davidson solver and the complex factorisation live in libmispec_extras.so, built on
    # libmispec.so; the hot-path library must not export them, the extras library must export nothing else
    core_lib = C.CDLL(_capi.LIB_PATH)
    extras_lib = C.CDLL(_capi.EXTRAS_LIB_PATH)
    for nm in names:
        assert hasattr(lib, nm), f"{nm} declared in include/mispec.h / mispec_extras.h but not exported"
        in_extras = nm.startswith(_capi.EXTRAS_PREFIXES)
        assert hasattr(extras_lib if in_extras else core_lib, nm), nm
        if in_extras:
            with pytest.raises(AttributeError):
                getattr(core_lib, nm)
    assert sum(nm.startswith(_capi.EXTRAS_PREFIXES) for nm in names) >= 28
    assert names == set(_capi.SIGNATURES), names ^ set(_capi.SIGNATURES)
    assert b"gfx950" in lib.mispec_version()
    # the thin shim of the hot path knows nothing of the components outside it
    core = header_symbols(("mispec.h",))
    assert not [nm for nm in core if re.search(r"dense|davidson|complex_shift|set_shift_complex|geigs_shift", nm)]
    assert len(core) + len(header_symbols(("mispec_extras.h",))) == len(names)


def test_no_silent_cpu_fallback():
    import torch  # plumbing only: tells us whether this box has a GPU

    if torch.cuda.is_available():
        pytest.skip("GPU present: the failure path cannot be exercised")
    with pytest.raises(sa.MispecError, match="no HIP device"):
        sa.Context(0)


def test_error_classes_map_like_the_reference():
    lib = sa.lib()
    h = C.c_void_p()
    assert lib.mispec_ctx_create(0, None, None) == _capi.MISPEC_EINVAL  # NULL out pointer -> invalid argument
    assert b"NULL" in lib.mispec_last_error()
    assert lib.mispec_fac_factorize(None, 1, 2, None) == _capi.MISPEC_EINVAL
    assert lib.mispec_symeigs_info(None) == int(sa.CompInfo.NotComputed)
    with pytest.raises(ValueError):
        _capi.check(lib.mispec_csr_upload(None, 1, 1, None, None, None, C.byref(h)))


def test_row_partition():
    # equal even-sized blocks; the last ranks may be short or empty; blocks tile [0, n)
    for n, world in [(10, 4), (10**7, 8), (1001, 2), (5, 8), (128, 1), (7, 3)]:
        blk = sa.lib().mispec_shard_block(n, world)
        assert world == 1 or blk % 2 == 0
        assert blk * world >= n
        edges = [sa.shard_range(n, world, r) for r in range(world)]
        assert edges[0][0] == 0 and edges[-1][1] == n
        for (b0, e0), (b1, e1) in zip(edges, edges[1:]):
            assert e0 == b1 and b0 <= e0
        assert all(e - b <= blk for b, e in edges)
    with pytest.raises(ValueError):
        sa.shard_range(10, 4, 4)


def test_python_mirror_enums_match_cpp():
    hdr = open(os.path.join(ROOT, "include", "Spectra", "Util", "SelectionRule.h")).read()
    body = re.search(r"enum class SortRule\s*\{(.*?)\};", hdr, flags=re.S).group(1)
    names = re.findall(r"^\s*([A-Za-z]+),?\s*//", body, flags=re.M)
    assert names == [r.name for r in sa.SortRule]
    import oracle
    assert [getattr(oracle, r.name) for r in sa.SortRule] == [int(r) for r in sa.SortRule]


def test_options_replace_the_environment_switches():
    # mispec_set_option / mispec_get_option (round 6): one reader for every switch; an unknown name is refused, so that a typo
    # cannot pass for a measurement; a name that has not been set falls back to MISPEC_<NAME> (the tests' override)
    assert sa.get_option("orth_kernel") in (None, os.environ.get("MISPEC_ORTH_KERNEL"))
    try:
        sa.set_option("orth_kernel", "reg")
        assert sa.get_option("orth_kernel") == "reg"
        sa.set_option("orth_kernel", "dma")
        assert sa.get_option("orth_kernel") == "dma"
    finally:
        sa.set_option("orth_kernel", None)
    assert sa.get_option("orth_kernel") in (None, os.environ.get("MISPEC_ORTH_KERNEL"))
    with pytest.raises(ValueError):
        sa.set_option("orth_kernal", "dma")
    with pytest.raises(ValueError):
        sa.set_option("vq_out_of_place", "1")  # (a name registered in round 6's first session and never read: removed)
    os.environ["MISPEC_SPEC_CORR"] = "3"
    try:
        assert sa.get_option("spec_corr") == "3"
        sa.set_option("spec_corr", "1")
        assert sa.get_option("spec_corr") == "1"
    finally:
        sa.set_option("spec_corr", None)
        del os.environ["MISPEC_SPEC_CORR"]


# every value of the option table (include/mispec.h) with a meaning; each one is accepted and read back as set
OPTION_VALUES = {
    "orth": ["onesweep", "onesweep-eager", "reference"], "one_reduction": ["1", "0"], "orth_kernel": ["dma", "dma2", "reg"],
    "host_turn": ["fast", "copy"], "small": ["host", "host-serial", "device"], "restart_sync": ["0", "1"],
    "host_steps": ["0", "1"], "overlap": ["0", "1"], "csr_win": ["0", "1"], "spec_corr": ["1", "2", "3", "4"],
    "exchange": ["allgather", "halo"], "reorder": ["auto", "rcm", "none"], "spmv_staged": ["auto", "0", "1"],
    "spmv_tiles": ["auto", "0", "1"], "host_threads": ["1", "3", "64", "1000"],
    "shift": ["lds=0", "lds=1", "batch=8", "batch=16", "batch=32", "lanes=8", "lanes=16", "lanes=32", "lanes=64", "block_inverse=0",
              "block_inverse=256", "factor=host", "factor=device", "wave=0", "wave=1", "profile=0", "profile=1", "lanes=16,batch=16",
              "lds=0,batch=8,lanes=32,block_inverse=0,factor=host,wave=0,profile=1"],
}


def test_every_option_value_is_accepted_and_read_back():
    for name, values in OPTION_VALUES.items():
        try:
            for v in values:
                sa.set_option(name, v)
                assert sa.get_option(name) == v
        finally:
            sa.set_option(name, None)
        assert sa.get_option(name) == os.environ.get("MISPEC_" + name.upper())


@pytest.mark.parametrize("name,value", [
    ("orth_kernel", "dam"), ("orth_kernel", "dmac"), ("orth_kernel", "dmap"), ("orth_kernel", "dmacp"), ("orth", "eager"),
    ("small", "Device"), ("small", ""), ("host_turn", "slow"), ("exchange", "ring"), ("reorder", "amd"), ("spmv_tiles", "2"),
    ("one_reduction", "2"), ("overlap", "off"), ("spec_corr", "9"), ("spec_corr", "0"), ("spec_corr", "-1"), ("spec_corr", "2x"),
    ("host_threads", "0"), ("host_threads", "abc"), ("host_threads", " 3"), ("host_threads", "99999999999"), ("shift", "lanes=7"),
    ("shift", "bogus=1"), ("shift", "lds"), ("shift", "lds=0,lds=1"), ("shift", "block_inverse=-1"), ("shift", "factor=1"),
    ("shift", "lds=0,"), ("shift", "")])
def test_an_option_value_without_a_meaning_is_refused(name, value):
    # refused with the accepted values in the message, and the value in effect stays what it was
    before = sa.get_option(name)
    with pytest.raises(ValueError, match=r"mispec_set_option: '.*' is not a value of option %s .*; accepted: " % name):
        sa.set_option(name, value)
    assert sa.get_option(name) == before


def test_the_accepted_values_are_listed_when_one_is_refused():
    for name, accepted in [("orth_kernel", "dma | dma2 | reg"), ("spec_corr", "an integer from 1 to 4"),
                           ("host_threads", "an integer from 1 on"), ("shift", "lanes=8|16|32|64")]:
        with pytest.raises(ValueError) as e:
            sa.set_option(name, "x")
        assert accepted in str(e.value), str(e.value)


@pytest.mark.parametrize("name", ["vq", "csr_win_iters", "csr_win_pf", "csr_win_nt", "kernel_probe", "dia2", "orth_kernal", ""])
def test_a_removed_or_unknown_option_name_is_refused(name):
    with pytest.raises(ValueError, match="unknown option"):
        sa.set_option(name, "1")
    assert sa.get_option(name) is None


def test_an_invalid_environment_value_is_refused_when_it_is_read():
    # MISPEC_<NAME> goes through the option's check when the library reads it: the entry point that reads it fails with
    # MISPEC_EINVAL naming the variable (a Python ValueError), no exception crosses the C boundary; get_option shows the raw string
    import subprocess
    import sys

    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import scipy.sparse as sp, spectra_amd as sa\n"
        "M = sp.random(300, 300, density=0.05, format='csc', random_state=0)\n"
        "print('get_option', sa.get_option('host_threads'))\n"
        "print('ingest_threads', sa.lib().mispec_ingest_threads())\n"
        "try:\n"
        "    sa.mirror_triangle_host(M, 'L')\n"
        "    print('accepted')\n"
        "except ValueError as e:\n"
        "    print('ValueError', e)\n"
    ) % ROOT
    for value, refused in (("abc", True), ("0", True), ("2", False), ("", False)):
        env = dict(os.environ, MISPEC_HOST_THREADS=value)
        r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert lines[0] == "get_option %s" % (value or None)
        threads = int(lines[1].split()[1])
        if refused:
            assert threads == _capi.MISPEC_EINVAL
            assert lines[2].startswith("ValueError MISPEC_HOST_THREADS: '%s' is not a value of option host_threads" % value), lines
        else:
            assert threads >= 1 and lines[2] == "accepted", lines
            assert value == "" or threads <= int(value)
