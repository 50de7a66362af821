"""tests/zprim_checks.py on the host build of the complex factorisation's control flow (tests/cpp/zfac_host_capi.cpp): no GPU.
What this run establishes is that the probe, its long-double references, its bounds and its sensitivity conditions are right
on a backend whose primitives are plain loops; tests/test_gpu_zprims.py applies the same module to the HIP kernels.

The host backend sums the n rows of X^H y in one running sum, so its bound is gamma_(n + 3), not the kernels'
gamma_(29 + ceil(nchunks / 256)).  At n = 10^7 + 3 that bound (1.1e-9) is wider than the weight of one row (1e-7) / 100 and the
sensitivity condition of the probe cannot hold: the host run stops at n = 524 289; the GPU run covers every size."""
import ctypes as C
import os
import subprocess

import pytest

import zfac_checks as Z
import zprim_checks as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("zprims") / "libzfac_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "spectra_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "zfac_host_capi.cpp"), "-o", so])
    lib = C.CDLL(so)
    i64, vp = C.c_int64, C.c_void_p
    dp, vpp = C.POINTER(C.c_double), C.POINTER(C.c_void_p)
    lib.mispec_zdense_upload.argtypes = [vp, i64, i64, dp, i64, C.c_int, C.c_char, vpp]
    for nm in ("mispec_zdense_destroy", "mispec_zfac_destroy", "mispec_zfac_subspace_dim"):
        getattr(lib, nm).argtypes = [vp]
    lib.mispec_zfac_create_dense.argtypes = [vp, vp, C.c_int, C.c_int, vpp]
    lib.mispec_zfac_create_op.argtypes = [vp, Z.op_fn, vp, i64, C.c_int, C.c_int, vpp]
    lib.mispec_zfac_init.argtypes = [vp, dp, C.POINTER(i64)]
    lib.mispec_zfac_factorize.argtypes = [vp, C.c_int, C.c_int, C.POINTER(i64)]
    lib.mispec_zfac_f_norm.argtypes = [vp, dp]
    lib.mispec_zfac_get_H.argtypes = [vp, dp]
    lib.mispec_zfac_get_V.argtypes = [vp, C.c_int, dp]
    lib.mispec_zfac_get_f.argtypes = [vp, dp]
    return lib


@pytest.mark.parametrize("n", [n for n in P.PROBE_SIZES if n <= 524289])
def test_probe_on_the_host_backend(hostlib, n):
    P.run_probe(hostlib, None, n, P.host_dot_roundings)


@pytest.mark.parametrize("n,m", P.STEP_SHAPES)
def test_single_steps_on_the_host_backend(hostlib, n, m):
    P.run_steps(hostlib, None, n, m)
