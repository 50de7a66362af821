"""SparseSymMatProd::from_device of the header-only C++ API: tests/cpp/device_ingest.cpp puts a triangle into device memory with
hipMalloc / hipMemcpy, builds the operator from the addresses and compares a solve, exactly, with the host-built operator."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_program():
    """Compiled here, the way __graft_entry__.build_cpp_tests compiles dropin_symeigs.cpp, but with hipcc: the program itself
    calls the HIP runtime (host code only; the headers of include/Spectra contain no device code)."""
    cpp = os.path.join(ROOT, "tests", "cpp")
    src, exe = os.path.join(cpp, "device_ingest.cpp"), os.path.join(cpp, "device_ingest.bin")
    lib = os.path.join(ROOT, "spectra_amd", "libmispec.so")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(lib)):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), src,
                               "-L" + os.path.join(ROOT, "spectra_amd"), "-lmispec_extras", "-lmispec",
                               "-Wl,-rpath,$ORIGIN/../../spectra_amd", "-o", exe])
    return exe


def test_cpp_from_device_program():
    exe = build_program()
    out = subprocess.run(["timeout", "-k", "10", "120", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    assert "ALL PASSED" in out.stdout and out.stdout.count("lambda[") == 4
