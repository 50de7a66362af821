"""GenEigsComplexShiftSolver<SparseGenComplexShiftSolve<double>> on the iterative path (ShiftSolver::Auto) used from C++:
tests/cpp/shift_zbicgstab_dropin.cpp (a normal non-symmetric matrix on a 20 x 21 x 22 grid against its closed-form complex
eigenvalues), compiled here by a plain host compiler twice — on include/Spectra alone, and with tests/cpp/eigen_lite in front of it
— and run on the GPU."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "shift_zbicgstab_dropin.cpp")


def compile_program(exe, extra):
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall"] + extra + ["-I" + os.path.join(ROOT, "include"), SRC,
                           "-L" + os.path.join(ROOT, "spectra_amd"), "-lmispec_extras", "-lmispec",
                           "-Wl,-rpath," + os.path.join(ROOT, "spectra_amd"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("shift_zbicgstab_cpp")
    return {"plain": compile_program(str(d / "shift_zbicgstab_dropin.bin"), []),
            "eigen_lite": compile_program(str(d / "shift_zbicgstab_dropin_eigenapi.bin"),
                                          ["-I" + os.path.join(ROOT, "tests", "cpp", "eigen_lite")])}


@pytest.mark.parametrize("which", ["plain", "eigen_lite"])
def test_shift_zbicgstab_dropin_program(programs, which):
    out = subprocess.run([programs[which]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    assert "ALL PASSED" in out.stdout and out.stdout.count("||AX-XD||") == 1, out.stdout
