"""Host side of the complex-shift iterative path of the general operator (no GPU): the path rule of
mispec_symshift_create_general_complex, the refusals of the new entry points and arguments, the numpy restatement of the iteration
(shift_cplx_checks.zbicgstab_reference) against SuperLU on every fixture of tests/test_gpu_shift_zbicgstab.py — which shows that
the bars and the iteration-count caps of that file are attainable — and the closed form of the fixture's spectrum."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import shift_cplx_checks as Z
import spectra_amd as sa
from spectra_amd import _capi

DIRECT, AUTO, ITERATIVE = 0, 1, 2
REFUSED = _capi.MISPEC_EINVAL


@pytest.mark.parametrize("n,direct,auto", [(1, 0, 0), (4096, 0, 0), (4097, REFUSED, 3)])
def test_path_rule(n, direct, auto, monkeypatch):
    monkeypatch.setenv("MISPEC_SHIFT_SOLVER", "iterative")  # option shift_solver is not read
    lib = sa.lib()
    assert lib.mispec_symshift_general_complex_solver_path(n, DIRECT) == direct
    if direct == REFUSED:
        assert "only n <= 4096" in lib.mispec_last_error().decode()
        with pytest.raises(ValueError, match="only n <= 4096"):
            sa.general_complex_shift_solver_path(n, "direct")
    else:
        assert sa.general_complex_shift_solver_path(n, "direct") == direct
    assert lib.mispec_symshift_general_complex_solver_path(n, AUTO) == auto
    assert lib.mispec_symshift_general_complex_solver_path(n, ITERATIVE) == 3
    assert sa.general_complex_shift_solver_path(n, "auto") == auto and sa.general_complex_shift_solver_path(n, "iterative") == 3


def test_bad_arguments():
    lib = sa.lib()
    for n, solver in [(0, AUTO), (-5, ITERATIVE), (10, 3), (10, -1), (10, -2)]:
        assert lib.mispec_symshift_general_complex_solver_path(n, solver) == REFUSED, (n, solver)
    for solver in ("bicgstab", None):
        with pytest.raises(ValueError, match="unknown shift solver"):
            sa.general_complex_shift_solver_path(10, solver)


def test_null_and_bad_arguments_of_the_constructor_are_refused():
    lib = sa.lib()
    outer = np.array([0, 1], dtype=np.int32)
    inner = np.array([0], dtype=np.int32)
    val = np.array([1.0])
    ip, dp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))
    h = C.c_void_p()
    for solver in (-1, DIRECT, AUTO, ITERATIVE, 3):
        assert lib.mispec_symshift_create_general_complex(None, 1, ip(outer), ip(inner), dp(val), 1, solver, C.byref(h)) == REFUSED
        assert "bad argument" in lib.mispec_last_error().decode()
        assert lib.mispec_symshift_create_general_complex(None, 1, ip(outer), ip(inner), dp(val), 1, solver, None) == REFUSED
        assert h.value is None


def test_the_python_class_refuses_what_it_cannot_build():
    A = Z.random_gen(8, 8)
    with pytest.raises(ValueError, match="unknown shift solver"):
        sa.SparseGenComplexShiftSolve(A, complex_solver="bicgstab")
    for solver in ("auto", "iterative"):  # the real operator's argument keeps its refusal, whatever complex_solver says
        with pytest.raises(ValueError, match="real shifts only"):
            sa.SparseGenComplexShiftSolve(A, solver=solver)
        with pytest.raises(ValueError, match="real shifts only"):
            sa.SparseGenComplexShiftSolve(A, solver=solver, complex_solver="iterative")


# ---- the restatement against SuperLU, at the bars of the GPU tests ----------------------------------------------------------------
def reference_against_superlu(A, sigma, cap, compare=True):
    n = A.shape[0]
    x = Z.solve_rhs(n)
    y, iters, passes, omega = Z.zbicgstab_reference(A, sigma, x)
    err = 0.0
    if compare:
        ref = Z.superlu_solve(A, sigma, x)
        err = np.abs(y.real - ref).max() / max(1.0, np.abs(ref).max())
    print("n %d sigma %s: %d iterations, %d passes, omega %.1e, error %.1e" % (n, sigma, iters, passes, omega, err))
    assert err <= 1e-12 and omega <= Z.TOL and passes == 1 and iters <= cap, (err, omega, passes, iters)
    return iters


# the caps are sanity bounds on the counts this restatement gave when the file was written (73, 31, 416); 2 + 0.9i lies 0.046 from
# the spectrum, where the count moves by tens with the order of a sum
@pytest.mark.parametrize("sigma,cap", [(1.5 + 1j, 80), (0.5j, 40), (2 + 0.9j, 600)])
def test_reference_on_the_rotating_flow(sigma, cap):
    A, _ = Z.rot3(20, 21, 22, 0.5)
    assert A.shape[0] == 9240
    reference_against_superlu(A, sigma, cap)


def test_reference_on_the_small_rotating_flow():
    reference_against_superlu(Z.rot3(8, 9, 10, 0.5)[0], 1.5 + 1j, 60)
    reference_against_superlu(Z.rot3(12, 13, 14, 0.5)[0], 1.5 + 1j, 70)


@pytest.mark.parametrize("n", Z.SHAPES)
def test_reference_on_the_kernel_shapes(n):
    for sigma in (0.25 + 0.5j, -1j):
        reference_against_superlu(Z.random_gen(n, n), sigma, 12)


def test_reference_special_cases():
    n = 257
    x = Z.solve_rhs(n)
    y, iters, passes, _ = Z.zbicgstab_reference(sp.identity(n, format="csc") * 4.0, 2 + 1j, x)  # one iteration exhausts the space
    want = (x / (2 - 1j)).real
    assert iters == 1 and passes == 1 and np.all(np.abs(y.real - want) <= 4 * np.spacing(np.abs(want)))
    assert Z.zbicgstab_reference(sp.identity(n, format="csc"), 1j, np.zeros(n))[1] == 0
    A = Z.rot3(8, 9, 10, 0.5)[0]
    with pytest.raises(ArithmeticError, match="did not converge in 200 iterations"):  # inside the spectrum's hull: the cap ends it
        Z.zbicgstab_reference(A, 6 + 0.3j, Z.solve_rhs(A.shape[0]), max_iterations=200)


def test_closed_form_of_the_rotating_flow():
    A, lam = Z.rot3(5, 4, 3, 0.5)
    D = A.toarray()
    assert np.abs(D @ D.T - D.T @ D).max() == 0  # normal: the eigenvalues are as well conditioned as a symmetric matrix's
    ev = np.linalg.eigvals(D)
    ev = ev[np.lexsort((ev.imag, ev.real))]
    assert Z.match_up_to_conjugation(ev, lam) <= 1e-10 and Z.match_up_to_conjugation(lam, ev) <= 1e-10
    assert lam.real.min() > 2 and np.abs(lam.imag).max() > 0.5 and abs(A - A.T).max() == 1.0
