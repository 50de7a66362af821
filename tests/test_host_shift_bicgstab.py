"""Host side of the general operator's iterative shift-solve path (no GPU): the path a solver kind selects for a general matrix,
option and environment precedence, the refusals of the new entry points, and the numpy restatement of the iteration
(shift_gen_checks.bicgstab_reference) against SuperLU on every fixture of tests/test_gpu_shift_bicgstab.py — which shows that the
iteration-count caps of that file are attainable."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import shift_gen_checks as G
import spectra_amd as sa
from spectra_amd import _capi

DEFAULT, DIRECT, AUTO, ITERATIVE = -1, 0, 1, 2
REFUSED = _capi.MISPEC_EINVAL


@pytest.fixture
def restore_options():
    yield
    sa.set_option("shift_solver", None)


@pytest.mark.parametrize("n,direct,auto", [(1, 0, 0), (4096, 0, 0), (4097, REFUSED, 3)])
def test_general_solver_path(n, direct, auto, restore_options, monkeypatch):
    monkeypatch.delenv("MISPEC_SHIFT_SOLVER", raising=False)
    lib = sa.lib()
    assert lib.mispec_symshift_general_solver_path(n, DIRECT) == direct
    assert lib.mispec_symshift_general_solver_path(n, AUTO) == auto
    assert lib.mispec_symshift_general_solver_path(n, ITERATIVE) == 3
    assert lib.mispec_symshift_general_solver_path(n, DEFAULT) == direct  # option unset: direct
    if direct == REFUSED:
        assert "only n <= 4096" in lib.mispec_last_error().decode()
        with pytest.raises(ValueError, match="only n <= 4096"):
            sa.general_shift_solver_path(n, "direct")
    assert sa.general_shift_solver_path(n, "auto") == auto and sa.general_shift_solver_path(n, "iterative") == 3


def test_option_and_environment_precedence(restore_options, monkeypatch):
    monkeypatch.delenv("MISPEC_SHIFT_SOLVER", raising=False)
    lib = sa.lib()
    assert lib.mispec_symshift_general_solver_path(4097, DEFAULT) == REFUSED
    sa.set_option("shift_solver", "auto")
    assert lib.mispec_symshift_general_solver_path(4097, DEFAULT) == 3 and lib.mispec_symshift_general_solver_path(4096, DEFAULT) == 0
    assert lib.mispec_symshift_general_solver_path(4097, DIRECT) == REFUSED  # the argument overrides the option
    sa.set_option("shift_solver", "iterative")
    assert lib.mispec_symshift_general_solver_path(1, DEFAULT) == 3
    sa.set_option("shift_solver", None)
    monkeypatch.setenv("MISPEC_SHIFT_SOLVER", "iterative")
    assert lib.mispec_symshift_general_solver_path(4096, DEFAULT) == 3 and sa.general_shift_solver_path(4096) == 3
    assert sa.general_shift_solver_path(4096, "direct") == 0  # ... and the environment
    sa.set_option("shift_solver", "direct")  # a set option wins over the environment
    assert lib.mispec_symshift_general_solver_path(4096, DEFAULT) == 0


def test_bad_arguments():
    lib = sa.lib()
    for n, solver in [(0, AUTO), (-5, ITERATIVE), (10, 3), (10, -2)]:
        assert lib.mispec_symshift_general_solver_path(n, solver) == REFUSED
    with pytest.raises(ValueError, match="unknown shift solver"):
        sa.general_shift_solver_path(10, "bicgstab")


def test_null_arguments_of_the_constructor_are_refused():
    lib = sa.lib()
    outer = np.array([0, 1], dtype=np.int32)
    inner = np.array([0], dtype=np.int32)
    val = np.array([1.0])
    ip, dp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))
    h = C.c_void_p()
    for solver in (DEFAULT, DIRECT, AUTO, ITERATIVE):
        assert lib.mispec_symshift_create_general_solver(None, 1, ip(outer), ip(inner), dp(val), 1, solver, C.byref(h)) == REFUSED
        assert "bad argument" in lib.mispec_last_error().decode()
        assert h.value is None
    assert lib.mispec_symshift_set_shift_complex(None, 1.0, 1.0) == REFUSED


def test_the_complex_operator_refuses_a_solver_kind(monkeypatch):
    A = G.random_gen(8, 8)
    for solver in ("auto", "iterative"):
        with pytest.raises(ValueError, match="real shifts only"):
            sa.SparseGenComplexShiftSolve(A, solver=solver)


# ---- the restatement against SuperLU, at check_solve's bars ------------------------------------------------------------------------
def reference_against_superlu(A, sigma, cap):
    n = A.shape[0]
    M = (A - sigma * sp.identity(n)).tocsc()
    x = G.solve_rhs(n)
    y, iters, passes, omega = G.bicgstab_reference(M, x, mnorm=(abs(A).sum(axis=1) + abs(sigma)).max())
    ref = spla.splu(M).solve(x)
    res, err = np.linalg.norm(M @ y - x) / np.linalg.norm(x), np.abs(y - ref).max() / max(1.0, np.abs(ref).max())
    print("n %d sigma %g: %d iterations, %d passes, omega %.1e, residual %.1e, error %.1e" % (n, sigma, iters, passes, omega, res, err))
    assert res <= 1e-12 and err <= 1e-12 and omega <= G.TOL and passes == 1 and iters <= cap, (res, err, omega, passes, iters)


@pytest.mark.parametrize("sigma", [0.0, -1.5])
def test_reference_on_the_digraph(sigma):
    reference_against_superlu(G.digraph(), sigma, 30)


@pytest.mark.parametrize("dims,c,sigma", [((17, 17, 17), 0.4, 0.0), ((17, 17, 17), 0.4, -1.0), ((12, 13, 14), 0.4, 0.0),
                                          ((12, 13, 14), 0.1, 0.0), ((26, 28, 30), 0.1, 0.0)])
def test_reference_on_convection_diffusion(dims, c, sigma):
    reference_against_superlu(G.cd3(*dims, c)[0], sigma, 150)


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 1023, 1025, 4097])
def test_reference_on_the_kernel_shapes(n):
    for sigma in (0.0, 0.25):
        reference_against_superlu(G.random_gen(n, n), sigma, 12)


def test_reference_special_cases():
    n = 257
    x = G.solve_rhs(n)
    y, iters, passes, _ = G.bicgstab_reference(sp.identity(n) * 2.0, x)  # 4 I at sigma = 2: one iteration exhausts the Krylov space
    assert iters == 1 and passes == 1 and np.all(np.abs(y - x / 2) <= 4 * np.spacing(np.abs(x / 2)))
    assert G.bicgstab_reference(sp.identity(n), np.zeros(n))[:2][1] == 0
    A = G.upper_bidiagonal(n)
    with pytest.raises(ArithmeticError, match="did not converge in 200 iterations"):  # exactly singular
        G.bicgstab_reference(A - 3.0 * sp.identity(n), x, max_iterations=200)
    reference_against_superlu(A, 0.5, 20)


def test_closed_form_of_the_convection_diffusion_eigenvalues():
    A, lam = G.cd3(5, 4, 3, 0.4)
    ev = np.linalg.eigvals(A.toarray())
    assert np.abs(ev.imag).max() <= 1e-7 and np.abs(np.sort(ev.real) - lam).max() <= 1e-7  # (defective-like: eigvals is no better)
    assert abs(A - A.T).max() > 0.5
