"""Fixtures of the complex-shift iterative path of the general operator (csrc/shift_zbicgstab.hip), shared by
tests/test_host_shift_zbicgstab.py, tests/test_gpu_shift_zbicgstab.py and tools/bench_shift_zbicgstab.py: a normal non-symmetric
matrix with a closed-form complex spectrum, and a numpy restatement of the iteration and its acceptance loop in complex arithmetic
— the oracle of the iteration-count caps."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from shift_gen_checks import MARGIN, MAX_ITERATIONS, RESTARTS, STAGNATION, TOL, random_gen, solve_rhs  # noqa: F401 - re-exported

SHAPES = [1, 2, 3, 255, 256, 257, 1023, 1025, 4097]


def _t(m, g=0.0):
    """tridiag(lower -1, 2, upper -1), or with g: tridiag(lower -g, 2, upper +g)"""
    lo, up = (-1.0, -1.0) if g == 0.0 else (-g, g)
    return sp.diags([2 * np.ones(m), up * np.ones(m - 1), lo * np.ones(m - 1)], [0, 1, -1])


@functools.lru_cache(maxsize=None)
def rot3(p, q, r, g):
    """(A, lam): on a p x q x r grid numbered along p first, the Kronecker sum of tridiag(-1, 2, -1) over the p and q axes and of
    tridiag(lower -g, 2, upper +g) — 2 I plus a skew-symmetric part — over the r axis.  A is normal; its eigenvalues are
    (2 - 2 cos(a pi / (p+1))) + (2 - 2 cos(b pi / (q+1))) + 2 + 2 i g cos(c pi / (r+1)): conjugate pairs with real parts > 2.
    lam: all of them, sorted by (real, imag)"""
    Ip, Iq, Ir = sp.identity(p), sp.identity(q), sp.identity(r)
    A = (sp.kron(_t(r, g), sp.kron(Iq, Ip)) + sp.kron(Ir, sp.kron(_t(q), Ip)) + sp.kron(Ir, sp.kron(Iq, _t(p)))).tocsc()
    ev = lambda m: 2 - 2 * np.cos(np.arange(1, m + 1) * np.pi / (m + 1))  # noqa: E731
    skew = 2 + 2j * g * np.cos(np.arange(1, r + 1) * np.pi / (r + 1))
    lam = (ev(p)[:, None, None] + ev(q)[None, :, None] + skew[None, None, :]).ravel()
    return A, lam[np.lexsort((lam.imag, lam.real))]


def mnorm_of(A, sigma):
    """the device's bound on |A - sigma I|_inf: max_i (sum_j |A_ij| + |sigma|)"""
    return float((abs(A).sum(axis=1) + abs(sigma)).max())


def zbicgstab_reference(A, sigma, x, tol=TOL, max_iterations=MAX_ITERATIONS):
    """(y, iterations, passes, omega): right-preconditioned BiCGStab in complex arithmetic with the complex Jacobi preconditioner
    on (A - sigma I) y = x as csrc/shift_zbicgstab.hip runs it — shift_gen_checks.bicgstab_reference's ten steps, stop, breakdown
    rules, cap rule and acceptance loop, with <a, b> = np.vdot(a, b) and moduli of complex entries in omega.  y is complex: the
    operator's result is its real part.  Plain numpy sums: the device's sums have another order."""
    A = sp.csr_matrix(A)
    sigma = complex(sigma)
    x = np.asarray(x, dtype=float)
    n = x.size
    M = (A - sigma * sp.identity(n)).tocsr()
    d = A.diagonal() - sigma
    maxd = np.abs(d).max()
    d = np.where(np.abs(d) > maxd * 2.0 ** -26, d, maxd if maxd > 0 else 1.0)
    minv = 1.0 / d
    mnorm = mnorm_of(A, sigma)
    y = np.zeros(n, dtype=complex)
    if not x.any():
        return y, 0, 1, 0.0
    used, omega_b, prev = 0, 1.0, np.inf
    for npass in range(RESTARTS + 1):
        rhs = x.astype(complex) if npass == 0 else x - M @ y
        r = rhs.copy()
        rhat = rhs.copy()
        sol, p, v = np.zeros(n, dtype=complex), np.zeros(n, dtype=complex), np.zeros(n, dtype=complex)
        rho = np.vdot(rhat, r)
        stop = MARGIN * min(1.0, tol / omega_b) * np.sqrt(rho.real)
        alpha = om = beta = 0.0
        end = "cap"
        while used < max_iterations:
            p = r + beta * (p - om * v)
            ph = minv * p
            v = M @ ph
            rv = np.vdot(rhat, v)
            if rv == 0.0:
                end = "breakdown"
                break
            alpha = rho / rv
            s = r - alpha * v
            sh = minv * s
            t = M @ sh
            tt = np.vdot(t, t).real
            om = 0.0 if tt == 0.0 else np.vdot(t, s) / tt
            sol += alpha * ph + om * sh
            r = s - om * t
            used += 1
            rho1 = np.vdot(rhat, r)
            if np.sqrt(np.vdot(r, r).real) <= stop:
                end = "converged"
                break
            if not np.isfinite(rho1) or om == 0.0 or rho1 == 0.0:
                end = "breakdown"
                break
            beta = (rho1 / rho) * (alpha / om)
            if not np.isfinite(beta):
                end = "breakdown"
                break
            rho = rho1
        y = y + sol
        omega_b = np.abs(x - M @ y).max() / (mnorm * np.abs(y).max() + np.abs(x).max())
        if end == "cap":  # an iterate cut off at the cap is not judged by omega
            raise ArithmeticError("did not converge in %d iterations (backward error %.3e)" % (used, omega_b))
        if not omega_b <= tol:
            if npass == RESTARTS or used >= max_iterations or (npass >= 1 and omega_b > 0.9 * prev):
                if omega_b <= max(tol, STAGNATION):
                    break
                raise ArithmeticError("did not converge in %d iterations (backward error %.3e)" % (used, omega_b))
            prev = omega_b
            continue
        break
    return y, used, npass + 1, omega_b


def fixture(name, args):
    A = {"rot3": rot3, "random_gen": random_gen}[name](*args)
    return A[0] if isinstance(A, tuple) else A


@functools.lru_cache(maxsize=None)
def reference_count(name, args, sigma):
    """iterations of zbicgstab_reference on the fixture `name(*args)` at `sigma` with the right-hand side solve_rhs gives"""
    A = fixture(name, args)
    return zbicgstab_reference(A, sigma, solve_rhs(A.shape[0]))[1]


def superlu_solve(A, sigma, x):
    """Re((A - sigma I)^{-1} x) by SuperLU on the complex matrix"""
    n = A.shape[0]
    M = (A - complex(sigma) * sp.identity(n)).tocsc()
    return spla.splu(M.astype(complex)).solve(x.astype(complex)).real


def check_solve(op, A, sigma, x, ref=None, err_tol=1e-12):
    """shift_minres_checks.check_solve's bars for the real part of a complex solve: error against the reference
    <= 1e-12 max(1, max |ref|) and last_backward_error <= 1e-13.  (The residual of the real part alone is no measure: the imaginary
    part of the solution stays on the device.)"""
    y = op.perform_op(x)
    ref = superlu_solve(A, sigma, x) if ref is None else ref
    err = np.abs(y - ref).max() / max(1.0, np.abs(ref).max())
    info = op.iterative_info()
    print("sigma %s: error against the reference %.2e, %s" % (sigma, err, info))
    assert err <= err_tol, err
    assert info["last_backward_error"] <= 1e-13 and info["last_iterations"] >= 0, info
    return y, info


def match_up_to_conjugation(got, want, relative=True):
    """max over got of the distance (relative to |got|, or absolute) to the nearest of want and conj(want)"""
    both = np.concatenate([want, np.conj(want)])
    return max(np.abs(both - g).min() / (abs(g) if relative else 1.0) for g in got)
