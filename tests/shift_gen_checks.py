"""Fixtures of the general (non-symmetric) operator's iterative shift-solve path (csrc/shift_bicgstab.hip), shared by
tests/test_host_shift_bicgstab.py, tests/test_gpu_shift_bicgstab.py and tools/bench_shift_bicgstab.py: non-symmetric matrices,
their closed forms, and a numpy restatement of the iteration and its acceptance loop — the oracle of the iteration-count caps."""
import functools

import numpy as np
import scipy.sparse as sp

from shift_minres_checks import check_solve  # noqa: F401 - the bars of the SuperLU comparisons, re-exported

TOL, STAGNATION, RESTARTS, MARGIN, MAX_ITERATIONS = 4.0e-15, 1.0e-13, 3, 0.25, 20000


def _t(m, c):
    return sp.diags([2 * np.ones(m), (-1 + c) * np.ones(m - 1), (-1 - c) * np.ones(m - 1)], [0, 1, -1])


@functools.lru_cache(maxsize=None)
def cd3(p, q, r, c):
    """(A, lam): the convection-diffusion operator of a p x q x r grid numbered along p first — the Kronecker sum of
    tridiag(lower -1 - c, 2, upper -1 + c) over the three axes — and its eigenvalues, ascending: sums over the axes of
    2 - 2 sqrt(1 - c^2) cos(k pi / (m + 1)), real for |c| < 1"""
    Ip, Iq, Ir = sp.identity(p), sp.identity(q), sp.identity(r)
    A = (sp.kron(_t(r, c), sp.kron(Iq, Ip)) + sp.kron(Ir, sp.kron(_t(q, c), Ip)) + sp.kron(Ir, sp.kron(Iq, _t(p, c)))).tocsc()
    ev = lambda m: 2 - 2 * np.sqrt(1 - c * c) * np.cos(np.arange(1, m + 1) * np.pi / (m + 1))  # noqa: E731
    lam = ev(p)[:, None, None] + ev(q)[None, :, None] + ev(r)[None, None, :]
    return A, np.sort(lam, axis=None)


@functools.lru_cache(maxsize=None)
def digraph(n=5000):
    """A = diag(outdeg + 1) - W for the directed graph W of 3 random edges per vertex with weights U(0.5, 1.5): the expander of
    shift_minres_checks without the symmetrisation"""
    rng = np.random.default_rng(1)
    rows = np.repeat(np.arange(n), 3)
    cols = rng.integers(0, n, 3 * n)
    w = rng.uniform(0.5, 1.5, 3 * n)
    keep = rows != cols
    W = sp.coo_matrix((w[keep], (rows[keep], cols[keep])), shape=(n, n)).tocsr()
    deg = np.asarray(W.sum(axis=1)).ravel()
    return (sp.diags(deg + 1.0) - W).tocsc()


def random_gen(n, seed):
    """random sparse non-symmetric matrix with diagonal in [3, 4] and about 4 off-diagonal entries per row in (-0.5, 0.5)"""
    rng = np.random.default_rng(seed)
    m = 4 * n if n > 1 else 0
    r, c = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = r != c
    S = sp.coo_matrix((rng.uniform(-0.5, 0.5, m)[keep], (r[keep], c[keep])), shape=(n, n)).tocsr()
    return (S + sp.diags(rng.uniform(3.0, 4.0, n))).tocsc()


def upper_bidiagonal(n=257):
    """diagonal 1 ... n, superdiagonal 1: A - k I is exactly singular for k = 1 ... n"""
    return sp.diags([np.arange(1.0, n + 1), np.ones(n - 1)], [0, 1]).tocsc()


def bicgstab_reference(M, x, mnorm=None, tol=TOL, max_iterations=MAX_ITERATIONS):
    """(y, iterations, passes, omega): right-preconditioned BiCGStab with the Jacobi preconditioner on M y = x as
    csrc/shift_bicgstab.hip runs it — the ten steps of an iteration, a pass's stop at |r|_2 <= 0.25 min(1, tol / omega) |rhs|_2, the
    breakdown rules, the refusal of a pass that the iteration cap ended, and the acceptance loop on the explicit residual's
    backward error omega = |x - M y|_inf / (mnorm |y|_inf + |x|_inf) with up to 3 restarts.  mnorm: the bound on |M|_inf in omega
    (default: |M|_inf itself).  Plain numpy sums: the device's sums have another order, so its counts differ by a few iterations."""
    M = sp.csr_matrix(M)
    x = np.asarray(x, dtype=float)
    n = x.size
    d = M.diagonal()
    maxd = np.abs(d).max()
    d = np.where(np.abs(d) > maxd * 2.0 ** -26, d, maxd if maxd > 0 else 1.0)
    minv = 1.0 / d
    if mnorm is None:
        mnorm = abs(M).sum(axis=1).max()
    y = np.zeros(n)
    if not x.any():
        return y, 0, 1, 0.0
    used, omega_b, prev = 0, 1.0, np.inf
    for npass in range(RESTARTS + 1):
        rhs = x if npass == 0 else x - M @ y
        r = rhs.copy()
        rhat = rhs.copy()
        sol, p, v = np.zeros(n), np.zeros(n), np.zeros(n)
        rho = rhat @ r
        stop = MARGIN * min(1.0, tol / omega_b) * np.sqrt(rho)
        alpha = om = beta = 0.0
        end = "cap"
        while used < max_iterations:
            p = r + beta * (p - om * v)
            ph = minv * p
            v = M @ ph
            rv = rhat @ v
            if rv == 0.0:
                end = "breakdown"
                break
            alpha = rho / rv
            s = r - alpha * v
            sh = minv * s
            t = M @ sh
            tt = t @ t
            om = 0.0 if tt == 0.0 else (t @ s) / tt
            sol += alpha * ph + om * sh
            r = s - om * t
            used += 1
            rho1 = rhat @ r
            if np.sqrt(r @ r) <= stop:
                end = "converged"
                break
            if not np.isfinite(rho1) or om == 0.0 or rho1 == 0.0:
                end = "breakdown"
                break
            beta = (rho1 / rho) * (alpha / om)
            rho = rho1
        y = y + sol
        omega_b = np.abs(x - M @ y).max() / (mnorm * np.abs(y).max() + np.abs(x).max())
        if end == "cap":  # BiCGStab's iterates are not monotone in any norm: one cut off at the cap is not judged by omega
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


@functools.lru_cache(maxsize=None)
def reference_count(name, args, sigma):
    """iterations of bicgstab_reference on the fixture `name(*args)` at `sigma` with the right-hand side solve_rhs gives, with the
    device's bound on |M|_inf"""
    A = fixture(name, args)
    n = A.shape[0]
    mnorm = (abs(A).sum(axis=1) + abs(sigma)).max()
    return bicgstab_reference(A - sigma * sp.identity(n), solve_rhs(n), mnorm=mnorm)[1]


def fixture(name, args):
    A = {"cd3": cd3, "digraph": digraph, "random_gen": random_gen}[name](*args)
    return A[0] if isinstance(A, tuple) else A


def solve_rhs(n):
    return np.random.default_rng(n).uniform(-1, 1, n)
