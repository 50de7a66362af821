"""Fixtures of the iterative shift-solve path (csrc/shift_minres.hip), shared by tests/test_gpu_shift_minres.py and
tools/bench_shift_minres.py: matrices no direct path takes, their closed forms, and the bars of tests/test_gpu_shift_wide.py."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def _t(m):
    return sp.diags([2 * np.ones(m), -np.ones(m - 1), -np.ones(m - 1)], [0, 1, -1])


@functools.lru_cache(maxsize=None)
def lap3(p, q, r):
    """the 7-point Laplacian of a p x q x r grid numbered along p first (half-bandwidth p q), and its eigenvalues (closed form),
    ascending"""
    Ip, Iq, Ir = sp.identity(p), sp.identity(q), sp.identity(r)
    A = (sp.kron(_t(r), sp.kron(Iq, Ip)) + sp.kron(Ir, sp.kron(_t(q), Ip)) + sp.kron(Ir, sp.kron(Iq, _t(p)))).tocsc()
    ev = lambda m: 2 - 2 * np.cos(np.arange(1, m + 1) * np.pi / (m + 1))  # noqa: E731
    lam = ev(p)[:, None, None] + ev(q)[None, :, None] + ev(r)[None, None, :]
    return A, np.sort(lam, axis=None)


@functools.lru_cache(maxsize=None)
def expander(n=5000):
    """(A, W): A = the Laplacian of W plus I, W = 3 random edges per vertex with weights U(0.5, 1.5), symmetrised.  Its band is
    nearly full and reverse Cuthill-McKee cannot narrow it."""
    rng = np.random.default_rng(1)
    rows = np.repeat(np.arange(n), 3)
    cols = rng.integers(0, n, 3 * n)
    w = rng.uniform(0.5, 1.5, 3 * n)
    keep = rows != cols
    W = sp.coo_matrix((w[keep], (rows[keep], cols[keep])), shape=(n, n)).tocsr()
    W = (W + W.T).tocsr()
    deg = np.asarray(W.sum(axis=1)).ravel()
    return (sp.diags(deg + 1.0) - W).tocsc(), W


@functools.lru_cache(maxsize=None)
def expander_pencil(n=5000):
    """(A, B): A the expander, B = diag(1 + deg / deg_max) + 0.05 W / max W: positive definite, A's pattern"""
    A, W = expander(n)
    deg = np.asarray(W.sum(axis=1)).ravel()
    B = (sp.diags(1.0 + deg / deg.max()) + 0.05 * W / W.max()).tocsc()
    return A, B


def random_sym(n, seed):
    """random sparse symmetric matrix with diagonal in [3, 4] and about 4 off-diagonal entries per row in (-0.5, 0.5):
    diagonally dominant by a small margin only where the row is short"""
    rng = np.random.default_rng(seed)
    m = 2 * n if n > 1 else 0
    r, c = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = r != c
    S = sp.coo_matrix((rng.uniform(-0.5, 0.5, m)[keep], (r[keep], c[keep])), shape=(n, n)).tocsr()
    return (S + S.T + sp.diags(rng.uniform(3.0, 4.0, n))).tocsc()


def lower(M):
    return sp.tril(M).tocsc()


def check_solve(op, M, x, res_tol=1e-12, err_tol=1e-12, ref=None):
    """the bars of tests/test_gpu_shift_wide.py's check_solve, with the iterative path's own record"""
    y = op.perform_op(x)
    ref = spla.splu(M.tocsc()).solve(x) if ref is None else ref
    res, err = np.linalg.norm(M @ y - x) / np.linalg.norm(x), np.abs(y - ref).max() / max(1.0, np.abs(ref).max())
    info = op.iterative_info()
    print("relative residual %.2e, error against the reference %.2e, %s" % (res, err, info))
    assert res <= res_tol and err <= err_tol, (res, err)
    return y, info
