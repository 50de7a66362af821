"""Synthetic host-side matrices of the secondary workloads (bench.py, tools/, tests): none of them has the fixed-offset structure
of the headline matrix M-band, so none of them can use its diagonal storage.

* m_rand:       every row has 7 partners at uniformly random columns, symmetrised — all far gathers (SURVEY.md 8d "M-rand")
* jitter_band:  M-band's 14 off-diagonals with every entry moved by a per-entry jitter of at most +-64 columns, symmetrised:
                variable row lengths, ~1800 distinct diagonals (no offset codes, no diagonal storage), columns local but not on
                constant offsets — what a mesh matrix looks like after a bandwidth-reducing ordering
* stencil7:     3-D 7-point stencil on an m^3 grid with random symmetric values, natural order
"""
import numpy as np
import scipy.sparse as sp

BAND_OFFSETS = (1, 2, 3, 1000, 1001, 100000, 100001)


def m_rand(n, seed=20240607):
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n, dtype=np.int64), 7)
    cols = rng.integers(0, n, size=rows.size, dtype=np.int64)
    vals = rng.uniform(-0.5, 0.5, size=rows.size)
    U = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    U.sum_duplicates()
    A = (U + U.T + sp.diags(rng.uniform(-0.5, 0.5, n))).tocsr()
    A.sort_indices()
    return A


def jitter_band(n, seed=20250925, jitter=64, offsets=BAND_OFFSETS):
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    rows, cols = [], []
    for off in offsets:
        c = i + off + rng.integers(-jitter, jitter + 1, size=n, dtype=np.int64)
        keep = (c >= 0) & (c < n) & (c != i)
        rows.append(i[keep])
        cols.append(c[keep])
    rows = np.concatenate(rows)
    cols = np.concatenate(cols)
    vals = rng.uniform(-0.5, 0.5, size=rows.size)
    U = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    U.sum_duplicates()
    A = (U + U.T + sp.diags(rng.uniform(-0.5, 0.5, n))).tocsr()
    A.sort_indices()
    return A


def stencil7(m, seed=0):
    I = sp.identity(m, format="csr")
    T = sp.diags([np.ones(m - 1), np.ones(m - 1)], [-1, 1], format="csr")
    A = (sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T) + 6 * sp.identity(m ** 3)).tocsr()
    rng = np.random.default_rng(seed)
    A.data[:] = rng.uniform(-0.5, 0.5, A.nnz)
    A = (sp.tril(A) + sp.tril(A, -1).T).tocsr()
    A.sort_indices()
    return A


_M1, _M2, _M3, _M4 = (np.uint64(v) for v in (0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB, 0xD6E8FEB86659FD93))


def _mix64(z):
    z = z + _M1
    z = (z ^ (z >> np.uint64(30))) * _M2
    z = (z ^ (z >> np.uint64(27))) * _M3
    return z ^ (z >> np.uint64(31))


def hash_value(seed, a, b):
    """U(-0.5, 0.5) from the splitmix64-style counter hash of the synthetic matrices, for uint64 arrays a, b."""
    with np.errstate(over="ignore"):
        k = _mix64(_mix64(np.uint64(seed) ^ a) ^ (b * _M4))
    return (k >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0) - 0.5


def herm_band(n, seed=20240607, offsets=BAND_OFFSETS):
    """The complex Hermitian M-band: the LOWER triangle (CSR, complex128) of the matrix with M-band's offsets, entry (r, r - off)
    = h(seed, r - off, r) + i h(seed + 1, r - off, r) with independent counter hashes for the two parts, and a real diagonal
    h(seed, r, r).  HermEigsSolver / SparseHermMatProd(uplo="L") read exactly this triangle."""
    r_all = np.arange(n, dtype=np.uint64)
    rows, cols, vals = [r_all], [r_all], [hash_value(seed, r_all, r_all).astype(np.complex128)]
    for off in offsets:
        if off >= n:
            continue
        r = r_all[off:]
        c = r - np.uint64(off)
        rows.append(r)
        cols.append(c)
        vals.append(hash_value(seed, c, r) + 1j * hash_value(seed + 1, c, r))
    L = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows).astype(np.int64), np.concatenate(cols).astype(np.int64))),
                      shape=(n, n)).tocsr()
    L.sort_indices()
    return L
