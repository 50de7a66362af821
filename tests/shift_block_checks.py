"""Fixtures shared by the block shift solve tests (tests/test_host_shift_block.py, tests/test_gpu_shift_block.py,
tests/test_gpu_lobpcg_solver_pre.py): the banded builders of tests/test_gpu_shift.py restated, the K + E fixture of the solver
preconditioner, and the size lists."""
import functools

import numpy as np
import scipy.sparse as sp

COLUMN_COUNTS = (1, 2, 3, 4, 5, 8, 9, 21)   # cross the panel edges 2|3 and 4|5; 21 is LOBPCG's widest block
PLAN_PANELS = ("0", "2", "4")

# (n, b) of the narrow-band partitioned levels: 2049 is the first partitioned size (16 chunks, less than a wavefront); 64 * 128 + 128
# is one full group of chunks plus the tail workgroup, then one row more; 65 * 128 + 5 a second, short group
NARROW_SHAPES = [(2049, 1), (2049, 3), (2049, 4), (2049, 5), (2049, 8), (64 * 128 + 128, 3), (64 * 128 + 129, 3), (64 * 128 + 129, 8),
                 (65 * 128 + 5, 1), (65 * 128 + 5, 4), (65 * 128 + 5, 5)]
# two partitioned levels then the dense one; a wide second level (Schur band 15: the column loop); above 2048 chunks (sweeps by default)
DEEP_SHAPES = [(100_003, 3), (100_003, 8), (300_001, 3)]

# the solver preconditioner's cases: (n, m), dense path and banded path; iterations of the flow on the host backend with T = K^{-1}
PRE_CASES = [(1000, 4), (4500, 8)]
PRE_HOST_ITERATIONS = {(1000, 4): 20, (4500, 8): 21}
PRE_MAXIT = 40            # twice the host backend's count (the device sums in other orders): a condition, not a measurement
PRE_MAXIT_JACOBI = 300
COUPLING, COUPLING_OFFSET = 0.002, 70


def banded_spd(n, b, seed=0):
    rng = np.random.default_rng(seed)
    diags = [rng.uniform(-0.5, 0.5, n - d) for d in range(1, b + 1)]
    return sp.diags([rng.uniform(-0.5, 0.5, n) + b + 0.5] + diags + diags, [0] + list(range(1, b + 1)) + [-d for d in range(1, b + 1)],
                    format="csc")


def banded_indefinite(n, b, seed=0):
    rng = np.random.default_rng(seed)
    diags = [rng.uniform(-1.0, 1.0, n - d) for d in range(1, b + 1)]
    return sp.diags([rng.uniform(-2.0, 2.0, n)] + diags + diags, [0] + list(range(1, b + 1)) + [-d for d in range(1, b + 1)], format="csc")


def rhs_block(n, k, ld=None, seed=1):
    """An n x k block inside a Fortran-ordered ld x k array (ld >= n), entries in (-1, 1); the rows beyond n hold a sentinel."""
    ld = n if ld is None else ld
    full = np.full((ld, k), 7.25, order="F")
    full[:n] = np.random.default_rng(seed).uniform(-1, 1, (n, k))
    return full


@functools.lru_cache(maxsize=None)
def Kmat(n):
    """tridiag(-1, 2, -1)"""
    return sp.diags([np.full(n - 1, -1.0), np.full(n, 2.0), np.full(n - 1, -1.0)], [-1, 0, 1], shape=(n, n), format="csr")


@functools.lru_cache(maxsize=None)
def Emat(n):
    """0.002 x the graph Laplacian of the edges (i, i + 70): +0.002 on both end points' diagonal entries, -0.002 at offsets +-70"""
    k = COUPLING_OFFSET
    d = np.zeros(n)
    d[:n - k] += COUPLING
    d[k:] += COUPLING
    off = np.full(n - k, -COUPLING)
    return sp.diags([off, d, off], [-k, 0, k], shape=(n, n), format="csr")


@functools.lru_cache(maxsize=None)
def Amat(n):
    """A = K + E: SPD, half-bandwidth 70; K is the nearby matrix whose factorisation preconditions it"""
    return (Kmat(n) + Emat(n)).tocsr()
