"""Fixtures and checks shared by the LOBPCG tests: tests/test_host_lobpcg.py runs the control flow (spectra_amd/csrc/lobpcg_flow.hpp) on
a host backend, tests/test_gpu_lobpcg.py the library on the device, tests/test_gpu_lobpcg_kernels.py the three kernels alone."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALLEST, LARGEST = 7, 3                     # Util/SelectionRule.h SmallestAlge / LargestAlge
SUCCESS, NUMERICAL_ISSUE, NO_CONVERGENCE, INVALID_INPUT = 0, 1, 2, 3
TOL = 1e-8
MAXIT_JACOBI, MAXIT_PLAIN = 100, 500         # conditions, not measurements
BAND_OFFSETS = (1, 2, 5, 64)
LAMBDA_MIN_B = 1.4                           # tridiagonal (0.3, 2, 0.3): eigenvalues 2 + 0.6 cos(.) >= 1.4

# mirrors of the kernels' constants (spectra_amd/csrc/lobpcg.hip)
GRAM_TILE_ROWS, GRAM_MAX_GROUPS, GRAM_SLOT = 32, 512, 16
RESID_GROUP_ROWS, RESID_MAX_GROUPS = 512, 1024
MAX_BLOCK = 21


def kernel_row_counts():
    """1, 2, 3; one row tile of k_gram -1/0/+1; the chunk of a k_lobpcg_resid workgroup -1/0/+1; the last n at which every k_gram
    workgroup has one tile -1/0/+1 (beyond it a workgroup walks a chunk of two); a ragged size of many workgroups with chunks of two
    tiles, a last chunk of one and a short last tile."""
    t, g = GRAM_TILE_ROWS, GRAM_MAX_GROUPS
    return [1, 2, 3, t - 1, t, t + 1, RESID_GROUP_ROWS - 1, RESID_GROUP_ROWS, RESID_GROUP_ROWS + 1, t * g - 1, t * g, t * g + 1, 20011]


@functools.lru_cache(maxsize=None)
def band(n):
    rng = np.random.default_rng(n)
    diags, offs = [np.arange(1, n + 1, dtype=np.float64)], [0]
    for k in BAND_OFFSETS:
        if k < n:
            v = rng.uniform(-0.5, 0.5, n - k)
            diags += [v, v]
            offs += [k, -k]
    return sp.diags(diags, offs, shape=(n, n), format="csr")


@functools.lru_cache(maxsize=None)
def Bmat(n):
    return sp.diags([np.full(n - 1, 0.3), np.full(n, 2.0), np.full(n - 1, 0.3)], [-1, 0, 1], shape=(n, n), format="csr")


def X0(n, m):
    return np.asfortranarray(np.random.default_rng(1).uniform(-1, 1, (n, m)))


@functools.lru_cache(maxsize=None)
def reference_eigenvalues(n, with_B):
    """All eigenvalues (n <= 4099: numpy.linalg.eigvalsh / scipy.linalg.eigh(A, B), as dense matrices), ascending.  Beyond that size
    the dense problem takes minutes, and only the 24 smallest are computed: shift-and-invert Lanczos below the spectrum
    (Gershgorin: lambda_min(A) >= 1 - 4, lambda_min(B) >= 1.4) to working accuracy."""
    A = band(n)
    if n <= 4099:
        if with_B:
            return sla.eigh(A.toarray(), Bmat(n).toarray(), eigvals_only=True)
        return np.linalg.eigvalsh(A.toarray())
    w = spla.eigsh(A.tocsc(), k=24, M=Bmat(n).tocsc() if with_B else None, sigma=-10.0, which="LM", tol=0, return_eigenvectors=False)
    return np.sort(w)


def check_solution(n, m, lam, X, with_B=False, largest=False, tol=TOL, skip=0, msg=""):
    """The bars of every solve: the sorted eigenvalues equal the m extreme ones (after `skip` deflated ones) to 2 tol — |theta - lambda| <=
    |r|_2 for the standard problem, <= |r|_2 / sqrt(lambda_min(B)) for the pencil; the numpy residual of the returned vectors is below
    2 tol (two evaluations of the residual differ by about 9 * 2^-52 * |A|_max ~ 1e-11); X' B X = I to 1e-10."""
    A = band(n)
    ref = reference_eigenvalues(n, with_B)
    want = ref[::-1][skip:skip + m] if largest else ref[skip:skip + m]
    assert np.abs(np.sort(lam) - np.sort(want)).max() <= 2 * tol, (msg, lam, want)
    BX = Bmat(n) @ X if with_B else X
    res = np.linalg.norm(A @ X - BX * lam, axis=0)
    assert res.max() < 2 * tol, (msg, res)
    assert np.abs(X.T @ BX - np.eye(m)).max() < 1e-10, msg
    return res


# ---- the control flow on a host backend (tests/cpp/lobpcg_host_capi.cpp)
def build_host_library(directory):
    so = os.path.join(str(directory), "liblobpcg_host.so")
    # -Bsymbolic: the flow's inline functions bind to THIS library's copies even when libmispec_extras.so (which holds its own, loaded
    # with RTLD_GLOBAL) is already in the process
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-Wl,-Bsymbolic", "-I" + os.path.join(ROOT, "spectra_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "lobpcg_host_capi.cpp"), "-o", so])
    lib = C.CDLL(so)
    i64, vp, dp, ip = C.c_int64, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib.lobpcg_host_create.argtypes = [i64, ip, ip, dp, i64, C.POINTER(vp)]
    lib.lobpcg_host_destroy.argtypes = [vp]
    lib.lobpcg_host_set_B.argtypes = [vp, ip, ip, dp]
    lib.lobpcg_host_set_preconditioner.argtypes = [vp, ip, ip, dp]
    lib.lobpcg_host_set_jacobi.argtypes = [vp, C.c_int]
    lib.lobpcg_host_set_constraints.argtypes = [vp, dp, i64, i64]
    lib.lobpcg_host_set_initial.argtypes = [vp, dp, i64]
    lib.lobpcg_host_compute.argtypes = [vp, C.c_int, i64, C.c_double, C.POINTER(i64)]
    lib.lobpcg_host_info.argtypes = [vp]
    for nm in ("num_iterations", "num_operations", "num_retries", "active_column_sum"):
        getattr(lib, "lobpcg_host_" + nm).argtypes = [vp]
        getattr(lib, "lobpcg_host_" + nm).restype = i64
    lib.lobpcg_host_eigenvalues.argtypes = [vp, dp]
    lib.lobpcg_host_residual_norms.argtypes = [vp, dp]
    lib.lobpcg_host_eigenvectors.argtypes = [vp, dp, i64]
    return lib


def _csr_args(M):
    M = sp.csr_matrix(M)
    M.sort_indices()
    rp, ci, v = M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float64)
    return (rp, ci, v), (rp.ctypes.data_as(C.POINTER(C.c_int32)), ci.ctypes.data_as(C.POINTER(C.c_int32)),
                         v.ctypes.data_as(C.POINTER(C.c_double)))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class HostSolver:
    """The host-backend library behind the interface of spectra_amd.LOBPCGSolver."""

    def __init__(self, lib, A, X0=None, nev=None, B=None, preconditioner=None, constraints=None):
        self.lib, self.n = lib, A.shape[0]
        self.m = X0.shape[1] if X0 is not None else int(nev)
        self.h = C.c_void_p()
        keep, args = _csr_args(A)
        rc = lib.lobpcg_host_create(self.n, *args, self.m, C.byref(self.h))
        if rc != 0:
            raise ValueError("lobpcg_host_create: %d" % rc)
        if B is not None:
            keep, args = _csr_args(B)
            assert lib.lobpcg_host_set_B(self.h, *args) == 0
        if isinstance(preconditioner, str):
            assert preconditioner == "jacobi"
            assert lib.lobpcg_host_set_jacobi(self.h, 1) == 0
        elif preconditioner is not None:
            keep, args = _csr_args(preconditioner)
            assert lib.lobpcg_host_set_preconditioner(self.h, *args) == 0
        if constraints is not None:
            Y = np.asfortranarray(constraints, dtype=np.float64)
            rc = lib.lobpcg_host_set_constraints(self.h, _dp(Y), Y.shape[0], Y.shape[1])
            if rc != 0:
                raise ValueError("lobpcg_host_set_constraints: %d" % rc)
        if X0 is not None:
            X = np.asfortranarray(X0, dtype=np.float64)
            assert lib.lobpcg_host_set_initial(self.h, _dp(X), X.shape[0]) == 0

    def compute(self, selection=SMALLEST, maxit=100, tol=TOL):
        nconv = C.c_int64()
        rc = self.lib.lobpcg_host_compute(self.h, int(selection), maxit, tol, C.byref(nconv))
        if rc != 0:
            raise ValueError("lobpcg_host_compute: %d" % rc)
        return nconv.value

    def info(self):
        return self.lib.lobpcg_host_info(self.h)

    def num_iterations(self):
        return self.lib.lobpcg_host_num_iterations(self.h)

    def num_operations(self):
        return self.lib.lobpcg_host_num_operations(self.h)

    def num_retries(self):
        return self.lib.lobpcg_host_num_retries(self.h)

    def active_column_sum(self):
        return self.lib.lobpcg_host_active_column_sum(self.h)

    def eigenvalues(self):
        out = np.empty(self.m)
        self.lib.lobpcg_host_eigenvalues(self.h, _dp(out))
        return out

    def residual_norms(self):
        out = np.empty(self.m)
        self.lib.lobpcg_host_residual_norms(self.h, _dp(out))
        return out

    def eigenvectors(self):
        out = np.empty((self.n, self.m), order="F")
        self.lib.lobpcg_host_eigenvectors(self.h, _dp(out), self.n)
        return out

    def __del__(self):
        try:
            self.lib.lobpcg_host_destroy(self.h)
        except Exception:
            pass


# Iterations of the flow on the host backend at tol = 1e-8 (g++ -O2, x86-64), recorded for the tests' messages; the caps above are what
# is asserted.  (preconditioner, with B, selection, n, m) -> iterations.
RECORDED_ITERATIONS = {
    ("jacobi", False, SMALLEST, 300, 3): 17, ("jacobi", False, SMALLEST, 1000, 4): 19, ("jacobi", False, SMALLEST, 1000, 8): 24,
    ("jacobi", False, SMALLEST, 4099, 8): 28, ("jacobi", False, SMALLEST, 4099, 16): 32, ("jacobi", False, SMALLEST, 20011, 8): 25,
    ("jacobi", True, SMALLEST, 300, 3): 16, ("jacobi", True, SMALLEST, 1000, 8): 21, ("jacobi", True, SMALLEST, 4099, 16): 37,
    (None, False, SMALLEST, 300, 3): 178, (None, False, LARGEST, 300, 3): 215,
}
JACOBI_CASES = [(300, 3), (1000, 4), (1000, 8), (4099, 8), (4099, 16)]
B_JACOBI_CASES = [(300, 3), (1000, 8), (4099, 16)]


def rank_loss_case(n=60, m=3):
    """(A, X0, T, ritz): a preconditioner T = U V' of rank m (not symmetric: T r = U (V' r) is not annihilated by residuals orthogonal
    to U).  R = T (A X - X diag lambda) and P always lie in span(U), so [R | P] has rank m from the second iteration on and the
    iterates stay in Z = span[X0, U]; ritz are the m smallest Ritz values of A on Z."""
    rng = np.random.default_rng(7)
    U, V = rng.uniform(-1, 1, (n, m)), rng.uniform(-1, 1, (n, m))
    A, X = band(n), X0(n, m)
    Q, _ = np.linalg.qr(np.hstack([X, U]))
    ritz = np.linalg.eigvalsh(Q.T @ (A @ Q))[:m]
    return A, X, sp.csr_matrix(U @ V.T), ritz
