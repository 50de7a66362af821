"""Checks of the restart primitives of the complex Hermitian solver (mispec_zfac_set_H / _compress_real / _ritz_vectors,
include/mispec_extras.h), written against a ctypes library object so that they run on libmispec_extras.so on the GPU
(tests/test_gpu_zcsr.py) and, without a GPU, on the host build of the same control flow (tests/cpp/zfac_restart_host_capi.cpp,
tests/test_host_hermeigs.py).  The shifted QR sweeps are numpy's here: what is under test is V <- V Q, the new residual and the
Ritz-vector product, and the Lanczos identity they must leave behind."""
import ctypes as C

import numpy as np

from zfac_checks import dp, ok


def shifted_qr(T, shifts):
    """Q and Q'TQ after one explicit shifted QR step per shift on the real symmetric tridiagonal T (band kept exact)."""
    m = T.shape[0]
    Q = np.eye(m)
    for mu in shifts:
        Qi, R = np.linalg.qr(T - mu * np.eye(m))
        T = R @ Qi + mu * np.eye(m)
        T = np.diag(np.diag(T)) + np.diag(np.diag(T, -1), -1) + np.diag(np.diag(T, -1), 1)
        Q = Q @ Qi
    return Q, T


def restart_checks(lib, fac, A, m, k, seed=7, tol=1e-12):
    """fac: a Hermitian factorisation handle (ncv = m) over the n x n Hermitian A.  Factorises, restarts to k with exact shifts and
    checks V Q, f, the identity A V_k - V_k H_k = f e_k' and V_k^H V_k = I, then the Ritz vectors V Y."""
    n = A.shape[0]
    rng = np.random.default_rng(seed)
    v0 = rng.uniform(-0.5, 0.5, n) + 1j * rng.uniform(-0.5, 0.5, n)
    cnt = C.c_int64(0)
    ok(lib.mispec_zfac_init(fac, dp(v0), C.byref(cnt)))
    ok(lib.mispec_zfac_factorize(fac, 1, m, C.byref(cnt)))
    H = np.empty((m, m), dtype=np.complex128, order="F")
    V = np.empty((n, m), dtype=np.complex128, order="F")
    f = np.empty(n, dtype=np.complex128)
    ok(lib.mispec_zfac_get_H(fac, dp(H)))
    ok(lib.mispec_zfac_get_V(fac, m, dp(V)))
    ok(lib.mispec_zfac_get_f(fac, dp(f)))
    T = H.real
    T = np.diag(np.diag(T)) + np.diag(np.diag(T, -1), -1) + np.diag(np.diag(T, -1), 1)
    shifts = np.linalg.eigvalsh(T)[: m - k]  # the m - k smallest: any exact shifts will do
    Q, Tn = shifted_qr(T, sorted(shifts, key=abs, reverse=True))
    Q = np.asfortranarray(Q)
    Hn = np.asfortranarray(Tn.astype(np.complex128))
    ok(lib.mispec_zfac_set_H(fac, dp(Hn)))
    ok(lib.mispec_zfac_compress_real(fac, dp(Q), k))
    assert lib.mispec_zfac_subspace_dim(fac) == k
    Vn = np.empty((n, m), dtype=np.complex128, order="F")
    fn = np.empty(n, dtype=np.complex128)
    beta = C.c_double()
    ok(lib.mispec_zfac_get_V(fac, m, dp(Vn)))
    ok(lib.mispec_zfac_get_f(fac, dp(fn)))
    ok(lib.mispec_zfac_f_norm(fac, C.byref(beta)))
    scale = max(1.0, float(abs(A).sum(axis=1).max()))
    # V <- V Q for the first k + 1 columns (column i uses the first m - k + i + 1 rows of Q), the rest untouched
    Vexp = V @ Q[:, : k + 1]
    assert np.abs(Vn[:, : k + 1] - Vexp).max() <= tol
    assert np.array_equal(Vn[:, k + 1:], V[:, k + 1:])
    fexp = f * Q[m - 1, k - 1] + Vexp[:, k] * Hn[k, k - 1]
    assert np.abs(fn - fexp).max() <= tol * scale
    assert abs(np.linalg.norm(fn) - beta.value) <= tol * scale
    # the k-step factorisation the restart must leave
    Vk = Vn[:, :k]
    R = A @ Vk - Vk @ Hn[:k, :k]
    R[:, -1] -= fn
    assert np.abs(R).max() <= tol * scale
    assert np.abs(Vk.conj().T @ Vk - np.eye(k)).max() <= 1e-12
    # Ritz vectors: X = V Y over all m columns, into a separate buffer
    Y = np.asfortranarray(rng.uniform(-1, 1, (m, 3)))
    X = np.empty((n, 3), dtype=np.complex128, order="F")
    ok(lib.mispec_zfac_ritz_vectors(fac, dp(Y), 3, dp(X)))
    assert np.abs(X - Vn @ Y).max() <= tol
