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


# ---------------------------------------------------------------------------------------------------------------------------
# k_zvq at every tile height (csrc/zfac.hip): the product V Q in place, the new residual, the Ritz vectors into a buffer
# ---------------------------------------------------------------------------------------------------------------------------
# The kernel stages R rows x m columns of V in at most 64 KiB of LDS: R = vq_rows(m) = 64, 32, 16, 8, 4, 2, 1 for m up to 64, 128,
# 256, 512, 1024, 2048, 4096, and thread (r, cl) of a workgroup forms row r of the columns cl, cl + CL, ... with CL = 256 / R.
# Each m below is the last one of a tile height (exactly 64 KiB) or the first of the next.
VQ_WIDTHS = [64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096]


def vq_rows(m):
    R = 64
    while R > 1 and R * m * 16 > 65536:
        R >>= 1
    return R


def hip_vq_roundings(nnz):
    """k_zvq: one fma per term, per real component."""
    return nnz


def host_vq_roundings(nnz):
    """cpp/zfac_restart_host_capi.cpp: acc += v * q, a product and an addition per term."""
    return 2 * nnz


def _sample_rows(n, R, rng, extra=16):
    rows = set(range(min(R, n))) | set(range(max(0, n - R), n)) | set(int(r) for r in rng.integers(0, n, extra))
    return np.array(sorted(rows))


def _check_product(X, V, Q, nnz_of, roundings, rows, cols, what):
    """X[:, c] = V[:, :nnz_of(c)] Q[:nnz_of(c), c] for every column c of Q (real).  Two references:
      all rows, float64 BLAS — bound: the kernel's gamma_k(nnz) plus the reference's own gamma_(m + 1) (m additions in whatever order
        the BLAS takes them and the product), times sum_j |V_ij| |Q_jc| per real component;
      the rows `rows` x the columns `cols`, long double — the kernel's bound alone.
    Sensitivity (CPU): one row of Q fewer — the last term V[i, nnz - 1] Q[nnz - 1, c] — must move every checked column, in at
    least one checked row, by 100 tolerances."""
    from zprim_checks import LD, gamma

    m, ncols = Q.shape
    Qm = Q.copy()
    for c in range(ncols):
        Qm[nnz_of(c):, c] = 0.0  # what the kernel may not read must not count (the contracted pattern has zeros there anyway)
    kmax = max(roundings(nnz_of(c)) for c in range(ncols))
    Vr, Vi = np.asfortranarray(V.real), np.asfortranarray(V.imag)  # contiguous: numpy hands these products to the BLAS
    Tr, Ti = np.abs(Vr) @ np.abs(Qm), np.abs(Vi) @ np.abs(Qm)
    bound = gamma(kmax) + gamma(m + 1)
    er, ei = np.abs(X.real - Vr @ Qm), np.abs(X.imag - Vi @ Qm)
    print(f"{what}: all rows, worst error / bound = {max((er / (bound * Tr)).max(), (ei / (bound * Ti)).max()):.3e} "
          f"(k = {kmax}, + {m + 1} for the float64 reference)")
    assert np.all(er <= bound * Tr) and np.all(ei <= bound * Ti), what
    Vs_r, Vs_i = Vr[rows].astype(LD), Vi[rows].astype(LD)
    worst = 0.0
    for c in cols:
        nnz = nnz_of(c)
        q = Qm[:nnz, c].astype(LD)
        tol = gamma(roundings(nnz))
        for Vs, Xs in ((Vs_r[:, :nnz], X.real[rows, c]), (Vs_i[:, :nnz], X.imag[rows, c])):
            ref, T = Vs @ q, np.abs(Vs) @ np.abs(q)
            err = np.abs(Xs - ref)
            worst = max(worst, float((err / (tol * T)).max()))
            assert np.all(err <= tol * T), (what, c)
            last = np.abs(Vs[:, nnz - 1] * q[nnz - 1])
            assert float((last / (tol * T)).max()) >= 100.0, (what, c, "the last row of Q would not be missed: change the data")
    print(f"{what}: {len(rows)} rows x {len(cols)} columns in long double, worst error / bound = {worst:.3e}")


def tile_height_checks(lib, fac, n, m, vq_roundings, dot_roundings, seed=5):
    """fac: a Hermitian factorisation handle with ncv = m over any n x n Hermitian operator.  An m-step factorisation, then

    compress_real with a real random Q of exactly the contracted pattern (column i has m - k + i + 1 leading non-zeros, exact zeros
    below; k = CL + 2 columns or m - 2, so that ncols = k + 1 wraps round the CL column slots of a workgroup): the first k + 1
    columns of V Q, bit-equality of the columns that are not touched, the residual f Q(m-1, k-1) + V_k H(k, k-1) and beta;
    ritz_vectors with nvec in {1, CL - 1, CL, CL + 1, m} (those within 1 ... m).
    No shifted QR here: what is under test is the product and the residual formula, restart_checks keeps the Lanczos identity.

    Roundings: V Q — vq_roundings(nnz) (HIP: nnz fma).  Residual: k_zscale_copy (1), the complex product of k_zaxpy (3), its
    addition (1): k = 5 on terms |Q(m-1, k-1) f| + |H(k, k-1)| |V_k| per component.  beta: k_dot + 1 (zprim_checks.py).
    The long-double reference covers a seeded sample of rows that always holds the first R and the last R rows; for nvec > 32 it is
    CAPPED to the columns {0, CL - 1, CL, nvec - 1} and 12 seeded ones (all columns are checked against float64 BLAS)."""
    from zprim_checks import LD, assert_long_double, dotc_ref, gamma, parts

    assert_long_double()
    R = vq_rows(m)
    CL = 256 // R
    rng = np.random.default_rng(seed + m)
    v0 = rng.uniform(-0.5, 0.5, n) + 1j * rng.uniform(-0.5, 0.5, n)
    cnt = C.c_int64(0)
    ok(lib.mispec_zfac_init(fac, dp(v0), C.byref(cnt)))
    ok(lib.mispec_zfac_factorize(fac, 1, m, C.byref(cnt)))
    assert lib.mispec_zfac_subspace_dim(fac) == m
    V = np.empty((n, m), dtype=np.complex128, order="F")
    f = np.empty(n, dtype=np.complex128)
    ok(lib.mispec_zfac_get_V(fac, m, dp(V)))
    ok(lib.mispec_zfac_get_f(fac, dp(f)))
    rows = _sample_rows(n, R, rng)

    # --- in place: compress_real ---
    k = min(m - 2, CL + 2)
    first_nnz = m - k + 1
    Q = np.asfortranarray(rng.uniform(0.25, 1.0, (m, m)) * rng.choice([-1.0, 1.0], (m, m)))
    for i in range(k + 1):
        Q[min(m, first_nnz + i):, i] = 0.0
    assert np.count_nonzero(Q[:, 0]) == m - k + 1 and np.count_nonzero(Q[:, k - 1]) == m and Q[m - 1, k - 1] != 0.0
    Hn = np.zeros((m, m), dtype=np.complex128, order="F")
    Hn[np.arange(m), np.arange(m)] = rng.uniform(-1, 1, m)
    hk = 0.37109375
    Hn[k, k - 1] = Hn[k - 1, k] = hk
    ok(lib.mispec_zfac_set_H(fac, dp(Hn)))
    ok(lib.mispec_zfac_compress_real(fac, dp(Q), k))
    assert lib.mispec_zfac_subspace_dim(fac) == k
    Vn = np.empty((n, m), dtype=np.complex128, order="F")
    fn = np.empty(n, dtype=np.complex128)
    beta = C.c_double()
    ok(lib.mispec_zfac_get_V(fac, m, dp(Vn)))
    ok(lib.mispec_zfac_get_f(fac, dp(fn)))
    ok(lib.mispec_zfac_f_norm(fac, C.byref(beta)))
    assert np.array_equal(Vn[:, k + 1:], V[:, k + 1:])  # bit for bit: the kernel writes k + 1 columns and no more
    _check_product(Vn[:, : k + 1], V, Q[:, : k + 1], lambda c: min(m, first_nnz + c), vq_roundings, rows, range(k + 1),
                   f"V Q in place, m={m} R={R} CL={CL} k={k} n={n}")
    # the residual from the f of before and the column k the library now holds
    alpha = Q[m - 1, k - 1]
    fr, fi = parts(f)
    vr, vi = parts(Vn[:, k])
    for got, t1, t2 in ((fn.real, fr * LD(alpha), vr * LD(hk)), (fn.imag, fi * LD(alpha), vi * LD(hk))):
        tol = gamma(5) * (np.abs(t1) + np.abs(t2))
        assert np.all(np.abs(got - (t1 + t2)) <= tol)
        # either term left out moves the reference by far more than 100 tolerances
        assert float((np.abs(t1) / tol).max()) >= 100.0 and float((np.abs(t2) / tol).max()) >= 100.0
    (s, _), _ = dotc_ref(fn, fn)
    nrm = float(np.sqrt(s))
    kb = dot_roundings(n) + 1
    print(f"residual after the restart: beta={beta.value:.17e} |dbeta|/beta={abs(beta.value - nrm) / nrm:.3e} (tol {gamma(kb):.3e})")
    assert abs(beta.value - nrm) <= gamma(kb) * nrm
    (s1, _), _ = dotc_ref(fn, fn, n - 1)
    assert abs(float(np.sqrt(s1)) - nrm) >= 100.0 * gamma(kb) * nrm

    # --- into a buffer: ritz_vectors over all m columns of the V the library holds now ---
    for nvec in sorted({nv for nv in (1, CL - 1, CL, CL + 1, m) if 1 <= nv <= m}):
        Y = np.asfortranarray(rng.uniform(0.25, 1.0, (m, nvec)) * rng.choice([-1.0, 1.0], (m, nvec)))
        X = np.full((n, nvec), np.nan + 0j, dtype=np.complex128, order="F")
        ok(lib.mispec_zfac_ritz_vectors(fac, dp(Y), nvec, dp(X)))
        cols = range(nvec)
        if nvec > 32:
            cols = sorted({0, CL - 1, CL, nvec - 1} & set(range(nvec)) | set(int(c) for c in rng.integers(0, nvec, 12)))
        _check_product(X, Vn, Y, lambda c: m, vq_roundings, rows, cols, f"Ritz vectors, m={m} R={R} CL={CL} nvec={nvec} n={n}")
    Vafter = np.empty((n, m), dtype=np.complex128, order="F")
    ok(lib.mispec_zfac_get_V(fac, m, dp(Vafter)))
    assert np.array_equal(Vafter, Vn)  # the Ritz vectors go to their own buffer
