"""Checks of the vector primitives of the complex factorisation (spectra_amd/csrc/zfac.hip: the two-stage reductions
k_zdotc_partial / k_zdotc_final and k_zabsmax_partial / k_zabsmax_final, k_zscale_copy in place, k_zupdate, the transfers) at the
sizes their code branches on, written against a ctypes library object like zfac_checks.py: tests/test_gpu_zprims.py runs them on
libmispec.so, tests/test_host_zprims.py on the host build of the same control flow (tests/cpp/zfac_host_capi.cpp).

The probe.  A callback operator (mispec_zfac_create_op, ncv = 1) ignores its input, records it, and answers y1 to the first call
and y2 to the second.  mispec_zfac_init (zfac_flow.hpp init) then runs: upload(v0), norm, apply -> y1, norm, scale_copy in place,
apply -> y2, a one-column X^H y, a one-column update, absmax and, unless the residual is judged zero, norm.  It leaves
v = y1 / |y1|, H(0, 0) = v^H y2, f = y2 - v H(0, 0) and beta = |f| to be read back, each of them one primitive applied to data the
test chose; the references are numpy.longdouble.

Tolerances: Higham's gamma_k = k u / (1 - k u), u = 2^-53, times the sum of the absolute values of the terms, per real component,
k = the roundings on the longest path, counted from the source:
  X^H y, HIP (zfac.hip): a thread adds its 2048 / 256 = 8 rows of the chunk (8), the wavefront's shuffle tree (6), the four
      wavefronts (3); the final kernel's thread adds ceil(nchunks / 256) partial sums, then 6 + 3 again; the product conj(a) b costs
      2 multiplications and an addition per component (3): k = 29 + ceil(nchunks / 256)                       -> hip_dot_roundings
  X^H y, host backend (cpp/zfac_host_backend.hpp): one running sum over the n rows: k = n + 3              -> host_dot_roundings
  v = y1 * (1 / sqrt(y1^H y1)): the sum, the square root, the division, the product: k = k_dot + 3
  f = w - v h (k_zupdate, one column; the same on the host): the complex product (3) and the subtraction: k = 4
  beta = sqrt(f^H f): k = k_dot + 1
A bound is never tuned from an observation.  Every case also asserts, on the CPU, that the defect it is aimed at would be seen:
the reference with the last row (and with the last chunk of 2048 rows) left out moves by at least 100 x the tolerance."""
import ctypes as C

import numpy as np

import zfac_checks as Z
from zfac_checks import dp, ok

LD = np.longdouble
U = 2.0 ** -53
CHUNK = 2048  # kChunk of zfac.hip: the rows of one stage-1 partial sum
PROBE_SIZES = [1, 63, 64, 255, 256, 257, 2047, 2048, 2049, 4097, 524287, 524288, 524289, 10**7 + 3]
STEP_SHAPES = [(2049, 9), (4097, 17), (300, 40)]  # the column count crosses 8 | 9 and 16 | 17 (kColGroup = 8)


def assert_long_double():
    assert np.finfo(LD).eps < 1e-18, "numpy.longdouble is not wider than double here: the references would prove nothing"


def gamma(k):
    return k * U / (1.0 - k * U)


def hip_dot_roundings(n):
    nchunks = (n + CHUNK - 1) // CHUNK
    return 8 + 6 + 3 + (nchunks + 255) // 256 + 6 + 3 + 3


def host_dot_roundings(n):
    return n + 3


def parts(a):
    return a.real.astype(LD), a.imag.astype(LD)


def dotc_ref(x, y, rows=None):
    """x^H y over the first `rows` rows in long double: (re, im) and, per component, the sum of the absolute values of its terms."""
    if rows is not None:
        x, y = x[:rows], y[:rows]
    xr, xi = parts(x)
    yr, yi = parts(y)
    a, b, c, d = xr * yr, xi * yi, xr * yi, xi * yr
    return (a.sum() + b.sum(), c.sum() - d.sum()), (np.abs(a).sum() + np.abs(b).sum(), np.abs(c).sum() + np.abs(d).sum())


def update_ref(w, v, h):
    """w - v h in long double, and the per-component term sums |w| + |v.x h.x| + |v.y h.y| (re), |w| + |v.x h.y| + |v.y h.x| (im)."""
    wr, wi = parts(w)
    vr, vi = parts(v)
    hr, hi = LD(h.real), LD(h.imag)
    re, im = wr - (vr * hr - vi * hi), wi - (vr * hi + vi * hr)
    tre = np.abs(wr) + np.abs(vr * hr) + np.abs(vi * hi)
    tim = np.abs(wi) + np.abs(vr * hi) + np.abs(vi * hr)
    return (re, im), (tre, tim)


class Probe:
    """One factorisation handle of one column over the recording operator."""

    def __init__(self, lib, ctxh, n):
        self.lib, self.n = lib, n
        self.seen, self.answers = [], []

        def op(user, x, y):
            self.seen.append(np.ctypeslib.as_array(x, shape=(2 * n,)).view(np.complex128).copy())
            np.ctypeslib.as_array(y, shape=(2 * n,)).view(np.complex128)[:] = self.answers[len(self.seen) - 1]
            return 0

        self.cb = Z.op_fn(op)
        self.fac = C.c_void_p()
        ok(lib.mispec_zfac_create_op(ctxh, self.cb, None, n, 1, 0, C.byref(self.fac)))

    def close(self):
        ok(self.lib.mispec_zfac_destroy(self.fac))

    def init(self, v0, y1, y2):
        """Run init; y2 may be a function of the normalised v (the second input the operator sees)."""
        n, lib = self.n, self.lib
        self.seen = []
        self.answers = [y1, None]
        # the second answer may depend on the first result: fill it in when the second call arrives
        if callable(y2):
            make, outer = y2, self

            class Lazy(list):
                def __getitem__(self, i):
                    if i == 1 and list.__getitem__(self, 1) is None:
                        self[1] = make(outer.seen[1])
                    return list.__getitem__(self, i)

            self.answers = Lazy(self.answers)
        else:
            self.answers[1] = y2
        ops = C.c_int64(0)
        ok(lib.mispec_zfac_init(self.fac, dp(v0), C.byref(ops)))
        assert ops.value == 2 and len(self.seen) == 2 and lib.mispec_zfac_subspace_dim(self.fac) == 1
        v = np.zeros(n, dtype=np.complex128)
        f = np.zeros(n, dtype=np.complex128)
        H = np.zeros((1, 1), dtype=np.complex128)
        beta = C.c_double(-1.0)
        ok(lib.mispec_zfac_get_V(self.fac, 1, dp(v)))
        ok(lib.mispec_zfac_get_f(self.fac, dp(f)))
        ok(lib.mispec_zfac_get_H(self.fac, dp(H)))
        ok(lib.mispec_zfac_f_norm(self.fac, C.byref(beta)))
        return v, complex(H[0, 0]), f, beta.value, self.answers[1]


def unit_phases(n, rng):
    """n entries of modulus 1 (to rounding): after the normalisation every |v_i| is 1 / sqrt(n), as small as it can be."""
    t = rng.uniform(0.0, 2.0 * np.pi, n)
    return np.cos(t) + 1j * np.sin(t)


def defect_rows(n):
    """Row counts of the targeted defects: the last row dropped; the last chunk of the fixed partition dropped."""
    out = [n - 1]
    last_chunk_start = ((n - 1) // CHUNK) * CHUNK
    if last_chunk_start > 0:
        out.append(last_chunk_start)
    return out


def check_common(n, v0, y1, seen, v, h00, y2, kdot, last_row_weighs=True):
    """What every probe run shares: the transfers, v = y1 / |y1| and H(0, 0) = v^H y2."""
    assert np.array_equal(seen[0], v0)   # upload, then the download in front of the operator: exact
    assert np.array_equal(seen[1], v)    # the operator's second input is the normalised column, bit for bit
    # v: relative to each component of the long-double quotient
    (s, _), _ = dotc_ref(y1, y1)
    nrm = np.sqrt(s)
    yr, yi = parts(y1)
    kv = kdot + 3
    assert np.all(np.abs(v.real - yr / nrm) <= gamma(kv) * np.abs(yr / nrm))
    assert np.all(np.abs(v.imag - yi / nrm) <= gamma(kv) * np.abs(yi / nrm))
    if n > 1 and last_row_weighs:  # the last row dropped from the sum: every entry of v grows by about |v_n|^2 / 2
        (s1, _), _ = dotc_ref(y1, y1, n - 1)
        assert abs(1.0 / np.sqrt(s1) - 1.0 / nrm) >= 100.0 * gamma(kv) / nrm
    # H(0, 0) against the long-double product of the downloaded v with y2
    (re, im), (tre, tim) = dotc_ref(v, y2)
    tol_re, tol_im = gamma(kdot) * tre, gamma(kdot) * tim
    print(f"n={n} k_dot={kdot} |dRe H00|={float(abs(h00.real - re)):.3e} (tol {float(tol_re):.3e}) "
          f"|dIm H00|={float(abs(h00.imag - im)):.3e} (tol {float(tol_im):.3e})")
    assert abs(h00.real - re) <= tol_re and abs(h00.imag - im) <= tol_im
    return (re, im), (tol_re, tol_im)


def check_residual(n, v, h00, y2, f, beta, kdot):
    """f = y2 - v H(0, 0) (from the H(0, 0) the library reports) and beta = |f| (from the f it reports)."""
    (fr, fi), (tre, tim) = update_ref(y2, v, h00)
    assert np.all(np.abs(f.real - fr) <= gamma(4) * tre) and np.all(np.abs(f.imag - fi) <= gamma(4) * tim)
    (s, _), _ = dotc_ref(f, f)
    nrm = float(np.sqrt(s))
    print(f"n={n} beta={beta:.17e} |dbeta|/beta={abs(beta - nrm) / nrm:.3e} (tol {gamma(kdot + 1):.3e})")
    assert beta > 0.0 and abs(beta - nrm) <= gamma(kdot + 1) * nrm
    return nrm


def branch_is_forced(n, kdot):
    """A residual of rounding noise over unit-modulus data is below eps |H(0, 0)| for certain (see probe_parallel)."""
    return (3 * kdot + 18) < 2.0 * np.sqrt(n)


def check_branch(n, v, h00, y2, f, beta, kdot, must_be_zero):
    """The decision absmax(f) < eps |H(0, 0)| of init on a residual that is rounding noise (see probe_parallel)."""
    eps = np.finfo(np.float64).eps
    (fr, fi), (tre, tim) = update_ref(y2, v, h00)
    hi = float((np.hypot(np.abs(fr) + gamma(4) * tre, np.abs(fi) + gamma(4) * tim)).max()) * (1 + 2 * U)
    lo = float(np.hypot(np.maximum(np.abs(fr) - gamma(4) * tre, 0), np.maximum(np.abs(fi) - gamma(4) * tim, 0)).max()) * (1 - 2 * U)
    thresh = eps * abs(h00)
    print(f"n={n} noise residual: max|f_ref| in [{lo:.3e}, {hi:.3e}] threshold {thresh:.3e} -> beta={beta:.3e}")
    if must_be_zero:
        assert hi < thresh, "the data does not force the zero branch: change the data"
    if hi < thresh:
        assert beta == 0.0 and not f.any()
    elif beta == 0.0:
        assert not f.any() and lo < thresh
    else:
        assert np.abs(f).max() * (1 + 2 * U) >= thresh
        check_residual(n, v, h00, y2, f, beta, kdot)


def probe_generic(probe, rng, kdot):
    """Independent random y1, y2: both components of X^H y, the update and the norm carry full-size terms in every row."""
    n = probe.n
    v0 = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
    y1 = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
    y2 = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
    if n > 1:  # no row may be negligible in any sum (the defects below are one row, one chunk)
        y1[-1], y2[-1] = 0.75 - 0.5j, -0.5 + 0.875j
    v, h00, f, beta, _ = probe.init(v0, y1, y2)
    (re, im), (tol_re, tol_im) = check_common(n, v0, y1, probe.seen, v, h00, y2, kdot)
    for rows in defect_rows(n) if n > 1 else []:
        (re1, im1), _ = dotc_ref(v, y2, rows)
        assert abs(re1 - re) >= 100.0 * tol_re and abs(im1 - im) >= 100.0 * tol_im, (n, rows)
    if n == 1:  # one row: every y2 is a multiple of v and the residual is rounding noise
        check_branch(n, v, h00, y2, f, beta, kdot, must_be_zero=False)
        return
    nrm = check_residual(n, v, h00, y2, f, beta, kdot)
    for rows in defect_rows(n):
        (s1, _), _ = dotc_ref(f, f, rows)
        assert abs(float(np.sqrt(s1)) - nrm) >= 100.0 * gamma(kdot + 1) * nrm, (n, rows)


def probe_parallel(probe, rng, kdot, c=1.5 - 0.75j):
    """y2 = c v: f is rounding noise and init must take the branch absmax(f) < eps |H(0, 0)|: f == 0 exactly and beta == 0.

    Whether the branch is CERTAIN is decided here on the CPU: with f_ref = y2 - v H(0, 0) in long double and t the update's bound
    gamma_4 * terms, the device's f lies within t of f_ref and its |f_i| (hypot: one more rounding) within (1 + 2u): if
    max(|f_ref| + |t|) (1 + 2u) < eps |H(0, 0)| the branch must be taken, and f == 0, beta == 0 are asserted.  When that cannot be
    shown, both outcomes are legitimate roundings and the test asserts that the outcome is consistent: zero only if the lower
    bound of max |f_ref| is below the threshold, non-zero only if the f that came back is itself not below it (and then f, beta
    are checked like any residual).  So that the case cannot pass empty-handed, the certain branch is DEMANDED wherever it follows
    a priori (branch_is_forced): |f_ref_i| <= |c| |v_i| | |v|^2 - 1 | with | |v|^2 - 1 | <= 2 gamma_(k_dot + 3) + gamma_k_dot, and
    t <= 12 u |c| |v_i|, against eps |c| = 2 u |c|: certain when (3 k_dot + 18) / sqrt(n) < 2 — for the kernels from n = 4097 on."""
    n = probe.n
    v0 = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
    y1 = unit_phases(n, rng)
    v, h00, f, beta, y2 = probe.init(v0, y1, lambda vv: c * vv)
    check_common(n, v0, y1, probe.seen, v, h00, y2, kdot)
    check_branch(n, v, h00, y2, f, beta, kdot, must_be_zero=branch_is_forced(n, kdot))


def probe_spike(probe, rng, kdot, j, c=1.5 - 0.75j):
    """y2 = c v + 1e-9 c e_j: the residual is one entry of 1e-9 |c| in row j over rounding noise, far above eps |H(0, 0)|, so init
    must NOT zero it — absmax has to see row j (the first row, the last row of a full chunk, the last row).

    The projection spreads the spike over the other rows: f_i = -c v_i conj(v_j) 1e-9 for i != j.  With |v_j| = 1 / sqrt(n) that is
    above eps |c| for every n below 4.5e6 and row j would decide nothing; so y1_j is shrunk by 1e-6 (|v_j| = 1e-6 / sqrt(n)), which
    puts the other rows at 1e-15 |c| / n.  (The norm of y1 then does not feel row j: check_common's last-row condition on v is left
    to the other runs when j = n - 1.)"""
    n = probe.n
    v0 = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
    y1 = unit_phases(n, rng)
    y1[j] *= 1e-6

    def make(vv):
        y = c * vv
        y[j] += 1e-9 * c
        return y

    v, h00, f, beta, y2 = probe.init(v0, y1, make)
    check_common(n, v0, y1, probe.seen, v, h00, y2, kdot, last_row_weighs=j != n - 1)
    eps = np.finfo(np.float64).eps
    (fr, fi), (tre, tim) = update_ref(y2, v, h00)
    lo = np.hypot(np.maximum(np.abs(fr) - gamma(4) * tre, 0), np.maximum(np.abs(fi) - gamma(4) * tim, 0))
    # the branch is certain, and (where that follows a priori, see probe_parallel) it is row j alone that decides it: without
    # row j the maximum is below the threshold
    assert float(lo[j]) * (1 - 2 * U) > 100.0 * eps * abs(h00)
    if branch_is_forced(n, kdot):
        assert float(np.delete(np.hypot(np.abs(fr) + gamma(4) * tre, np.abs(fi) + gamma(4) * tim), j).max()) < eps * abs(h00)
    nrm = check_residual(n, v, h00, y2, f, beta, kdot)
    # a norm that missed row j would be rounding noise: far more than 100 tolerances away
    (s1, _), _ = dotc_ref(np.delete(f, j), np.delete(f, j))
    assert nrm - float(np.sqrt(s1)) >= 100.0 * gamma(kdot + 1) * nrm


def spike_rows(n):
    rows = {0, n - 1}
    if n >= CHUNK:
        rows.add((n // CHUNK) * CHUNK - 1)  # the last row of the last full chunk
        rows.add(CHUNK - 1)                 # ... and of the first
    return sorted(rows)


def run_probe(lib, ctxh, n, dot_roundings):
    assert_long_double()
    kdot = dot_roundings(n)
    rng = np.random.default_rng(1000 + n % 9973)
    probe = Probe(lib, ctxh, n)
    try:
        probe_generic(probe, rng, kdot)
        probe_parallel(probe, rng, kdot)
        for j in spike_rows(n) if n > 1 else []:  # with one row every y2 is a multiple of v: no residual to find
            probe_spike(probe, rng, kdot, j)
    finally:
        probe.close()


# ---------------------------------------------------------------------------------------------------------------------------
# X^H y and f = w - V h over several columns: the general (Arnoldi.h) flow over a dense device operator, one step per call
# ---------------------------------------------------------------------------------------------------------------------------
def matvec_ld(A, x, block=256):
    """A x in long double, a block of rows at a time (A stays complex128 in memory)."""
    xr, xi = parts(x)
    out_r, out_i = np.empty(A.shape[0], dtype=LD), np.empty(A.shape[0], dtype=LD)
    for r0 in range(0, A.shape[0], block):
        ar, ai = parts(A[r0: r0 + block])
        out_r[r0: r0 + block] = ar @ xr - ai @ xi
        out_i[r0: r0 + block] = ar @ xi + ai @ xr
    return out_r, out_i


def run_steps(lib, ctxh, n, m):
    """After every single step i -> i + 1 of the general flow: H[:i+1, i] against the long-double V^H (A v_i) of the downloaded
    basis, f against A v_i - V H[:i+1, i], and zfac_checks.check_identities — all three at the bar of zfac_checks.py (1e-12 for
    n <= 100, else 1e-11, times max(1, the largest absolute row sum of A)); that bar is the suite's existing one and is reused, not
    derived.  i + 1 runs through 2 ... m, so X^H y and the update run with every column count up to m."""
    assert_long_double()
    A = Z.matrix(n, False, 200 + n)
    tol = 1e-12 if n <= 100 else 1e-11
    scale = max(1.0, float(np.abs(A).sum(axis=1).max()))
    D, fac = C.c_void_p(), C.c_void_p()
    ok(lib.mispec_zdense_upload(ctxh, n, n, dp(A), n, 0, b"\0", C.byref(D)))
    ok(lib.mispec_zfac_create_dense(ctxh, D, m, 0, C.byref(fac)))
    try:
        rng = np.random.default_rng(11)
        v0 = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
        ops = C.c_int64(0)
        ok(lib.mispec_zfac_init(fac, dp(v0), C.byref(ops)))
        H = np.zeros((m, m), dtype=np.complex128, order="F")
        V = np.zeros((n, m), dtype=np.complex128, order="F")
        f = np.zeros(n, dtype=np.complex128)
        beta = C.c_double()
        worst = 0.0
        for i in range(0, m):
            if i > 0:
                ok(lib.mispec_zfac_factorize(fac, i, i + 1, C.byref(ops)))
            assert lib.mispec_zfac_subspace_dim(fac) == i + 1
            ok(lib.mispec_zfac_get_H(fac, dp(H)))
            ok(lib.mispec_zfac_get_V(fac, m, dp(V)))
            ok(lib.mispec_zfac_get_f(fac, dp(f)))
            ok(lib.mispec_zfac_f_norm(fac, C.byref(beta)))
            Z.check_identities(A, V, H, f, i + 1, beta.value, tol)
            wr, wi = matvec_ld(A, V[:, i])
            Vr, Vi = parts(V[:, : i + 1])
            hr, hi = Vr.T @ wr + Vi.T @ wi, Vr.T @ wi - Vi.T @ wr           # V^H w
            err_h = max(float(np.abs(H[: i + 1, i].real - hr).max()), float(np.abs(H[: i + 1, i].imag - hi).max()))
            Hr, Hi = parts(H[: i + 1, i])
            fr, fi = wr - (Vr @ Hr - Vi @ Hi), wi - (Vr @ Hi + Vi @ Hr)     # w - V h
            err_f = max(float(np.abs(f.real - fr).max()), float(np.abs(f.imag - fi).max()))
            worst = max(worst, err_h, err_f)
            assert err_h <= tol * scale and err_f <= tol * scale, (i, err_h, err_f)
            # the defects this is aimed at: the last row left out of every sum; the last column (its group of 8) left out
            dr = np.abs(Vr[-1] * wr[-1] + Vi[-1] * wi[-1]).max()
            assert dr >= 100.0 * tol * scale and abs(H[i, i]) >= 100.0 * tol * scale, (i, float(dr), abs(H[i, i]))
            assert float(np.abs(Vr[:, i] * Hr[i] - Vi[:, i] * Hi[i]).max()) >= 100.0 * tol * scale  # f without the last column
        print(f"steps n={n} m={m}: worst |dH|, |df| = {worst:.3e} (bar {tol * scale:.3e})")
        assert ops.value == 2 + (m - 1)
    finally:
        ok(lib.mispec_zfac_destroy(fac))
        ok(lib.mispec_zdense_destroy(D))
