"""Checks of the REAL orthogonalisation and V*Q kernels (spectra_amd/csrc/krylov.hip: k_orth, k_reduce_partials, k_scale,
k_lanczos_epilogue, k_vq, k_axpby; csrc/orth_dma_modes.hip: k_orth_dma; their launchers' slot dispatch: csrc/orth_launch.hpp; the
step code of csrc/fac.hip) one step at a time, written
against the Factorization interface (init, factorize_from, matrix_V / matrix_H, vector_f, f_norm, num_operations, ritz_vectors,
compress_V): tests/test_gpu_krylov_kernels.py runs them on sa.Factorization, tests/test_host_krylov_checks.py on a float64 numpy
stand-in of the reference's control flow, honest and with targeted defects.

The probe.  A scripted operator ignores its input and answers column j of a matrix W (n x (m + 1), uniform in (-1, 1)) to its
j-th call; call 0 and 1 belong to init (v = y0 / |y0|, then H(0, 0) = <v, y1>, f = y1 - v H(0, 0)), call i + 1 is the w of step i.
Every readable quantity of a factorisation is then one kernel applied to known data.  collect() advances the factorisation ONE
step per call and reads f and beta after each, so every step's residual (overwritten by the next step) and the beta a Lanczos step
used (overwritten in H by the correction) are known; the number of operator calls must equal num_operations() and m + 1.

Tolerances are Higham's gamma_k = k u / (1 - k u), u = 2^-53, times the sum of the absolute values of the terms; k is the number
of roundings on the longest path, counted from the source (HipModel below; HostModel for the numpy stand-in); references are
numpy.longdouble.  The sums of absolute values are formed in float64 (all terms positive: their own relative error is below 1e-10
and is ignored).  A bound is never tuned from an observation.

  k_dot (one coefficient of V'x; the same path carries sum f^2):
      a lane multiplies (1) and adds the two products of each of its R row pairs of a tile to its running sum: 2 R additions
      per tile, T tiles per workgroup; the wavefront's shuffle tree (6); k_reduce_partials: a lane adds its ceil(nrec / 64)
      records, then the shuffle tree (6):                       k_dot = 1 + 2 R T + 6 + ceil(nrec / 64) + 6
      k_orth: R = 2 while ceil(ncol / 4) <= 10, else 1; tiles of 128 R rows; nrec = min(tiles, 4 CUs); a basis of more than 64
      columns goes in panels of 64 on ONE grid min(ceil(n / 256), 4 CUs), each panel with its own R.
      k_orth_dma (one panel, n >= 131072, unless option orth_kernel=reg): tiles of 128 rows (R = 1), nrec = min(tiles, CUs).
      The largest k over the launches of a step is used for every column of the step.
  k_upd (one row of dst = src - V c): the product (1), the S slot sums of a wavefront (S additions), the four-wavefront sum
      through LDS (2), the subtraction (1): S + 4 per panel, panels subtract one after the other: k_upd = sum over panels (S + 4);
      S = ceil(panel columns / 4) for k_orth, rounded up to an even number (at least 2) for k_orth_dma.
  f = w - alpha v (ORTH_RESID_VTF, init and every Lanczos step): 2.  w - beta v_prev in k_lanczos_epilogue: 2.
  alpha = <v, w> (k_lanczos_epilogue + k_reduce_sum): product (1), 2 additions per row pair and I = ceil(pairs / (256 grid))
      pairs per thread, shuffle tree (6), four wavefronts (2), k_reduce_sum: ceil(grid / 1024) + 6 + 16.
  v = f / beta (k_scale, k_scale_step): one division: 1.
  V Q (k_vq): one running sum over the m terms, continued across the input panels of 64: the issue's m + ceil(m / 64).
  f q + x h (k_axpby): a product and the addition on either term's path: gamma_2 (|f q| + |x h|); its sum f^2: 1 + 2 I + 6 + 2 +
      ceil(grid / 64) + 6 with I = ceil(pairs / (256 grid)), grid = min(4 CUs, ceil(pairs / 256)).
  H(i, i) = alpha + c_i, H(i, i - 1) = beta_i + c_(i-1) (Lanczos): one addition per correction pass, at most five: gamma_5 of
      the two terms, beside the bounds of the dot products that made them.
  beta = sqrt(sum f^2): the square root halves the relative error of the sum and adds one rounding: gamma_(k + 1) throughout.

Where the correction loop of a step ran (Arnoldi.h:264-291, Lanczos.h:156-182: at most five passes), every pass repeats the
update on terms that are, to first order, bounded by the first pass's (|f_p| <= |w| + |V||h|, and the later coefficients are of
the size of the first pass's error — asserted on the CPU: the long-double residual is not larger than w), and H collects one
addition per pass: k = 6 k_upd + 5 there (Arnoldi: first pass + 5; Lanczos: 4 + 5 k_upd + 5 with the residual's 4).

Large vectors (n > 4099): per-row references are long double on the first 256 rows, the last 256 rows and 16 seeded rows, and
float64 BLAS on all rows at the bar tests/herm_checks.py derives for that comparison: the kernel's gamma_k plus the reference's own
gamma (one running sum of the same number of terms in whatever order the BLAS takes them, + 1 for the product), times the same sum
of absolute values.  Dot products over all n rows are long double at the column counts LD_NCOLS, float64 at the others."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
EPS = 2.0 ** -52
LD_ALL_ROWS = 4099  # up to here every row is checked in long double
LD_NCOLS = (1, 4, 5, 40, 41, 44, 45, 63, 64)  # larger n: the column counts whose dot products are checked in long double
PANEL = 64  # kPanelCols
_POOL = ThreadPoolExecutor(8)  # numpy's long-double products are single-threaded loops that release the GIL


def assert_long_double():
    assert np.finfo(LD).eps < 1e-18, "numpy.longdouble is not wider than double here: the references would prove nothing"


def gamma(k):
    return k * U / (1.0 - k * U)


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------
# the roundings, counted from the launch code
# ---------------------------------------------------------------------------------------------------------------------------
class HipModel:
    """What launch_orth / launch_orth_panel / launch_orth_dma_mode / launch_vq / launch_axpby (csrc) launch for given sizes."""

    def __init__(self, cus, force_reg=False):
        self.cus, self.force_reg = int(cus), force_reg

    def orth_launches(self, n, ncol):
        """One dict per launch of a pass over V[:, :ncol]: kernel, S (slots per wavefront), R, T (tiles per workgroup), nrec."""
        if ncol <= PANEL:
            slots = cdiv(ncol, 4)
            if not self.force_reg and ncol >= 1 and n >= 1024 * 128:
                tiles = cdiv(n, 128)
                grid = min(tiles, self.cus)
                S = min(2 * max(1, (slots + 1) // 2), 16)
                return [dict(kernel="k_orth_dma", S=S, R=1, T=cdiv(tiles, grid), nrec=grid, col0=0, depth=3 if S <= 10 else 2)]
            R = 2 if slots <= 10 else 1
            tiles = cdiv(n, 128 * R)
            grid = max(1, min(tiles, 4 * self.cus))
            return [dict(kernel="k_orth", S=min(max(slots, 1), 16), R=R, T=cdiv(tiles, grid), nrec=grid, col0=0)]
        grid = max(1, min(cdiv(n, 256), 4 * self.cus))
        out = []
        for col0 in range(0, ncol, PANEL):
            slots = cdiv(min(PANEL, ncol - col0), 4)
            R = 2 if slots <= 10 else 1
            out.append(dict(kernel="k_orth", S=min(slots, 16), R=R, T=cdiv(cdiv(n, 128 * R), grid), nrec=grid, col0=col0))
        return out

    def k_dot(self, n, ncol):
        return max(1 + 2 * L["R"] * L["T"] + 6 + cdiv(L["nrec"], 64) + 6 for L in self.orth_launches(n, ncol))

    def k_upd(self, n, ncol):
        return sum(L["S"] + 4 for L in self.orth_launches(n, ncol))

    def _stream(self, n):
        pairs = (n + 1) // 2
        grid = max(1, min(4 * self.cus, cdiv(pairs, 256)))
        return grid, cdiv(pairs, 256 * grid)

    def k_epilogue(self, n):
        grid, per_thread = self._stream(n)
        return 1 + 2 * per_thread + 6 + 2 + cdiv(grid, 1024) + 6 + 16

    def k_axpby_norm(self, n):
        grid, per_thread = self._stream(n)
        return 1 + 2 * per_thread + 6 + 2 + cdiv(grid, 64) + 6

    def k_vq(self, m):
        return m + cdiv(m, PANEL)

    def k_ref_dot(self, n):  # the float64 reference's own roundings
        return n + 1

    def describe(self, n, ncol):
        return "; ".join(f"{L['kernel']}<S={L['S']},R={L['R']}> col0={L['col0']} tiles/wg={L['T']} records={L['nrec']}"
                         for L in self.orth_launches(n, ncol))


class HostModel:
    """The numpy stand-in: every sum is one float64 BLAS / pairwise sum of the full length, in whatever order."""

    def k_dot(self, n, ncol):
        return n + 1

    def k_upd(self, n, ncol):
        return ncol + 2

    def k_epilogue(self, n):
        return n + 1

    def k_axpby_norm(self, n):
        return n + 1

    def k_vq(self, m):
        return m + 1

    def k_ref_dot(self, n):
        return n + 1


# ---------------------------------------------------------------------------------------------------------------------------
# the scripted operators
# ---------------------------------------------------------------------------------------------------------------------------
def script_matrix(n, m, seed):
    """W: n x (m + 1), uniform in (-1, 1), column-major; no entry of the last row negligible (the defects aimed at are one row)."""
    rng = np.random.default_rng(seed)
    W = np.asfortranarray(rng.uniform(-1.0, 1.0, (n, m + 1)))
    W[-1, :] = np.where(W[-1, :] < 0, -1.0, 1.0) * (0.5 + 0.5 * np.abs(W[-1, :]))
    return W


class HostScript:
    """rows / cols / perform_op on host arrays (the reference's operator concept): answers W[:, j] to call j, records its inputs.
    forced: from call 2 on the answer is V c + 1e-3 r with the columns seen so far (V[:, i] is the input of call i + 1), c and r
    uniform in (-1, 1): the residual is 1e-3 of the projected part, so the 0.717 test fails and the correction loop runs."""

    def __init__(self, W, forced=False, seed=0, record=True):
        self.W, self.n, self.calls, self.forced = W, W.shape[0], 0, forced
        self.seen = np.zeros(W.shape, order="F") if (record or forced) else None  # (large vectors: the count alone)
        self.rng = np.random.default_rng(seed)

    def rows(self):
        return self.n

    def cols(self):
        return self.n

    def perform_op(self, x):
        j = self.calls
        assert j < self.W.shape[1], "the factorisation applied the operator more often than the script is long"
        if self.seen is not None:
            self.seen[:, j] = x
        if self.forced and j >= 2:
            c = self.rng.uniform(-1.0, 1.0, j)
            self.W[:, j] = self.seen[:, 1: j + 1] @ c + 1e-3 * self.rng.uniform(-1.0, 1.0, self.n)
        self.calls += 1
        return self.W[:, j]


class DeviceScript:
    """The callback of sa.DeviceOp: call j enqueues a device-to-device copy of W[:, j] into y on the given stream (hipMemcpyAsync
    through ctypes; W lives in a torch device tensor, one column per contiguous row of W.T)."""

    def __init__(self, W):
        import torch

        self.W, self.n, self.calls = W, W.shape[0], 0
        self.Wd = torch.from_numpy(np.ascontiguousarray(W.T)).to("cuda")
        torch.cuda.synchronize()
        # the HIP runtime this process already runs on (the one torch and libmispec.so loaded), not a second copy
        loaded = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64.so" in line})
        self.hip = ctypes.CDLL(loaded[0] if loaded else "libamdhip64.so")
        self.hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
        self.hip.hipMemcpyAsync.restype = ctypes.c_int

    def __call__(self, x_ptr, y_ptr, stream):
        j = self.calls
        if j >= self.W.shape[1]:
            raise RuntimeError("the factorisation applied the operator more often than the script is long")
        src = self.Wd.data_ptr() + j * self.n * 8
        rc = self.hip.hipMemcpyAsync(y_ptr, src, self.n * 8, 3, stream)  # 3: hipMemcpyDeviceToDevice
        if rc != 0:
            raise RuntimeError(f"hipMemcpyAsync: {rc}")
        self.calls += 1


# ---------------------------------------------------------------------------------------------------------------------------
# running a factorisation one step at a time
# ---------------------------------------------------------------------------------------------------------------------------
class Run:
    pass


def collect(fac, script, m, v0, symmetric):
    """init(v0), then one step per factorize_from call; f and beta after every step, V and H once at the end."""
    r = Run()
    r.n, r.m, r.symmetric, r.W, r.v0 = script.n, m, symmetric, script.W, v0
    fac.init(v0)
    r.fs, r.betas = [fac.vector_f()], [fac.f_norm()]
    for i in range(1, m):
        fac.factorize_from(i, i + 1)
        r.fs.append(fac.vector_f())
        r.betas.append(fac.f_norm())
    r.ops = fac.num_operations()
    assert script.calls == r.ops == m + 1, (script.calls, r.ops, m + 1)  # init: 2, every step: 1 — no restart, no repeated step
    r.V, r.H = np.asfortranarray(fac.matrix_V()), fac.matrix_H()
    r.seen = getattr(script, "seen", None)
    return r


def collect_at_once(fac, script, m, v0):
    """The same factorisation in ONE factorize_from(1, m): (V, H, f, beta), to be compared with collect() bit for bit — the sums
    are taken in a fixed order, so the steps enqueued in one run must equal the same steps run one by one.
    Also returns the host synchronisations factorize_from took (0 where the factorisation keeps no such count)."""
    syncs = (lambda: fac.get_profile()["n_host_sync"]) if hasattr(fac, "get_profile") else (lambda: 0)
    fac.init(v0)
    before = syncs()
    fac.factorize_from(1, m)
    took = syncs() - before
    assert script.calls == fac.num_operations() == m + 1, (script.calls, fac.num_operations(), m + 1)
    return (np.asfortranarray(fac.matrix_V()), fac.matrix_H(), fac.vector_f(), fac.f_norm()), took


def assert_same_factorisation(run, at_once):
    V, H, f, beta = at_once
    assert np.array_equal(V, run.V) and np.array_equal(H, run.H)
    assert np.array_equal(f, run.fs[-1]) and beta == run.betas[-1]


# ---------------------------------------------------------------------------------------------------------------------------
# long-double helpers
# ---------------------------------------------------------------------------------------------------------------------------
def _chunks(n, parts=8, least=8192):
    step = max(least, cdiv(n, parts))
    return [(a, min(n, a + step)) for a in range(0, n, step)]


def ld_rows_dot(AT, x, ncol):
    """AT[:ncol] @ x in long double (AT: the transposed basis, C-contiguous long double)."""
    parts = list(_POOL.map(lambda ab: AT[:ncol, ab[0]: ab[1]] @ x[ab[0]: ab[1]], _chunks(x.shape[0])))
    return np.sum(parts, axis=0, dtype=LD)


def sample_rows(n, seed=0):
    if n <= LD_ALL_ROWS:
        return np.arange(n)
    rng = np.random.default_rng(seed)
    return np.array(sorted(set(range(256)) | set(range(n - 256, n)) | set(int(r) for r in rng.integers(0, n, 16))))


class Basis:
    """The downloaded basis with its long-double transpose and, on demand, the long-double Gram matrix (column by column)."""

    def __init__(self, V):
        self.V = V
        self.n, self.m = V.shape
        self.VT = np.ascontiguousarray(V.T).astype(LD)
        self.absV = np.abs(V)
        self.G = np.zeros((self.m, self.m), dtype=LD)
        self.gcols = 0
        self.rows = sample_rows(self.n)
        self.Vrows = self.VT[:, self.rows].T.copy()  # long double, rows x m

    def gram(self, ncol):
        while self.gcols < ncol:
            j = self.gcols
            g = ld_rows_dot(self.VT, self.VT[j], j + 1)
            self.G[: j + 1, j] = g
            self.G[j, : j + 1] = g
            self.gcols += 1
        return self.G[:ncol, :ncol]

    def orth_defect(self, ncol):
        return np.abs(np.eye(ncol, dtype=LD) - self.gram(ncol))


def ld_dot_wanted(n, ncol):
    return n <= LD_ALL_ROWS or ncol in LD_NCOLS


def ld_norm(x):
    xl = x.astype(LD)
    return np.sqrt(xl @ xl)


def _ratio(err, tol):
    """max err / tol over the entries; an exact hit on a zero tolerance counts as 0, a miss as infinite."""
    err, tol = np.atleast_1d(np.asarray(err, dtype=LD)), np.atleast_1d(np.asarray(tol, dtype=LD))
    out = np.zeros(err.shape, dtype=np.float64)
    pos = tol > 0
    out[pos] = (err[pos] / tol[pos]).astype(np.float64)
    out[~pos & (err > 0)] = np.inf
    return float(out.max()) if out.size else 0.0


class Ratios(dict):
    """Worst error / tolerance per kind of check."""

    def add(self, key, value, where):
        if value > self.get(key, (-1.0, None))[0]:
            self[key] = (value, where)

    def worst(self):
        return max(v for v, _ in self.values())

    def assert_ok(self, what):
        print(what + ": " + ", ".join(f"{k} {v:.3e} of its bound (step {w})" for k, (v, w) in sorted(self.items())))
        bad = {k: vw for k, vw in self.items() if not vw[0] <= 1.0}
        assert not bad, (what, bad)


# ---------------------------------------------------------------------------------------------------------------------------
# the checks of the steps
# ---------------------------------------------------------------------------------------------------------------------------
def check_init(run, B, model, out):
    """Step 0, both flows: v = y0 / |y0| (k_scale), H(0, 0) = <v, y1> (k_lanczos_epilogue), f = y1 - v H(0, 0) (ORTH_RESID_VTF,
    one column), beta = |f|.  With one row f is rounding noise and init may zero it: every bound below holds either way."""
    n, W, V, H = run.n, run.W, run.V, run.H
    if run.seen is not None:
        assert np.array_equal(run.seen[:, 0], run.v0)  # upload and the download in front of the operator: exact
        assert np.array_equal(run.seen[:, 1], V[:, 0])  # the second input is the normalised column, bit for bit
    y0 = W[:, 0].astype(LD)
    q = y0 / np.sqrt(y0 @ y0)
    k0 = model.k_dot(n, 0)  # the norm of y0: the pass with no column
    out.add("v0", _ratio(np.abs(V[:, 0] - q), gamma(k0 + 1 + 1) * np.abs(q)), 0)
    w = W[:, 1].astype(LD)
    v = B.VT[0]
    out.add("h", _ratio(abs(H[0, 0] - v @ w), gamma(model.k_epilogue(n)) * (B.absV[:, 0] @ np.abs(W[:, 1]))), 0)
    f = run.fs[0].astype(LD)
    out.add("inv", _ratio(np.abs(w - v * LD(H[0, 0]) - f), gamma(2) * (np.abs(w) + np.abs(v * LD(H[0, 0])))), 0)
    nrm = ld_norm(run.fs[0])
    out.add("beta", _ratio(abs(run.betas[0] - nrm), gamma(model.k_dot(n, 1) + 1) * nrm), 0)


def check_scale(run, B, i, out):
    """V[:, i + 1] = f_i / beta_i: one division per entry (k_scale / k_scale_step), all rows in long double."""
    q = run.fs[i].astype(LD) / LD(run.betas[i])
    out.add("scale", _ratio(np.abs(run.V[:, i + 1] - q), gamma(1) * np.abs(q)), i)
    if run.seen is not None:
        assert np.array_equal(run.seen[:, i + 2], run.V[:, i + 1]), i  # ... and it is what the operator was given next


def check_arnoldi(run, model):
    """The four checks of every Arnoldi step (see the module text); returns the worst error / bound per check."""
    assert_long_double()
    n, m, W, V, H = run.n, run.m, run.W, run.V, run.H
    B = Basis(V)
    out = Ratios()
    check_init(run, B, model, out)
    if m > 1:
        check_scale(run, B, 0, out)
    rows = B.rows
    beta_thresh = EPS * np.sqrt(n)
    for i in range(1, m):
        ncol = i + 1
        w64, h64, f64, beta = W[:, i + 1], H[:ncol, i], run.fs[i], run.betas[i]
        assert H[i, i - 1] == run.betas[i - 1] and not H[i + 2:, i].any()  # Arnoldi.h:239; nothing below the subdiagonal
        kdot, kupd = model.k_dot(n, ncol), model.k_upd(n, ncol)
        S = B.absV[:, :ncol].T @ np.abs(w64)
        # 1. h = V'w
        if ld_dot_wanted(n, ncol):
            href = ld_rows_dot(B.VT, w64.astype(LD), ncol)
            tol_h = gamma(kdot) * S
        else:
            href = V[:, :ncol].T @ w64
            tol_h = (gamma(kdot) + gamma(model.k_ref_dot(n))) * S
        # did the correction loop run?  Decided from the reference, far from the 0.717 threshold (Arnoldi.h:257)
        wn2 = float(w64 @ w64)
        hn = float(np.sqrt(np.sum(np.asarray(href, dtype=np.float64) ** 2)))
        beta_ref = np.sqrt(max(wn2 - hn * hn, 0.0)) if ncol < n else 0.0
        ratio = beta_ref / (0.717 * hn)
        assert abs(ratio - 1.0) > 1e-3, ("the script puts a step on the 0.717 threshold: change the data", i, ratio)
        loop = ratio < 1.0
        if loop:
            tol_h = tol_h + B.orth_defect(ncol) @ np.abs(h64).astype(LD)
            assert float(ld_norm(f64)) <= np.sqrt(wn2)  # the later passes' terms stay below the first pass's
        if ncol < n:  # (with as many columns as rows the residual is rounding noise and any branch may be taken)
            assert beta > 1e3 * beta_thresh, ("a tiny-beta branch is within reach: change the data", i, beta)
        out.add("h", _ratio(np.abs(h64 - href), tol_h), i)
        # 2. w - V h - f = 0, row by row, with the h and f the device reports
        K = 6 * kupd + 5 if loop else kupd
        hl = h64.astype(LD)
        res = w64[rows].astype(LD) - B.Vrows[:, :ncol] @ hl - f64[rows].astype(LD)
        terms = np.abs(w64[rows]) + B.absV[rows, :ncol] @ np.abs(h64)
        out.add("inv", _ratio(np.abs(res), gamma(K) * terms), i)
        if n > LD_ALL_ROWS:
            res64 = w64 - V[:, :ncol] @ h64 - f64
            terms64 = np.abs(w64) + B.absV[:, :ncol] @ np.abs(h64)
            out.add("inv64", _ratio(np.abs(res64), (gamma(K) + gamma(ncol + 2)) * terms64), i)
        # 3. beta = |f|
        nrm = ld_norm(f64)
        out.add("beta", _ratio(abs(beta - nrm), gamma(kdot + 1) * nrm), i)
        # 4. the next column
        if i + 1 < m:
            check_scale(run, B, i, out)
    return out


def check_lanczos(run, model):
    """Every Lanczos step (reference flow) against the converged projection r = (I - V V')(w - beta v_prev): two classical
    Gram-Schmidt passes in long double, the second through the long-double Gram matrix (V'(f0 - V c) = (I - V'V) c)."""
    assert_long_double()
    n, m, W, V, H = run.n, run.m, run.W, run.V, run.H
    B = Basis(V)
    out = Ratios()
    check_init(run, B, model, out)
    if m > 1:
        check_scale(run, B, 0, out)
    rows = B.rows
    beta_thresh = EPS * np.sqrt(n)
    assert np.array_equal(H, H.T) and not np.triu(H, 2).any()  # tridiagonal and symmetric, exactly (Lanczos.h:85-86, :174)
    kepi = model.k_epilogue(n)
    for i in range(1, m):
        ncol = i + 1
        w64, f64, beta_i, beta = W[:, i + 1], run.fs[i], run.betas[i - 1], run.betas[i]
        kdot, kupd = model.k_dot(n, ncol), model.k_upd(n, ncol)
        K = 4 + 5 * kupd + 5
        use_ld = ld_dot_wanted(n, ncol)
        T = LD if use_ld else np.float64
        vp, vi = (B.VT[i - 1], B.VT[i]) if use_ld else (V[:, i - 1], V[:, i])
        t = w64.astype(T) - T(beta_i) * vp                      # Lanczos.h:139
        alpha = vi @ t                                          # :142
        f0 = t - alpha * vi                                     # :145 — the three-term residual
        absf0 = np.abs(np.asarray(f0, dtype=np.float64))
        c = ld_rows_dot(B.VT, f0, ncol) if use_ld else (V[:, :ncol].T @ f0).astype(LD)
        D = B.orth_defect(ncol)
        c2 = (np.eye(ncol, dtype=LD) - B.gram(ncol)) @ c        # V'(f0 - V c)
        ref_dot = 0.0 if use_ld else gamma(model.k_ref_dot(n))
        tol_c = (gamma(kdot) + ref_dot) * (B.absV[:, :ncol].T @ absf0) + D @ np.abs(c)   # per coefficient
        absc = np.abs(c).astype(np.float64)
        # the residual the device holds after the step, against r
        r_rows = np.asarray(f0[rows], dtype=LD) - B.Vrows[:, :ncol] @ (c + c2)
        part1 = np.abs(w64[rows]) + np.abs(beta_i * V[rows, i - 1]) + B.absV[rows, :ncol] @ absc
        tol_r = gamma(K) * part1 + B.absV[rows, :ncol].astype(LD) @ tol_c
        if use_ld:
            out.add("r", _ratio(np.abs(f64[rows].astype(LD) - r_rows), tol_r), i)
        if n > LD_ALL_ROWS or not use_ld:
            cc = (c + c2).astype(np.float64)
            r64 = np.asarray(f0, dtype=np.float64) - V[:, :ncol] @ cc
            p1 = np.abs(w64) + np.abs(beta_i * V[:, i - 1]) + B.absV[:, :ncol] @ absc
            tol64 = (gamma(K) + gamma(ncol + 4)) * p1 + B.absV[:, :ncol] @ tol_c.astype(np.float64)
            out.add("r64", _ratio(np.abs(f64 - r64), tol64), i)
        r_norm = float(ld_norm(f64))
        if ncol < n:
            assert r_norm > 1e3 * beta_thresh, ("a tiny-beta branch is within reach: change the data", i, r_norm)
            assert r_norm <= float(np.sqrt(w64 @ w64)) * 1.0001 + abs(beta_i)  # the later passes' terms stay below the first's
        # H(i, i) = alpha + c_i and H(i, i - 1) = beta_i + c_(i-1): the epilogue's dot, the pass's dot, the orthogonality term
        tol_a = (gamma(kepi + 2) + ref_dot) * (B.absV[:, i] @ (np.abs(w64) + np.abs(beta_i * V[:, i - 1])))
        out.add("alpha", _ratio(abs(LD(H[i, i]) - (alpha + c[i])), tol_a + tol_c[i] + gamma(5) * (abs(alpha) + abs(c[i]))), i)
        out.add("subd", _ratio(abs(LD(H[i, i - 1]) - (LD(beta_i) + c[i - 1])), tol_c[i - 1] + gamma(5) * (beta_i + abs(c[i - 1]))), i)
        nrm = ld_norm(f64)
        out.add("beta", _ratio(abs(beta - nrm), gamma(kdot + 1) * nrm), i)
        if i + 1 < m:
            check_scale(run, B, i, out)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# V * Q
# ---------------------------------------------------------------------------------------------------------------------------
def check_product(X, V, Q, model, out, key, where):
    """X = V Q, element by element: gamma_(k_vq(m)) (|V||Q|); long double on the sampled rows, float64 BLAS on all rows of a
    large vector at the kernel's gamma plus the reference's own gamma_(m + 1)."""
    n, m = V.shape
    k = model.k_vq(m)
    rows = sample_rows(n)
    absT = np.abs(V) @ np.abs(Q)
    ref = V[rows].astype(LD) @ Q.astype(LD)
    out.add(key, _ratio(np.abs(X[rows] - ref), gamma(k) * absT[rows]), where)
    if n > LD_ALL_ROWS:
        out.add(key + "64", _ratio(np.abs(X - V @ Q), (gamma(k) + gamma(m + 1)) * absT), where)


def check_ritz(fac, V, p, model, out, seed=5):
    m = V.shape[1]
    Y = np.asfortranarray(np.random.default_rng(seed + p).uniform(-1.0, 1.0, (m, p)))
    X = fac.ritz_vectors(Y)
    assert X.shape == (V.shape[0], p)
    check_product(X, V, Y, model, out, "ritz", p)


def check_compress(fac, V, f, k, model, out, seed=9):
    """compress_V(Q, H, k) with a random dense Q: columns 0..k = V Q[:, :k+1], the others untouched bit for bit, the new residual
    f Q(m-1, k-1) + X[:, k] H(k, k-1) (k_axpby: two products, one addition) and beta = its norm."""
    assert_long_double()
    n, m = V.shape
    rng = np.random.default_rng(seed + k)
    Q = np.asfortranarray(rng.uniform(-1.0, 1.0, (m, m)))
    Hn = np.asfortranarray(rng.uniform(-1.0, 1.0, (m, m)))
    fac.compress_V(Q, Hn, k)
    Vn, fn, beta = fac.matrix_V(), fac.vector_f(), fac.f_norm()
    check_product(Vn[:, : k + 1], V, Q[:, : k + 1], model, out, "compress", k)
    assert np.array_equal(Vn[:, k + 1:], V[:, k + 1:]), "compress_V wrote a column beyond k"
    q, h = LD(Q[m - 1, k - 1]), LD(Hn[k, k - 1])
    a, b = f.astype(LD) * q, Vn[:, k].astype(LD) * h
    out.add("newf", _ratio(np.abs(fn - (a + b)), gamma(2) * (np.abs(a) + np.abs(b))), k)
    nrm = ld_norm(fn)
    out.add("newbeta", _ratio(abs(beta - nrm), gamma(model.k_axpby_norm(n) + 1) * nrm), k)
