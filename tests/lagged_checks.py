"""Checks of the one-sweep ("lagged") Lanczos kernels ONE PASS AT A TIME (csrc/krylov.hip k_orth_lagged, csrc/orth_dma.hip
k_orth_lagged_dma, csrc/orth_wide.hip k_lagged_last_panel / k_lagged_dots behind the subtracting ORTH_CORRECT_ONLY panels,
k_reduce_partials with the tails finish_lagged / start_next_onered / finish_fused_restart, k_vq_fused), written against the two
test hooks sa.lagged_pass and sa.fused_restart_pass (include/mispec.h): they run one pass, its reduction and its tail on the
caller's data through the launchers and argument helpers the factorisation uses.  tests/test_gpu_lagged_kernels.py runs the
checks on the GPU, tests/test_host_lagged_checks.py on a float64 numpy stand-in, honest and with targeted defects.

Rules (those of tests/krylov_checks.py): references are numpy.longdouble; a tolerance is Higham's gamma_k = k u / (1 - k u),
u = 2^-53, times the sum of the absolute values of the terms; k is the number of roundings on the longest path, counted from the
source, a product-and-add counted as two (so the bound holds whether or not the compiler contracts it); sums of absolute values
are formed in float64; a bound is never tuned from an observation.  Because the hooks take arbitrary data every output is one
operation on known inputs; dot products are referred to the STORED bits of column i and of the new f.

Pass (a), step i over V[:, :i]  (LaggedModel.lagged(n, i): kernel, MAXS, R, NW, ring depth, grid, tiles per workgroup T, records)
  v_i = (f - V c_in) / beta     a wavefront's sum p of its MAXS columns: product (1), MAXS additions; the sum of the NW
      wavefronts' p through LDS: 2 (NW = 4: (p0 + p1) + (p2 + p3)) or 3 (NW = 8: the second four are added to the first);
      f - p (1); / beta (1):                                         k_vi = MAXS + 5 (NW = 4), MAXS + 6 (NW = 8)
      in panels (i >= 128, npan = ceil(i / 64)): a term of panel q < npan - 1 goes through k_orth<CORRECT_ONLY, 16, 1> — product
      (1), 16 additions, LDS (2) — and one subtraction per panel q ... npan - 1, then the division: 19 + (npan - q) + 1; a term
      of the last panel (MAXS = ceil(width / 4)): 1 + MAXS + 2 + 1 + 1:      k_vi = max(20 + npan, MAXS + 5)
      pending = 0: c_in counts as zero and column i must equal f / beta in float64 BIT FOR BIT.
  w = src (two reductions: exact) or src / beta - beta V[:, i-1] (one reduction: division or product, subtraction: 2)
  dst = w - alpha v_i           from the stored v_i: product (1), subtraction (1), behind w's 2:   k_dst = 2 (+ 1 one-reduction: 3)
  c_j = <V_j, dst>, slot i = <v_i, dst>, chk_j = <V_j, v_i>, sum dst^2     per lane and row pair acc += a x + b y: product (1),
      the pair's addition (1), one addition to acc per row pair of the lane (R T); the wavefront's shuffle tree (6);
      k_reduce_partials: a lane adds its ceil(records / 64) records, shuffle tree (6) — the one-round form (at most 256 records,
      2 i + 3 <= 96: RPL = 1, 2, 4 records per lane) and the passes of 48 columns add in the same order:
                                                                     k_dot = 2 + R T + 6 + ceil(records / 64) + 6
  max |dst|: exact.  Rows from n (rounded up to even) on: untouched.  The odd pad row n: written with 0 (the hooks' contract).
Tail of (a) (finish_lagged, start_next_onered), restated in float64 below (tail_lagged): decisions and integers exactly (the data
keeps every comparison at least 0.1 % from its threshold: asserted); values against the long-double value of the same formula
on the reduced record:
  beta = sqrt(sum f^2): 1.  c2 = sum_{j <= i} red[j]^2 in index order (scan_abs_sq): product (1) + i + 1 additions;
  beta = sqrt(gamma2 - c2): (gamma_(i + 3) (gamma2 + c2) / (gamma2 - c2) + gamma_1) beta (the root is not credited with halving)
  diag[i] = (alpha - cp1) + red[i]: 2.  subd[i-1] = (beta - (subd[i-2] cp2 + diag[i-1] cp1) / beta) + red[i-1]: product, addition,
  division, subtraction, addition: 5.  lag_rel_c_max = sqrt(c2) / gamma: i + 2, root, root, division: gamma_(i + 5).
  alpha~ = s1 / beta^2 - red[i], s1 the sum of the product's partial sums in k_reduce_sum's order: a thread adds its
  ceil(count / 1024) entries, shuffle tree (6), the 16 wavefront sums one after the other (16); beta beta (1), division (1),
  subtraction (1):                                                   k_alpha = ceil(count / 1024) + 25
Pass (b), k_vq_fused<S, J> on 128-row tiles, grid min(tiles, 3 CUs)  (LaggedModel.vq_fused)
  X = V Q: one running sum over the m terms — k_vq's summation: krylov_checks' k_vq(m) = m + 1 for m <= 64
  f_corr = ftilde - V c: product (1), m additions, subtraction (1): m + 2; it is NOT stored, so what is formed from it carries
      e = gamma_(m + 2) (|ftilde| + |V||c|) row by row next to its own roundings:
  chk_j = <V_j, f_corr>: gamma_kdot |V_j|'(|f_corr| + e) + |V_j|'e ;  |f_corr|^2: gamma_kdot sum (|f_corr| + e)^2 + sum (2 |f_corr| e + e^2)
  fnew = f_corr q_last + X[:, kcol] h_sub (stored X): gamma_2 ((|f_corr| + e) |q| + |X h|) + |q| e ;  |fnew|^2 of the stored fnew: k_dot
  with k_dot = 2 + T + 6 + ceil(records / 64) + 6 (R = 1).  Tail: beta = sqrt(red[m]), rst_beta_corr = sqrt(red[1024]): 1 each;
  rst_err = max |red[j]| exact; kStepRestartCheck iff rst_err > eps rst_beta_corr.

Large vectors (n > 4099) follow krylov_checks: long double on the first 256 rows, the last 256 rows and 16 seeded rows (and, for
dot products, on the columns 0, 1, i - 2, i - 1 and 8 seeded ones as well as slot i and the norms), float64 BLAS on everything at the
kernel's gamma plus the reference's own (gamma_(n + 1) for a dot product, gamma_(terms + 2) for a row)."""
import numpy as np

import krylov_checks as K
from krylov_checks import EPS, LD, Ratios, _ratio, cdiv, gamma, sample_rows

RECORD_LD = 1032
SLOT_BETA2, SLOT_MAXABS, SLOT_BETA, SLOT_ERR = 1024, 1025, 1026, 1027
OK, SMALL_BETA, MORE_CORR, TINY_F, LAG_CHECK, RESTART_CHECK = range(6)  # csrc/krylov.hpp kStep*
PANEL = 64
EPS_SQRT = float(np.sqrt(EPS))
PAD = 6  # rows behind the even-padded vector that the kernels may neither read (NaN) nor write (canaries)


# ---------------------------------------------------------------------------------------------------------------------------
# what the launchers launch
# ---------------------------------------------------------------------------------------------------------------------------
class LaggedModel:
    """launch_orth(ORTH_LAGGED) -> launch_orth_panel -> launch_orth_lagged | launch_orth_lagged_dma | (CORRECT_ONLY panels +
    launch_orth_lagged_wide), and launch_vq_fused (csrc/krylov.hip, orth_dma.hip, orth_wide.hip), restated.
    orth_kernel: the option of that name (None: unset)."""

    def __init__(self, cus, orth_kernel=None):
        self.cus, self.orth_kernel = int(cus), orth_kernel

    def lagged(self, n, i):
        assert 1 <= i and 2 * i + 1 <= 1024
        if i >= 2 * PANEL:
            npan = cdiv(i, PANEL)
            grid = max(1, min(cdiv(n, 256), 4 * self.cus))
            last = i - (npan - 1) * PANEL
            return dict(kernel="panels", MAXS=cdiv(last, 4), R=1, NW=4, depth=0, grid=grid, T=cdiv(cdiv(n, 128), grid), nrec=grid,
                        npan=npan)
        slots = cdiv(i, 4)
        dma = i < PANEL and (n >= 1024 * 128 if self.orth_kernel is None else self.orth_kernel != "reg")
        if dma:
            tiles = cdiv(n, 128)
            grid = min(tiles, self.cus)
            depth = 3 if slots <= 11 and self.orth_kernel != "dma2" else 2
            return dict(kernel="k_orth_lagged_dma", MAXS=slots, R=1, NW=4, depth=depth, grid=grid, T=cdiv(tiles, grid), nrec=grid, npan=1)
        if i >= PANEL:
            maxs, R, NW, per_cu = min(max(cdiv(i, 8), 8), 16), 1, 8, 2
        else:
            maxs, R, NW, per_cu = min(slots, 16), (2 if slots <= 10 else 1), 4, 4
        tiles = cdiv(n, 128 * R)
        grid = max(1, min(tiles, per_cu * self.cus))
        return dict(kernel="k_orth_lagged", MAXS=maxs, R=R, NW=NW, depth=0, grid=grid, T=cdiv(tiles, grid), nrec=grid, npan=1)

    def k_vi(self, n, i):
        L = self.lagged(n, i)
        if L["kernel"] == "panels":
            return max(20 + L["npan"], L["MAXS"] + 5)
        return L["MAXS"] + (5 if L["NW"] == 4 else 6)

    def k_dot(self, n, i):
        L = self.lagged(n, i)
        return 2 + L["R"] * L["T"] + 6 + cdiv(L["nrec"], 64) + 6

    def k_alpha(self, count):
        return cdiv(count, 1024) + 25

    def vq_fused(self, n, m, p):
        slots = cdiv(p, 4)
        maxs = 4 if slots <= 4 else 8 if slots <= 8 else 12 if slots <= 12 else 16
        tiles = cdiv(n, 128)
        grid = max(1, min(tiles, 3 * self.cus))
        return dict(kernel="k_vq_fused<%d,%d>" % (maxs, 10 if (maxs == 8 and m <= 40) else 16), grid=grid, T=cdiv(tiles, grid), nrec=grid)

    def k_vq(self, m):
        return K.HipModel(self.cus).k_vq(m)

    def k_fcorr(self, m):
        return m + 2

    def k_vq_dot(self, n, m, p):
        L = self.vq_fused(n, m, p)
        return 2 + L["T"] + 6 + cdiv(L["nrec"], 64) + 6

    def reduce_form(self, nrec, ncol):
        """k_reduce_partials: 'round1' | 'round2' | 'round4' (one round, RPL records per lane) or 'passes' (48 columns a pass)."""
        if nrec <= 256 and ncol + 2 <= 96:
            return "round1" if nrec <= 64 else "round2" if nrec <= 128 else "round4"
        return "passes"

    def describe(self, n, i):
        L = self.lagged(n, i)
        return "%s MAXS=%d R=%d NW=%d depth=%d grid=%d tiles/wg=%d records=%d panels=%d" % tuple(
            L[k] for k in ("kernel", "MAXS", "R", "NW", "depth", "grid", "T", "nrec", "npan"))


class HostLaggedModel:
    """The numpy stand-in: every sum is one float64 BLAS / pairwise sum of its full length, in whatever order."""

    def lagged(self, n, i):
        return dict(kernel="numpy", nrec=1)

    def k_vi(self, n, i):
        return i + 3

    def k_dot(self, n, i):
        return n + 1

    def k_alpha(self, count):
        return count + 3

    def vq_fused(self, n, m, p):
        return dict(kernel="numpy", nrec=1)

    def k_vq(self, m):
        return m + 1

    def k_fcorr(self, m):
        return m + 2

    def k_vq_dot(self, n, m, p):
        return n + 1


# ---------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------
def even(n):
    return n + (n & 1)


def padded(x, n, ld):
    """A vector of ld rows: x on [0, n), 0 on the odd pad row n (contract: it is loaded with row n - 1), NaN behind."""
    v = np.full(ld, np.nan)
    v[:n] = x
    v[n: even(n)] = 0.0
    return v


def not_negligible(x):
    return np.where(x < 0, -1.0, 1.0) * (0.5 + 0.5 * np.abs(x))


def basis(n, ncols, seed):
    """V (ld x ncols, column-major, ld = even(n) + PAD): uniform in (-1, 1), column j scaled by 2^(j mod 24) so that a coefficient
    or a record slot taken from the wrong column cannot pass; no entry of the last row negligible."""
    rng = np.random.default_rng(seed)
    ld = even(n) + PAD
    V = np.full((ld, ncols), np.nan, order="F")
    V[:n] = rng.uniform(-1.0, 1.0, (n, ncols))
    V[n - 1] = not_negligible(V[n - 1])
    V[:n] *= 2.0 ** (np.arange(ncols) % 24)
    V[n: even(n)] = 0.0
    return V


class Case:
    pass


def lagged_case(V, n, i, pending, onered, seed, alpha_count=300):
    """Generic data of step i on the first i columns of a basis(): f, src uniform; c_in of order one, all entries distinct;
    alpha, beta of order one and no powers of two; H entries of order one with sentinels where the tail writes."""
    rng = np.random.default_rng(seed)
    c = Case()
    c.V, c.n, c.i, c.ld, c.pending, c.onered = V, n, i, V.shape[0], int(pending), int(onered)
    f, src = rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)
    f[-1], src[-1] = not_negligible(f[-1]), not_negligible(src[-1])
    c.f, c.src = padded(f, n, c.ld), padded(src, n, c.ld)
    c.c_in = (0.5 + 0.5 * (np.arange(i) + 1.0) / (i + 1.0)) * np.where(np.arange(i) % 2, -1.0, 1.0)
    c.alpha, c.beta = 0.7304881, 1.3171942
    c.diag, c.subd = rng.uniform(0.5, 1.5, i + 1), rng.uniform(0.5, 1.5, i + 1)
    c.diag[i], c.subd[i - 1] = 777.5, -555.25
    c.status, c.lag_last, c.lag_limit, c.n_op = OK, 0, 1e-6, n
    c.lag_chk_max, c.lag_rel_c_max, c.lag_steps, c.onered_steps = 3e-17, 2e-5, 7, 3
    c.alpha_parts = rng.uniform(-1.0, 1.0, alpha_count) if (onered and alpha_count) else None
    c.red_in = np.arange(RECORD_LD) * 0.5 + 0.25  # what the record half held before: must not survive a live step
    c.vout_in = np.full(c.ld, -7.25)              # what column i held before
    return c


def unit_case(n, i, pending, seed, kind, parts=0):
    """Constructed data for the branches of the tail: V = the first i unit vectors (orthonormal exactly), so that every record
    entry is an input: chk_j = (f_j - c_in_j) / beta, c_j = w_j - alpha v_ij.  kind:
      none     no correction needed (w and f on disjoint rows, alpha = 0: every c_j is 0 exactly)
      lag      |c| about 1e-4 |f|: the correction is carried (lag_pending = 1)
      more     |c|^2 above lag_limit |f|^2: kStepMoreCorr
      check    pending, chk = 1e-10 > eps: kStepLagCheck
      tiny     |f| < eps sqrt(n) with a correction needed: kStepTinyF
      small    no correction needed and |f| < sqrt(eps): the one-reduction tail stops the next step (kStepSmallBeta)
    parts > 0: that many partial sums of <f~, u>, so that the one-reduction tail runs behind the step."""
    rng = np.random.default_rng(seed)
    ld = even(n) + PAD
    V = np.full((ld, i), np.nan, order="F")
    V[: even(n)] = 0.0
    V[np.arange(i), np.arange(i)] = 1.0
    c = lagged_case(V, n, i, pending, 0, seed)
    half = i + (n - i) // 2
    f, w = np.zeros(n), np.zeros(n)
    f[i: half] = rng.uniform(0.5, 1.0, half - i)
    w[half:] = rng.uniform(0.5, 1.0, n - half)
    c.c_in = 1e-4 * (0.5 + 0.5 * (np.arange(i) + 1.0) / (i + 1.0)) * np.where(np.arange(i) % 2, -1.0, 1.0)
    if pending:
        f[:i] = c.c_in + (1e-10 if kind == "check" else 0.0)  # chk_j = (f_j - c_in_j) / beta
    small = 1e-4 * (0.5 + 0.5 * rng.uniform(0.0, 1.0, i)) * np.where(np.arange(i) % 2, 1.0, -1.0)
    if kind in ("none", "small"):
        c.alpha = 0.0
        if kind == "small":
            w *= 1e-9
    elif kind in ("lag", "more", "check"):
        f[half:] = rng.uniform(0.5, 1.0, n - half)  # f and w overlap: alpha = <v_i, w> is of order one
        w[:i] = small * (1.0 if kind != "more" else 100.0) * np.sqrt(n)
    elif kind == "tiny":
        f[half:] = rng.uniform(0.5, 1.0, n - half)
        w *= 1e-18
        w[:i] = small * 1e-18
    if kind in ("lag", "more", "check", "tiny"):
        vi = (f - (V[:n] @ c.c_in if pending else 0.0)) / c.beta
        c.alpha = float(vi @ w) / float(vi @ vi)  # <v_i, w - alpha v_i> is then at rounding level
    c.f, c.src = padded(f, n, ld), padded(w, n, ld)
    c.alpha_parts = rng.uniform(-1.0, 1.0, parts) if parts else None
    return c


def qr_case(n, i, seed):
    """A lagged correction on realistic data: V orthonormal from a QR, f and w projected on its complement, w then given a
    component 1e-4 |w| inside span V; pending = 0 (chk of a QR basis is AT rounding level, so its test could go either way)."""
    rng = np.random.default_rng(seed)
    ld = even(n) + PAD
    Q, _ = np.linalg.qr(rng.uniform(-1.0, 1.0, (n, i)))
    V = np.full((ld, i), np.nan, order="F")
    V[:n], V[n: even(n)] = Q, 0.0
    c = lagged_case(V, n, i, 0, 0, seed)
    proj = lambda x: x - Q @ (Q.T @ (x - Q @ (Q.T @ x))) - Q @ (Q.T @ x)
    f, w = proj(rng.uniform(-1.0, 1.0, n)), proj(rng.uniform(-1.0, 1.0, n))
    w = w + 1e-4 * np.linalg.norm(w) * (Q @ rng.uniform(-1.0, 1.0, i)) / np.sqrt(i)
    c.beta = float(np.linalg.norm(f)) * 1.0000001
    vi = f / c.beta
    c.alpha = float(vi @ w) / float(vi @ vi)
    c.f, c.src = padded(f, n, ld), padded(w, n, ld)
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# the tail of pass (a), restated in float64 from finish_lagged and start_next_onered (csrc/krylov.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def _clear(a, b, what):
    """a > b, with the comparison at least 0.1 % from its threshold (the device may round a or b differently)."""
    assert abs(a - b) > 1e-3 * max(abs(a), abs(b)) or a == b == 0.0, ("the data puts a decision of the tail on its threshold", what, a, b)
    return a > b


def scan_abs_sq(v):
    mx, sq = 0.0, 0.0
    for x in v:
        mx = max(mx, abs(float(x)))
        sq += float(x) * float(x)
    return mx, sq


def tail_lagged(case, red, one_reduction_tail):
    """The state finish_lagged (and start_next_onered) leave, from the REDUCED record `red` of the device (slots c, <v_i, f>,
    chk, sum f^2 and the root the device took of it): a dict of the hook's outputs; 'written': whether H and beta were written."""
    i = case.i
    s = dict(status=case.status, stop_step=0, stop_count=0, count=0, need_corr=0, lag_pending=case.pending, beta=case.beta,
             alpha=0.0, diag=case.diag.copy(), subd=case.subd.copy(), lag_chk_max=case.lag_chk_max, lag_rel_c_max=case.lag_rel_c_max,
             lag_steps=case.lag_steps, onered_steps=case.onered_steps, alpha_out=case.alpha, written=False, carried=False, live=False)
    if case.status != OK:
        return s
    s["live"] = True
    pend = case.pending != 0
    bprev = case.beta
    if pend:
        cerr, _ = scan_abs_sq(red[i + 1: 2 * i + 1])
        s["lag_chk_max"] = max(case.lag_chk_max, cerr)
        if _clear(cerr, EPS, "chk > eps"):
            s.update(status=LAG_CHECK, stop_step=i, stop_count=1)
            return s
    d, sub = case.alpha, bprev
    if pend:
        cp1, cp2 = case.c_in[i - 1], (case.c_in[i - 2] if i >= 2 else 0.0)
        d -= cp1
        sub -= ((case.subd[i - 2] * cp2 if i >= 2 else 0.0) + case.diag[i - 1] * cp1) / bprev
    gamma2 = float(red[SLOT_BETA2])
    g = float(red[SLOT_BETA])  # the root the device took (checked against long double by check_lagged_tail)
    err, c2 = scan_abs_sq(red[: i + 1])
    s.update(alpha=case.alpha, err=err, lag_steps=case.lag_steps + 1, written=True, lag_pending=0)
    d_out, sub_out, beta = d, sub, g
    need = _clear(err, EPS * g, "err > eps gamma")
    if need and _clear(case_beta_thresh(case), g, "gamma < beta_thresh"):
        s.update(status=TINY_F, stop_step=i, stop_count=0)
    elif case.lag_last:
        s["need_corr"] = int(need)
    elif need:
        b2 = gamma2 - c2
        if not _clear(c2, case.lag_limit * gamma2, "c2 <= lag_limit gamma2") and b2 > 0.0 and not _clear(EPS_SQRT, np.sqrt(b2), "root >= sqrt(eps)"):
            sub_out, d_out, beta = sub + float(red[i - 1]), d + float(red[i]), float(np.sqrt(b2))
            s.update(lag_pending=1, count=1, carried=True, lag_rel_c_max=max(case.lag_rel_c_max, float(np.sqrt(c2)) / g))
        else:
            s.update(status=MORE_CORR, stop_step=i, stop_count=0)
    s["diag"][i], s["subd"][i - 1], s["beta"] = d_out, sub_out, beta
    if one_reduction_tail and s["status"] == OK:
        if _clear(EPS_SQRT, beta, "beta < sqrt(eps)"):
            s.update(status=SMALL_BETA, stop_step=i + 1, stop_count=0)
        else:
            s["alpha_out"] = float(np.sum(case.alpha_parts)) / (beta * beta) - float(red[i])
            s["onered_steps"] = case.onered_steps + 1
    return s


def case_beta_thresh(case):
    return EPS * float(np.sqrt(float(case.n_op)))


# ---------------------------------------------------------------------------------------------------------------------------
# the float64 numpy stand-in of both passes (tests/test_host_lagged_checks.py), with the targeted defects
# ---------------------------------------------------------------------------------------------------------------------------
def host_lagged_pass(case, defect=None, col=0):
    """What sa.lagged_pass returns plus 'vout' and 'f' (ld rows each), computed by plain float64 numpy.  defect:
    'c_last_row', 'chk_last_row' (the last row left out of slot `col`), 'last_tile' (the last 128-row tile left out of every sum),
    'skip_column' (column `col` skipped in V c_in), 'panel0' (the c_in of panel `col // 64` taken from panel 0), 'prev_column'
    (column i - 2 for i - 1 in the one-reduction w), 'swap_slots' (c and chk of column `col` exchanged), 'no_division' (column i
    formed without the division when nothing is pending)."""
    n, i, V = case.n, case.i, case.V[: case.n, : case.i]
    f, src = case.f[:n], case.src[:n]
    out = dict(vout=case.vout_in.copy(), f=case.f.copy(), nrec=1)
    red = case.red_in.copy()
    if case.status == OK:
        cin = case.c_in.copy() if case.pending else np.zeros(i)
        if defect == "skip_column":
            cin[col] = 0.0
        if defect == "panel0":
            q = col // PANEL
            width = min(PANEL, i - q * PANEL)
            cin[q * PANEL: q * PANEL + width] = cin[:width]
        vi = (f - V @ cin) / case.beta if case.pending else f / case.beta
        if defect == "no_division" and not case.pending:
            vi = f.copy()
        w = src
        if case.onered:
            w = src / case.beta - case.beta * V[:, i - 2 if defect == "prev_column" else i - 1]
        dst = w - case.alpha * vi
        rows = n - (n - 1) % 128 - 1 if defect == "last_tile" else n  # the rows the sums see
        red[:] = 0.0
        red[:i] = V[:rows].T @ dst[:rows]
        red[i] = vi[:rows] @ dst[:rows]
        red[i + 1: 2 * i + 1] = V[:rows].T @ vi[:rows]
        if defect == "c_last_row":
            red[col] = V[: n - 1, col] @ dst[: n - 1]
        if defect == "chk_last_row":
            red[i + 1 + col] = V[: n - 1, col] @ vi[: n - 1]
        if defect == "swap_slots":
            red[col], red[i + 1 + col] = red[i + 1 + col], red[col]
        red[SLOT_BETA2], red[SLOT_MAXABS] = dst[:rows] @ dst[:rows], np.abs(dst[:rows]).max(initial=0.0)
        red[SLOT_BETA] = np.sqrt(red[SLOT_BETA2])
        red[SLOT_ERR] = np.abs(red[: i + 1]).max()
        out["vout"][:n], out["f"][:n] = vi, dst
        out["vout"][n: even(n)], out["f"][n: even(n)] = 0.0, 0.0
    s = tail_lagged(case, red, case.alpha_parts is not None)
    if not s["written"] and case.status == OK:  # kStepLagCheck: the record is stored, its two finish slots are not filled
        red[SLOT_BETA] = red[SLOT_ERR] = 0.0
    out.update(s, red=red)
    return out


def host_fused_pass(case, defect=None, col=0):
    """sa.fused_restart_pass plus 'V' (after) and 'fnew', in float64 numpy.  defect: 'kcol' (column kcol + 1, or kcol - 1 for the
    last, enters fnew), 'zero_q' (column `col` of Q zeroed)."""
    n, m, p = case.n, case.m, case.p
    V, Q = case.V[:n, :m], case.Q.copy()
    if defect == "zero_q":
        Q[:, col] = 0.0
    X = V @ Q
    fc = case.ftilde[:n] - V @ case.c
    k = case.kcol
    if defect == "kcol":
        k = k + 1 if k + 1 < p else k - 1
    fnew = fc * case.q_last + X[:, k] * case.h_sub
    red = np.zeros(RECORD_LD)
    red[:m] = V.T @ fc
    red[m], red[SLOT_BETA2] = fnew @ fnew, fc @ fc
    red[SLOT_BETA], red[SLOT_ERR] = np.sqrt(red[SLOT_BETA2]), np.abs(red[:m]).max()
    Vn = case.V.copy()
    Vn[:n, :p], Vn[n: even(n), :p] = X, 0.0
    fout = case.fnew_in.copy()
    fout[:n], fout[n: even(n)] = fnew, 0.0
    out = dict(V=Vn, fnew=fout, red=red, nrec=1)
    out.update(tail_fused(case, red))
    return out


def tail_fused(case, red):
    """finish_fused_restart (csrc/krylov.hip) from the device's reduced record."""
    m = case.m
    s = dict(status=case.status, stop_step=0, stop_count=0, beta=0.0, rst_err=0.0, rst_beta_corr=0.0)
    if case.status != OK:
        return s
    err = float(np.abs(red[:m]).max())
    s.update(beta=float(np.sqrt(red[m])), rst_err=err, rst_beta_corr=float(red[SLOT_BETA]))
    if case.force_check or _clear(err, EPS * float(red[SLOT_BETA]), "rst_err > eps beta_corr"):
        s.update(status=RESTART_CHECK, stop_step=case.kcol, stop_count=1)
    return s


# ---------------------------------------------------------------------------------------------------------------------------
# the checks of pass (a)
# ---------------------------------------------------------------------------------------------------------------------------
def _bits(a, b):
    """equal bit for bit (NaN canaries included)"""
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def _ld_cols(n, i, seed=0):
    if n <= K.LD_ALL_ROWS:
        return np.arange(i)
    rng = np.random.default_rng(seed + i)
    return np.array(sorted({0, min(1, i - 1), max(i - 2, 0), i - 1} | set(int(j) for j in rng.integers(0, i, 8))))


def check_lagged_pass(case, res, model, out, where=None, strict=True):
    """Every vector and record entry of one live step (status OK on entry) against its reference; returns nothing, adds the
    worst error / bound of every kind of check to `out` (a Ratios).  strict=False (the defect tests, which read the ratios):
    the exact comparisons — canaries, f / beta bit for bit, max |f|, empty slots — are left out."""
    K.assert_long_double()
    assert case.status == OK
    n, i, ld = case.n, case.i, case.ld
    where = where if where is not None else (n, i, case.pending, case.onered)
    V = case.V[:n, :i]
    f0, src = case.f[:n], case.src[:n]
    vout, dst, red = res["vout"], res["f"], res["red"]
    L = model.lagged(n, i)
    vi, fn = vout[:n], dst[:n]
    if strict:
        assert res["nrec"] == L["nrec"], ("records of the pass", res["nrec"], L)
        # canaries: nothing behind the even-padded length is written; the odd pad row is written with 0
        assert _bits(vout[even(n):], case.vout_in[even(n):]) and _bits(dst[even(n):], case.f[even(n):]), where
        assert not vout[n: even(n)].any() and not dst[n: even(n)].any(), where
        assert np.isfinite(vi).all() and np.isfinite(fn).all() and np.isfinite(red).all(), where
    big = n > K.LD_ALL_ROWS
    rows = sample_rows(n)
    absV = np.abs(V)
    cin = case.c_in if case.pending else np.zeros(i)
    # v_i
    if not case.pending and strict:
        assert _bits(vi, f0 / case.beta), ("column i is not f / beta bit for bit", where)
    kvi = model.k_vi(n, i)
    ref = (f0[rows].astype(LD) - V[rows].astype(LD) @ cin.astype(LD)) / LD(case.beta)
    terms = (np.abs(f0) + absV @ np.abs(cin)) / abs(case.beta)
    out.add("v_i", _ratio(np.abs(vi[rows] - ref), gamma(kvi) * terms[rows]), where)
    if big:
        out.add("v_i64", _ratio(np.abs(vi - (f0 - V @ cin) / case.beta), (gamma(kvi) + gamma(i + 3)) * terms), where)
    # dst = w - alpha v_i from the stored v_i
    if case.onered:
        a, b = src[rows].astype(LD) / LD(case.beta), LD(case.beta) * V[rows, i - 1].astype(LD)
        w, wabs, kdst = a - b, np.abs(a) + np.abs(b), 3
        w64, wabs64 = src / case.beta - case.beta * V[:, i - 1], np.abs(src / case.beta) + np.abs(case.beta * V[:, i - 1])
    else:
        w, wabs, kdst = src[rows].astype(LD), np.abs(src[rows]).astype(LD), 2
        w64, wabs64 = src, np.abs(src)
    av = LD(case.alpha) * vi[rows].astype(LD)
    out.add("dst", _ratio(np.abs(fn[rows] - (w - av)), gamma(kdst) * (wabs + np.abs(av))), where)
    if big:
        out.add("dst64", _ratio(np.abs(fn - (w64 - case.alpha * vi)), (gamma(kdst) + gamma(4)) * (wabs64 + np.abs(case.alpha * vi))), where)
    # the record: dot products with the stored bits of column i and of the new f
    kdot = model.k_dot(n, i)
    absf, absv = np.abs(fn), np.abs(vi)
    got_c, got_chk = red[:i], red[i + 1: 2 * i + 1]
    cols = _ld_cols(n, i)
    VT = np.ascontiguousarray(V[:, cols].T).astype(LD)
    fl, vl = fn.astype(LD), vi.astype(LD)
    out.add("c", _ratio(np.abs(got_c[cols] - K.ld_rows_dot(VT, fl, len(cols))), gamma(kdot) * (absV[:, cols].T @ absf)), where)
    out.add("chk", _ratio(np.abs(got_chk[cols] - K.ld_rows_dot(VT, vl, len(cols))), gamma(kdot) * (absV[:, cols].T @ absv)), where)
    if big:
        g64 = gamma(kdot) + gamma(n + 1)
        out.add("c64", _ratio(np.abs(got_c - V.T @ fn), g64 * (absV.T @ absf)), where)
        out.add("chk64", _ratio(np.abs(got_chk - V.T @ vi), g64 * (absV.T @ absv)), where)
    out.add("slot_i", _ratio(abs(red[i] - vl @ fl), gamma(kdot) * (absv @ absf)), where)
    out.add("sum_f2", _ratio(abs(red[SLOT_BETA2] - fl @ fl), gamma(kdot) * (absf @ absf)), where)
    if strict:
        assert red[SLOT_MAXABS] == absf.max(), ("max |f|", where)
        assert not red[2 * i + 1: SLOT_BETA2].any() and not red[SLOT_ERR + 1:].any(), ("slots outside the record", where)


def check_lagged_tail(case, res, model, out, where=None):
    """The state the tail leaves: integers and decisions exactly as tail_lagged restates them from the reduced record, the values
    against the long-double value of the same formula.  Returns the restated state (for assertions on the branch taken)."""
    K.assert_long_double()
    i, red = case.i, res["red"]
    where = where if where is not None else (case.n, i, case.pending, case.onered)
    if case.status != OK:  # nothing may have changed: vectors, record, state
        assert _bits(res["vout"], case.vout_in) and _bits(res["f"], case.f) and _bits(red, case.red_in), where
    s = tail_lagged(case, red, case.alpha_parts is not None)
    for key in ("status", "stop_step", "stop_count", "count", "need_corr", "lag_pending", "lag_steps", "onered_steps"):
        assert res[key] == s[key], (key, res[key], s[key], where)
    assert res["lag_chk_max"] == s["lag_chk_max"], where  # a maximum of absolute values: exact
    untouched = np.ones(i + 1, dtype=bool)
    if s["written"]:
        untouched[i] = False
        assert _bits(res["subd"][: i - 1], case.subd[: i - 1]) and res["subd"][i] == case.subd[i], where
    else:
        assert _bits(res["subd"], case.subd) and res["beta"] == case.beta and res["lag_rel_c_max"] == case.lag_rel_c_max, where
    assert _bits(res["diag"][untouched], case.diag[untouched]), where
    if not s["written"]:
        if s["live"]:  # kStepLagCheck: the record itself is stored, the finish slots are not filled
            assert red[SLOT_BETA] == 0.0 and red[SLOT_ERR] == 0.0, where
        assert res["alpha_out"] == case.alpha, where
        return s
    g2 = LD(red[SLOT_BETA2])
    g = np.sqrt(g2)
    out.add("gamma", _ratio(abs(red[SLOT_BETA] - g), gamma(1) * g), where)
    assert red[SLOT_ERR] == np.abs(red[: i + 1]).max() == res["err"] and res["alpha"] == case.alpha, where
    d, dabs, sub, sabs, ksub = LD(case.alpha), abs(case.alpha), LD(case.beta), abs(case.beta), 0
    if case.pending:
        cp1, cp2 = LD(case.c_in[i - 1]), LD(case.c_in[i - 2] if i >= 2 else 0.0)
        t1, t2 = (LD(case.subd[i - 2]) * cp2 if i >= 2 else LD(0)), LD(case.diag[i - 1]) * cp1
        d, dabs = d - cp1, dabs + abs(cp1)
        sub, sabs, ksub = sub - (t1 + t2) / LD(case.beta), sabs + (abs(t1) + abs(t2)) / abs(case.beta), 4
    beta_ref, beta_tol = g, gamma(1) * g
    if s["carried"]:
        d, dabs = d + LD(red[i]), dabs + abs(red[i])
        sub, sabs, ksub = sub + LD(red[i - 1]), sabs + abs(red[i - 1]), ksub + 1
        c2 = np.sum(red[: i + 1].astype(LD) ** 2)
        beta_ref = np.sqrt(g2 - c2)
        beta_tol = (gamma(i + 3) * (g2 + c2) / (g2 - c2) + gamma(1)) * beta_ref
        rel = np.sqrt(c2) / g
        if rel > case.lag_rel_c_max:
            out.add("rel_c", _ratio(abs(res["lag_rel_c_max"] - rel), gamma(i + 5) * rel), where)
        else:
            assert res["lag_rel_c_max"] == case.lag_rel_c_max, where
    else:
        assert res["lag_rel_c_max"] == case.lag_rel_c_max, where
    out.add("H_diag", _ratio(abs(res["diag"][i] - d), gamma(2) * dabs), where)
    out.add("H_subd", _ratio(abs(res["subd"][i - 1] - sub), gamma(max(ksub, 1)) * sabs), where)
    out.add("beta", _ratio(abs(res["beta"] - beta_ref), beta_tol), where)
    if case.alpha_parts is not None and s["status"] == OK:
        b = LD(res["beta"])  # the stored beta
        t = np.sum(case.alpha_parts.astype(LD)) / (b * b)
        tabs = np.sum(np.abs(case.alpha_parts)) / float(b * b)
        out.add("alpha_next", _ratio(abs(res["alpha_out"] - (t - LD(red[i]))), gamma(model.k_alpha(case.alpha_parts.size)) * (tabs + abs(red[i]))), where)
    else:
        assert res["alpha_out"] == case.alpha, where
    return s


# ---------------------------------------------------------------------------------------------------------------------------
# pass (b)
# ---------------------------------------------------------------------------------------------------------------------------
def fused_case(V, n, m, p, kcol, seed, status=OK, force_check=False):
    rng = np.random.default_rng(seed)
    c = Case()
    c.V, c.n, c.m, c.p, c.kcol, c.ld, c.status, c.force_check = V, n, m, p, kcol, V.shape[0], status, int(force_check)
    c.Q = np.asfortranarray(rng.uniform(-1.0, 1.0, (m, p)))
    c.c = (0.5 + 0.5 * (np.arange(m) + 1.0) / (m + 1.0)) * np.where(np.arange(m) % 2, -1.0, 1.0)
    ft = rng.uniform(-1.0, 1.0, n)
    ft[-1] = not_negligible(ft[-1])
    c.ftilde = padded(ft, n, c.ld)
    c.q_last, c.h_sub = 0.6180339, -1.4142135
    c.red_in = np.arange(RECORD_LD) * 0.5 + 0.25
    c.fnew_in = np.full(c.ld, -7.25)
    return c


def unit_fused_case(n, m, p, kcol, seed):
    """V = the first m unit vectors and ftilde_j = c_j on them: f_corr vanishes on the rows of the basis EXACTLY, every chk_j is 0
    and the restart's test passes (kStepOk stays)."""
    ld = even(n) + PAD
    V = np.full((ld, m), np.nan, order="F")
    V[: even(n)] = 0.0
    V[np.arange(m), np.arange(m)] = 1.0
    c = fused_case(V, n, m, p, kcol, seed)
    c.ftilde[:m] = c.c
    return c


def check_fused_pass(case, res, model, out, where=None, strict=True):
    K.assert_long_double()
    n, m, p, kcol, ld = case.n, case.m, case.p, case.kcol, case.ld
    where = where if where is not None else (n, m, p, kcol)
    V0, Q = case.V[:n, :m], case.Q
    Vn, fnew, red = res["V"], res["fnew"], res["red"]
    L = model.vq_fused(n, m, p)
    if strict:
        assert res["nrec"] == L["nrec"], ("records of the pass", res["nrec"], L)
        assert _bits(Vn[:, p:m], case.V[:, p:m]), ("a column beyond p was written", where)
        assert _bits(Vn[even(n):, :p], case.V[even(n):, :p]) and _bits(fnew[even(n):], case.fnew_in[even(n):]), where
        assert not Vn[n: even(n), :p].any() and not fnew[n: even(n)].any(), where
    X = Vn[:n, :p]
    K.check_product(X, V0, Q, model, out, "X", where)
    rows = sample_rows(n)
    big = n > K.LD_ALL_ROWS
    absV, ft = np.abs(V0), case.ftilde[:n]
    e = gamma(model.k_fcorr(m)) * (np.abs(ft) + absV @ np.abs(case.c))  # the rounding of the f_corr that is not stored
    if big:
        fc = ft - V0 @ case.c
        e = e + gamma(m + 2) * (np.abs(ft) + absV @ np.abs(case.c))  # ... and of this float64 reference
        fc_rows = ft[rows].astype(LD) - V0[rows].astype(LD) @ case.c.astype(LD)
    else:
        fcl = ft.astype(LD) - V0.astype(LD) @ case.c.astype(LD)
        fc, fc_rows = np.asarray(fcl, dtype=np.float64), fcl
        e = e + 2.0 ** -52 * np.abs(fc)  # (fc rounded to float64 for the sums of absolute values and the dots below)
    absfc = np.abs(fc) + e
    kdot = model.k_vq_dot(n, m, p)
    gd = gamma(kdot) + (gamma(n + 1) if big else 0.0)
    chk_ref = V0.T @ fc if big else K.ld_rows_dot(np.ascontiguousarray(V0.T).astype(LD), fcl, m)
    out.add("chk", _ratio(np.abs(red[:m] - chk_ref), gd * (absV.T @ absfc) + absV.T @ e), where)
    b2c = (fc @ fc) if big else (fcl @ fcl)
    out.add("fcorr2", _ratio(abs(red[SLOT_BETA2] - b2c), gd * (absfc @ absfc) + (2.0 * np.abs(fc)) @ e + e @ e), where)
    xh = X[rows, kcol].astype(LD) * LD(case.h_sub)
    ref = fc_rows[rows] * LD(case.q_last) + xh if not big else fc_rows * LD(case.q_last) + xh
    e_rows = gamma(model.k_fcorr(m)) * (np.abs(ft[rows]) + absV[rows] @ np.abs(case.c))
    tol = gamma(2) * ((np.abs(np.asarray(fc_rows[rows] if not big else fc_rows, dtype=np.float64)) + e_rows) * abs(case.q_last) + np.abs(xh)) + abs(case.q_last) * e_rows
    out.add("fnew", _ratio(np.abs(fnew[rows] - ref), tol), where)
    if big:
        ref64 = fc * case.q_last + X[:, kcol] * case.h_sub
        out.add("fnew64", _ratio(np.abs(fnew[:n] - ref64), (gamma(2) + gamma(2)) * (absfc * abs(case.q_last) + np.abs(X[:, kcol] * case.h_sub)) + abs(case.q_last) * e), where)
    fl = fnew[:n].astype(LD)
    out.add("fnew2", _ratio(abs(red[m] - fl @ fl), gamma(kdot) * float(fl @ fl)), where)
    if strict:
        assert not red[m + 1: SLOT_BETA2].any() and red[SLOT_MAXABS] == 0.0 and not red[SLOT_ERR + 1:].any(), where
        check_fused_tail(case, res, out, where)


def check_fused_tail(case, res, out, where):
    red, m = res["red"], case.m
    s = tail_fused(case, red)
    for key in ("status", "stop_step", "stop_count"):
        assert res[key] == s[key], (key, res[key], s[key], where)
    if case.status != OK:  # the reducing kernel leaves the record and the state alone (the pass itself has no predicate)
        assert _bits(red, case.red_in) and res["beta"] == 0.0 and res["rst_err"] == 0.0 and res["rst_beta_corr"] == 0.0, where
        return s
    bc, bn = np.sqrt(LD(red[SLOT_BETA2])), np.sqrt(LD(red[m]))
    out.add("beta_corr", _ratio(abs(res["rst_beta_corr"] - bc), gamma(1) * bc), where)
    out.add("beta_new", _ratio(abs(res["beta"] - bn), gamma(1) * bn), where)
    assert res["rst_beta_corr"] == red[SLOT_BETA] and res["rst_err"] == red[SLOT_ERR] == np.abs(red[:m]).max(), where
    return s
