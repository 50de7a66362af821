// Complex shifts on the iterative path of the general shift-and-invert operator: y = Re((A - sigma I)^{-1} x) for real sparse A of
// any pattern, real x and sigma = sigmar + i sigmai, sigmai != 0, by right-preconditioned BiCGStab in complex arithmetic with the
// complex Jacobi preconditioner — shift_bicgstab.hip's iteration with complex vectors and scalars.  For handles of
// mispec_symshift_create_general_complex; DESIGN.md 3.5.4.
//
// Layout: planar.  A complex vector is two planes (re, im) of n + 2 doubles, each one laid out as a real work vector, so the pair
// loop (for_rows), the 16-byte accesses (ld2 / st2) and the scalar last row apply per plane, and a plane is an operand of the real
// SpMV as it is.  A stays real and M = A - sigma I is never formed: u = A h is product() on the re plane and product() on the im
// plane, both predicated on the record's done flag, and - sigma h is added in the pass that follows.
//
// One iteration — the ten steps of shift_bicgstab.hip; <a, b> = sum conj(a_i) b_i, so <t, t> and <r, r> are real:
//   pass D    d = r + beta (d - omega v) ; dhat = minv .* d
//   product   u = A dhat                                            two real products
//   pass V    v = u - sigma dhat ; records <rhat, v>                2 slots
//   tail V    alpha = rho / <rhat, v>
//   pass S    s = r - alpha v (in place of r) ; shat = minv .* s
//   product   u = A shat                                            two real products
//   pass T    t = u - sigma shat ; records <t, s>, <t, t>           3 slots
//   tail T    omega = <t, s> / <t, t>
//   pass X    x += alpha dhat + omega shat ; r = s - omega t (in place of s) ; records <rhat, r>, <r, r>      3 slots
//   tail X    rho' = <rhat, r>, |r|, beta = (rho' / rho)(alpha / omega), the stop decision
// Reductions, tails, the done flag, the stops, the breakdown rules and the acceptance loop are shift_bicgstab.hip's, with moduli of
// complex entries in the backward error.  The first pass has the caller's real x as its right-hand side (im = 0), a restart the
// complex residual; k_finish writes Re(y) to the caller and keeps the complex y, which the residual's product reads.
//
// Order of operations, the same in every kernel (fma is explicit, nothing else is contracted); a = (ar, ai) etc.:
//   a b            (fma(-ai, bi, ar br),               fma(ai, br, ar bi))                          cmul
//   c + a b        (fma(-ai, bi, fma(ar, br, cr)),     fma(ai, br, fma(ar, bi, ci)))                cmadd
//   c - a b        (fma(ai, bi, fma(-ar, br, cr)),     fma(-ai, br, fma(-ar, bi, ci)))              cmsub
//   s += conj(a) b (fma(ai, bi, fma(ar, br, sr)),      fma(-ai, br, fma(ar, bi, si)))               dot_acc
//   s += |a|^2     fma(ai, ai, fma(ar, ar, s))                                                      norm_acc
//   |a|^2          fma(ai, ai, ar ar), and |a| its sqrt                                             abs2
//   a / b          (fma(ai, bi, ar br) / abs2(b),      fma(-ar, bi, ai br) / abs2(b))               cdiv
//   a / real t     (ar / t, ai / t)
// The rows i and i + 1 of a pair are accumulated in that order.
#include "shift_zbicgstab.hpp"

#include <cmath>
#include <memory>

#include "shift_iterative.hpp"

// the bits of every sum and update are those of the operations written here: products and sums are not contracted, fma is explicit
#pragma clang fp contract(off)

using namespace mispec;
using namespace mispec::shift_iter;

namespace {

constexpr double kHuge = 1.7e308;

struct cx
{
    double re, im;
};
struct cx2  // rows i and i + 1
{
    cx a, b;
};
struct ZP  // the two planes of a complex vector
{
    double* re;
    double* im;
};

__device__ __forceinline__ cx cmul(cx a, cx b) { return {fma(-a.im, b.im, a.re * b.re), fma(a.im, b.re, a.re * b.im)}; }
__device__ __forceinline__ cx cmadd(cx a, cx b, cx c) { return {fma(-a.im, b.im, fma(a.re, b.re, c.re)), fma(a.im, b.re, fma(a.re, b.im, c.im))}; }
__device__ __forceinline__ cx cmsub(cx a, cx b, cx c) { return {fma(a.im, b.im, fma(-a.re, b.re, c.re)), fma(-a.im, b.re, fma(-a.re, b.im, c.im))}; }
__device__ __forceinline__ void dot_acc(cx& s, cx a, cx b)
{
    s.re = fma(a.im, b.im, fma(a.re, b.re, s.re));
    s.im = fma(-a.im, b.re, fma(a.re, b.im, s.im));
}
__device__ __forceinline__ void norm_acc(double& s, cx a) { s = fma(a.im, a.im, fma(a.re, a.re, s)); }
__device__ __forceinline__ double abs2(cx a) { return fma(a.im, a.im, a.re * a.re); }
__device__ __forceinline__ cx cdiv(cx a, cx b)
{
    const double den = abs2(b);
    return {fma(a.im, b.im, a.re * b.re) / den, fma(-a.re, b.im, a.im * b.re) / den};
}
__device__ __forceinline__ bool all_finite(cx a) { return fabs(a.re) <= kHuge && fabs(a.im) <= kHuge; }
__device__ __forceinline__ bool is_zero(cx a) { return a.re == 0.0 && a.im == 0.0; }
__device__ __forceinline__ cx pair_of(const double* v) { return {v[0], v[1]}; }

__device__ __forceinline__ cx2 ldz2(ZP p, int64_t i)
{
    const double2 r = ld2(p.re, i), m = ld2(p.im, i);
    return {{r.x, m.x}, {r.y, m.y}};
}
__device__ __forceinline__ void stz2(ZP p, int64_t i, cx a, cx b)
{
    st2(p.re, i, make_double2(a.re, b.re));
    st2(p.im, i, make_double2(a.im, b.im));
}
__device__ __forceinline__ cx ldz(ZP p, int64_t i) { return {p.re[i], p.im[i]}; }
__device__ __forceinline__ void stz(ZP p, int64_t i, cx a)
{
    p.re[i] = a.re;
    p.im[i] = a.im;
}

// ---- set_shift: max |d_i - sigma| and max_i (|A|_i + |sigma|), then the preconditioner ----------------------------------------
__global__ __launch_bounds__(kThreads) void k_zshift_scan(int64_t n, double sr, double si, double sabs, const double* __restrict__ dA,
                                                           const double* __restrict__ aA, double* __restrict__ partials)
{
    __shared__ double red[4];
    double md = 0.0, mn = 0.0;
    for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += int64_t(gridDim.x) * kThreads)
    {
        md = nan_max(md, sqrt(abs2(cx{dA[i] - sr, si})));
        mn = nan_max(mn, aA[i] + sabs);
    }
    md = block_reduce_max(md, red);
    mn = block_reduce_max(mn, red);
    if (threadIdx.x == 0)
    {
        partials[blockIdx.x] = md;
        partials[gridDim.x + blockIdx.x] = mn;
    }
}
// minv_i = 1 / (d_i - sigma) = conj(d_i - sigma) / |d_i - sigma|^2; an entry with |d_i - sigma| <= 2^-26 max counts as the real max
__global__ __launch_bounds__(kThreads) void k_zprecond(int64_t n, double sr, double si, const double* __restrict__ dA,
                                                        const double* __restrict__ norms, ZP minv)
{
    const double maxd = norms[0];
    const double floor_d = maxd * (1.0 / 67108864.0);
    for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += int64_t(gridDim.x) * kThreads)
    {
        const double dr = dA[i] - sr;
        const double den = abs2(cx{dr, si});
        if (sqrt(den) > floor_d)
            stz(minv, i, cx{dr / den, si / den});  // d_i - sigma = (dr, -si)
        else
            stz(minv, i, cx{maxd > 0.0 ? 1.0 / maxd : 1.0, 0.0});
    }
}

// ---- a pass's start: r = rhat = rhs, d = v = x = 0; records <rhs, rhs> = rho_0 ---------------------------------------------------
// First: the right-hand side is the caller's real vector (im = 0); otherwise the complex residual
template <bool AL, bool First>
__global__ __launch_bounds__(kThreads) void k_zstart(int64_t n, const double* __restrict__ x, ZP rhs, ZP r, ZP rhat, ZP d, ZP v, ZP sol,
                                                      double* __restrict__ partials)
{
    __shared__ double red[4];
    double acc = 0.0;
    const cx zero = {0.0, 0.0};
    for_rows(
        n,
        [&](int64_t i) {
            cx2 b;
            if (First)
            {
                const double2 xv = ext_ld2<AL>(x, i);
                b = {{xv.x, 0.0}, {xv.y, 0.0}};
            }
            else
                b = ldz2(rhs, i);
            stz2(r, i, b.a, b.b);
            stz2(rhat, i, b.a, b.b);
            stz2(d, i, zero, zero);
            stz2(v, i, zero, zero);
            stz2(sol, i, zero, zero);
            norm_acc(acc, b.a);
            norm_acc(acc, b.b);
        },
        [&](int64_t i) {
            const cx b = First ? cx{x[i], 0.0} : ldz(rhs, i);
            stz(r, i, b);
            stz(rhat, i, b);
            stz(d, i, zero);
            stz(v, i, zero);
            stz(sol, i, zero);
            norm_acc(acc, b);
        });
    acc = block_sum(acc, red);
    if (threadIdx.x == 0)
        partials[blockIdx.x] = acc;
}

__global__ __launch_bounds__(kThreads) void k_ztail_start(ZBicgstabState* __restrict__ st, const double* __restrict__ partials, int nblocks,
                                                           double need, int cap)
{
    __shared__ double red[4];
    const double rr = sum_partials(partials, nblocks, red);
    if (threadIdx.x != 0)
        return;
    ZBicgstabState s;
    s.iter = 0;
    s.cap = cap;
    s.pad = 0;
    s.rho[0] = rr;
    s.rho[1] = 0.0;
    s.alpha[0] = s.alpha[1] = s.omega[0] = s.omega[1] = s.beta[0] = s.beta[1] = 0.0;  // pass D of the first iteration: d = r
    s.rnorm = s.rhs_norm = sqrt(rr);
    s.stop = need * s.rhs_norm;
    // rr == 0 is rhs == 0: nothing to iterate on
    s.done = !(rr >= 0.0) || !(rr <= kHuge) ? 3 : (rr == 0.0 ? 1 : (cap <= 0 ? 2 : 0));
    *st = s;
}

// pass D: d = r + beta (d - omega v), dhat = minv .* d
__global__ __launch_bounds__(kThreads) void k_zpass_d(const ZBicgstabState* __restrict__ st, int64_t n, ZP r, ZP v, ZP minv, ZP d, ZP dhat)
{
    const ZBicgstabState s = *st;
    if (s.done)
        return;
    const cx beta = pair_of(s.beta), omega = pair_of(s.omega);
    const auto row = [&](cx rv, cx vv, cx dv) { return cmadd(beta, cmsub(omega, vv, dv), rv); };
    for_rows(
        n,
        [&](int64_t i) {
            const cx2 rv = ldz2(r, i), vv = ldz2(v, i), dv = ldz2(d, i), m = ldz2(minv, i);
            const cx da = row(rv.a, vv.a, dv.a), db = row(rv.b, vv.b, dv.b);
            stz2(d, i, da, db);
            stz2(dhat, i, cmul(m.a, da), cmul(m.b, db));
        },
        [&](int64_t i) {
            const cx dn = row(ldz(r, i), ldz(v, i), ldz(d, i));
            stz(d, i, dn);
            stz(dhat, i, cmul(ldz(minv, i), dn));
        });
}

// pass V: v = u - sigma dhat; records <rhat, v>
__global__ __launch_bounds__(kThreads) void k_zpass_v(const ZBicgstabState* __restrict__ st, int64_t n, double sr, double si, ZP u, ZP dhat,
                                                       ZP rhat, ZP v, double* __restrict__ partials)
{
    __shared__ double red[4];
    if (st->done)
        return;
    const cx sigma = {sr, si};
    cx acc = {0.0, 0.0};
    for_rows(
        n,
        [&](int64_t i) {
            const cx2 uv = ldz2(u, i), h = ldz2(dhat, i), rh = ldz2(rhat, i);
            const cx va = cmsub(sigma, h.a, uv.a), vb = cmsub(sigma, h.b, uv.b);
            stz2(v, i, va, vb);
            dot_acc(acc, rh.a, va);
            dot_acc(acc, rh.b, vb);
        },
        [&](int64_t i) {
            const cx vn = cmsub(sigma, ldz(dhat, i), ldz(u, i));
            stz(v, i, vn);
            dot_acc(acc, ldz(rhat, i), vn);
        });
    acc.re = block_sum(acc.re, red);
    acc.im = block_sum(acc.im, red);
    if (threadIdx.x == 0)
    {
        partials[blockIdx.x] = acc.re;
        partials[gridDim.x + blockIdx.x] = acc.im;
    }
}

__global__ __launch_bounds__(kThreads) void k_ztail_v(ZBicgstabState* __restrict__ st, const double* __restrict__ partials, int nblocks)
{
    __shared__ double red[4];
    if (st->done)
        return;
    cx rv;  // (the sums' barriers lie between the read of done above and the writes below)
    rv.re = sum_partials(partials, nblocks, red);
    rv.im = sum_partials(partials + nblocks, nblocks, red);
    if (threadIdx.x != 0)
        return;
    if (!all_finite(rv))
        st->done = 3;
    else if (is_zero(rv))
        st->done = 4;
    else
    {
        const cx alpha = cdiv(pair_of(st->rho), rv);
        st->alpha[0] = alpha.re;
        st->alpha[1] = alpha.im;
    }
}

// pass S: s = r - alpha v in place of r, shat = minv .* s
__global__ __launch_bounds__(kThreads) void k_zpass_s(const ZBicgstabState* __restrict__ st, int64_t n, ZP r, ZP v, ZP minv, ZP shat)
{
    const ZBicgstabState s = *st;
    if (s.done)
        return;
    const cx alpha = pair_of(s.alpha);
    for_rows(
        n,
        [&](int64_t i) {
            const cx2 rv = ldz2(r, i), vv = ldz2(v, i), m = ldz2(minv, i);
            const cx sa = cmsub(alpha, vv.a, rv.a), sb = cmsub(alpha, vv.b, rv.b);
            stz2(r, i, sa, sb);
            stz2(shat, i, cmul(m.a, sa), cmul(m.b, sb));
        },
        [&](int64_t i) {
            const cx sn = cmsub(alpha, ldz(v, i), ldz(r, i));
            stz(r, i, sn);
            stz(shat, i, cmul(ldz(minv, i), sn));
        });
}

// pass T: t = u - sigma shat; records <t, s> and <t, t>
__global__ __launch_bounds__(kThreads) void k_zpass_t(const ZBicgstabState* __restrict__ st, int64_t n, double sr, double si, ZP u, ZP shat,
                                                       ZP s, ZP t, double* __restrict__ partials)
{
    __shared__ double red[4];
    if (st->done)
        return;
    const cx sigma = {sr, si};
    cx ts = {0.0, 0.0};
    double tt = 0.0;
    for_rows(
        n,
        [&](int64_t i) {
            const cx2 uv = ldz2(u, i), h = ldz2(shat, i), sv = ldz2(s, i);
            const cx ta = cmsub(sigma, h.a, uv.a), tb = cmsub(sigma, h.b, uv.b);
            stz2(t, i, ta, tb);
            dot_acc(ts, ta, sv.a);
            dot_acc(ts, tb, sv.b);
            norm_acc(tt, ta);
            norm_acc(tt, tb);
        },
        [&](int64_t i) {
            const cx tn = cmsub(sigma, ldz(shat, i), ldz(u, i));
            stz(t, i, tn);
            dot_acc(ts, tn, ldz(s, i));
            norm_acc(tt, tn);
        });
    ts.re = block_sum(ts.re, red);
    ts.im = block_sum(ts.im, red);
    tt = block_sum(tt, red);
    if (threadIdx.x == 0)
    {
        partials[blockIdx.x] = ts.re;
        partials[gridDim.x + blockIdx.x] = ts.im;
        partials[2 * gridDim.x + blockIdx.x] = tt;
    }
}

__global__ __launch_bounds__(kThreads) void k_ztail_t(ZBicgstabState* __restrict__ st, const double* __restrict__ partials, int nblocks)
{
    __shared__ double red[4];
    if (st->done)
        return;
    cx ts;
    ts.re = sum_partials(partials, nblocks, red);
    ts.im = sum_partials(partials + nblocks, nblocks, red);
    const double tt = sum_partials(partials + 2 * nblocks, nblocks, red);
    if (threadIdx.x != 0)
        return;
    if (!(tt >= 0.0) || !(tt <= kHuge) || !all_finite(ts))
        st->done = 3;
    else
    {
        // t = 0: r = s, and tail X decides between converged and breakdown
        st->omega[0] = tt == 0.0 ? 0.0 : ts.re / tt;
        st->omega[1] = tt == 0.0 ? 0.0 : ts.im / tt;
    }
}

// pass X: x += alpha dhat + omega shat; r = s - omega t in place of s; records <rhat, r> and <r, r>
__global__ __launch_bounds__(kThreads) void k_zpass_x(const ZBicgstabState* __restrict__ st, int64_t n, ZP dhat, ZP shat, ZP r, ZP t, ZP rhat,
                                                       ZP sol, double* __restrict__ partials)
{
    __shared__ double red[4];
    const ZBicgstabState s = *st;
    if (s.done)
        return;
    const cx alpha = pair_of(s.alpha), omega = pair_of(s.omega);
    cx hr = {0.0, 0.0};
    double rr = 0.0;
    for_rows(
        n,
        [&](int64_t i) {
            const cx2 dh = ldz2(dhat, i), sh = ldz2(shat, i), sv = ldz2(r, i), tv = ldz2(t, i), rh = ldz2(rhat, i), x = ldz2(sol, i);
            const cx ra = cmsub(omega, tv.a, sv.a), rb = cmsub(omega, tv.b, sv.b);
            stz2(sol, i, cmadd(omega, sh.a, cmadd(alpha, dh.a, x.a)), cmadd(omega, sh.b, cmadd(alpha, dh.b, x.b)));
            stz2(r, i, ra, rb);
            dot_acc(hr, rh.a, ra);
            dot_acc(hr, rh.b, rb);
            norm_acc(rr, ra);
            norm_acc(rr, rb);
        },
        [&](int64_t i) {
            stz(sol, i, cmadd(omega, ldz(shat, i), cmadd(alpha, ldz(dhat, i), ldz(sol, i))));
            const cx rn = cmsub(omega, ldz(t, i), ldz(r, i));
            stz(r, i, rn);
            dot_acc(hr, ldz(rhat, i), rn);
            norm_acc(rr, rn);
        });
    hr.re = block_sum(hr.re, red);
    hr.im = block_sum(hr.im, red);
    rr = block_sum(rr, red);
    if (threadIdx.x == 0)
    {
        partials[blockIdx.x] = hr.re;
        partials[gridDim.x + blockIdx.x] = hr.im;
        partials[2 * gridDim.x + blockIdx.x] = rr;
    }
}

__global__ __launch_bounds__(kThreads) void k_ztail_x(ZBicgstabState* __restrict__ st, const double* __restrict__ partials, int nblocks)
{
    __shared__ double red[4];
    if (st->done)
        return;
    cx hr;
    hr.re = sum_partials(partials, nblocks, red);
    hr.im = sum_partials(partials + nblocks, nblocks, red);
    const double rr = sum_partials(partials + 2 * nblocks, nblocks, red);
    if (threadIdx.x != 0)
        return;
    ZBicgstabState s = *st;
    s.iter += 1;
    s.rnorm = sqrt(rr);
    const cx omega = pair_of(s.omega);
    const cx beta = cmul(cdiv(hr, pair_of(s.rho)), cdiv(pair_of(s.alpha), omega));
    if (!(rr >= 0.0) || !(rr <= kHuge) || !all_finite(hr))
        s.done = 3;
    else if (s.rnorm <= s.stop)
        s.done = 1;
    else if (is_zero(omega) || is_zero(hr) || !all_finite(beta))
        s.done = 4;  // the recurrence cannot go on from here: the host restarts it from the explicit residual
    else if (s.iter >= s.cap)
        s.done = 2;
    s.beta[0] = beta.re;
    s.beta[1] = beta.im;
    s.rho[0] = hr.re;
    s.rho[1] = hr.im;
    *st = s;
}

// after a pass: y = sol (first pass) or y += sol (a restart's correction); the complex y stays on the handle, where the residual's
// product reads it, and Re(y) goes to the caller's vector
template <bool AL>
__global__ __launch_bounds__(kThreads) void k_zfinish(int64_t n, ZP sol, int first, ZP ycur, double* __restrict__ y)
{
    for_rows(
        n,
        [&](int64_t i) {
            cx2 x = ldz2(sol, i);
            if (!first)
            {
                const cx2 y0 = ldz2(ycur, i);
                x.a = {y0.a.re + x.a.re, y0.a.im + x.a.im};
                x.b = {y0.b.re + x.b.re, y0.b.im + x.b.im};
            }
            stz2(ycur, i, x.a, x.b);
            ext_st2<AL>(y, i, make_double2(x.a.re, x.b.re));
        },
        [&](int64_t i) {
            cx x = ldz(sol, i);
            if (!first)
            {
                const cx y0 = ldz(ycur, i);
                x = {y0.re + x.re, y0.im + x.im};
            }
            stz(ycur, i, x);
            y[i] = x.re;
        });
}

// res = x - (p - sigma y) with p = A y and the caller's real x; records max |res|, max |y|, max |x| (moduli of complex entries)
template <bool AL>
__global__ __launch_bounds__(kThreads) void k_zresidual(int64_t n, double sr, double si, const double* __restrict__ x, ZP y, ZP p, ZP res,
                                                         double* __restrict__ partials)
{
    __shared__ double red[4];
    const cx sigma = {sr, si};
    double mr = 0.0, my = 0.0, mx = 0.0;
    const auto row = [&](double xv, cx yv, cx pv) {
        const cx m = cmsub(sigma, yv, pv);
        const cx r = {xv - m.re, -m.im};
        mr = nan_max(mr, sqrt(abs2(r)));
        my = nan_max(my, sqrt(abs2(yv)));
        mx = nan_max(mx, fabs(xv));
        return r;
    };
    for_rows(
        n,
        [&](int64_t i) {
            const double2 xv = ext_ld2<AL>(x, i);
            const cx2 yv = ldz2(y, i), pv = ldz2(p, i);
            const cx ra = row(xv.x, yv.a, pv.a), rb = row(xv.y, yv.b, pv.b);
            stz2(res, i, ra, rb);
        },
        [&](int64_t i) { stz(res, i, row(x[i], ldz(y, i), ldz(p, i))); });
    mr = block_reduce_max(mr, red);
    my = block_reduce_max(my, red);
    mx = block_reduce_max(mx, red);
    if (threadIdx.x == 0)
    {
        partials[blockIdx.x] = mr;
        partials[gridDim.x + blockIdx.x] = my;
        partials[2 * gridDim.x + blockIdx.x] = mx;
    }
}

ZP planes(const ZVec& v) { return ZP{v.re.p, v.im.p}; }

// u = A h, plane by plane, where the pass still iterates (status: the record's done flag) or unconditionally (nullptr)
void zproduct(const ShiftIterative& M, const ZVec& h, const ZVec& u, const int* status)
{
    product(M, *M.A, h.re.p, u.re.p, status);
    product(M, *M.A, h.im.p, u.im.p, status);
}

// backward_error of shift_iterative.hpp with the complex residual; synchronises the stream
double zbackward_error(ShiftIterative& M, ShiftZBicgstab& Z, const mispec_ctx& ctx, int64_t n, double sr, double si, const double* x_dev)
{
    hipStream_t st = ctx.stream;
    const dim3 g(unsigned(M.grid)), b(kThreads);
    if (aligned16(x_dev))
        hipLaunchKernelGGL(k_zresidual<true>, g, b, 0, st, n, sr, si, x_dev, planes(Z.ycur), planes(Z.p), planes(Z.res), M.partials.p);
    else
        hipLaunchKernelGGL(k_zresidual<false>, g, b, 0, st, n, sr, si, x_dev, planes(Z.ycur), planes(Z.p), planes(Z.res), M.partials.p);
    hipLaunchKernelGGL(k_max_slots, dim3(1), b, 0, st, M.partials.p, M.grid, 3, M.norms.p);
    MISPEC_HIP(hipGetLastError());
    MISPEC_HIP(hipMemcpyAsync(M.h_norms.p, M.norms.p, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    MISPEC_HIP(hipStreamSynchronize(st));
    const double nr = M.h_norms.p[0], ny = M.h_norms.p[1], nx = M.h_norms.p[2];
    return nr / (M.mnorm * ny + nx);
}

}  // namespace

namespace mispec {

void zbicgstab_create(mispec_symshift& S) { S.zbicgstab = std::make_unique<ShiftZBicgstab>(); }

void zbicgstab_set_shift(mispec_symshift& S, double sigmar, double sigmai)
{
    ShiftBicgstab& M = *S.bicgstab;
    ShiftZBicgstab& Z = *S.zbicgstab;
    const mispec_ctx& ctx = *S.ctx;
    const int64_t n = S.n;
    bicgstab_alloc(S);  // the grid, the reduction records and the norms are the real method's
    if (!Z.state.p)
    {
        const size_t np = size_t(n) + 2;
        for (ZVec* v : {&Z.minv, &Z.rs, &Z.rhat, &Z.d, &Z.dhat, &Z.v, &Z.shat, &Z.t, &Z.sol, &Z.p, &Z.ycur, &Z.res})
            v->alloc(np);
        Z.state.alloc(1);
        Z.h_state.alloc(1);
    }
    hipStream_t st = ctx.stream;
    const dim3 g(unsigned(M.grid)), b(kThreads);
    hipLaunchKernelGGL(k_zshift_scan, g, b, 0, st, n, sigmar, sigmai, std::hypot(sigmar, sigmai), M.diagA.p, M.absA.p, M.partials.p);
    hipLaunchKernelGGL(k_max_slots, dim3(1), b, 0, st, M.partials.p, M.grid, 2, M.norms.p);
    hipLaunchKernelGGL(k_zprecond, g, b, 0, st, n, sigmar, sigmai, M.diagA.p, M.norms.p, planes(Z.minv));
    MISPEC_HIP(hipGetLastError());
    MISPEC_HIP(hipMemcpyAsync(M.h_norms.p, M.norms.p, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    MISPEC_HIP(hipStreamSynchronize(st));
    M.mnorm = M.h_norms.p[1];
    if (!(M.mnorm == M.mnorm) || !(sigmar == sigmar) || !(sigmai == sigmai))
        throw Error(MISPEC_EINVAL, "SparseSymShiftSolve: the matrix or the shift is not finite");
    S.sigma_im = sigmai;
    solve_probe(S, M, sigmar, [&](const double* x, double* y) { zbicgstab_solve(S, x, y, true); });
}

void zbicgstab_solve(const mispec_symshift& S, const double* x_dev, double* y_dev, bool probe)
{
    ShiftBicgstab& M = *S.bicgstab;
    ShiftZBicgstab& Z = *S.zbicgstab;
    const mispec_ctx& ctx = *S.ctx;
    const int64_t n = S.n;
    const double sr = S.sigma, si = S.sigma_im;
    hipStream_t st = ctx.stream;
    const dim3 g(unsigned(M.grid)), b(kThreads), one(1);
    const int check = std::max(1, std::min(shift_options().minres_check, kMinresMaxCheck));
    ZBicgstabState& hs = *Z.h_state.p;
    const int* done = &Z.state.p->done;
    const ZP minv = planes(Z.minv), rs = planes(Z.rs), rhat = planes(Z.rhat), d = planes(Z.d), dhat = planes(Z.dhat), v = planes(Z.v),
             shat = planes(Z.shat), t = planes(Z.t), sol = planes(Z.sol), p = planes(Z.p), ycur = planes(Z.ycur), res = planes(Z.res);
    SolveRecord rec{M, probe};
    for (int pass = 0;; pass++)
    {
        const int cap = rec.cap();
        if (pass > 0)
            hipLaunchKernelGGL((k_zstart<true, false>), g, b, 0, st, n, x_dev, res, rs, rhat, d, v, sol, M.partials.p);
        else if (aligned16(x_dev))
            hipLaunchKernelGGL((k_zstart<true, true>), g, b, 0, st, n, x_dev, res, rs, rhat, d, v, sol, M.partials.p);
        else
            hipLaunchKernelGGL((k_zstart<false, true>), g, b, 0, st, n, x_dev, res, rs, rhat, d, v, sol, M.partials.p);
        hipLaunchKernelGGL(k_ztail_start, one, b, 0, st, Z.state.p, M.partials.p, M.grid, rec.need(), cap);
        MISPEC_HIP(hipGetLastError());
        int enq = 0;
        for (;;)
        {
            for (int c = 0; c < check && enq < cap; c++, enq++)
            {
                hipLaunchKernelGGL(k_zpass_d, g, b, 0, st, Z.state.p, n, rs, v, minv, d, dhat);
                zproduct(M, Z.dhat, Z.p, done);
                hipLaunchKernelGGL(k_zpass_v, g, b, 0, st, Z.state.p, n, sr, si, p, dhat, rhat, v, M.partials.p);
                hipLaunchKernelGGL(k_ztail_v, one, b, 0, st, Z.state.p, M.partials.p, M.grid);
                hipLaunchKernelGGL(k_zpass_s, g, b, 0, st, Z.state.p, n, rs, v, minv, shat);
                zproduct(M, Z.shat, Z.p, done);
                hipLaunchKernelGGL(k_zpass_t, g, b, 0, st, Z.state.p, n, sr, si, p, shat, rs, t, M.partials.p);
                hipLaunchKernelGGL(k_ztail_t, one, b, 0, st, Z.state.p, M.partials.p, M.grid);
                hipLaunchKernelGGL(k_zpass_x, g, b, 0, st, Z.state.p, n, dhat, shat, rs, t, rhat, sol, M.partials.p);
                hipLaunchKernelGGL(k_ztail_x, one, b, 0, st, Z.state.p, M.partials.p, M.grid);
                MISPEC_HIP(hipGetLastError());
            }
            MISPEC_HIP(hipMemcpyAsync(&hs, Z.state.p, sizeof(ZBicgstabState), hipMemcpyDeviceToHost, st));
            MISPEC_HIP(hipStreamSynchronize(st));
            if (hs.done != 0)
                break;
            if (enq >= cap)
                throw Error(MISPEC_ERUNTIME, "internal: the iterative shift solve ran past its iteration cap");
        }
        rec.used += hs.iter;
        rec.passes++;
        if (hs.done == 3)
            rec.not_finite();
        if (pass == 0 && hs.rhs_norm == 0.0)  // x = 0: y = 0, nothing iterated
        {
            MISPEC_HIP(hipMemsetAsync(y_dev, 0, size_t(n) * sizeof(double), st));
            rec.omega = 0.0;
            break;
        }
        // (a breakdown, done == 4, is the end of a pass like any other: x holds every completed iteration)
        if (aligned16(y_dev))
            hipLaunchKernelGGL(k_zfinish<true>, g, b, 0, st, n, sol, pass == 0 ? 1 : 0, ycur, y_dev);
        else
            hipLaunchKernelGGL(k_zfinish<false>, g, b, 0, st, n, sol, pass == 0 ? 1 : 0, ycur, y_dev);
        zproduct(M, Z.ycur, Z.p, nullptr);
        const double w = zbackward_error(M, Z, ctx, n, sr, si, x_dev);
        if (hs.done == 2)
        {
            // an iterate that the cap cut off is not judged by omega (bicgstab_solve)
            rec.omega = w;
            rec.fail(w == w ? "; the recurrence's residual " + sci(hs.rnorm / hs.rhs_norm) + " of the last pass's right-hand side"
                            : "; the solution is not finite");
        }
        if (rec.accepted(pass, w))
            break;
    }
    rec.close();
}

}  // namespace mispec
