// Iterative path of the shift-and-invert operators: y = (A - sigma B)^{-1} x by Jacobi-preconditioned MINRES (Paige & Saunders 1975)
// for matrices no direct path takes — any sparsity pattern, definite and indefinite shifts alike.  Opt-in (option shift_solver,
// mispec_symshift_create_solver); DESIGN.md 3.5.2.
//
// One iteration k, with M = diag(1 / minv), z_k = minv .* r_k un-normalised and v_k = z_k / beta_k carried as (z_k, s = 1 / beta_k):
//   product   p = A z_k (q = B z_k for a pencil)                                             launch_spmv, predicated by its epilogue
//   pass A    t = s p - sigma s (z_k | q) - (beta_k / beta_{k-1}) r_{k-1}   -> r_{k-1}'s buffer ; records sum v_k t  (alpha_k)
//             and, one iteration late: w_{k-1} = (v_{k-1} - oldeps w_{k-3} - delta w_{k-2}) / gamma ; sol += phi w_{k-1}
//   tail A    alpha_k, alpha_k / beta_k
//   pass B    r_{k+1} = t - (alpha_k / beta_k) r_k (in place of t) ; z_{k+1} = minv .* r_{k+1} ; records sum r_{k+1} z_{k+1}
//   tail B    beta_{k+1}, the two rotations, phi, phibar (the residual estimate |r|_{M^-1}), the stop decision
// The update of w and x needs gamma_k, which needs beta_{k+1} — pass B's own reduction — so it runs in pass A of iteration k + 1
// (k_finish runs the last one).  Both reductions are two-stage and fixed-order; their second stage (one workgroup) runs the scalar
// recurrences into MinresState.  Every kernel returns at once when MinresState::done is set, so the iterations the host enqueued
// behind the one that finished change nothing, and the result does not depend on how often the host looks (shift=minres_check=N).
//
// A solve is up to 1 + kMinresRestarts passes: after each, the explicit residual r = x - (A - sigma B) y gives the backward error
// omega = |r|_inf / (|M|_inf |y|_inf + |x|_inf) of calibrate_refinement (shiftsolve.hip); accepted at `tol`, otherwise MINRES
// restarts on r and the correction is added.  A pass ends where its residual estimate has dropped by what omega still needs
// (tol / omega, with the margin kMargin), at an exact breakdown, or at the iteration cap.
#include "shift_minres.hpp"

#include <cmath>
#include <cstring>
#include <limits>
#include <memory>

#include "csr.hpp"
#include "device_helpers.hpp"

// the bits of every sum and update are those of the operations written here: products and sums are not contracted, fma is explicit
#pragma clang fp contract(off)

using namespace mispec;

namespace {

constexpr int kThreads = 256;
constexpr double kMargin = 0.25;

__device__ __forceinline__ double2 ld2(const double* p, int64_t i) { return *reinterpret_cast<const double2*>(p + i); }
__device__ __forceinline__ void st2(double* p, int64_t i, double2 v) { *reinterpret_cast<double2*>(p + i) = v; }
// a caller's vector may be only 8-byte aligned (a column of a block with an odd leading dimension): two 8-byte accesses then
template <bool AL>
__device__ __forceinline__ double2 ext_ld2(const double* p, int64_t i)
{
    if (AL)
        return ld2(p, i);
    double2 v;
    v.x = p[i];
    v.y = p[i + 1];
    return v;
}
template <bool AL>
__device__ __forceinline__ void ext_st2(double* p, int64_t i, double2 v)
{
    if (AL)
        st2(p, i, v);
    else
    {
        p[i] = v.x;
        p[i + 1] = v.y;
    }
}
__device__ __forceinline__ double nan_max(double m, double a) { return (a > m || a != a) ? a : m; }  // a NaN wins

// The loop of every vector pass: pairs of rows by 16-byte accesses in a grid-stride loop, then the last row of an odd n by the
// thread that follows the last pair's.  pair(i) handles rows i and i + 1, one(i) row i.
template <typename Pair, typename One>
__device__ __forceinline__ void for_rows(int64_t n, Pair&& pair, One&& one)
{
    const int64_t npair = n >> 1, stride = int64_t(gridDim.x) * kThreads;
    const int64_t first = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    for (int64_t j = first; j < npair; j += stride)
        pair(2 * j);
    if ((n & 1) && first == npair % stride)
        one(n - 1);
}

// max over the workgroup; every thread returns it
__device__ __forceinline__ double block_reduce_max(double v, double* red)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = nan_max(v, __shfl_down(v, off, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
        red[threadIdx.x >> 6] = v;
    __syncthreads();
    return nan_max(nan_max(red[0], red[1]), nan_max(red[2], red[3]));
}
__device__ __forceinline__ double block_sum(double v, double* red)
{
    __syncthreads();
    return block_reduce_sum(v, red);
}

// ---- construction: diagonal and row sums of |.| of a CSR matrix (stored order) ------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_diag_rowsum(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                           const double* __restrict__ val, int64_t n, double* __restrict__ diag,
                                                           double* __restrict__ rowsum)
{
    const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= n)
        return;
    double d = 0.0, a = 0.0;
    for (int32_t p = rowptr[i]; p < rowptr[i + 1]; p++)
    {
        const double v = val[p];
        if (colind[p] == i)
            d += v;
        a += fabs(v);
    }
    diag[i] = d;
    rowsum[i] = a;
}

// ---- set_shift: max |d_i| and max_i (|A|_i + |sigma| |B|_i), then the preconditioner ------------------------------------------
__global__ __launch_bounds__(kThreads) void k_shift_scan(int64_t n, double sigma, const double* __restrict__ dA, const double* __restrict__ dB,
                                                          const double* __restrict__ aA, const double* __restrict__ aB,
                                                          double* __restrict__ partials)
{
    __shared__ double red[4];
    double md = 0.0, mn = 0.0;
    for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += int64_t(gridDim.x) * kThreads)
    {
        md = nan_max(md, fabs(fma(-sigma, dB ? dB[i] : 1.0, dA[i])));
        mn = nan_max(mn, fma(fabs(sigma), aB ? aB[i] : 1.0, aA[i]));
    }
    md = block_reduce_max(md, red);
    mn = block_reduce_max(mn, red);
    if (threadIdx.x == 0)
    {
        partials[blockIdx.x] = md;
        partials[gridDim.x + blockIdx.x] = mn;
    }
}
// minv_i = 1 / |d_i|; an entry with |d_i| <= 2^-26 max |d| counts as max |d|: the preconditioner stays positive definite
__global__ __launch_bounds__(kThreads) void k_precond(int64_t n, double sigma, const double* __restrict__ dA, const double* __restrict__ dB,
                                                       const double* __restrict__ norms, double* __restrict__ minv)
{
    const double maxd = norms[0];
    const double floor_d = maxd * (1.0 / 67108864.0);
    for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += int64_t(gridDim.x) * kThreads)
    {
        const double d = fabs(fma(-sigma, dB ? dB[i] : 1.0, dA[i]));
        minv[i] = (d > floor_d) ? 1.0 / d : (maxd > 0.0 ? 1.0 / maxd : 1.0);
    }
}
// out[s] = max_b partials[s][b], s < nslots
__global__ __launch_bounds__(kThreads) void k_max_slots(const double* __restrict__ partials, int nblocks, int nslots, double* __restrict__ out)
{
    __shared__ double red[4];
    for (int s = 0; s < nslots; s++)
    {
        double m = 0.0;
        for (int i = threadIdx.x; i < nblocks; i += kThreads)
            m = nan_max(m, partials[s * nblocks + i]);
        m = block_reduce_max(m, red);
        if (threadIdx.x == 0)
            out[s] = m;
    }
}

// ---- a pass's start: r_1 = rhs, z_1 = minv .* rhs, everything else zero; records sum rhs z_1 = beta_1^2 ------------------------
template <bool AL>
__global__ __launch_bounds__(kThreads) void k_start(int64_t n, const double* __restrict__ rhs, const double* __restrict__ minv,
                                                     double* __restrict__ r2, double* __restrict__ r1, double* __restrict__ z1,
                                                     double* __restrict__ w0, double* __restrict__ w1, double* __restrict__ sol,
                                                     double* __restrict__ partials)
{
    __shared__ double red[4];
    double acc = 0.0;
    const double2 zero = make_double2(0.0, 0.0);
    for_rows(
        n,
        [&](int64_t i) {
            const double2 r = ext_ld2<AL>(rhs, i), m = ld2(minv, i);
            double2 z;
            z.x = m.x * r.x;
            z.y = m.y * r.y;
            st2(r2, i, r);
            st2(z1, i, z);
            st2(r1, i, zero);
            st2(w0, i, zero);
            st2(w1, i, zero);
            st2(sol, i, zero);
            acc = fma(r.x, z.x, acc);
            acc = fma(r.y, z.y, acc);
        },
        [&](int64_t i) {
            const double r = rhs[i], z = minv[i] * r;
            r2[i] = r;
            z1[i] = z;
            r1[i] = w0[i] = w1[i] = sol[i] = 0.0;
            acc = fma(r, z, acc);
        });
    acc = block_sum(acc, red);
    if (threadIdx.x == 0)
        partials[blockIdx.x] = acc;
}

// sum of the workgroups' records in a fixed order; every thread returns it
__device__ __forceinline__ double sum_partials(const double* __restrict__ partials, int nblocks, double* red)
{
    double a = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += kThreads)
        a += partials[i];
    return block_sum(a, red);
}

__global__ __launch_bounds__(kThreads) void k_tail_start(MinresState* __restrict__ st, const double* __restrict__ partials, int nblocks,
                                                          double need, int cap)
{
    __shared__ double red[4];
    const double bb = sum_partials(partials, nblocks, red);
    if (threadIdx.x != 0)
        return;
    MinresState s;
    s.iter = 0;
    s.cap = cap;
    s.pad = 0;
    s.beta1 = s.beta = sqrt(bb);
    s.oldb = 0.0;
    s.s = 1.0 / s.beta;
    s.c_r1 = 0.0;
    s.c_r2 = 0.0;
    s.alfa = 0.0;
    s.dbar = 0.0;
    s.epsln = 0.0;
    s.phibar = s.beta1;
    s.cs = -1.0;
    s.sn = 0.0;
    s.l_s = s.l_oldeps = s.l_delta = s.l_phi = 0.0;
    s.l_gamma = 1.0;
    s.stop = need * s.beta1;
    // minv is positive, so bb >= 0; bb == 0 is rhs == 0: nothing to iterate on
    s.done = !(bb >= 0.0) || !(s.beta1 <= 1.7e308) ? 3 : (bb == 0.0 ? 1 : (cap <= 0 ? 2 : 0));
    *st = s;
}

// the late update of one row: w <- (v - oldeps w_old - delta w_mid) / gamma, sol += phi w
__device__ __forceinline__ void lag_update(const MinresState& s, double zp, double& wa, double wb, double& x)
{
    double wn = zp * s.l_s;
    wn = fma(-s.l_oldeps, wa, wn);
    wn = fma(-s.l_delta, wb, wn);
    wn = wn / s.l_gamma;
    wa = wn;
    x = fma(s.l_phi, wn, x);
}

// pass A (see the head of the file).  q == nullptr: B = I.
__global__ __launch_bounds__(kThreads) void k_pass_a(const MinresState* __restrict__ st, int64_t n, double sigma, const double* __restrict__ p,
                                                      const double* __restrict__ q, const double* __restrict__ zc,
                                                      const double* __restrict__ zp, double* __restrict__ r1, double* __restrict__ wa,
                                                      const double* __restrict__ wb, double* __restrict__ sol, double* __restrict__ partials)
{
    __shared__ double red[4];
    const MinresState s = *st;
    if (s.done)
        return;
    const bool lag = s.iter > 0;
    double acc = 0.0;
    const auto row = [&](double pv, double qv, double zv, double rv, double& t) {
        const double v = zv * s.s;
        t = pv * s.s;
        t = fma(-sigma, qv * s.s, t);
        t = fma(-s.c_r1, rv, t);
        acc = fma(v, t, acc);
    };
    for_rows(
        n,
        [&](int64_t i) {
            const double2 pv = ld2(p, i), zv = ld2(zc, i), rv = ld2(r1, i), qv = q ? ld2(q, i) : zv;
            double2 t;
            row(pv.x, qv.x, zv.x, rv.x, t.x);
            row(pv.y, qv.y, zv.y, rv.y, t.y);
            st2(r1, i, t);
            if (lag)
            {
                const double2 zo = ld2(zp, i), b = ld2(wb, i);
                double2 a = ld2(wa, i), x = ld2(sol, i);
                lag_update(s, zo.x, a.x, b.x, x.x);
                lag_update(s, zo.y, a.y, b.y, x.y);
                st2(wa, i, a);
                st2(sol, i, x);
            }
        },
        [&](int64_t i) {
            const double zv = zc[i];
            double t;
            row(p[i], q ? q[i] : zv, zv, r1[i], t);
            r1[i] = t;
            if (lag)
            {
                double a = wa[i], x = sol[i];
                lag_update(s, zp[i], a, wb[i], x);
                wa[i] = a;
                sol[i] = x;
            }
        });
    acc = block_sum(acc, red);
    if (threadIdx.x == 0)
        partials[blockIdx.x] = acc;
}

__global__ __launch_bounds__(kThreads) void k_tail_a(MinresState* __restrict__ st, const double* __restrict__ partials, int nblocks)
{
    __shared__ double red[4];
    if (st->done)
        return;
    const double alfa = sum_partials(partials, nblocks, red);  // (its barriers lie between the read of done above and the writes below)
    if (threadIdx.x != 0)
        return;
    st->alfa = alfa;
    st->c_r2 = alfa / st->beta;
}

// pass B: r_{k+1} = t - (alpha / beta) r_k in place of t, z_{k+1} = minv .* r_{k+1}; records sum r_{k+1} z_{k+1}
__global__ __launch_bounds__(kThreads) void k_pass_b(const MinresState* __restrict__ st, int64_t n, double* __restrict__ t,
                                                      const double* __restrict__ r2, const double* __restrict__ minv,
                                                      double* __restrict__ zn, double* __restrict__ partials)
{
    __shared__ double red[4];
    const MinresState s = *st;
    if (s.done)
        return;
    double acc = 0.0;
    for_rows(
        n,
        [&](int64_t i) {
            const double2 tv = ld2(t, i), rv = ld2(r2, i), m = ld2(minv, i);
            double2 rn, z;
            rn.x = fma(-s.c_r2, rv.x, tv.x);
            rn.y = fma(-s.c_r2, rv.y, tv.y);
            z.x = m.x * rn.x;
            z.y = m.y * rn.y;
            st2(t, i, rn);
            st2(zn, i, z);
            acc = fma(rn.x, z.x, acc);
            acc = fma(rn.y, z.y, acc);
        },
        [&](int64_t i) {
            const double rn = fma(-s.c_r2, r2[i], t[i]), z = minv[i] * rn;
            t[i] = rn;
            zn[i] = z;
            acc = fma(rn, z, acc);
        });
    acc = block_sum(acc, red);
    if (threadIdx.x == 0)
        partials[blockIdx.x] = acc;
}

// tail B: beta_{k+1}, the rotations (Paige & Saunders; the variable names are those of the usual MINRES listings), the stop decision
__global__ __launch_bounds__(kThreads) void k_tail_b(MinresState* __restrict__ st, const double* __restrict__ partials, int nblocks)
{
    __shared__ double red[4];
    if (st->done)
        return;
    const double bb = sum_partials(partials, nblocks, red);
    if (threadIdx.x != 0)
        return;
    MinresState s = *st;
    s.l_s = s.s;
    s.oldb = s.beta;
    s.beta = sqrt(bb);
    const double oldeps = s.epsln;
    const double delta = fma(s.cs, s.dbar, s.sn * s.alfa);
    const double gbar = fma(s.sn, s.dbar, -(s.cs * s.alfa));
    s.epsln = s.sn * s.beta;
    s.dbar = -s.cs * s.beta;
    double gamma = sqrt(fma(gbar, gbar, s.beta * s.beta));
    if (!(gamma >= 2.2250738585072014e-308))  // A - sigma B is singular on the Krylov space: the residual estimate stays where it is
        gamma = gamma == gamma ? 2.2250738585072014e-308 : gamma;
    s.cs = gbar / gamma;
    s.sn = s.beta / gamma;
    s.l_oldeps = oldeps;
    s.l_delta = delta;
    s.l_gamma = gamma;
    s.l_phi = s.cs * s.phibar;
    s.phibar = s.sn * s.phibar;
    s.iter += 1;
    s.s = 1.0 / s.beta;
    s.c_r1 = s.beta / s.oldb;
    if (!(bb >= 0.0) || !(fabs(s.phibar) <= 1.7e308) || !(fabs(s.l_phi) <= 1.7e308))
        s.done = 3;
    else if (s.beta == 0.0 || fabs(s.phibar) <= s.stop)
        s.done = 1;  // beta == 0: the Krylov space is exhausted and the iterate exact
    else if (s.iter >= s.cap)
        s.done = 2;
    *st = s;
}

// After a pass of k >= 1 iterations: the update of iteration k that no pass A ran, then y = sol (first pass) or y += sol (a
// restart's correction); y goes to the caller's vector and to the handle's aligned copy, which the residual's product reads.
template <bool AL>
__global__ __launch_bounds__(kThreads) void k_finish(const MinresState* __restrict__ st, int64_t n, const double* __restrict__ zp,
                                                      const double* __restrict__ wa, const double* __restrict__ wb,
                                                      const double* __restrict__ sol, int first, double* __restrict__ ycur,
                                                      double* __restrict__ y)
{
    const MinresState s = *st;
    const bool lag = s.iter > 0;
    for_rows(
        n,
        [&](int64_t i) {
            double2 x = ld2(sol, i);
            if (lag)
            {
                const double2 zo = ld2(zp, i), b = ld2(wb, i);
                double2 a = ld2(wa, i);
                lag_update(s, zo.x, a.x, b.x, x.x);
                lag_update(s, zo.y, a.y, b.y, x.y);
            }
            if (!first)
            {
                const double2 y0 = ld2(ycur, i);
                x.x = y0.x + x.x;
                x.y = y0.y + x.y;
            }
            st2(ycur, i, x);
            ext_st2<AL>(y, i, x);
        },
        [&](int64_t i) {
            double x = sol[i];
            if (lag)
            {
                double a = wa[i];
                lag_update(s, zp[i], a, wb[i], x);
            }
            if (!first)
                x = ycur[i] + x;
            ycur[i] = x;
            y[i] = x;
        });
}

// res = x - (p - sigma (q | y)) with p = A y, q = B y; records max |res|, max |y|, max |x|
template <bool AL>
__global__ __launch_bounds__(kThreads) void k_residual(int64_t n, double sigma, const double* __restrict__ x, const double* __restrict__ y,
                                                        const double* __restrict__ p, const double* __restrict__ q,
                                                        double* __restrict__ res, double* __restrict__ partials)
{
    __shared__ double red[4];
    double mr = 0.0, my = 0.0, mx = 0.0;
    const auto row = [&](double xv, double yv, double pv, double qv) {
        const double r = xv - fma(-sigma, qv, pv);
        mr = nan_max(mr, fabs(r));
        my = nan_max(my, fabs(yv));
        mx = nan_max(mx, fabs(xv));
        return r;
    };
    for_rows(
        n,
        [&](int64_t i) {
            const double2 xv = ext_ld2<AL>(x, i), yv = ld2(y, i), pv = ld2(p, i), qv = q ? ld2(q, i) : yv;
            double2 r;
            r.x = row(xv.x, yv.x, pv.x, qv.x);
            r.y = row(xv.y, yv.y, pv.y, qv.y);
            st2(res, i, r);
        },
        [&](int64_t i) { res[i] = row(x[i], y[i], p[i], q ? q[i] : y[i]); });
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

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

std::string sci(double v)
{
    char buf[48];
    std::snprintf(buf, sizeof(buf), "%.3e", v);
    return buf;
}

mispec_csr* ingest(mispec_ctx* ctx, int64_t n, const TriangleView& T)
{
    mispec_csr* out = nullptr;
    if (mispec_csr_from_triangle(ctx, n, T.outer, T.inner, T.val, T.uplo, T.row_major, &out) != MISPEC_OK)
        throw Error(MISPEC_EINVAL, mispec_last_error());
    return out;
}

// diag and row sums of |.| in the caller's index order
void diag_rowsum(const mispec_csr& A, int64_t n, DevBuf<double>& diag, DevBuf<double>& rowsum)
{
    diag.alloc(size_t(n) + 2);
    rowsum.alloc(size_t(n) + 2);
    hipStream_t st = A.ctx->stream;
    const dim3 grid(unsigned((n + kThreads - 1) / kThreads));
    if (!A.reordered())
    {
        hipLaunchKernelGGL(k_diag_rowsum, grid, dim3(kThreads), 0, st, A.rowptr.p, A.colind.p, A.val.p, n, diag.p, rowsum.p);
        MISPEC_HIP(hipGetLastError());
        return;
    }
    // the stored matrix is P A P': entry i of what the kernel computes belongs to row perm[i]
    DevBuf<double> d, r;
    d.alloc(size_t(n));
    r.alloc(size_t(n));
    hipLaunchKernelGGL(k_diag_rowsum, grid, dim3(kThreads), 0, st, A.rowptr.p, A.colind.p, A.val.p, n, d.p, r.p);
    MISPEC_HIP(hipGetLastError());
    launch_from_stored_order(A, d.p, diag.p);
    launch_from_stored_order(A, r.p, rowsum.p);
    MISPEC_HIP(hipStreamSynchronize(st));  // d and r are freed on return
}

// p = Op v where the pass still iterates: the stop predicate rides on the product's epilogue, whose records nobody reads
void product(const ShiftMinres& M, const mispec_csr& Op, const double* v, double* out, bool predicated)
{
    if (!predicated)
    {
        launch_spmv(Op, v, out, nullptr);
        return;
    }
    SpmvEpilogue epi;
    epi.v_rows = v;
    epi.partials = M.epi_partials.p;
    epi.status = &M.state.p->done;
    launch_spmv(Op, v, out, &epi);
}

}  // namespace

mispec::ShiftMinres::~ShiftMinres()
{
    if (A)
        (void) mispec_csr_destroy(A);
    if (B)
        (void) mispec_csr_destroy(B);
}

namespace mispec {

void minres_create(mispec_symshift& S, const TriangleView& A, const TriangleView& B)
{
    auto M = std::make_unique<ShiftMinres>();
    M->A = ingest(S.ctx, S.n, A);
    if (B.outer)
        M->B = ingest(S.ctx, S.n, B);
    S.ctx->make_current();
    diag_rowsum(*M->A, S.n, M->diagA, M->absA);
    if (M->B)
        diag_rowsum(*M->B, S.n, M->diagB, M->absB);
    MISPEC_HIP(hipStreamSynchronize(S.ctx->stream));
    S.minres = std::move(M);
}

void minres_set_shift(mispec_symshift& S, double sigma)
{
    ShiftMinres& M = *S.minres;
    const mispec_ctx& ctx = *S.ctx;
    const int64_t n = S.n;
    hipStream_t st = ctx.stream;
    if (!M.minv.p)
    {
        const size_t np = size_t(n) + 2;
        M.grid = int(std::max<int64_t>(1, std::min<int64_t>(((n + 1) / 2 + kThreads - 1) / kThreads, int64_t(ctx.num_cu) * 4)));
        M.minv.alloc(np);
        for (DevBuf<double>* v : {&M.rb[0], &M.rb[1], &M.z[0], &M.z[1], &M.w[0], &M.w[1], &M.p, &M.sol, &M.ycur, &M.res})
            v->alloc(np);
        if (M.B)
            M.q.alloc(np);
        M.partials.alloc(3 * size_t(M.grid));
        M.epi_partials.alloc(size_t(spmv_num_blocks(n)) + 1);
        M.norms.alloc(3);
        M.state.alloc(1);
        M.h_state.alloc(1);
        M.h_norms.alloc(3);
    }
    const dim3 g(unsigned(M.grid)), b(kThreads);
    const double* dB = M.B ? M.diagB.p : nullptr;
    hipLaunchKernelGGL(k_shift_scan, g, b, 0, st, n, sigma, M.diagA.p, dB, M.absA.p, M.B ? M.absB.p : nullptr, M.partials.p);
    hipLaunchKernelGGL(k_max_slots, dim3(1), b, 0, st, M.partials.p, M.grid, 2, M.norms.p);
    hipLaunchKernelGGL(k_precond, g, b, 0, st, n, sigma, M.diagA.p, dB, M.norms.p, M.minv.p);
    MISPEC_HIP(hipGetLastError());
    MISPEC_HIP(hipMemcpyAsync(M.h_norms.p, M.norms.p, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    MISPEC_HIP(hipStreamSynchronize(st));
    M.mnorm = M.h_norms.p[1];
    if (!(M.mnorm == M.mnorm) || !(sigma == sigma))
        throw Error(MISPEC_EINVAL, "SparseSymShiftSolve: the matrix or the shift is not finite");
    // the probe right-hand side of the direct paths' calibration, solved to the same acceptance rule
    DevBuf<double> px, py;
    px.alloc(size_t(n) + 2);
    py.alloc(size_t(n) + 2);
    launch_probe_fill(ctx, n, px.p);
    S.sigma = sigma;
    minres_solve(S, px.p, py.p, true);
    MISPEC_HIP(hipStreamSynchronize(st));
    S.refine_steps = 0;
    S.boosted_pivots = 0;
    S.min_pivot_ratio = 0.0;
    S.probe_backward_error = M.last_backward_error;
    M.probe_iterations = M.last_iterations;
}

void minres_solve(const mispec_symshift& S, const double* x_dev, double* y_dev, bool probe)
{
    ShiftMinres& M = *S.minres;
    const mispec_ctx& ctx = *S.ctx;
    const int64_t n = S.n;
    const double sigma = S.sigma;
    hipStream_t st = ctx.stream;
    const dim3 g(unsigned(M.grid)), b(kThreads), one(1);
    const int check = std::max(1, std::min(shift_options().minres_check, kMinresMaxCheck));
    const double* q = M.B ? M.q.p : nullptr;
    MinresState& hs = *M.h_state.p;
    const bool xal = aligned16(x_dev), yal = aligned16(y_dev);
    const double accept = std::max(M.tol, kMinresStagnation);

    int64_t used = 0;
    int passes = 0;
    double omega = 1.0, prev = std::numeric_limits<double>::infinity();
    const auto fail = [&](const std::string& why) {
        M.last_iterations = used;
        M.last_passes = passes;
        M.last_backward_error = omega;
        M.total_iterations += used;
        M.solves += 1;
        throw Error(probe ? MISPEC_EINVAL : MISPEC_ERUNTIME,
                    "SparseSymShiftSolve: the iterative solve with the given shift did not converge in " + std::to_string(used) +
                        " iterations (backward error " + sci(omega) + why + ")");
    };
    for (int pass = 0;; pass++)
    {
        const double* rhs = pass == 0 ? x_dev : M.res.p;
        const double need = kMargin * std::min(1.0, M.tol / omega);
        const int cap = int(std::max<int64_t>(0, int64_t(M.max_iterations) - used));
        if (pass == 0 && !xal)
            hipLaunchKernelGGL(k_start<false>, g, b, 0, st, n, rhs, M.minv.p, M.rb[0].p, M.rb[1].p, M.z[1].p, M.w[0].p, M.w[1].p, M.sol.p,
                               M.partials.p);
        else
            hipLaunchKernelGGL(k_start<true>, g, b, 0, st, n, rhs, M.minv.p, M.rb[0].p, M.rb[1].p, M.z[1].p, M.w[0].p, M.w[1].p, M.sol.p,
                               M.partials.p);
        hipLaunchKernelGGL(k_tail_start, one, b, 0, st, M.state.p, M.partials.p, M.grid, need, cap);
        MISPEC_HIP(hipGetLastError());
        int enq = 0;
        for (;;)
        {
            for (int c = 0; c < check && enq < cap; c++)
            {
                const int j = ++enq;
                double* zc = M.z[j & 1].p;
                product(M, *M.A, zc, M.p.p, true);
                if (M.B)
                    product(M, *M.B, zc, M.q.p, true);
                hipLaunchKernelGGL(k_pass_a, g, b, 0, st, M.state.p, n, sigma, M.p.p, q, zc, M.z[(j - 1) & 1].p, M.rb[j & 1].p,
                                   M.w[(j - 1) & 1].p, M.w[j & 1].p, M.sol.p, M.partials.p);
                hipLaunchKernelGGL(k_tail_a, one, b, 0, st, M.state.p, M.partials.p, M.grid);
                hipLaunchKernelGGL(k_pass_b, g, b, 0, st, M.state.p, n, M.rb[j & 1].p, M.rb[(j - 1) & 1].p, M.minv.p, M.z[(j + 1) & 1].p,
                                   M.partials.p);
                hipLaunchKernelGGL(k_tail_b, one, b, 0, st, M.state.p, M.partials.p, M.grid);
                MISPEC_HIP(hipGetLastError());
            }
            MISPEC_HIP(hipMemcpyAsync(&hs, M.state.p, sizeof(MinresState), hipMemcpyDeviceToHost, st));
            MISPEC_HIP(hipStreamSynchronize(st));
            if (hs.done != 0)
                break;
            if (enq >= cap)
                throw Error(MISPEC_ERUNTIME, "internal: the iterative shift solve ran past its iteration cap");
        }
        const int k = hs.iter;
        used += k;
        passes++;
        if (hs.done == 3)
        {
            omega = std::numeric_limits<double>::quiet_NaN();
            fail("; the recurrence is not finite");
        }
        if (pass == 0 && hs.beta1 == 0.0)  // x = 0: y = 0, nothing iterated
        {
            MISPEC_HIP(hipMemsetAsync(y_dev, 0, size_t(n) * sizeof(double), st));
            omega = 0.0;
            break;
        }
        {
            const double *zp = M.z[k & 1].p, *wa = M.w[k & 1].p, *wb = M.w[(k + 1) & 1].p;
            if (yal)
                hipLaunchKernelGGL(k_finish<true>, g, b, 0, st, M.state.p, n, zp, wa, wb, M.sol.p, pass == 0 ? 1 : 0, M.ycur.p, y_dev);
            else
                hipLaunchKernelGGL(k_finish<false>, g, b, 0, st, M.state.p, n, zp, wa, wb, M.sol.p, pass == 0 ? 1 : 0, M.ycur.p, y_dev);
        }
        product(M, *M.A, M.ycur.p, M.p.p, false);
        if (M.B)
            product(M, *M.B, M.ycur.p, M.q.p, false);
        if (xal)
            hipLaunchKernelGGL(k_residual<true>, g, b, 0, st, n, sigma, x_dev, M.ycur.p, M.p.p, q, M.res.p, M.partials.p);
        else
            hipLaunchKernelGGL(k_residual<false>, g, b, 0, st, n, sigma, x_dev, M.ycur.p, M.p.p, q, M.res.p, M.partials.p);
        hipLaunchKernelGGL(k_max_slots, one, b, 0, st, M.partials.p, M.grid, 3, M.norms.p);
        MISPEC_HIP(hipGetLastError());
        MISPEC_HIP(hipMemcpyAsync(M.h_norms.p, M.norms.p, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        MISPEC_HIP(hipStreamSynchronize(st));
        const double nr = M.h_norms.p[0], ny = M.h_norms.p[1], nx = M.h_norms.p[2];
        omega = nr / (M.mnorm * ny + nx);
        if (!(omega == omega))
            fail("; the solution is not finite");
        if (omega <= M.tol)
            break;
        const bool capped = used >= M.max_iterations;
        if (pass == kMinresRestarts || capped || (pass >= 1 && omega > 0.9 * prev))
        {
            if (omega <= accept)  // stagnation at a backward error below the eigensolvers' tolerances
                break;
            fail(capped ? "" : "; stagnating after " + std::to_string(passes) + " passes");
        }
        prev = omega;
    }
    M.last_iterations = used;
    M.last_passes = passes;
    M.last_backward_error = omega;
    M.total_iterations += used;
    M.solves += 1;
}

}  // namespace mispec

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" int mispec_symshift_set_iterative(mispec_symshift* S, double tol, int max_iterations)
{
    return guarded([&] {
        MISPEC_REQUIRE(S, "mispec_symshift_set_iterative: NULL argument");
        MISPEC_REQUIRE(S->minres != nullptr, "mispec_symshift_set_iterative: the operator is not on the iterative path");
        MISPEC_REQUIRE(tol == tol, "mispec_symshift_set_iterative: tol is not a number");
        S->minres->tol = tol > 0.0 ? tol : kMinresTol;
        S->minres->max_iterations = max_iterations > 0 ? max_iterations : kMinresMaxIterations;
    });
}

extern "C" int mispec_symshift_iterative_info(const mispec_symshift* S, int64_t* last_iterations, int64_t* total_iterations, int64_t* solves,
                                              int* last_passes, double* last_backward_error, int64_t* probe_iterations)
{
    return guarded([&] {
        MISPEC_REQUIRE(S, "mispec_symshift_iterative_info: NULL argument");
        const ShiftMinres* M = S->minres.get();  // an operator on a direct path reports zeros
        if (last_iterations)
            *last_iterations = M ? M->last_iterations : 0;
        if (total_iterations)
            *total_iterations = M ? M->total_iterations : 0;
        if (solves)
            *solves = M ? M->solves : 0;
        if (last_passes)
            *last_passes = M ? M->last_passes : 0;
        if (last_backward_error)
            *last_backward_error = M ? M->last_backward_error : 0.0;
        if (probe_iterations)
            *probe_iterations = M ? M->probe_iterations : 0;
    });
}
