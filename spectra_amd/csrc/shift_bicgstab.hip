// Iterative path of the general (non-symmetric) shift-and-invert operator: y = (A - sigma I)^{-1} x by right-preconditioned BiCGStab
// (van der Vorst 1992) with the Jacobi preconditioner, for any sparsity pattern.  Opt-in (option shift_solver,
// mispec_symshift_create_general_solver); DESIGN.md 3.5.3.  MINRES (shift_minres.hip) needs A = A'; what the two share is in
// shift_iterative.hpp.
//
// One iteration, with M = A - sigma I never formed, minv = 1 / diag M, d the direction (the p of the usual listings):
//   pass D    d = r + beta (d - omega v) ; dhat = minv .* d         beta, omega of the previous iteration (0 at the first: d = r)
//   product   u = A dhat                                            launch_spmv, predicated by its epilogue
//   pass V    v = u - sigma dhat ; records sum rhat v
//   tail V    alpha = rho / <rhat, v>
//   pass S    s = r - alpha v (in place of r) ; shat = minv .* s
//   product   u = A shat
//   pass T    t = u - sigma shat ; records sum t s, sum t t
//   tail T    omega = <t, s> / <t, t>
//   pass X    x += alpha dhat + omega shat ; r = s - omega t (in place of s) ; records sum rhat r, sum r r
//   tail X    rho' = <rhat, r>, |r|, beta = (rho' / rho)(alpha / omega), the stop decision
// The update of d needs beta, which pass X's own reduction gives: it is the first pass of the next iteration, where beta lies in
// device memory.  The three reductions are two-stage and fixed-order; their second stage (one workgroup) runs the scalar
// recurrence into BicgstabState.  Every kernel returns at once when BicgstabState::done is set, so the iterations the host
// enqueued behind the one that finished change nothing, and the result does not depend on how often the host looks
// (shift=minres_check=N).
//
// A solve is up to 1 + kMinresRestarts passes with the acceptance rule of shift_minres.hip: after each, the explicit residual gives
// the backward error omega; accepted at `tol`, otherwise BiCGStab restarts on the residual (rhat = that residual) and the
// correction is added.  A pass ends where the recurrence's |r|_2 has dropped by what omega still needs, at the iteration cap, or
// at a breakdown (rho = 0, <rhat, v> = 0, or omega = 0 with |r| = |s| above the stop), which is the end of a pass and no error.
// One difference to MINRES: a pass that the iteration cap ended fails the solve whatever omega says (bicgstab_solve).
#include "shift_bicgstab.hpp"

#include <cstring>
#include <memory>

#include "shift_iterative.hpp"

// the bits of every sum and update are those of the operations written here: products and sums are not contracted, fma is explicit
#pragma clang fp contract(off)

using namespace mispec;
using namespace mispec::shift_iter;

namespace {

constexpr double kHuge = 1.7e308;

// ---- a pass's start: r = rhat = rhs, d = v = x = 0; records sum rhs rhs = rho_0 ------------------------------------------------
template <bool AL>
__global__ __launch_bounds__(kThreads) void k_start(int64_t n, const double* __restrict__ rhs, double* __restrict__ r,
                                                     double* __restrict__ rhat, double* __restrict__ d, double* __restrict__ v,
                                                     double* __restrict__ sol, double* __restrict__ partials)
{
    __shared__ double red[4];
    double acc = 0.0;
    const double2 zero = make_double2(0.0, 0.0);
    for_rows(
        n,
        [&](int64_t i) {
            const double2 b = ext_ld2<AL>(rhs, i);
            st2(r, i, b);
            st2(rhat, i, b);
            st2(d, i, zero);
            st2(v, i, zero);
            st2(sol, i, zero);
            acc = fma(b.x, b.x, acc);
            acc = fma(b.y, b.y, acc);
        },
        [&](int64_t i) {
            const double b = rhs[i];
            r[i] = rhat[i] = b;
            d[i] = v[i] = sol[i] = 0.0;
            acc = fma(b, b, acc);
        });
    acc = block_sum(acc, red);
    if (threadIdx.x == 0)
        partials[blockIdx.x] = acc;
}

__global__ __launch_bounds__(kThreads) void k_tail_start(BicgstabState* __restrict__ st, const double* __restrict__ partials, int nblocks,
                                                          double need, int cap)
{
    __shared__ double red[4];
    const double rr = sum_partials(partials, nblocks, red);
    if (threadIdx.x != 0)
        return;
    BicgstabState s;
    s.iter = 0;
    s.cap = cap;
    s.pad = 0;
    s.rho = rr;
    s.alpha = s.omega = s.beta = 0.0;  // pass D of the first iteration: d = r
    s.rnorm = s.rhs_norm = sqrt(rr);
    s.stop = need * s.rhs_norm;
    // rr == 0 is rhs == 0: nothing to iterate on
    s.done = !(rr >= 0.0) || !(rr <= kHuge) ? 3 : (rr == 0.0 ? 1 : (cap <= 0 ? 2 : 0));
    *st = s;
}

// pass D: d = r + beta (d - omega v), dhat = minv .* d
__global__ __launch_bounds__(kThreads) void k_pass_d(const BicgstabState* __restrict__ st, int64_t n, const double* __restrict__ r,
                                                      const double* __restrict__ v, const double* __restrict__ minv,
                                                      double* __restrict__ d, double* __restrict__ dhat)
{
    const BicgstabState s = *st;
    if (s.done)
        return;
    const auto row = [&](double rv, double vv, double dv) { return fma(s.beta, fma(-s.omega, vv, dv), rv); };
    for_rows(
        n,
        [&](int64_t i) {
            const double2 rv = ld2(r, i), vv = ld2(v, i), dv = ld2(d, i), m = ld2(minv, i);
            double2 dn, h;
            dn.x = row(rv.x, vv.x, dv.x);
            dn.y = row(rv.y, vv.y, dv.y);
            h.x = m.x * dn.x;
            h.y = m.y * dn.y;
            st2(d, i, dn);
            st2(dhat, i, h);
        },
        [&](int64_t i) {
            const double dn = row(r[i], v[i], d[i]);
            d[i] = dn;
            dhat[i] = minv[i] * dn;
        });
}

// pass V: v = u - sigma dhat; records sum rhat v
__global__ __launch_bounds__(kThreads) void k_pass_v(const BicgstabState* __restrict__ st, int64_t n, double sigma,
                                                      const double* __restrict__ u, const double* __restrict__ dhat,
                                                      const double* __restrict__ rhat, double* __restrict__ v,
                                                      double* __restrict__ partials)
{
    __shared__ double red[4];
    if (st->done)
        return;
    double acc = 0.0;
    for_rows(
        n,
        [&](int64_t i) {
            const double2 uv = ld2(u, i), h = ld2(dhat, i), rh = ld2(rhat, i);
            double2 vn;
            vn.x = fma(-sigma, h.x, uv.x);
            vn.y = fma(-sigma, h.y, uv.y);
            st2(v, i, vn);
            acc = fma(rh.x, vn.x, acc);
            acc = fma(rh.y, vn.y, acc);
        },
        [&](int64_t i) {
            const double vn = fma(-sigma, dhat[i], u[i]);
            v[i] = vn;
            acc = fma(rhat[i], vn, acc);
        });
    acc = block_sum(acc, red);
    if (threadIdx.x == 0)
        partials[blockIdx.x] = acc;
}

__global__ __launch_bounds__(kThreads) void k_tail_v(BicgstabState* __restrict__ st, const double* __restrict__ partials, int nblocks)
{
    __shared__ double red[4];
    if (st->done)
        return;
    const double rv = sum_partials(partials, nblocks, red);  // (its barriers lie between the read of done above and the writes below)
    if (threadIdx.x != 0)
        return;
    if (!(fabs(rv) <= kHuge))
        st->done = 3;
    else if (rv == 0.0)
        st->done = 4;
    else
        st->alpha = st->rho / rv;
}

// pass S: s = r - alpha v in place of r, shat = minv .* s
__global__ __launch_bounds__(kThreads) void k_pass_s(const BicgstabState* __restrict__ st, int64_t n, double* __restrict__ r,
                                                      const double* __restrict__ v, const double* __restrict__ minv,
                                                      double* __restrict__ shat)
{
    const BicgstabState s = *st;
    if (s.done)
        return;
    for_rows(
        n,
        [&](int64_t i) {
            const double2 rv = ld2(r, i), vv = ld2(v, i), m = ld2(minv, i);
            double2 sn, h;
            sn.x = fma(-s.alpha, vv.x, rv.x);
            sn.y = fma(-s.alpha, vv.y, rv.y);
            h.x = m.x * sn.x;
            h.y = m.y * sn.y;
            st2(r, i, sn);
            st2(shat, i, h);
        },
        [&](int64_t i) {
            const double sn = fma(-s.alpha, v[i], r[i]);
            r[i] = sn;
            shat[i] = minv[i] * sn;
        });
}

// pass T: t = u - sigma shat; records sum t s and sum t t
__global__ __launch_bounds__(kThreads) void k_pass_t(const BicgstabState* __restrict__ st, int64_t n, double sigma,
                                                      const double* __restrict__ u, const double* __restrict__ shat,
                                                      const double* __restrict__ s, double* __restrict__ t, double* __restrict__ partials)
{
    __shared__ double red[4];
    if (st->done)
        return;
    double ts = 0.0, tt = 0.0;
    for_rows(
        n,
        [&](int64_t i) {
            const double2 uv = ld2(u, i), h = ld2(shat, i), sv = ld2(s, i);
            double2 tn;
            tn.x = fma(-sigma, h.x, uv.x);
            tn.y = fma(-sigma, h.y, uv.y);
            st2(t, i, tn);
            ts = fma(tn.x, sv.x, ts);
            ts = fma(tn.y, sv.y, ts);
            tt = fma(tn.x, tn.x, tt);
            tt = fma(tn.y, tn.y, tt);
        },
        [&](int64_t i) {
            const double tn = fma(-sigma, shat[i], u[i]);
            t[i] = tn;
            ts = fma(tn, s[i], ts);
            tt = fma(tn, tn, tt);
        });
    ts = block_sum(ts, red);
    tt = block_sum(tt, red);
    if (threadIdx.x == 0)
    {
        partials[blockIdx.x] = ts;
        partials[gridDim.x + blockIdx.x] = tt;
    }
}

__global__ __launch_bounds__(kThreads) void k_tail_t(BicgstabState* __restrict__ st, const double* __restrict__ partials, int nblocks)
{
    __shared__ double red[4];
    if (st->done)
        return;
    const double ts = sum_partials(partials, nblocks, red);
    const double tt = sum_partials(partials + nblocks, nblocks, red);
    if (threadIdx.x != 0)
        return;
    if (!(tt >= 0.0) || !(tt <= kHuge) || !(fabs(ts) <= kHuge))
        st->done = 3;
    else
        st->omega = tt == 0.0 ? 0.0 : ts / tt;  // t = 0: r = s, and tail X decides between converged and breakdown
}

// pass X: x += alpha dhat + omega shat; r = s - omega t in place of s; records sum rhat r and sum r r
__global__ __launch_bounds__(kThreads) void k_pass_x(const BicgstabState* __restrict__ st, int64_t n, const double* __restrict__ dhat,
                                                      const double* __restrict__ shat, double* __restrict__ r,
                                                      const double* __restrict__ t, const double* __restrict__ rhat,
                                                      double* __restrict__ sol, double* __restrict__ partials)
{
    __shared__ double red[4];
    const BicgstabState s = *st;
    if (s.done)
        return;
    double hr = 0.0, rr = 0.0;
    for_rows(
        n,
        [&](int64_t i) {
            const double2 dh = ld2(dhat, i), sh = ld2(shat, i), sv = ld2(r, i), tv = ld2(t, i), rh = ld2(rhat, i);
            double2 x = ld2(sol, i), rn;
            x.x = fma(s.omega, sh.x, fma(s.alpha, dh.x, x.x));
            x.y = fma(s.omega, sh.y, fma(s.alpha, dh.y, x.y));
            rn.x = fma(-s.omega, tv.x, sv.x);
            rn.y = fma(-s.omega, tv.y, sv.y);
            st2(sol, i, x);
            st2(r, i, rn);
            hr = fma(rh.x, rn.x, hr);
            hr = fma(rh.y, rn.y, hr);
            rr = fma(rn.x, rn.x, rr);
            rr = fma(rn.y, rn.y, rr);
        },
        [&](int64_t i) {
            sol[i] = fma(s.omega, shat[i], fma(s.alpha, dhat[i], sol[i]));
            const double rn = fma(-s.omega, t[i], r[i]);
            r[i] = rn;
            hr = fma(rhat[i], rn, hr);
            rr = fma(rn, rn, rr);
        });
    hr = block_sum(hr, red);
    rr = block_sum(rr, red);
    if (threadIdx.x == 0)
    {
        partials[blockIdx.x] = hr;
        partials[gridDim.x + blockIdx.x] = rr;
    }
}

__global__ __launch_bounds__(kThreads) void k_tail_x(BicgstabState* __restrict__ st, const double* __restrict__ partials, int nblocks)
{
    __shared__ double red[4];
    if (st->done)
        return;
    const double hr = sum_partials(partials, nblocks, red);
    const double rr = sum_partials(partials + nblocks, nblocks, red);
    if (threadIdx.x != 0)
        return;
    BicgstabState s = *st;
    s.iter += 1;
    s.rnorm = sqrt(rr);
    const double beta = (hr / s.rho) * (s.alpha / s.omega);
    if (!(rr >= 0.0) || !(rr <= kHuge) || !(fabs(hr) <= kHuge))
        s.done = 3;
    else if (s.rnorm <= s.stop)
        s.done = 1;
    else if (s.omega == 0.0 || hr == 0.0 || !(fabs(beta) <= kHuge))
        s.done = 4;  // the recurrence cannot go on from here: the host restarts it from the explicit residual
    else if (s.iter >= s.cap)
        s.done = 2;
    s.beta = beta;
    s.rho = hr;
    *st = s;
}

// after a pass: y = sol (first pass) or y += sol (a restart's correction); y goes to the caller's vector and to the handle's
// aligned copy, which the residual's product reads
template <bool AL>
__global__ __launch_bounds__(kThreads) void k_finish(int64_t n, const double* __restrict__ sol, int first, double* __restrict__ ycur,
                                                      double* __restrict__ y)
{
    for_rows(
        n,
        [&](int64_t i) {
            double2 x = ld2(sol, i);
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
            const double x = first ? sol[i] : ycur[i] + sol[i];
            ycur[i] = x;
            y[i] = x;
        });
}

}  // namespace

namespace mispec {

void bicgstab_create(mispec_symshift& S, const int32_t* outer, const int32_t* inner, const double* val, int row_major)
{
    auto M = std::make_unique<ShiftBicgstab>();
    // the general ingest of SparseGenMatProd: CSR as it is, CSC transposed (rows in column order) — one operator for both orders
    const int rc = row_major ? mispec_csr_upload(S.ctx, S.n, S.n, outer, inner, val, &M->A)
                             : mispec_csr_from_csc(S.ctx, S.n, S.n, outer, inner, val, &M->A);
    if (rc != MISPEC_OK)
        throw Error(rc, mispec_last_error());
    S.ctx->make_current();
    diag_rowsum(*M->A, S.n, M->diagA, M->absA);
    MISPEC_HIP(hipStreamSynchronize(S.ctx->stream));
    S.bicgstab = std::move(M);
}

void bicgstab_alloc(mispec_symshift& S)
{
    ShiftBicgstab& M = *S.bicgstab;
    if (M.minv.p)
        return;
    const size_t np = size_t(S.n) + 2;
    alloc_shared(M, *S.ctx, S.n);
    for (DevBuf<double>* v : {&M.rs, &M.rhat, &M.d, &M.dhat, &M.v, &M.shat, &M.t, &M.sol})
        v->alloc(np);
    M.state.alloc(1);
    M.h_state.alloc(1);
}

void bicgstab_set_shift(mispec_symshift& S, double sigma)
{
    ShiftBicgstab& M = *S.bicgstab;
    const mispec_ctx& ctx = *S.ctx;
    const int64_t n = S.n;
    bicgstab_alloc(S);
    form_preconditioner<true>(M, ctx, n, sigma, nullptr, nullptr);
    solve_probe(S, M, sigma, [&](const double* x, double* y) { bicgstab_solve(S, x, y, true); });
}

void bicgstab_solve(const mispec_symshift& S, const double* x_dev, double* y_dev, bool probe)
{
    ShiftBicgstab& M = *S.bicgstab;
    const mispec_ctx& ctx = *S.ctx;
    const int64_t n = S.n;
    const double sigma = S.sigma;
    hipStream_t st = ctx.stream;
    const dim3 g(unsigned(M.grid)), b(kThreads), one(1);
    const int check = std::max(1, std::min(shift_options().minres_check, kMinresMaxCheck));
    BicgstabState& hs = *M.h_state.p;
    const int* done = &M.state.p->done;
    SolveRecord rec{M, probe};
    for (int pass = 0;; pass++)
    {
        const double* rhs = pass == 0 ? x_dev : M.res.p;
        const int cap = rec.cap();
        if (pass == 0 && !aligned16(x_dev))
            hipLaunchKernelGGL(k_start<false>, g, b, 0, st, n, rhs, M.rs.p, M.rhat.p, M.d.p, M.v.p, M.sol.p, M.partials.p);
        else
            hipLaunchKernelGGL(k_start<true>, g, b, 0, st, n, rhs, M.rs.p, M.rhat.p, M.d.p, M.v.p, M.sol.p, M.partials.p);
        hipLaunchKernelGGL(k_tail_start, one, b, 0, st, M.state.p, M.partials.p, M.grid, rec.need(), cap);
        MISPEC_HIP(hipGetLastError());
        int enq = 0;
        for (;;)
        {
            for (int c = 0; c < check && enq < cap; c++, enq++)
            {
                hipLaunchKernelGGL(k_pass_d, g, b, 0, st, M.state.p, n, M.rs.p, M.v.p, M.minv.p, M.d.p, M.dhat.p);
                product(M, *M.A, M.dhat.p, M.p.p, done);
                hipLaunchKernelGGL(k_pass_v, g, b, 0, st, M.state.p, n, sigma, M.p.p, M.dhat.p, M.rhat.p, M.v.p, M.partials.p);
                hipLaunchKernelGGL(k_tail_v, one, b, 0, st, M.state.p, M.partials.p, M.grid);
                hipLaunchKernelGGL(k_pass_s, g, b, 0, st, M.state.p, n, M.rs.p, M.v.p, M.minv.p, M.shat.p);
                product(M, *M.A, M.shat.p, M.p.p, done);
                hipLaunchKernelGGL(k_pass_t, g, b, 0, st, M.state.p, n, sigma, M.p.p, M.shat.p, M.rs.p, M.t.p, M.partials.p);
                hipLaunchKernelGGL(k_tail_t, one, b, 0, st, M.state.p, M.partials.p, M.grid);
                hipLaunchKernelGGL(k_pass_x, g, b, 0, st, M.state.p, n, M.dhat.p, M.shat.p, M.rs.p, M.t.p, M.rhat.p, M.sol.p, M.partials.p);
                hipLaunchKernelGGL(k_tail_x, one, b, 0, st, M.state.p, M.partials.p, M.grid);
                MISPEC_HIP(hipGetLastError());
            }
            MISPEC_HIP(hipMemcpyAsync(&hs, M.state.p, sizeof(BicgstabState), hipMemcpyDeviceToHost, st));
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
            hipLaunchKernelGGL(k_finish<true>, g, b, 0, st, n, M.sol.p, pass == 0 ? 1 : 0, M.ycur.p, y_dev);
        else
            hipLaunchKernelGGL(k_finish<false>, g, b, 0, st, n, M.sol.p, pass == 0 ? 1 : 0, M.ycur.p, y_dev);
        product(M, *M.A, M.ycur.p, M.p.p, nullptr);
        const double w = backward_error(M, ctx, n, sigma, x_dev, nullptr);
        if (hs.done == 2)
        {
            // BiCGStab's iterates are monotone in no norm, and on a singular A - sigma I they grow without bound, which alone makes
            // omega small (|y| is in its denominator): an iterate that the cap cut off is not judged by omega, unlike MINRES's
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
