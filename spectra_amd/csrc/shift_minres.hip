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

#include <cstring>
#include <memory>

#include "shift_iterative.hpp"

// the bits of every sum and update are those of the operations written here: products and sums are not contracted, fma is explicit
#pragma clang fp contract(off)

using namespace mispec;
using namespace mispec::shift_iter;

namespace {

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

mispec_csr* ingest(mispec_ctx* ctx, int64_t n, const TriangleView& T)
{
    mispec_csr* out = nullptr;
    if (mispec_csr_from_triangle(ctx, n, T.outer, T.inner, T.val, T.uplo, T.row_major, &out) != MISPEC_OK)
        throw Error(MISPEC_EINVAL, mispec_last_error());
    return out;
}

}  // namespace

mispec::ShiftMinres::~ShiftMinres()
{
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
    if (!M.minv.p)
    {
        const size_t np = size_t(n) + 2;
        alloc_shared(M, ctx, n);
        for (DevBuf<double>* v : {&M.rb[0], &M.rb[1], &M.z[0], &M.z[1], &M.w[0], &M.w[1], &M.sol})
            v->alloc(np);
        if (M.B)
            M.q.alloc(np);
        M.state.alloc(1);
        M.h_state.alloc(1);
    }
    form_preconditioner<false>(M, ctx, n, sigma, M.B ? M.diagB.p : nullptr, M.B ? M.absB.p : nullptr);
    solve_probe(S, M, sigma, [&](const double* x, double* y) { minres_solve(S, x, y, true); });
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
    SolveRecord rec{M, probe};
    for (int pass = 0;; pass++)
    {
        const double* rhs = pass == 0 ? x_dev : M.res.p;
        const double need = rec.need();
        const int cap = rec.cap();
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
                product(M, *M.A, zc, M.p.p, &M.state.p->done);
                if (M.B)
                    product(M, *M.B, zc, M.q.p, &M.state.p->done);
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
        rec.used += k;
        rec.passes++;
        if (hs.done == 3)
            rec.not_finite();
        if (pass == 0 && hs.beta1 == 0.0)  // x = 0: y = 0, nothing iterated
        {
            MISPEC_HIP(hipMemsetAsync(y_dev, 0, size_t(n) * sizeof(double), st));
            rec.omega = 0.0;
            break;
        }
        {
            const double *zp = M.z[k & 1].p, *wa = M.w[k & 1].p, *wb = M.w[(k + 1) & 1].p;
            if (yal)
                hipLaunchKernelGGL(k_finish<true>, g, b, 0, st, M.state.p, n, zp, wa, wb, M.sol.p, pass == 0 ? 1 : 0, M.ycur.p, y_dev);
            else
                hipLaunchKernelGGL(k_finish<false>, g, b, 0, st, M.state.p, n, zp, wa, wb, M.sol.p, pass == 0 ? 1 : 0, M.ycur.p, y_dev);
        }
        product(M, *M.A, M.ycur.p, M.p.p, nullptr);
        if (M.B)
            product(M, *M.B, M.ycur.p, M.q.p, nullptr);
        if (rec.accepted(pass, backward_error(M, ctx, n, sigma, x_dev, q)))
            break;
    }
    rec.close();
}

}  // namespace mispec

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" int mispec_symshift_set_iterative(mispec_symshift* S, double tol, int max_iterations)
{
    return guarded([&] {
        MISPEC_REQUIRE(S, "mispec_symshift_set_iterative: NULL argument");
        ShiftIterative* M = S->iterative();
        MISPEC_REQUIRE(M != nullptr, "mispec_symshift_set_iterative: the operator is not on the iterative path");
        MISPEC_REQUIRE(tol == tol, "mispec_symshift_set_iterative: tol is not a number");
        M->tol = tol > 0.0 ? tol : kMinresTol;
        M->max_iterations = max_iterations > 0 ? max_iterations : kMinresMaxIterations;
    });
}

extern "C" int mispec_symshift_iterative_info(const mispec_symshift* S, int64_t* last_iterations, int64_t* total_iterations, int64_t* solves,
                                              int* last_passes, double* last_backward_error, int64_t* probe_iterations)
{
    return guarded([&] {
        MISPEC_REQUIRE(S, "mispec_symshift_iterative_info: NULL argument");
        const ShiftIterative* M = S->iterative();  // an operator on a direct path reports zeros
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
