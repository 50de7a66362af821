// Test hooks (include/mispec.h: mispec_lagged_pass, mispec_fused_restart_pass): ONE pass of the one-sweep Lanczos step, or of the
// fused restart, with its reduction and scalar tail, on the caller's data.  They call the launchers the factorisation calls
// (launch_orth, launch_vq_fused, launch_reduce_partials) with the arguments lagged_args.hpp fills for fac.hip as well; the kernel
// choice stays the launchers'.  Not on the hot path: every call allocates its scratch and synchronises.
#include "krylov.hpp"
#include "lagged_args.hpp"

#include <cstring>

using namespace mispec;

namespace {

void upload(const mispec_ctx& ctx, void* dst, const void* src, size_t bytes)
{
    if (bytes)
        MISPEC_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx.stream));
}

bool aligned16(const void* p)
{
    return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

// the partial records: NaN everywhere (0xff bytes), so a slot the reduction reads and no workgroup wrote shows in the result
void alloc_partials(const mispec_ctx& ctx, DevBuf<double>& partials, int64_t pstride)
{
    partials.alloc(size_t(pstride) * kPartialLd);
    MISPEC_HIP(hipMemsetAsync(partials.p, 0xff, partials.n * sizeof(double), ctx.stream));
}

}  // namespace

extern "C" int mispec_lagged_pass(mispec_ctx* ctx, const double* V_dev, int64_t ldv, int i, int64_t n, double* f_dev, const double* src_dev,
                                  double* vout_dev, const double* c_in_host, const double* alpha_parts_host, int64_t alpha_count,
                                  const double* scal_in, const int* flags_in, int64_t pstride, double* diag_host, double* subd_host,
                                  double* red_host, double* scal_out, int64_t* int_out)
{
    return guarded([&] {
        MISPEC_REQUIRE(ctx, "mispec_lagged_pass: NULL context");
        MISPEC_REQUIRE(i >= 1 && 2 * i + 1 <= kMaxCols, "mispec_lagged_pass: needs 1 <= i and 2 i + 1 <= 1024");
        MISPEC_REQUIRE(n >= 1 && ldv >= n && ldv % 2 == 0 && ldv >= round_up(n, 2), "mispec_lagged_pass: needs 1 <= n <= ld, ld even");
        MISPEC_REQUIRE(V_dev && f_dev && src_dev && vout_dev && c_in_host && scal_in && flags_in && diag_host && subd_host && red_host &&
                           scal_out && int_out,
                       "mispec_lagged_pass: NULL argument");
        MISPEC_REQUIRE(aligned16(V_dev) && aligned16(f_dev) && aligned16(src_dev) && aligned16(vout_dev),
                       "mispec_lagged_pass: the vectors must be 16-byte aligned");
        MISPEC_REQUIRE(alpha_count >= 0 && (alpha_count == 0 || alpha_parts_host), "mispec_lagged_pass: partial sums missing");
        if (pstride == 0)
            pstride = int64_t(ctx->num_cu) * 8 + 8;  // the factorisation's
        MISPEC_REQUIRE(pstride >= 1, "mispec_lagged_pass: record stride smaller than the grid");
        ctx->make_current();

        DevBuf<StepState> st;
        DevBuf<double> red, cin, alpha, partials, parts;
        st.alloc(1);
        red.alloc(kPartialLd);
        cin.alloc(size_t(i));
        alpha.alloc(1);
        alloc_partials(*ctx, partials, pstride);
        parts.alloc(size_t(alpha_count));

        std::vector<StepState> h(1);
        StepState& s0 = h[0];
        std::memset(&s0, 0, sizeof(StepState));
        s0.beta = scal_in[1];
        s0.lag_chk_max = scal_in[2];
        s0.lag_rel_c_max = scal_in[3];
        s0.lag_pending = flags_in[0];
        s0.status = flags_in[2];
        s0.lag_steps = flags_in[4];
        s0.onered_steps = flags_in[5];
        std::memcpy(s0.diag, diag_host, size_t(i + 1) * sizeof(double));
        std::memcpy(s0.subd, subd_host, size_t(i + 1) * sizeof(double));
        upload(*ctx, st.p, &s0, sizeof(StepState));
        upload(*ctx, red.p, red_host, kPartialLd * sizeof(double));
        upload(*ctx, cin.p, c_in_host, size_t(i) * sizeof(double));
        upload(*ctx, alpha.p, &scal_in[0], sizeof(double));
        upload(*ctx, parts.p, alpha_parts_host, size_t(alpha_count) * sizeof(double));

        OrthArgs base;
        base.V = V_dev;
        base.ldv = ldv;
        base.ncol = i;
        base.n = n;
        base.partials = partials.p;
        base.pstride = pstride;
        const OrthArgs a = lagged_orth_args(base, src_dev, f_dev, vout_dev, cin.p, alpha.p, st.p, flags_in[1] != 0);
        FinishArgs fin = lagged_finish_args(st.p, i, int64_t(scal_in[5]), scal_in[4], flags_in[3] != 0, option_int(Opt::spec_corr, 2),
                                            alpha.p, cin.p);
        if (alpha_count > 0)
            lagged_onered_args(fin, parts.p, alpha_count, alpha.p);
        const int nrec = launch_orth(*ctx, ORTH_LAGGED, a);
        launch_reduce_partials(*ctx, partials.p, pstride, nrec, 2 * i + 1, red.p, fin);

        StepState& s1 = h[0];
        MISPEC_HIP(hipMemcpyAsync(&s1, st.p, sizeof(StepState), hipMemcpyDeviceToHost, ctx->stream));
        MISPEC_HIP(hipMemcpyAsync(red_host, red.p, kPartialLd * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        MISPEC_HIP(hipMemcpyAsync(&scal_out[6], alpha.p, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        MISPEC_HIP(hipStreamSynchronize(ctx->stream));
        std::memcpy(diag_host, s1.diag, size_t(i + 1) * sizeof(double));
        std::memcpy(subd_host, s1.subd, size_t(i + 1) * sizeof(double));
        scal_out[0] = s1.beta;
        scal_out[1] = s1.alpha;
        scal_out[2] = s1.lag_chk_max;
        scal_out[3] = s1.lag_rel_c_max;
        scal_out[4] = s1.err;
        scal_out[5] = 0.0;
        int_out[0] = s1.status;
        int_out[1] = s1.stop_step;
        int_out[2] = s1.stop_count;
        int_out[3] = s1.count;
        int_out[4] = s1.need_corr;
        int_out[5] = s1.lag_pending;
        int_out[6] = s1.lag_steps;
        int_out[7] = s1.onered_steps;
        int_out[8] = nrec;
    });
}

extern "C" int mispec_fused_restart_pass(mispec_ctx* ctx, double* V_dev, int64_t ldv, int m, int64_t n, const double* Q_host, int p,
                                         const double* c_host, const double* ftilde_dev, double* fnew_dev, double q_last, double h_sub,
                                         int kcol, int status_in, int force_check, int64_t pstride, double* red_host, double* scal_out,
                                         int64_t* int_out)
{
    return guarded([&] {
        MISPEC_REQUIRE(ctx, "mispec_fused_restart_pass: NULL context");
        MISPEC_REQUIRE(m >= 1 && m <= kPanelCols && p >= 1 && p <= m && kcol >= 0 && kcol < p,
                       "mispec_fused_restart_pass: needs 1 <= p <= m <= 64 and 0 <= kcol < p");
        MISPEC_REQUIRE(n >= 1 && ldv >= n && ldv % 2 == 0 && ldv >= round_up(n, 2), "mispec_fused_restart_pass: needs 1 <= n <= ld, ld even");
        MISPEC_REQUIRE(V_dev && Q_host && c_host && ftilde_dev && fnew_dev && red_host && scal_out && int_out,
                       "mispec_fused_restart_pass: NULL argument");
        MISPEC_REQUIRE(aligned16(V_dev) && aligned16(ftilde_dev) && aligned16(fnew_dev),
                       "mispec_fused_restart_pass: the vectors must be 16-byte aligned");
        if (pstride == 0)
            pstride = int64_t(ctx->num_cu) * 8 + 8;
        MISPEC_REQUIRE(pstride >= 1, "mispec_fused_restart_pass: record stride smaller than the grid");
        ctx->make_current();

        DevBuf<StepState> st;
        DevBuf<double> red, c, Q, partials;
        st.alloc(1);
        red.alloc(kPartialLd);
        c.alloc(size_t(m));
        Q.alloc(size_t(m) * p);
        alloc_partials(*ctx, partials, pstride);
        std::vector<StepState> h(1);
        std::memset(&h[0], 0, sizeof(StepState));
        h[0].status = status_in;
        upload(*ctx, st.p, &h[0], sizeof(StepState));
        upload(*ctx, red.p, red_host, kPartialLd * sizeof(double));
        upload(*ctx, c.p, c_host, size_t(m) * sizeof(double));
        upload(*ctx, Q.p, Q_host, size_t(m) * p * sizeof(double));

        // in place (X = V), as mispec_fac_restart_sym runs it
        const VqFusedArgs fa = fused_restart_args(c.p, ftilde_dev, fnew_dev, q_last, h_sub, kcol, partials.p, pstride);
        const int nrec = launch_vq_fused(*ctx, V_dev, ldv, m, Q.p, m, p, V_dev, ldv, n, fa);
        const FinishArgs fin = fused_restart_finish_args(st.p, kcol, force_check ? -1.0 : kLaggedEps);
        launch_reduce_partials(*ctx, partials.p, pstride, nrec, m + 1, red.p, fin);

        MISPEC_HIP(hipMemcpyAsync(&h[0], st.p, sizeof(StepState), hipMemcpyDeviceToHost, ctx->stream));
        MISPEC_HIP(hipMemcpyAsync(red_host, red.p, kPartialLd * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        MISPEC_HIP(hipStreamSynchronize(ctx->stream));
        scal_out[0] = h[0].beta;
        scal_out[1] = h[0].rst_err;
        scal_out[2] = h[0].rst_beta_corr;
        int_out[0] = h[0].status;
        int_out[1] = h[0].stop_step;
        int_out[2] = h[0].stop_count;
        int_out[3] = nrec;
    });
}
