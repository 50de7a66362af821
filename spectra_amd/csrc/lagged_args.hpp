// The arguments of the one-sweep Lanczos pass (ORTH_LAGGED + kFinishLagged) and of the fused restart pass (k_vq_fused +
// kFinishFusedRestart) as the factorisation fills them: fac.hip (lanczos_step_lagged, mispec_fac_restart_sym) and the test hooks
// of lagged_hooks.hip (mispec_lagged_pass, mispec_fused_restart_pass) both go through these, so the two cannot drift.  Internal.
#pragma once
#include "krylov.hpp"

#include <cmath>

namespace mispec {

constexpr double kLaggedEps = 2.220446049250313e-16;  // TypeTraits<double>::epsilon()

// The pass of step i: `base` carries the basis, the row count and the partial records (fac.hip orth_args).  f is read (a.vi)
// and overwritten with the next residual (a.dst): the same buffer.
inline OrthArgs lagged_orth_args(OrthArgs base, const double* w, double* f, double* v, const double* c_in, const double* alpha_dev,
                                 StepState* st, bool onered)
{
    OrthArgs a = base;
    a.src = w;
    a.vi = f;
    a.dst = f;
    a.vout = v;
    a.c_in = c_in;
    a.alpha_dev = alpha_dev;
    a.beta_dev = &st->beta;
    a.pending = &st->lag_pending;
    a.status = &st->status;
    a.onered = onered ? 1 : 0;
    return a;
}

// The scalar tail of step i; n_global: the order of the operator (Lanczos.h:163: beta < eps sqrt(n))
inline FinishArgs lagged_finish_args(StepState* st, int i, int64_t n_global, double lag_limit, bool lag_last, int max_spec,
                                     const double* alpha_dev, const double* prev_red)
{
    FinishArgs fin;
    fin.st = st;
    fin.step = i;
    fin.eps = kLaggedEps;
    fin.beta_thresh = kLaggedEps * std::sqrt(double(n_global));
    fin.eps_sqrt = std::sqrt(kLaggedEps);
    fin.lag_limit = lag_limit;
    fin.lag_last = lag_last ? 1 : 0;
    fin.max_spec = max_spec;
    fin.mode = kFinishLagged;
    fin.alpha_src = alpha_dev;
    fin.prev_red = prev_red;
    return fin;
}

// One reduction per step: the product's partial sums of <f~, A f~> travel with the record
inline void lagged_onered_args(FinishArgs& fin, const double* alpha_parts, int64_t alpha_count, double* alpha_out)
{
    fin.alpha_parts = alpha_parts;
    fin.alpha_count = alpha_count;
    fin.alpha_out = alpha_out;
}

// The restart's V*Q pass with the pending correction of the last step riding on it (new subspace dimension k)
inline VqFusedArgs fused_restart_args(const double* c, const double* ftilde, double* fnew, double q_last, double h_sub, int k,
                                      double* partials, int64_t pstride)
{
    VqFusedArgs fa;
    fa.c = c;
    fa.ftilde = ftilde;
    fa.fnew = fnew;
    fa.q_last = q_last;
    fa.h_sub = h_sub;
    fa.kcol = k;
    fa.partials = partials;
    fa.pstride = pstride;
    return fa;
}

inline FinishArgs fused_restart_finish_args(StepState* st, int k, double eps)
{
    FinishArgs fin;
    fin.mode = kFinishFusedRestart;
    fin.st = st;
    fin.step = k;
    fin.eps = eps;
    return fin;
}

}  // namespace mispec
