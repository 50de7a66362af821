// The part of a handle on ShiftPath::iterative that does not depend on its Krylov method (shift_minres.hip: MINRES for symmetric
// operators and pencils; shift_bicgstab.hip: BiCGStab for general ones), and the constants of the acceptance rule both follow.
#pragma once
#include "common.hpp"
#include "shiftsolve.hpp"

namespace mispec {

constexpr double kMinresTol = 4.0e-15;        // the backward error a solve is accepted at: kTarget of calibrate_refinement
constexpr double kMinresStagnation = 1.0e-13;  // ... and the one a stagnating solve is still accepted at
constexpr int kMinresMaxIterations = 20000;   // per solve, all passes together
constexpr int kMinresRestarts = 3;
constexpr int kMinresMaxCheck = 64;

struct ShiftIterative
{
    mispec_csr* A = nullptr;  // the full matrix, by the SpMV's own ingest
    // caller's index order: diag A and the row sums of |A|
    DevBuf<double> diagA, absA;
    // per shift
    DevBuf<double> minv;  // Jacobi preconditioner: 1 / |d_i| (MINRES, positive) or 1 / d_i (BiCGStab, signed)
    double mnorm = 0.0;   // the bound max_i (sum_j |A_ij| + |sigma| sum_j |B_ij|) on |A - sigma B|_inf
    // work vectors both methods have, n + 2 doubles each, allocated at the first set_shift: a product, the solution so far (the
    // residual's product reads it), the explicit residual
    DevBuf<double> p, ycur, res;
    DevBuf<double> partials;      // one record per workgroup of a pass and slot
    DevBuf<double> epi_partials;  // the product's epilogue records (its stop predicate rides on the epilogue)
    DevBuf<double> norms;         // 3: max |res|, |y|, |x|
    PinnedBuf<double> h_norms;
    int grid = 1;
    // settings (mispec_symshift_set_iterative) and counters (mispec_symshift_iterative_info)
    double tol = kMinresTol;
    int max_iterations = kMinresMaxIterations;
    int64_t last_iterations = 0, total_iterations = 0, solves = 0, probe_iterations = 0;
    int last_passes = 0;
    double last_backward_error = 0.0;
    ~ShiftIterative()
    {
        if (A)
            (void) mispec_csr_destroy(A);
    }
};

}  // namespace mispec
