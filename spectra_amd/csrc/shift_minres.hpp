// The iterative path of the shift-and-invert operators (shift_minres.hip): what a handle on ShiftPath::iterative owns.
#pragma once
#include "common.hpp"
#include "shiftsolve.hpp"

struct mispec_csr;

namespace mispec {

constexpr double kMinresTol = 4.0e-15;        // the backward error a solve is accepted at: kTarget of calibrate_refinement
constexpr double kMinresStagnation = 1.0e-13;  // ... and the one a stagnating solve is still accepted at
constexpr int kMinresMaxIterations = 20000;   // per solve, all passes together
constexpr int kMinresRestarts = 3;
constexpr int kMinresMaxCheck = 64;

// Scalars of the recurrences, in device memory; written by the one-thread tails of the two reductions, read by every kernel of an
// iteration.  No scalar of an iteration travels to the host: it reads this record every `check` iterations, for `done`.
struct MinresState
{
    int done;   // 0 iterating; 1 converged (the residual estimate reached `stop`, or an exact breakdown); 2 iteration cap; 3 not finite
    int iter;   // iterations completed in this pass
    int cap;    // iterations this pass may take
    int pad;
    double beta, oldb, s, c_r1, c_r2;  // beta_k, beta_{k-1}, 1 / beta_k, beta_k / beta_{k-1}, alpha_k / beta_k
    double alfa, dbar, epsln, phibar, cs, sn;
    double l_s, l_oldeps, l_delta, l_gamma, l_phi;  // of the last completed iteration: its w and x update runs one iteration late
    double beta1, stop;
};

struct ShiftMinres
{
    mispec_csr* A = nullptr;  // the full symmetric matrices, by the SpMV's own triangle ingest
    mispec_csr* B = nullptr;  // pencil only
    // caller's index order: diag A, diag B (ones without a pencil), row sums of |A| and |B|
    DevBuf<double> diagA, diagB, absA, absB;
    // per shift
    DevBuf<double> minv;  // Jacobi preconditioner 1 / |d_i|, positive
    double mnorm = 0.0;   // the bound max_i (sum_j |A_ij| + |sigma| sum_j |B_ij|) on |A - sigma B|_inf
    // work vectors, n + 2 doubles each, allocated at the first set_shift
    DevBuf<double> rb[2], z[2], w[2], p, q, sol, ycur, res;
    DevBuf<double> partials;  // one record per workgroup of a pass
    DevBuf<double> epi_partials;  // the product's epilogue records (its stop predicate rides on the epilogue)
    DevBuf<double> norms;     // 3: max |res|, |y|, |x|
    DevBuf<MinresState> state;
    PinnedBuf<MinresState> h_state;
    PinnedBuf<double> h_norms;
    int grid = 1;
    // settings (mispec_symshift_set_iterative) and counters (mispec_symshift_iterative_info)
    double tol = kMinresTol;
    int max_iterations = kMinresMaxIterations;
    int64_t last_iterations = 0, total_iterations = 0, solves = 0, probe_iterations = 0;
    int last_passes = 0;
    double last_backward_error = 0.0;
    ~ShiftMinres();
};

}  // namespace mispec
