// The iterative path of the shift-and-invert operators (shift_minres.hip): what a handle on ShiftPath::iterative owns.
#pragma once
#include "shift_iterative_state.hpp"

namespace mispec {

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

struct ShiftMinres : ShiftIterative
{
    mispec_csr* B = nullptr;  // pencil only (A and B: the full symmetric matrices, by the SpMV's own triangle ingest)
    DevBuf<double> diagB, absB;  // caller's index order: diag B and the row sums of |B| (ones without a pencil)
    // work vectors besides ShiftIterative's, n + 2 doubles each, allocated at the first set_shift
    DevBuf<double> rb[2], z[2], w[2], q, sol;
    DevBuf<MinresState> state;
    PinnedBuf<MinresState> h_state;
    ~ShiftMinres();
};

}  // namespace mispec
