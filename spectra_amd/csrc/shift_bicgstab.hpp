// The iterative path of the general (non-symmetric) shift-and-invert operator (shift_bicgstab.hip): what such a handle owns.
#pragma once
#include "shift_iterative_state.hpp"

namespace mispec {

// Scalars of the recurrence, in device memory; written by the one-thread tails of the three reductions, read by every kernel of an
// iteration.  No scalar of an iteration travels to the host: it reads this record every `check` iterations, for `done`.
struct BicgstabState
{
    int done;  // 0 iterating; 1 converged (|r| reached `stop`); 2 iteration cap; 3 not finite; 4 breakdown (rho, <rhat, v> or omega zero)
    int iter;  // iterations completed in this pass
    int cap;   // iterations this pass may take
    int pad;
    double rho, alpha, omega, beta;  // <rhat, r>, rho / <rhat, v>, <t, s> / <t, t>, (rho' / rho)(alpha / omega)
    double rnorm;                    // |r|_2 of the recurrence after the last completed iteration
    double rhs_norm, stop;           // |rhs|_2 of this pass and the value of |r|_2 it ends at
};

struct ShiftBicgstab : ShiftIterative
{
    // work vectors besides ShiftIterative's, n + 2 doubles each, allocated at the first set_shift: r (s in its place between the
    // two products), rhat, the direction d (the p of the usual listings) and minv .* d, v, minv .* s, t, the pass's solution
    DevBuf<double> rs, rhat, d, dhat, v, shat, t, sol;
    DevBuf<BicgstabState> state;
    PinnedBuf<BicgstabState> h_state;
};

}  // namespace mispec
