// Complex shifts on the iterative path of the general shift-and-invert operator (shift_zbicgstab.hip): what a handle of
// mispec_symshift_create_general_complex owns besides its ShiftBicgstab, whose operator, diagonal, row sums, reduction records,
// settings and counters both methods use.
#pragma once
#include "shift_bicgstab.hpp"

namespace mispec {

// BicgstabState with complex scalars (re, im); the same writers and readers
struct ZBicgstabState
{
    int done;  // 0 iterating; 1 converged; 2 iteration cap; 3 not finite; 4 breakdown — BicgstabState's values
    int iter;  // iterations completed in this pass
    int cap;   // iterations this pass may take
    int pad;
    double rho[2], alpha[2], omega[2], beta[2];  // <rhat, r>, rho / <rhat, v>, <t, s> / <t, t>, (rho' / rho)(alpha / omega)
    double rnorm;                                // |r|_2 of the recurrence after the last completed iteration
    double rhs_norm, stop;                       // |rhs|_2 of this pass and the value of |r|_2 it ends at
};

// a complex vector: two planes (re, im) of n + 2 doubles each, every plane laid out and aligned as a real work vector — and so
// directly an operand of the real SpMV
struct ZVec
{
    DevBuf<double> re, im;
    void alloc(size_t np)
    {
        re.alloc(np);
        im.alloc(np);
    }
};

struct ShiftZBicgstab
{
    // allocated at the first complex set_shift: the preconditioner 1 / (diag A - sigma), the vectors of ShiftBicgstab, and the
    // three of ShiftIterative (a product, the solution so far, the explicit residual)
    ZVec minv, rs, rhat, d, dhat, v, shat, t, sol, p, ycur, res;
    DevBuf<ZBicgstabState> state;
    PinnedBuf<ZBicgstabState> h_state;
};

}  // namespace mispec
