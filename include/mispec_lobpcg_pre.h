/* Additions to the LOBPCG solver of mispec_extras.h that tie it to another component of the library.  The solver's own entry
 * points (mispec_extras.h, mispec_lobpcg_*) are a closed list that tests/test_host_lobpcg.py pins; what joins the solver to the
 * shift-and-invert operator of mispec.h is declared here.  Defined in libmispec_extras.so (csrc/lobpcg.hip). */
#ifndef MISPEC_LOBPCG_PRE_H
#define MISPEC_LOBPCG_PRE_H

#include "mispec_extras.h"

#ifdef __cplusplus
extern "C" {
#endif

/* T = (K - sigma M)^{-1} held as a factorisation: the shift-and-invert operator F of a matrix near A (its near diagonals, say),
 * applied to the active columns by mispec_symshift_solve_block — one pass over the factor per panel of columns.  NULL removes it;
 * it replaces a matrix or Jacobi preconditioner and is replaced by either.  F is not owned and must outlive the solves.
 * MISPEC_EINVAL when F belongs to another context, has another size, is a general (non-symmetric) operator, or is banded and its
 * last factorisation met negative pivots (T must be positive definite).  On the dense path (n <= 4096) the library cannot see
 * definiteness: that F is positive definite is then the caller's duty.  The shift of F may be set again between two compute()
 * calls; compute() returns MISPEC_ELOGIC while F has not been factored, MISPEC_EINVAL when the new shift made it indefinite. */
int mispec_lobpcg_set_preconditioner_solver(mispec_lobpcg* S, const mispec_symshift* F);

#ifdef __cplusplus
}
#endif

#endif
