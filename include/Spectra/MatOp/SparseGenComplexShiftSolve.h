// y = Re((A - sigma I)^{-1} x) for a general real sparse A and a complex shift sigma = sigmar + i sigmai — the operator of
// GenEigsComplexShiftSolver.  Same members as the reference class (MatOp/SparseGenComplexShiftSolve.h:35-113: rows(),
// cols(), set_shift(sigmar, sigmai), perform_op()), which factors a complex Eigen::SparseLU; here the dense device path
// of SparseGenRealShiftSolve is used with the real part of the complex inverse (n <= 4096).  The iterative path takes real shifts
// only, so this class constructs its operator with ShiftSolver::Direct whatever option shift_solver says; an adopted handle that is
// on the iterative path makes set_shift(sigmar, sigmai != 0) throw std::invalid_argument.
#ifndef MISPEC_SPECTRA_SPARSE_GEN_COMPLEX_SHIFT_SOLVE_H
#define MISPEC_SPECTRA_SPARSE_GEN_COMPLEX_SHIFT_SOLVE_H

#include "../../mispec_extras.h"  // outside the hot path of SURVEY.md section 8: declared apart from the thin shim
#include "SparseGenRealShiftSolve.h"

namespace Spectra {

template <typename Scalar_, int Flags = ColMajor, typename StorageIndex = int>
class SparseGenComplexShiftSolve : public SparseGenRealShiftSolve<Scalar_, Flags, StorageIndex>
{
    using Base = SparseGenRealShiftSolve<Scalar_, Flags, StorageIndex>;

public:
    using Scalar = Scalar_;

    // always the dense path (ShiftSolver::Direct): option shift_solver is not read, and there is no solver argument
    explicit SparseGenComplexShiftSolve(const SparseView<Scalar, StorageIndex>& mat, internal::CtxPtr ctx = internal::CtxPtr()) :
        Base(mat, ctx, ShiftSolver::Direct)
    {}
#ifdef MISPEC_HAVE_EIGEN
    template <typename Derived>
    SparseGenComplexShiftSolve(const Eigen::SparseMatrixBase<Derived>& mat) : Base(mat, ShiftSolver::Direct)
    {}
#endif
    // adopt a solver created through the C ABI (not owned); one on the iterative path is refused by set_shift
    SparseGenComplexShiftSolve(mispec_ctx* ctx, mispec_symshift* solver) : Base(ctx, solver) {}

    // Factor A - (sigmar + i sigmai) I; throws std::invalid_argument if that fails (reference :96-98)
    void set_shift(const Scalar& sigmar, const Scalar& sigmai)
    {
        internal::check(mispec_symshift_set_shift_complex(const_cast<mispec_symshift*>(this->mispec_solver()), sigmar, sigmai));
    }
};

}  // namespace Spectra

#endif
