// y = Re((A - sigma I)^{-1} x) for a general real sparse A and a complex shift sigma = sigmar + i sigmai — the operator of
// GenEigsComplexShiftSolver.  Same members as the reference class (MatOp/SparseGenComplexShiftSolve.h:35-113: rows(),
// cols(), set_shift(sigmar, sigmai), perform_op()), which factors a complex Eigen::SparseLU; here the dense device path
// of SparseGenRealShiftSolve is used with the real part of the complex inverse (n <= 4096), which is what ShiftSolver::Direct, the
// default, constructs whatever option shift_solver says.  ShiftSolver::Auto (the dense path up to n = 4096, the iterative path
// beyond) and ShiftSolver::Iterative (that path at every n) construct the operator with mispec_symshift_create_general_complex:
// on its iterative path a complex shift is solved by Jacobi-preconditioned BiCGStab in complex arithmetic
// (csrc/shift_zbicgstab.hip) and a real one — GenEigsComplexShiftSolver's probe shift — by the real method, every solve to a
// backward error of 4e-15; set_shift() refuses a shift whose probe solve does not converge.  An adopted handle of
// mispec_symshift_create_general_solver on the iterative path takes real shifts only: set_shift(sigmar, sigmai != 0) throws
// std::invalid_argument on it.
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

    // option shift_solver is not read: ShiftSolver::Default counts as Direct, the dense path
    explicit SparseGenComplexShiftSolve(const SparseView<Scalar, StorageIndex>& mat, internal::CtxPtr ctx = internal::CtxPtr(),
                                        ShiftSolver solver = ShiftSolver::Direct) :
        Base(mat, ctx, kind(solver), creator(solver))
    {}
#ifdef MISPEC_HAVE_EIGEN
    template <typename Derived>
    SparseGenComplexShiftSolve(const Eigen::SparseMatrixBase<Derived>& mat, ShiftSolver solver = ShiftSolver::Direct) :
        Base(mat, kind(solver), creator(solver))
    {}
#endif
    // adopt a solver created through the C ABI (not owned); one on the iterative path is refused by set_shift
    SparseGenComplexShiftSolve(mispec_ctx* ctx, mispec_symshift* solver) : Base(ctx, solver) {}

private:
    static bool direct(ShiftSolver s) { return s == ShiftSolver::Direct || s == ShiftSolver::Default; }
    static ShiftSolver kind(ShiftSolver s) { return direct(s) ? ShiftSolver::Direct : s; }
    static typename Base::Creator creator(ShiftSolver s)
    {
        return direct(s) ? &mispec_symshift_create_general_solver : &mispec_symshift_create_general_complex;
    }

public:
    // Factor A - (sigmar + i sigmai) I; throws std::invalid_argument if that fails (reference :96-98)
    void set_shift(const Scalar& sigmar, const Scalar& sigmai)
    {
        internal::check(mispec_symshift_set_shift_complex(const_cast<mispec_symshift*>(this->mispec_solver()), sigmar, sigmai));
    }
};

}  // namespace Spectra

#endif
