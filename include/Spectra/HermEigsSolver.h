// Eigen solver for Hermitian matrices (reference: HermEigsSolver.h): the k largest / smallest eigenvalues of A given through an
// operator object, by the implicitly restarted Lanczos method on the GPU.
//
//     DenseHermMatProd<std::complex<double>> op(A);       // or SparseHermMatProd<std::complex<double>>, or any OpType
//     HermEigsSolver<DenseHermMatProd<std::complex<double>>> eigs(op, nev, ncv);
//     eigs.init();
//     int nconv = eigs.compute(SortRule::LargestAlge);
//     if (eigs.info() == CompInfo::Successful) { auto evalues = eigs.eigenvalues(); auto evecs = eigs.eigenvectors(); }
//
// A real Scalar (the default, DenseHermMatProd<double>) is the real symmetric solver, HermEigsBase unchanged.  For
// std::complex<double> the driver is internal/ComplexHermEigs.h: eigenvalues() is a real vector, eigenvectors() a complex n x nvec
// matrix.  (The second template parameter only selects the driver; leave it at its default.)
#ifndef MISPEC_SPECTRA_HERM_EIGS_SOLVER_H
#define MISPEC_SPECTRA_HERM_EIGS_SOLVER_H

#include <complex>
#include <type_traits>

#include "HermEigsBase.h"
#include "MatOp/DenseHermMatProd.h"
#include "Util/SelectionRule.h"
#include "internal/ComplexHermEigs.h"

namespace Spectra {

template <typename OpType = DenseHermMatProd<double>,
          bool IsComplex = std::is_same<typename OpType::Scalar, std::complex<double>>::value>
class HermEigsSolver : public HermEigsBase<OpType, IdentityBOp>
{
public:
    HermEigsSolver(OpType& op, Index nev, Index ncv) : HermEigsBase<OpType, IdentityBOp>(op, IdentityBOp(), nev, ncv) {}
};

template <typename OpType>
class HermEigsSolver<OpType, true> : public internal::ComplexHermEigs<OpType>
{
public:
    // op: the matrix operator; nev: number of eigenvalues wanted, 1 <= nev <= n-1;
    // ncv: Krylov dimension, nev < ncv <= n (ncv >= 2 nev advised).  Throws std::invalid_argument otherwise.
    HermEigsSolver(OpType& op, Index nev, Index ncv) : internal::ComplexHermEigs<OpType>(op, nev, ncv) {}
};

}  // namespace Spectra

#endif
