// LOBPCG (locally optimal block preconditioned conjugate gradient) eigen solver for the smallest eigenpairs of a sparse SPD pencil
// A x = lambda B x, with an optional preconditioner and optional constraints.  Same member names and defaults as the reference class
// (contrib/LOBPCGSolver.h:291-546): constructor (A, X), setConstraints(Y), setB(B), setPreconditioner(T), compute(maxit = 10,
// tol_div_n = 1e-7) with the threshold tol_div_n * n (LOBPCGSolver.h:330), eigenvalues(), eigenvectors(), residuals(), info()
// (0 Success, 1 NumericalIssue, 2 NoConvergence, 3 InvalidInput before compute()).  Additions: setJacobiPreconditioner() (1 / diag A),
// num_iterations(), and a constructor from an existing SparseSymMatProd.
//
// The blocks [X | R | P], their images under A and B and the constraints live in HBM; this class is a thin owner of a mispec_lobpcg
// handle (csrc/lobpcg.hip, control flow csrc/lobpcg_flow.hpp) and of the device matrices.  Limits: 1 <= X.cols() <= 21, X.cols() < n,
// at most 21 constraint vectors.
//
// Deviations from the reference, on purpose:
//   * eigenvectors() returns the n x m Ritz vectors (B-orthonormal).  The reference returns m_evectors, the 3m x m COEFFICIENT matrix of
//     its last Rayleigh-Ritz step (LOBPCGSolver.h:464, 536), which are not eigenvectors of A: a defect that is not reproduced.
//   * X, Y are dense blocks; the reference stores them as sparse matrices.
//   * a Rayleigh-Ritz step whose Gram matrix cannot be factored is retried once without the block P and then reported as
//     NumericalIssue (1); the reference maps it to NoConvergence.  The eigenpairs of the last completed iteration stay available; if the
//     failure is in the setup (linearly dependent start vectors) no iteration was completed, and eigenvalues() holds the Rayleigh
//     quotients of the start vectors.
//   * Gram matrices are factored by a Cholesky that refuses pivots below 1e-8 (an angle of 1e-4 between a column and the ones before
//     it).  A threshold that cannot be reached — a start block that holds an exact eigenvector and a tol below the rounding level of
//     its residual — therefore ends in NumericalIssue, with that pair returned to rounding, rather than in NoConvergence.
// Further: there is ONE product with A per iteration, on the unconverged columns (A P is carried along, not recomputed), and the Gram
// matrices of the Rayleigh-Ritz step are computed in full instead of assuming identity / diag(lambda) blocks.
#ifndef MISPEC_SPECTRA_LOBPCG_SOLVER_H
#define MISPEC_SPECTRA_LOBPCG_SOLVER_H

#include "../../mispec_extras.h"  // outside the hot path: declared apart from the thin shim
#include "../../mispec_lobpcg_pre.h"  // the solver preconditioner (ties the solver to the shift-and-invert operator)
#include <memory>
#include <stdexcept>
#include <type_traits>

#include "../MatOp/SparseSymMatProd.h"
#include "../MatOp/SparseSymShiftSolve.h"
#include "../MatOp/SymShiftInvert.h"
#include "../Util/SelectionRule.h"
#include "../internal/Dense.h"
#include "../internal/Device.h"

namespace Spectra {

template <typename Scalar = double>
class LOBPCGSolver
{
    static_assert(std::is_same<Scalar, double>::value, "the MI355X path computes in fp64: Scalar must be double");

public:
    using Operator = SparseSymMatProd<Scalar>;
    using Matrix = DenseMatrix<Scalar>;
    using Vector = DenseVector<Scalar>;

private:
    Operator m_A;
    std::shared_ptr<Operator> m_B, m_T;
    const Index m_n, m_nev;
    std::shared_ptr<mispec_lobpcg> m_solver;
    std::shared_ptr<const void> m_F;  // a shared copy of the solver given as the preconditioner

    template <typename Solver>
    void set_solver(const Solver& F)
    {
        if (F.rows() != m_n || F.cols() != m_n)
            throw std::invalid_argument("Wrong size");
        auto keep = std::make_shared<Solver>(F);
        internal::check(mispec_lobpcg_set_preconditioner_solver(m_solver.get(), keep->mispec_solver()));
        m_F = keep;
        m_T.reset();
    }

    void bind(const Matrix& X)
    {
        if (X.rows() != m_n)
            throw std::invalid_argument("Wrong size");  // LOBPCGSolver.h:301-302
        mispec_lobpcg* raw = nullptr;
        internal::check(mispec_lobpcg_create(m_A.mispec_context(), m_A.mispec_matrix(), m_nev, &raw));
        m_solver = std::shared_ptr<mispec_lobpcg>(raw, [](mispec_lobpcg* p) { (void) mispec_lobpcg_destroy(p); });
        internal::check(mispec_lobpcg_set_initial(raw, X.data(), X.rows()));
    }
    void check_shape(const Operator& M) const
    {
        if (M.rows() != m_n || M.cols() != m_n)
            throw std::invalid_argument("Wrong size");  // LOBPCGSolver.h:316-317
    }

public:
    // A: anything a SparseSymMatProd<Scalar> is constructed from (a SparseView of one triangle or the full symmetric matrix; with
    // Eigen, a sparse matrix); X: the n x m start block
    template <typename SparseArg>
    LOBPCGSolver(const SparseArg& A, const Matrix& X) : m_A(A), m_n(m_A.rows()), m_nev(X.cols())
    {
        bind(X);
    }
    // an operator that already lives on the device (shared, not copied)
    LOBPCGSolver(const Operator& A, const Matrix& X) : m_A(A), m_n(m_A.rows()), m_nev(X.cols()) { bind(X); }

    void setConstraints(const Matrix& Y)
    {
        if (Y.rows() != m_n)
            throw std::invalid_argument("Wrong size");
        internal::check(mispec_lobpcg_set_constraints(m_solver.get(), Y.data(), Y.rows(), Y.cols()));
    }

    void setB(const Operator& B)
    {
        check_shape(B);
        m_B = std::make_shared<Operator>(B);
        internal::check(mispec_lobpcg_set_B(m_solver.get(), m_B->mispec_matrix()));
    }
    template <typename SparseArg>
    void setB(const SparseArg& B)
    {
        setB(Operator(B));
    }

    // R <- T R every iteration
    void setPreconditioner(const Operator& T)
    {
        check_shape(T);
        m_T = std::make_shared<Operator>(T);
        internal::check(mispec_lobpcg_set_preconditioner(m_solver.get(), m_T->mispec_matrix()));
    }
    template <typename SparseArg>
    void setPreconditioner(const SparseArg& T)
    {
        setPreconditioner(Operator(T));
    }
    // R <- (K - sigma M)^{-1} R with the factorisation held by a shift-and-invert operator of a matrix near A (set_shift() before
    // compute(); positive definite), applied as one block solve per iteration.  A shared copy keeps the solver alive.
    template <int Uplo, int Flags, typename StorageIndex>
    void setPreconditioner(const SparseSymShiftSolve<Scalar, Uplo, Flags, StorageIndex>& F)
    {
        set_solver(F);
    }
    template <int UploA, int UploB, int FlagsA, int FlagsB, typename IndexA, typename IndexB>
    void setPreconditioner(const SymShiftInvert<Scalar, Sparse, Sparse, UploA, UploB, FlagsA, FlagsB, IndexA, IndexB>& F)
    {
        set_solver(F);
    }
    // R <- diag(A)^-1 R, fused into the residual kernel; needs a positive diagonal
    void setJacobiPreconditioner() { internal::check(mispec_lobpcg_set_jacobi(m_solver.get(), 1)); }

    void compute(int maxit = 10, Scalar tol_div_n = 1e-7)
    {
        int64_t nconv = 0;
        internal::check(mispec_lobpcg_compute(m_solver.get(), static_cast<int>(SortRule::SmallestAlge), maxit, tol_div_n * Scalar(m_n), &nconv));
    }

    Vector eigenvalues() const
    {
        Vector res(m_nev);
        internal::check(mispec_lobpcg_eigenvalues(m_solver.get(), res.data()));
        return res;
    }
    Matrix eigenvectors() const
    {
        Matrix res(m_n, m_nev);
        internal::check(mispec_lobpcg_eigenvectors(m_solver.get(), res.data(), m_n));
        return res;
    }
    Matrix residuals() const
    {
        Matrix res(m_n, m_nev);
        internal::check(mispec_lobpcg_residuals(m_solver.get(), res.data(), m_n));
        return res;
    }
    int info() const { return mispec_lobpcg_info(m_solver.get()); }
    Index num_iterations() const { return static_cast<Index>(mispec_lobpcg_num_iterations(m_solver.get())); }
};

}  // namespace Spectra

#endif
