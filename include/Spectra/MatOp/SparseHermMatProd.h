// y = A x for a complex Hermitian sparse A of which ONE triangle is given (reference: MatOp/SparseHermMatProd.h — the members of
// SparseSymMatProd, `mat.selfadjointView<Uplo>() * x`).  Same template signature as the reference; Scalar = double is the real
// symmetric operator (SparseSymMatProd).
//
// For std::complex<double> the `Uplo` triangle is mirrored conjugated into full int32 CSR in HBM at construction (mispec_zcsr,
// include/mispec_extras.h): entries of the other triangle are ignored, the diagonal's imaginary part is dropped, any StorageIndex is
// narrowed to int32 (rejected if it does not fit).  perform_op takes HOST pointers (a staged round trip); HermEigsSolver binds the
// device matrix directly and keeps every product in HBM.
#ifndef MISPEC_SPECTRA_SPARSE_HERM_MAT_PROD_H
#define MISPEC_SPECTRA_SPARSE_HERM_MAT_PROD_H

#include <complex>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../../mispec_extras.h"
#include "../internal/Dense.h"
#include "../internal/Device.h"
#include "SparseSymMatProd.h"

namespace Spectra {

template <typename Scalar_, int Uplo = Lower, int Flags = ColMajor, typename StorageIndex = int>
class SparseHermMatProd : public SparseSymMatProd<Scalar_, Uplo, Flags, StorageIndex>
{
public:
    using SparseSymMatProd<Scalar_, Uplo, Flags, StorageIndex>::SparseSymMatProd;
};

template <int Uplo, int Flags, typename StorageIndex>
class SparseHermMatProd<std::complex<double>, Uplo, Flags, StorageIndex>
{
public:
    using Scalar = std::complex<double>;

private:
    static_assert(Uplo == Lower || Uplo == Upper, "Uplo must be Lower or Upper");
    static_assert(std::is_integral<StorageIndex>::value, "StorageIndex must be an integer type");
    using Matrix = DenseMatrix<Scalar>;

    internal::CtxPtr m_ctx;
    std::shared_ptr<mispec_zcsr> m_mat;

    void ingest(const SparseView<Scalar, StorageIndex>& A)
    {
        if (A.rows != A.cols)
            throw std::invalid_argument("SparseHermMatProd: matrix must be square");
        if (A.row_major != (Flags == RowMajor))
            throw std::invalid_argument(
                "SparseHermMatProd: the \"Flags\" template parameter does not match the input matrix (ColMajor/RowMajor)");
        mispec_zcsr* raw = nullptr;
        const char uplo = Uplo == Lower ? 'L' : 'U';
        const double* values = reinterpret_cast<const double*>(A.values);
        if (std::is_signed<StorageIndex>::value && (sizeof(StorageIndex) == 4 || sizeof(StorageIndex) == 8))
            internal::check(mispec_zcsr_upload(m_ctx.get(), A.rows, A.cols, A.outer, A.inner, int(sizeof(StorageIndex)), values,
                                               A.row_major ? 1 : 0, uplo, &raw));
        else
        {
            // other widths: widened to int64 here, narrowed to int32 by the library
            const std::size_t outer_len = static_cast<std::size_t>(A.rows) + 1;
            const std::size_t nnz = A.rows ? static_cast<std::size_t>(A.outer[A.rows]) : 0;
            std::vector<std::int64_t> outer(A.outer, A.outer + outer_len), inner(A.inner, A.inner + nnz);
            internal::check(mispec_zcsr_upload(m_ctx.get(), A.rows, A.cols, outer.data(), inner.data(), 8, values, A.row_major ? 1 : 0,
                                               uplo, &raw));
        }
        m_mat = std::shared_ptr<mispec_zcsr>(raw, [](mispec_zcsr* p) { (void) mispec_zcsr_destroy(p); });
    }

public:
    // From a compressed sparse matrix in host memory.
    explicit SparseHermMatProd(const SparseView<Scalar, StorageIndex>& mat, internal::CtxPtr ctx = internal::CtxPtr()) :
        m_ctx(ctx ? ctx : internal::default_context())
    {
        ingest(mat);
    }

#ifdef MISPEC_HAVE_EIGEN
    // The reference's constructor: any Eigen sparse expression of matching storage order.
    template <typename Derived>
    SparseHermMatProd(const Eigen::SparseMatrixBase<Derived>& mat) : m_ctx(internal::default_context())
    {
        using Plain = Eigen::SparseMatrix<Scalar, Flags, StorageIndex>;
        static_assert(static_cast<int>(Derived::PlainObject::IsRowMajor) == static_cast<int>(Plain::IsRowMajor),
                      "SparseHermMatProd: the \"Flags\" template parameter does not match the input matrix");
        Plain tmp(mat);
        tmp.makeCompressed();
        SparseView<Scalar, StorageIndex> v;
        v.rows = tmp.rows();
        v.cols = tmp.cols();
        v.outer = tmp.outerIndexPtr();
        v.inner = tmp.innerIndexPtr();
        v.values = tmp.valuePtr();
        v.row_major = Plain::IsRowMajor;
        ingest(v);
    }
#endif

    Index rows() const { return static_cast<Index>(mispec_zcsr_rows(m_mat.get())); }
    Index cols() const { return static_cast<Index>(mispec_zcsr_cols(m_mat.get())); }

    // y_out = A * x_in, host pointers (the reference's contract)
    void perform_op(const Scalar* x_in, Scalar* y_out) const
    {
        internal::check(mispec_zcsr_spmv_host(m_mat.get(), reinterpret_cast<const double*>(x_in), reinterpret_cast<double*>(y_out)));
    }
    // Y = A * X, column by column
    Matrix operator*(const Matrix& mat_in) const
    {
        Matrix res(rows(), mat_in.cols());
        for (Index j = 0; j < mat_in.cols(); j++)
            perform_op(mat_in.data() + j * mat_in.rows(), res.data() + j * res.rows());
        return res;
    }
    // A(i, j) of the Hermitian operator (both triangles answer: the mirror is what is stored)
    Scalar operator()(Index i, Index j) const
    {
        double v[2] = {0.0, 0.0};
        internal::check(mispec_zcsr_coeff(m_mat.get(), i, j, v));
        return Scalar(v[0], v[1]);
    }

    // Device binding used by HermEigsSolver.
    mispec_ctx* mispec_context() const { return m_ctx.get(); }
    const mispec_zcsr* mispec_zcsr_matrix() const { return m_mat.get(); }
};

}  // namespace Spectra

#endif
