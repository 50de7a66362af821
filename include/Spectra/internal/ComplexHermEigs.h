// The implicitly restarted Lanczos driver for COMPLEX Hermitian problems: what HermEigsSolver<OpType> is when OpType::Scalar is
// std::complex<double> (reference: HermEigsBase.h:44-478 instantiated over DenseHermMatProd<complex> / SparseHermMatProd<complex>).
//
// The complex factorisation (mispec_zfac, include/mispec_extras.h: the three-term flow of Lanczos.h with V, f and the operator in
// HBM) does the n-sized work; H is m x m and its real part is all the restart needs (reference :105-155, :205-224: TridiagQR /
// TridiagEigen<RealScalar> on matrix_H().real()), so the m x m work runs here on the host with the arithmetic of
// internal/SmallDense.h.  The contract follows the reference: constructor checks and ncv clamp (:257-272), init() with
// SimpleRandom<complex>(0) and init(v0), compute(selection, maxit, tol, sorting) with the five symmetric rules, the convergence test
// (:158-175), ARPACK's nev adjustment (:178-202), exact shifts sorted by decreasing magnitude, eigenvalues() real and
// eigenvectors([nvec]) complex n x nvec.
//
// The operator: a DenseHermMatProd<complex> / SparseHermMatProd<complex> (their device matrices are bound directly), or any class
// with the reference's OpType concept (rows(), perform_op(const Scalar*, Scalar*) on host pointers), applied through a callback.
#ifndef MISPEC_SPECTRA_COMPLEX_HERM_EIGS_H
#define MISPEC_SPECTRA_COMPLEX_HERM_EIGS_H

#include <algorithm>
#include <cmath>
#include <complex>
#include <memory>
#include <stdexcept>
#include <type_traits>
#include <vector>

#include "../../mispec_extras.h"
#include "../Util/CompInfo.h"
#include "../Util/SelectionRule.h"
#include "../Util/SimpleRandom.h"
#include "../Util/TypeTraits.h"
#include "Dense.h"
#include "Device.h"
#include "SmallDense.h"

namespace Spectra {
namespace internal {

// Which device matrix an operator carries (detected by member function)
template <typename T, typename = void>
struct has_zcsr : std::false_type
{};
template <typename T>
struct has_zcsr<T, decltype((void) std::declval<const T&>().mispec_zcsr_matrix())> : std::true_type
{};
template <typename T, typename = void>
struct has_zdense : std::false_type
{};
template <typename T>
struct has_zdense<T, decltype((void) std::declval<const T&>().mispec_zdense_matrix())> : std::true_type
{};

template <typename OpType>
class ComplexHermEigs
{
public:
    using Scalar = std::complex<double>;
    using RealScalar = double;

private:
    using Matrix = DenseMatrix<Scalar>;
    using RealVector = DenseVector<RealScalar>;

    const OpType& m_op;
    const Index m_n;
    const Index m_nev;
    const Index m_ncv;
    Index m_nmatop = 0;
    Index m_niter = 0;
    CtxPtr m_ctx;
    std::shared_ptr<mispec_zfac> m_fac;
    std::vector<double> m_ritz_val;   // ncv Ritz values, wanted ones first
    std::vector<double> m_ritz_vec;   // ncv x nev, column-major
    std::vector<double> m_ritz_est;   // last row of the eigenvectors of Re(H)
    std::vector<char> m_ritz_conv;
    CompInfo m_info = CompInfo::NotComputed;

    // the widest basis the restart's V Q kernel takes (csrc/zfac.hip kMaxVqCols: one row of ncv complex columns in 64 KiB of LDS)
    static constexpr Index kMaxNcv = 4096;

    static Index check_args(Index n, Index nev, Index ncv)
    {
        if (nev < 1 || nev > n - 1)
            throw std::invalid_argument("nev must satisfy 1 <= nev <= n - 1, n is the size of matrix");
        if (ncv <= nev || ncv > n)
            throw std::invalid_argument("ncv must satisfy nev < ncv <= n, n is the size of matrix");
        if (ncv > kMaxNcv)
            throw std::invalid_argument("ncv must not exceed 4096 for complex Hermitian matrices");
        return ncv > n ? n : ncv;
    }

    static int call_op(void* user, const double* x, double* y)
    {
        try
        {
            static_cast<const OpType*>(user)->perform_op(reinterpret_cast<const Scalar*>(x), reinterpret_cast<Scalar*>(y));
            return 0;
        }
        catch (...)
        {
            return 1;
        }
    }

    template <typename O>
    static CtxPtr context_of(const O& op, std::true_type)
    {
        return borrow_context(op.mispec_context());
    }
    template <typename O>
    static CtxPtr context_of(const O&, std::false_type)
    {
        return default_context();
    }

    // the factorisation over the operator's device matrix, or over the host callback
    mispec_zfac* create_fac()
    {
        mispec_zfac* raw = nullptr;
        const int ncv = static_cast<int>(m_ncv);
        create_fac_impl(raw, ncv, has_zcsr<OpType>(), has_zdense<OpType>());
        return raw;
    }
    void create_fac_impl(mispec_zfac*& raw, int ncv, std::true_type, std::false_type)
    {
        check(mispec_zfac_create_csr(m_ctx.get(), m_op.mispec_zcsr_matrix(), ncv, 1, &raw));
    }
    void create_fac_impl(mispec_zfac*& raw, int ncv, std::false_type, std::true_type)
    {
        check(mispec_zfac_create_dense(m_ctx.get(), m_op.mispec_zdense_matrix(), ncv, 1, &raw));
    }
    void create_fac_impl(mispec_zfac*& raw, int ncv, std::false_type, std::false_type)
    {
        check(mispec_zfac_create_op(m_ctx.get(), &ComplexHermEigs::call_op, const_cast<OpType*>(&m_op), m_n, ncv, 1, &raw));
    }

    std::vector<Scalar> matrix_H() const
    {
        std::vector<Scalar> H(static_cast<std::size_t>(m_ncv * m_ncv));
        check(mispec_zfac_get_H(m_fac.get(), reinterpret_cast<double*>(H.data())));
        return H;
    }
    double f_norm() const
    {
        double b = 0.0;
        check(mispec_zfac_f_norm(m_fac.get(), &b));
        return b;
    }

    // diagonal and sub-diagonal of Re(H) (TridiagQR / TridiagEigen read nothing else)
    void real_tridiagonal(const std::vector<Scalar>& H, std::vector<double>& diag, std::vector<double>& subd) const
    {
        const std::size_t m = static_cast<std::size_t>(m_ncv);
        diag.assign(m, 0.0);
        subd.assign(m > 1 ? m - 1 : 1, 0.0);
        for (std::size_t i = 0; i < m; i++)
            diag[i] = H[i * m + i].real();
        for (std::size_t i = 0; i + 1 < m; i++)
            subd[i] = H[i * m + i + 1].real();
    }

    // Ritz pairs of Re(H), wanted ones first (reference :205-224)
    void retrieve_ritzpair(SortRule selection)
    {
        const int m = static_cast<int>(m_ncv);
        std::vector<double> evals, subd, evecs(static_cast<std::size_t>(m) * m, 0.0);
        real_tridiagonal(matrix_H(), evals, subd);
        for (int i = 0; i < m; i++)
            evecs[static_cast<std::size_t>(i) * m + i] = 1.0;
        if (mispec::small::tridiag_eigen(m, evals.data(), subd.data(), evecs.data(), m, mispec::small::Lanes{0, 1}) != 0)
            throw std::runtime_error("TridiagEigen: eigen decomposition failed");
        const std::vector<Index> ind = argsort(selection, evals.data(), m_ncv);
        for (Index i = 0; i < m_ncv; i++)
        {
            m_ritz_val[std::size_t(i)] = evals[std::size_t(ind[std::size_t(i)])];
            m_ritz_est[std::size_t(i)] = evecs[std::size_t(ind[std::size_t(i)]) * m + (m - 1)];
        }
        for (Index i = 0; i < m_nev; i++)
            for (Index r = 0; r < m_ncv; r++)
                m_ritz_vec[std::size_t(i * m_ncv + r)] = evecs[std::size_t(ind[std::size_t(i)]) * m + std::size_t(r)];
    }

    // |last component| * |f| < tol * max(eps^(2/3), |theta|)  (reference :158-175)
    Index num_converged(RealScalar tol)
    {
        const RealScalar eps23 = std::pow(TypeTraits<RealScalar>::epsilon(), RealScalar(2) / 3);
        const RealScalar fnorm = f_norm();
        Index count = 0;
        for (Index i = 0; i < m_nev; i++)
        {
            const RealScalar thresh = tol * (std::max)(eps23, std::abs(m_ritz_val[std::size_t(i)]));
            const RealScalar resid = std::abs(m_ritz_est[std::size_t(i)]) * fnorm;
            m_ritz_conv[std::size_t(i)] = (resid < thresh) ? 1 : 0;
            count += m_ritz_conv[std::size_t(i)];
        }
        return count;
    }

    // ARPACK's dsaup2 heuristic (reference :178-202)
    Index nev_adjusted(Index nconv)
    {
        const RealScalar near_0 = TypeTraits<RealScalar>::min() * RealScalar(10);
        Index nev_new = m_nev;
        for (Index i = m_nev; i < m_ncv; i++)
            if (std::abs(m_ritz_est[std::size_t(i)]) < near_0)
                nev_new++;
        nev_new += (std::min)(nconv, (m_ncv - nev_new) / 2);
        if (nev_new == 1 && m_ncv >= 6)
            nev_new = m_ncv / 2;
        else if (nev_new == 1 && m_ncv > 2)
            nev_new = 2;
        if (nev_new > m_ncv - 1)
            nev_new = m_ncv - 1;
        return nev_new;
    }

    // One implicit restart keeping k Ritz pairs (reference :105-155): the shifted QR sweeps on Re(H) and Q on the host, H <- Q'HQ (a
    // real tridiagonal), then V <- V Q and the new residual on the device, and back to an ncv-step factorisation
    void restart(Index k, SortRule selection)
    {
        if (k >= m_ncv)
            return;
        const int m = static_cast<int>(m_ncv);
        const Index nshift = m_ncv - k;
        std::vector<double> shifts(static_cast<std::size_t>(nshift));
        for (Index i = 0; i < nshift; i++)
            shifts[std::size_t(i)] = m_ritz_val[std::size_t(k + i)];
        std::sort(shifts.begin(), shifts.end(), [](double a, double b) { return std::abs(a) > std::abs(b); });
        std::vector<double> diag, subd, Q(static_cast<std::size_t>(m) * m, 0.0), work(4 * static_cast<std::size_t>(m));
        real_tridiagonal(matrix_H(), diag, subd);
        for (int i = 0; i < m; i++)
            Q[static_cast<std::size_t>(i) * m + i] = 1.0;
        for (Index i = 0; i < nshift; i++)
            mispec::small::tridiag_shifted_qr(m, diag.data(), subd.data(), shifts[std::size_t(i)], Q.data(), m, m, work.data(),
                                              mispec::small::Lanes{0, 1});
        std::vector<Scalar> H(static_cast<std::size_t>(m) * m, Scalar(0));
        for (int i = 0; i < m; i++)
        {
            H[static_cast<std::size_t>(i) * m + i] = Scalar(diag[std::size_t(i)]);
            if (i + 1 < m)
            {
                H[static_cast<std::size_t>(i) * m + i + 1] = Scalar(subd[std::size_t(i)]);
                H[static_cast<std::size_t>(i + 1) * m + i] = Scalar(subd[std::size_t(i)]);
            }
        }
        check(mispec_zfac_set_H(m_fac.get(), reinterpret_cast<const double*>(H.data())));
        check(mispec_zfac_compress_real(m_fac.get(), Q.data(), static_cast<int>(k)));
        int64_t nops = m_nmatop;
        check(mispec_zfac_factorize(m_fac.get(), static_cast<int>(k), m, &nops));
        m_nmatop = nops;
        retrieve_ritzpair(selection);
    }

    // final ordering of the nev wanted pairs (reference :229-251)
    void sort_ritzpair(SortRule sort_rule)
    {
        if (sort_rule != SortRule::LargestAlge && sort_rule != SortRule::LargestMagn && sort_rule != SortRule::SmallestAlge &&
            sort_rule != SortRule::SmallestMagn)
            throw std::invalid_argument("unsupported sorting rule");
        const std::vector<Index> ind = argsort(sort_rule, m_ritz_val.data(), m_nev);
        std::vector<double> new_val(std::size_t(m_ncv), 0.0), new_vec(m_ritz_vec.size());
        std::vector<char> new_conv(std::size_t(m_nev), 0);
        for (Index i = 0; i < m_nev; i++)
        {
            const std::size_t s = std::size_t(ind[std::size_t(i)]);
            new_val[std::size_t(i)] = m_ritz_val[s];
            std::copy(m_ritz_vec.begin() + std::ptrdiff_t(s * std::size_t(m_ncv)), m_ritz_vec.begin() + std::ptrdiff_t((s + 1) * std::size_t(m_ncv)),
                      new_vec.begin() + i * m_ncv);
            new_conv[std::size_t(i)] = m_ritz_conv[s];
        }
        m_ritz_val.swap(new_val);
        m_ritz_vec.swap(new_vec);
        m_ritz_conv.swap(new_conv);
    }

    Index num_flagged() const
    {
        Index c = 0;
        for (char b : m_ritz_conv)
            c += b;
        return c;
    }

    void reset()
    {
        m_ritz_val.assign(std::size_t(m_ncv), 0.0);
        m_ritz_vec.assign(std::size_t(m_ncv * m_nev), 0.0);
        m_ritz_est.assign(std::size_t(m_ncv), 0.0);
        m_ritz_conv.assign(std::size_t(m_nev), 0);
        m_nmatop = 0;
        m_niter = 0;
    }

public:
    ComplexHermEigs(const OpType& op, Index nev, Index ncv) :
        m_op(op),
        m_n(op.rows()),
        m_nev(nev),
        m_ncv(check_args(op.rows(), nev, ncv)),
        m_ctx(context_of(op, std::integral_constant<bool, has_zcsr<OpType>::value || has_zdense<OpType>::value>()))
    {
        m_fac = std::shared_ptr<mispec_zfac>(create_fac(), [](mispec_zfac* p) { (void) mispec_zfac_destroy(p); });
        reset();
    }

    // Start from a user-supplied residual vector (n entries, host memory).
    void init(const Scalar* init_resid)
    {
        reset();
        int64_t nops = 0;
        check(mispec_zfac_init(m_fac.get(), reinterpret_cast<const double*>(init_resid), &nops));
        m_nmatop = nops;
    }

    // The reference's default vector: SimpleRandom<std::complex<double>>(0), real part drawn first.
    void init()
    {
        SimpleRandom<double> rng(0);
        std::vector<Scalar> v0(static_cast<std::size_t>(m_n));
        for (auto& v : v0)
        {
            const double re = rng.random();
            const double im = rng.random();
            v = Scalar(re, im);
        }
        init(v0.data());
    }

    Index compute(SortRule selection = SortRule::LargestMagn, Index maxit = 1000, RealScalar tol = 1e-10,
                  SortRule sorting = SortRule::LargestAlge)
    {
        int64_t nops = m_nmatop;
        check(mispec_zfac_factorize(m_fac.get(), 1, static_cast<int>(m_ncv), &nops));
        m_nmatop = nops;
        retrieve_ritzpair(selection);
        Index i, nconv = 0;
        for (i = 0; i < maxit; i++)
        {
            nconv = num_converged(tol);
            if (nconv >= m_nev)
                break;
            restart(nev_adjusted(nconv), selection);
        }
        sort_ritzpair(sorting);
        m_niter += i + 1;
        m_info = (nconv >= m_nev) ? CompInfo::Successful : CompInfo::NotConverging;
        return (std::min)(m_nev, nconv);
    }

    CompInfo info() const { return m_info; }
    Index num_iterations() const { return m_niter; }
    Index num_operations() const { return m_nmatop; }

    // Converged eigenvalues (real), in the order requested by `sorting`.
    RealVector eigenvalues() const
    {
        RealVector res(num_flagged());
        Index j = 0;
        for (Index i = 0; i < m_nev; i++)
            if (m_ritz_conv[std::size_t(i)])
                res[j++] = m_ritz_val[std::size_t(i)];
        return res;
    }

    // Eigenvectors of the converged eigenvalues: V times the Ritz vectors of Re(H), formed on the device (n x nvec, complex).
    Matrix eigenvectors(Index nvec) const
    {
        nvec = (std::min)(nvec, num_flagged());
        Matrix res(m_n, nvec);
        if (nvec <= 0)
            return res;
        std::vector<double> Y(std::size_t(m_ncv * nvec));
        Index j = 0;
        for (Index i = 0; i < m_nev && j < nvec; i++)
        {
            if (!m_ritz_conv[std::size_t(i)])
                continue;
            std::copy(m_ritz_vec.begin() + i * m_ncv, m_ritz_vec.begin() + (i + 1) * m_ncv, Y.begin() + j * m_ncv);
            j++;
        }
        check(mispec_zfac_ritz_vectors(m_fac.get(), Y.data(), static_cast<int>(nvec), reinterpret_cast<double*>(res.data())));
        return res;
    }
    Matrix eigenvectors() const { return eigenvectors(m_nev); }
};

}  // namespace internal
}  // namespace Spectra

#endif
