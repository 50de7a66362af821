// Solver-level C entry points of the complex Hermitian eigensolver (mispec_hermeigs_*, include/mispec_extras.h): the header-only
// HermEigsSolver<OpType> for std::complex<double> (include/Spectra/HermEigsSolver.h, internal/ComplexHermEigs.h) instantiated inside
// libmispec_extras.so for bindings that cannot instantiate C++ templates, the way facade.hip does for SymEigsSolver.  Nothing here
// adds arithmetic: the operator is a device matrix created through the C ABI, bound to the solver by the members the driver looks for.
#include <Spectra/HermEigsSolver.h>

#include <cstring>
#include <memory>

#include "common.hpp"

using namespace mispec;

namespace {

using cd = std::complex<double>;

// a borrowed mispec_zcsr as an OpType
class ZcsrRef
{
    mispec_ctx* m_ctx;
    const mispec_zcsr* m_mat;

public:
    using Scalar = cd;
    ZcsrRef(mispec_ctx* ctx, const mispec_zcsr* A) : m_ctx(ctx), m_mat(A) {}
    Spectra::Index rows() const { return Spectra::Index(mispec_zcsr_rows(m_mat)); }
    Spectra::Index cols() const { return Spectra::Index(mispec_zcsr_cols(m_mat)); }
    void perform_op(const cd* x, cd* y) const
    {
        Spectra::internal::check(mispec_zcsr_spmv_host(m_mat, reinterpret_cast<const double*>(x), reinterpret_cast<double*>(y)));
    }
    mispec_ctx* mispec_context() const { return m_ctx; }
    const mispec_zcsr* mispec_zcsr_matrix() const { return m_mat; }
};

// a borrowed mispec_zdense (Hermitian: uploaded with uplo 'L' / 'U') as an OpType
class ZdenseRef
{
    mispec_ctx* m_ctx;
    const mispec_zdense* m_mat;

public:
    using Scalar = cd;
    ZdenseRef(mispec_ctx* ctx, const mispec_zdense* D) : m_ctx(ctx), m_mat(D) {}
    Spectra::Index rows() const { return Spectra::Index(mispec_zdense_rows(m_mat)); }
    Spectra::Index cols() const { return Spectra::Index(mispec_zdense_cols(m_mat)); }
    void perform_op(const cd* x, cd* y) const
    {
        Spectra::internal::check(mispec_zdense_gemv_host(m_mat, reinterpret_cast<const double*>(x), reinterpret_cast<double*>(y)));
    }
    mispec_ctx* mispec_context() const { return m_ctx; }
    const mispec_zdense* mispec_zdense_matrix() const { return m_mat; }
};

}  // namespace

struct mispec_hermeigs
{
    std::unique_ptr<ZcsrRef> csr_op;
    std::unique_ptr<ZdenseRef> dense_op;
    std::unique_ptr<Spectra::HermEigsSolver<ZcsrRef>> csr;
    std::unique_ptr<Spectra::HermEigsSolver<ZdenseRef>> dense;

    template <typename F>
    auto visit(F&& f) const
    {
        if (csr)
            return f(*csr);
        return f(*dense);
    }
};

extern "C" int mispec_hermeigs_create_csr(mispec_ctx* ctx, const mispec_zcsr* A, int64_t nev, int64_t ncv, mispec_hermeigs** out)
{
    return guarded([&] {
        MISPEC_REQUIRE(ctx && A && out, "mispec_hermeigs_create_csr: NULL argument");
        auto s = std::make_unique<mispec_hermeigs>();
        s->csr_op = std::make_unique<ZcsrRef>(ctx, A);
        s->csr = std::make_unique<Spectra::HermEigsSolver<ZcsrRef>>(*s->csr_op, nev, ncv);
        *out = s.release();
    });
}

extern "C" int mispec_hermeigs_create_dense(mispec_ctx* ctx, const mispec_zdense* D, int64_t nev, int64_t ncv, mispec_hermeigs** out)
{
    return guarded([&] {
        MISPEC_REQUIRE(ctx && D && out, "mispec_hermeigs_create_dense: NULL argument");
        MISPEC_REQUIRE(mispec_zdense_rows(D) == mispec_zdense_cols(D), "mispec_hermeigs_create_dense: the matrix must be square");
        auto s = std::make_unique<mispec_hermeigs>();
        s->dense_op = std::make_unique<ZdenseRef>(ctx, D);
        s->dense = std::make_unique<Spectra::HermEigsSolver<ZdenseRef>>(*s->dense_op, nev, ncv);
        *out = s.release();
    });
}

extern "C" int mispec_hermeigs_destroy(mispec_hermeigs* S)
{
    return guarded([&] { delete S; });
}

extern "C" int mispec_hermeigs_init(mispec_hermeigs* S, const double* v0_host)
{
    return guarded([&] {
        MISPEC_REQUIRE(S, "mispec_hermeigs_init: NULL argument");
        S->visit([&](auto& solver) {
            if (v0_host)
                solver.init(reinterpret_cast<const cd*>(v0_host));
            else
                solver.init();
            return 0;
        });
    });
}

extern "C" int mispec_hermeigs_compute(mispec_hermeigs* S, int selection, int64_t maxit, double tol, int sorting, int64_t* nconv)
{
    return guarded([&] {
        MISPEC_REQUIRE(S && nconv, "mispec_hermeigs_compute: NULL argument");
        MISPEC_REQUIRE(selection >= 0 && selection <= int(Spectra::SortRule::BothEnds) && sorting >= 0 &&
                           sorting <= int(Spectra::SortRule::BothEnds),
                       "mispec_hermeigs_compute: unknown SortRule value");
        *nconv = S->visit([&](auto& solver) {
            return int64_t(solver.compute(static_cast<Spectra::SortRule>(selection), Spectra::Index(maxit), tol,
                                          static_cast<Spectra::SortRule>(sorting)));
        });
    });
}

extern "C" int mispec_hermeigs_info(const mispec_hermeigs* S)
{
    return S ? S->visit([](auto& solver) { return int(solver.info()); }) : int(Spectra::CompInfo::NotComputed);
}
extern "C" int64_t mispec_hermeigs_num_iterations(const mispec_hermeigs* S)
{
    return S ? S->visit([](auto& solver) { return int64_t(solver.num_iterations()); }) : 0;
}
extern "C" int64_t mispec_hermeigs_num_operations(const mispec_hermeigs* S)
{
    return S ? S->visit([](auto& solver) { return int64_t(solver.num_operations()); }) : 0;
}

extern "C" int mispec_hermeigs_eigenvalues(const mispec_hermeigs* S, double* out_host, int64_t* count)
{
    return guarded([&] {
        MISPEC_REQUIRE(S && count, "mispec_hermeigs_eigenvalues: NULL argument");
        S->visit([&](auto& solver) {
            const auto ev = solver.eigenvalues();
            *count = ev.size();
            if (out_host)
                std::memcpy(out_host, ev.data(), size_t(ev.size()) * sizeof(double));
            return 0;
        });
    });
}

extern "C" int mispec_hermeigs_eigenvectors(const mispec_hermeigs* S, int64_t nvec, double* out_host, int64_t* ncols)
{
    return guarded([&] {
        MISPEC_REQUIRE(S && ncols, "mispec_hermeigs_eigenvectors: NULL argument");
        S->visit([&](auto& solver) {
            const auto X = solver.eigenvectors(Spectra::Index(nvec));
            *ncols = X.cols();
            if (out_host)
                std::memcpy(out_host, X.data(), size_t(X.rows()) * size_t(X.cols()) * sizeof(cd));
            return 0;
        });
    });
}
