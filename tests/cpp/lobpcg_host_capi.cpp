// The LOBPCG control flow (spectra_amd/csrc/lobpcg_flow.hpp) over a plain HOST backend, behind a small C ABI, so that
// tests/test_host_lobpcg.py can check the algorithm where there is no GPU.  Every block primitive is the obvious loop; the matrices
// are host CSR arrays.  g++ -std=c++17 -shared -fPIC -I spectra_amd/csrc -I include.
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <vector>

#include <Spectra/Util/SimpleRandom.h>

#include "lobpcg_flow.hpp"

namespace {

struct HostCsr
{
    int64_t n = 0;
    std::vector<int32_t> rowptr, colind;
    std::vector<double> val;
    bool set = false;
    void assign(int64_t rows, const int32_t* rp, const int32_t* ci, const double* v)
    {
        n = rows;
        rowptr.assign(rp, rp + rows + 1);
        colind.assign(ci, ci + rp[rows]);
        val.assign(v, v + rp[rows]);
        set = true;
    }
    void apply(const double* X, int64_t ld, int k, double* Y) const
    {
        for (int c = 0; c < k; c++)
            for (int64_t r = 0; r < n; r++)
            {
                double s = 0.0;
                for (int32_t p = rowptr[size_t(r)]; p < rowptr[size_t(r) + 1]; p++)
                    s += val[size_t(p)] * X[c * ld + colind[size_t(p)]];
                Y[c * ld + r] = s;
            }
    }
};

struct HostBackend
{
    int64_t n = 0;
    HostCsr A, B, T;
    std::vector<double> dinv;

    int64_t ld() const { return n; }
    double* alloc(size_t count) { return new double[count](); }
    void release(double* p) { delete[] p; }
    void copy(double* dst, const double* src, size_t count) { std::memmove(dst, src, count * sizeof(double)); }
    void random_col(double* col, uint64_t seed) { Spectra::SimpleRandom<double>(static_cast<unsigned long>(seed)).random_vec(col, std::ptrdiff_t(n)); }
    void apply_A(const double* X, int k, double* Y) { A.apply(X, n, k, Y); }
    void apply_B(const double* X, int k, double* Y) { B.apply(X, n, k, Y); }
    void apply_T(const double* X, int k, double* Y) { T.apply(X, n, k, Y); }
    void gram(const double* U, int p, const double* W, int q, bool symmetric, double* G)
    {
        for (int j = 0; j < q; j++)
            for (int i = 0; i < p; i++)
            {
                if (symmetric && i > j)
                    continue;
                double s = 0.0;
                for (int64_t r = 0; r < n; r++)
                    s += U[i * n + r] * W[j * n + r];
                G[size_t(j) * p + i] = s;
            }
        if (symmetric)
            for (int j = 0; j < q; j++)
                for (int i = j + 1; i < p; i++)
                    G[size_t(j) * p + i] = G[size_t(i) * p + j];
    }
    void vq(const double* V, int mm, const double* Q, int ldq, int p, double* X)
    {
        std::vector<double> row(static_cast<size_t>(mm)), out(static_cast<size_t>(p));
        for (int64_t r = 0; r < n; r++)
        {
            for (int k = 0; k < mm; k++)
                row[size_t(k)] = V[k * n + r];
            for (int c = 0; c < p; c++)
            {
                double s = 0.0;
                for (int k = 0; k < mm; k++)
                    s += row[size_t(k)] * Q[size_t(c) * ldq + k];
                out[size_t(c)] = s;
            }
            for (int c = 0; c < p; c++)
                X[c * n + r] = out[size_t(c)];
        }
    }
    void resid(const double* AX, const double* BX, int m, const double* lambda, const int* idx, int a, bool jacobi, double* R, double* norms2)
    {
        std::vector<int> pos(static_cast<size_t>(m), -1);
        for (int k = 0; k < a; k++)
            pos[size_t(idx[k])] = k;
        for (int j = 0; j < m; j++)
        {
            double s = 0.0;
            for (int64_t r = 0; r < n; r++)
            {
                const double v = AX[j * n + r] - lambda[j] * BX[j * n + r];
                s += v * v;
                if (pos[size_t(j)] >= 0)
                    R[pos[size_t(j)] * n + r] = jacobi ? v * dinv[size_t(r)] : v;
            }
            norms2[j] = s;
        }
    }
    void block_sub(double* Z, int q, const double* Y, int c, const double* C)
    {
        for (int j = 0; j < q; j++)
            for (int64_t r = 0; r < n; r++)
            {
                double z = Z[j * n + r];
                for (int k = 0; k < c; k++)
                    z -= Y[k * n + r] * C[size_t(j) * c + k];
                Z[j * n + r] = z;
            }
    }
};

struct Solver
{
    HostBackend be;
    std::unique_ptr<mispec::LobpcgFlow<HostBackend>> flow;
};

template <typename F>
int guarded(F&& f)
{
    try
    {
        f();
        return 0;
    }
    catch (const std::invalid_argument&)
    {
        return -1;
    }
    catch (...)
    {
        return -3;
    }
}

}  // namespace

extern "C" {

int lobpcg_host_create(int64_t n, const int32_t* rowptr, const int32_t* colind, const double* val, int64_t m, void** out)
{
    return guarded([&] {
        auto S = std::make_unique<Solver>();
        S->be.n = n;
        S->be.A.assign(n, rowptr, colind, val);
        if (m < 1 || m > mispec::kLobpcgMaxBlock)
            throw std::invalid_argument("block size");
        S->flow = std::make_unique<mispec::LobpcgFlow<HostBackend>>(S->be, n, int(m));
        *out = S.release();
    });
}
int lobpcg_host_destroy(void* h)
{
    delete static_cast<Solver*>(h);
    return 0;
}
int lobpcg_host_set_B(void* h, const int32_t* rowptr, const int32_t* colind, const double* val)
{
    return guarded([&] {
        Solver* S = static_cast<Solver*>(h);
        S->be.B.assign(S->be.n, rowptr, colind, val);
        S->flow->set_B(true);
    });
}
int lobpcg_host_set_preconditioner(void* h, const int32_t* rowptr, const int32_t* colind, const double* val)
{
    return guarded([&] {
        Solver* S = static_cast<Solver*>(h);
        S->be.T.assign(S->be.n, rowptr, colind, val);
        S->flow->set_T(true);
    });
}
int lobpcg_host_set_jacobi(void* h, int on)
{
    return guarded([&] {
        Solver* S = static_cast<Solver*>(h);
        const HostCsr& A = S->be.A;
        S->be.dinv.assign(size_t(A.n), 0.0);
        for (int64_t r = 0; r < A.n; r++)
        {
            double d = 0.0;
            for (int32_t p = A.rowptr[size_t(r)]; p < A.rowptr[size_t(r) + 1]; p++)
                if (A.colind[size_t(p)] == r)
                    d += A.val[size_t(p)];
            if (!(d > 0.0))
                throw std::invalid_argument("the Jacobi preconditioner needs a positive diagonal");
            S->be.dinv[size_t(r)] = 1.0 / d;
        }
        S->flow->set_jacobi(on != 0);
    });
}
int lobpcg_host_set_constraints(void* h, const double* Y, int64_t ld, int64_t c)
{
    return guarded([&] {
        Solver* S = static_cast<Solver*>(h);
        if (c < 0 || c > mispec::kLobpcgMaxBlock)
            throw std::invalid_argument("constraints");
        double* dst = S->flow->constraints_buffer(int(c));
        for (int64_t j = 0; j < c; j++)
            std::memcpy(dst + j * S->be.n, Y + j * ld, size_t(S->be.n) * sizeof(double));
    });
}
int lobpcg_host_set_initial(void* h, const double* X, int64_t ld)
{
    return guarded([&] {
        Solver* S = static_cast<Solver*>(h);
        double* dst = S->flow->initial_buffer();
        for (int j = 0; j < S->flow->block_size(); j++)
            std::memcpy(dst + j * S->be.n, X + j * ld, size_t(S->be.n) * sizeof(double));
        S->flow->initial_set();
    });
}
int lobpcg_host_compute(void* h, int selection, int64_t maxit, double tol, int64_t* nconv)
{
    return guarded([&] {
        Solver* S = static_cast<Solver*>(h);
        if (selection != 3 && selection != 7)
            throw std::invalid_argument("selection");
        *nconv = S->flow->compute(selection == 3, maxit, tol);
    });
}
int lobpcg_host_info(void* h) { return static_cast<Solver*>(h)->flow->info(); }
int64_t lobpcg_host_num_iterations(void* h) { return static_cast<Solver*>(h)->flow->num_iterations(); }
int64_t lobpcg_host_num_operations(void* h) { return static_cast<Solver*>(h)->flow->num_operations(); }
int64_t lobpcg_host_num_retries(void* h) { return static_cast<Solver*>(h)->flow->num_retries_without_p(); }
int64_t lobpcg_host_active_column_sum(void* h) { return static_cast<Solver*>(h)->flow->active_column_sum(); }
int lobpcg_host_eigenvalues(void* h, double* out)
{
    Solver* S = static_cast<Solver*>(h);
    std::copy(S->flow->eigenvalues().begin(), S->flow->eigenvalues().end(), out);
    return 0;
}
int lobpcg_host_residual_norms(void* h, double* out)
{
    Solver* S = static_cast<Solver*>(h);
    std::copy(S->flow->residual_norms().begin(), S->flow->residual_norms().end(), out);
    return 0;
}
int lobpcg_host_eigenvectors(void* h, double* out, int64_t ld)
{
    Solver* S = static_cast<Solver*>(h);
    for (int j = 0; j < S->flow->block_size(); j++)
        std::memcpy(out + j * ld, S->flow->vectors() + j * S->be.n, size_t(S->be.n) * sizeof(double));
    return 0;
}

}  // extern "C"
