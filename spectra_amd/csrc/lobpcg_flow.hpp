// Control flow of the LOBPCG block eigensolver (contrib/LOBPCGSolver.h of the reference: the smallest — or largest — m eigenpairs of
// the SPD pencil A x = lambda B x with an optional preconditioner and optional constraints), written once over a small set of BLOCK
// primitives (the `Backend`).  The library instantiates it with the HIP backend of lobpcg.hip (every n-row block in HBM, the
// primitives are kernels); tests/cpp/lobpcg_host_capi.cpp instantiates the same flow with a plain host backend, so the algorithm can be
// checked where there is no GPU.
//
// Layout.  m is the block size, a <= m the number of active (unconverged) columns.  S = [X | R | P] is ONE contiguous column-major
// block of s = m + 2a <= 63 columns (m + a in the first iteration), AS and BS are its images (BS is S itself when no B is set).  Each
// of the three families has two buffers that ping-pong: the Rayleigh-Ritz step writes X+ = S C from one into the other.
//
// Per iteration (host work: Cholesky factors of Gram matrices of order <= 63, the reduced symmetric eigenproblem, sorting, locking):
//   R_j = AX_j - lambda_j BX_j for the active columns and |R_j|_2 of every column     (backend.resid, one launch)
//   a column is converged while |R_j|_2 < tol: it leaves R and P and stays in X        (soft locking, LOBPCGSolver.h:266-288, 380-399)
//   R <- T R (or the Jacobi scaling inside resid); R <- R - Y (Y'BY)^-1 (BY)' R       (preconditioner, constraints)
//   BR = B R; CholQR of R in the B inner product (R, BR transformed); AR = A R         (the ONLY product with A of the iteration)
//   P = [R P]_old C_RP[:, active] from the previous iteration's block, CholQR with AP, BP transformed alongside — never A P
//   gramA = S'(AS), gramB = S'(BS) in full (the identity / diag(lambda) blocks the reference assumes are not assumed)
//   Cholesky of gramB, eigenproblem of L^-1 gramA L^-T, the m wanted pairs C;  X+ = S C, AX+ = AS C, BX+ = BS C
// If the Cholesky of gramB fails the iteration is retried once without P; a second failure, or a failed CholQR of R or P, ends the run
// with NumericalIssue and X, lambda of the last completed iteration.  At the end A X and B X are recomputed once; the reported
// residuals and info come from those fresh products.
//
// Backend concept (double* are whatever the backend allocates; every n-row block is column-major with leading dimension ld()):
//   int64_t ld() const;   double* alloc(size_t count);   void release(double*);
//   void copy(double* dst, const double* src, size_t count);
//   void random_col(double* col, uint64_t seed);                               SimpleRandom(seed) stream, n entries
//   void apply_A / apply_B / apply_T(const double* X, int k, double* Y);       Y[:, :k] = Op X[:, :k], X and Y do not overlap
//   void gram(const double* U, int p, const double* W, int q, bool symmetric, double* G_host);    G = U'W, p x q column-major
//   void vq(const double* V, int mm, const double* Q_host, int ldq, int p, double* X);            X[:, :p] = V[:, :mm] Q; X == V allowed
//   void resid(const double* AX, const double* BX, int m, const double* lambda_host, const int* idx_host, int a, bool jacobi, double* R,
//              double* norms2_host);      R[:, k] = (AX - lambda BX)[:, idx k] (* dinv), norms2[j] = |AX_j - lambda_j BX_j|^2, j < m
//   void block_sub(double* Z, int q, const double* Y, int c, const double* C_host);               Z -= Y C, C is c x q column-major
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <stdexcept>
#include <vector>

#include "sym_eigen.hpp"

namespace mispec {

constexpr int kLobpcgMaxBlock = 21;  // 3 m must fit one 64-column panel of the Gram and V*Q kernels
enum LobpcgInfo
{
    kLobpcgSuccess = 0,
    kLobpcgNumericalIssue = 1,
    kLobpcgNoConvergence = 2,
    kLobpcgInvalidInput = 3  // before compute()
};

// G (s x s, column-major, symmetric, positive diagonal) -> d[j] = 1 / sqrt(G_jj) and the lower Cholesky factor L of D G D in G's lower
// triangle.  With the unit diagonal a pivot is the squared sine of the angle between a column and the ones before it, computed with an
// absolute error of about s * 2^-53: below kLobpcgPivotMin = 1e-8 (an angle of 1e-4) its leading digits go, and with them the factor —
// at 1e-10 a start block holding an exact eigenvector gave Ritz values 33 below the spectrum.  Such a pivot (or a diagonal entry that
// is not positive and finite) reports the block as rank deficient.
constexpr double kLobpcgPivotMin = 1e-8;
inline bool lobpcg_scaled_cholesky(int s, std::vector<double>& G, std::vector<double>& d)
{
    auto g = [&](int i, int j) -> double& { return G[size_t(j) * s + i]; };
    d.resize(size_t(s));
    for (int j = 0; j < s; j++)
    {
        const double gjj = g(j, j);
        if (!(gjj > 0.0) || !std::isfinite(gjj))
            return false;
        d[size_t(j)] = 1.0 / std::sqrt(gjj);
    }
    for (int j = 0; j < s; j++)
        for (int i = 0; i < s; i++)
            g(i, j) *= d[size_t(i)] * d[size_t(j)];
    for (int j = 0; j < s; j++)
    {
        double piv = g(j, j);
        for (int k = 0; k < j; k++)
            piv -= g(j, k) * g(j, k);
        if (!(piv > kLobpcgPivotMin) || !std::isfinite(piv))
            return false;
        const double ljj = std::sqrt(piv);
        g(j, j) = ljj;
        for (int i = j + 1; i < s; i++)
        {
            double v = g(i, j);
            for (int k = 0; k < j; k++)
                v -= g(i, k) * g(j, k);
            g(i, j) = v / ljj;
        }
    }
    return true;
}

// Q = D L^-T (upper triangular, s x s column-major): U Q is orthonormal in the inner product whose Gram matrix was factored
inline void lobpcg_inverse_factor(int s, const std::vector<double>& L, const std::vector<double>& d, std::vector<double>& Q)
{
    Q.assign(size_t(s) * s, 0.0);
    // column j of L^-T: solve L' x = e_j (back substitution; x has entries 0..j)
    for (int j = 0; j < s; j++)
    {
        double* x = &Q[size_t(j) * s];
        x[j] = 1.0 / L[size_t(j) * s + j];
        for (int i = j - 1; i >= 0; i--)
        {
            double v = 0.0;
            for (int k = i + 1; k <= j; k++)
                v -= L[size_t(i) * s + k] * x[k];  // L'(i, k) = L(k, i)
            x[i] = v / L[size_t(i) * s + i];
        }
        for (int i = 0; i <= j; i++)
            x[i] *= d[size_t(i)];
    }
}

// The pencil (GA, GB) of order s, both symmetric, GB positive definite: the `keep` eigenpairs at the wanted end, C s x keep with
// C' GB C = I.  0: done, 1: the Cholesky of GB failed, 2: the eigenproblem did not converge.
inline int lobpcg_rayleigh_ritz(int s, const std::vector<double>& GA, std::vector<double> GB, bool largest, int keep,
                                std::vector<double>& theta, std::vector<double>& C)
{
    std::vector<double> d, Q, M(size_t(s) * s), T(size_t(s) * s), evals, evecs;
    if (!lobpcg_scaled_cholesky(s, GB, d))
        return 1;
    lobpcg_inverse_factor(s, GB, d, Q);
    // M = Q' GA Q
    for (int j = 0; j < s; j++)
        for (int i = 0; i < s; i++)
        {
            double v = 0.0;
            for (int k = 0; k <= j; k++)
                v += GA[size_t(k) * s + i] * Q[size_t(j) * s + k];
            T[size_t(j) * s + i] = v;
        }
    for (int j = 0; j < s; j++)
        for (int i = 0; i < s; i++)
        {
            double v = 0.0;
            for (int k = 0; k <= i; k++)
                v += Q[size_t(i) * s + k] * T[size_t(j) * s + k];
            M[size_t(j) * s + i] = v;
        }
    for (int j = 0; j < s; j++)
        for (int i = 0; i < j; i++)
        {
            const double sym = 0.5 * (M[size_t(j) * s + i] + M[size_t(i) * s + j]);
            M[size_t(j) * s + i] = sym;
            M[size_t(i) * s + j] = sym;
        }
    if (!symmetric_eigen(s, M, evals, evecs))
        return 2;
    std::vector<int> order(static_cast<size_t>(s));
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
        return largest ? evals[size_t(x)] > evals[size_t(y)] : evals[size_t(x)] < evals[size_t(y)];
    });
    theta.resize(size_t(keep));
    C.assign(size_t(s) * keep, 0.0);
    for (int c = 0; c < keep; c++)
    {
        const int e = order[size_t(c)];
        theta[size_t(c)] = evals[size_t(e)];
        for (int i = 0; i < s; i++)
        {
            double v = 0.0;
            for (int k = i; k < s; k++)
                v += Q[size_t(k) * s + i] * evecs[size_t(e) * s + k];
            C[size_t(c) * s + i] = v;
        }
    }
    return 0;
}

template <typename Backend>
class LobpcgFlow
{
    Backend& m_be;
    const int64_t m_n, m_ld;
    const int m_m;
    int m_c = 0;
    bool m_hasB = false, m_hasT = false, m_jacobi = false;
    double* m_S[2] = {nullptr, nullptr};
    double* m_AS[2] = {nullptr, nullptr};
    double* m_BS[2] = {nullptr, nullptr};  // m_S when no B is set
    double* m_W = nullptr;                 // n x m scratch (input of the sparse preconditioner)
    double* m_Y = nullptr;                 // constraints, n x c
    double* m_BY = nullptr;                // B Y (m_Y when no B is set)
    std::vector<double> m_YBYinv;          // (Y'BY)^-1, c x c
    int m_cur = 0;
    bool m_have_x = false, m_computed = false;
    std::vector<double> m_lambda, m_norms;
    int m_info = kLobpcgInvalidInput;
    int64_t m_niter = 0, m_nops = 0, m_retries = 0, m_active_sum = 0;

    double* col(double* base, int j) const { return base + int64_t(j) * m_ld; }
    size_t block(int cols) const { return size_t(m_ld) * size_t(cols); }

    void free_B()
    {
        for (int b = 0; b < 2; b++)
        {
            if (m_BS[b] && m_BS[b] != m_S[b])
                m_be.release(m_BS[b]);
            m_BS[b] = m_S[b];
        }
        if (m_BY && m_BY != m_Y)
            m_be.release(m_BY);
        m_BY = m_Y;
    }

    // Z <- Z - Y (Y'BY)^-1 (BY)' Z on q columns (LOBPCGSolver.h applyConstraintsInPlace)
    void apply_constraints(double* Z, int q)
    {
        std::vector<double> G(size_t(m_c) * q), Cf(size_t(m_c) * q, 0.0);
        m_be.gram(m_BY, m_c, Z, q, false, G.data());
        for (int j = 0; j < q; j++)
            for (int i = 0; i < m_c; i++)
            {
                double v = 0.0;
                for (int k = 0; k < m_c; k++)
                    v += m_YBYinv[size_t(k) * m_c + i] * G[size_t(j) * m_c + k];
                Cf[size_t(j) * m_c + i] = v;
            }
        m_be.block_sub(Z, q, m_Y, m_c, Cf.data());
    }

    // CholQR in the B inner product of the k columns U with BU = B U given (U itself when no B): U <- U Q, and the same transformation
    // on BU and — when given — AU.  false: the Gram matrix is not numerically positive definite.
    bool cholqr(double* U, double* BU, double* AU, int k)
    {
        std::vector<double> G(size_t(k) * k), d, Q;
        m_be.gram(U, k, BU, k, true, G.data());
        if (!lobpcg_scaled_cholesky(k, G, d))
            return false;
        lobpcg_inverse_factor(k, G, d, Q);
        m_be.vq(U, k, Q.data(), k, k, U);
        if (BU != U)
            m_be.vq(BU, k, Q.data(), k, k, BU);
        if (AU)
            m_be.vq(AU, k, Q.data(), k, k, AU);
        return true;
    }

public:
    LobpcgFlow(Backend& be, int64_t n, int m) : m_be(be), m_n(n), m_ld(be.ld()), m_m(m)
    {
        if (m < 1 || m > kLobpcgMaxBlock)
            throw std::invalid_argument("LOBPCGSolver: the block size must satisfy 1 <= m <= 21 (3 m columns fit one 64-column panel)");
        if (!(int64_t(m) < n))
            throw std::invalid_argument("LOBPCGSolver: the block size must be smaller than the matrix size");
        for (int b = 0; b < 2; b++)
        {
            m_S[b] = m_be.alloc(block(3 * m));
            m_AS[b] = m_be.alloc(block(3 * m));
            m_BS[b] = m_S[b];
        }
        m_lambda.assign(size_t(m), 0.0);
        m_norms.assign(size_t(m), 0.0);
    }
    LobpcgFlow(const LobpcgFlow&) = delete;
    LobpcgFlow& operator=(const LobpcgFlow&) = delete;
    ~LobpcgFlow()
    {
        free_B();
        for (int b = 0; b < 2; b++)
        {
            m_be.release(m_S[b]);
            m_be.release(m_AS[b]);
        }
        if (m_W)
            m_be.release(m_W);
        if (m_Y)
            m_be.release(m_Y);
    }

    int64_t rows() const { return m_n; }
    int block_size() const { return m_m; }
    int num_constraints() const { return m_c; }

    // the backend's apply_B / apply_T are ready (or no longer to be used)
    void set_B(bool on)
    {
        free_B();
        m_hasB = on;
        if (on)
        {
            for (int b = 0; b < 2; b++)
                m_BS[b] = m_be.alloc(block(3 * m_m));
            if (m_Y)
                m_BY = m_be.alloc(block(m_c));
        }
    }
    void set_T(bool on)
    {
        m_hasT = on;
        if (on)
            m_jacobi = false;
        if (on && !m_W)
            m_W = m_be.alloc(block(m_m));
    }
    void set_jacobi(bool on)
    {
        m_jacobi = on;
        if (on)
            m_hasT = false;
    }
    // the device block the caller fills with the constraints (n x c, leading dimension ld()); c == 0 removes them
    double* constraints_buffer(int c)
    {
        if (c < 0 || c > kLobpcgMaxBlock)
            throw std::invalid_argument("LOBPCGSolver: at most 21 constraint vectors");
        if (c > 0 && !(int64_t(m_m) + c < m_n))
            throw std::invalid_argument("LOBPCGSolver: block size plus constraints must be smaller than the matrix size");
        if (m_BY && m_BY != m_Y)
            m_be.release(m_BY);
        if (m_Y)
            m_be.release(m_Y);
        m_Y = m_BY = nullptr;
        m_c = c;
        if (c > 0)
        {
            m_Y = m_be.alloc(block(c));
            m_BY = m_hasB ? m_be.alloc(block(c)) : m_Y;
        }
        return m_Y;
    }
    // the device block of the initial vectors (n x m): the caller fills it and calls initial_set()
    double* initial_buffer() { return m_S[m_cur]; }
    void initial_set() { m_have_x = true; }

    int info() const { return m_info; }
    int64_t num_iterations() const { return m_niter; }
    int64_t num_operations() const { return m_nops; }         // columns multiplied by A
    int64_t num_retries_without_p() const { return m_retries; }  // iterations whose Rayleigh-Ritz step was repeated without P
    int64_t active_column_sum() const { return m_active_sum; }   // sum over the iterations of the active width a
    const std::vector<double>& eigenvalues() const { return m_lambda; }
    const std::vector<double>& residual_norms() const { return m_norms; }
    bool computed() const { return m_computed; }
    const double* vectors() const { return m_S[m_cur]; }                  // X, n x m
    const double* residuals() const { return col(m_S[m_cur], m_m); }      // A X - B X diag(lambda) from the fresh products

    // returns the number of columns whose fresh residual norm is below tol
    int compute(bool largest, int64_t maxit, double tol)
    {
        const int m = m_m;
        m_info = kLobpcgNoConvergence;
        m_niter = 0;
        m_nops = 0;
        m_retries = 0;
        m_active_sum = 0;
        m_computed = false;
        if (!m_have_x)
        {
            for (int j = 0; j < m; j++)
                m_be.random_col(col(m_S[m_cur], j), uint64_t(j) + 1);
            m_have_x = true;
        }
        bool numerical = false;
        // ---- setup
        if (m_c > 0)
        {
            if (m_hasB)
                m_be.apply_B(m_Y, m_c, m_BY);
            std::vector<double> G(size_t(m_c) * m_c), d, Q;
            m_be.gram(m_Y, m_c, m_BY, m_c, true, G.data());
            if (!lobpcg_scaled_cholesky(m_c, G, d))
                throw std::invalid_argument("LOBPCGSolver: the constraint vectors are linearly dependent");
            lobpcg_inverse_factor(m_c, G, d, Q);
            m_YBYinv.assign(size_t(m_c) * m_c, 0.0);  // (Y'BY)^-1 = Q Q'
            for (int j = 0; j < m_c; j++)
                for (int i = 0; i < m_c; i++)
                {
                    double v = 0.0;
                    for (int k = std::max(i, j); k < m_c; k++)
                        v += Q[size_t(k) * m_c + i] * Q[size_t(k) * m_c + j];
                    m_YBYinv[size_t(j) * m_c + i] = v;
                }
            apply_constraints(m_S[m_cur], m);
        }
        {
            double* X = m_S[m_cur];
            if (m_hasB)
                m_be.apply_B(X, m, m_BS[m_cur]);
            if (!cholqr(X, m_BS[m_cur], nullptr, m))
                numerical = true;
            m_be.apply_A(X, m, m_AS[m_cur]);
            m_nops += m;
            std::vector<double> GA(size_t(m) * m), GB(size_t(m) * m), C;
            m_be.gram(X, m, m_AS[m_cur], m, true, GA.data());
            m_be.gram(X, m, m_BS[m_cur], m, true, GB.data());
            if (!numerical && lobpcg_rayleigh_ritz(m, GA, GB, largest, m, m_lambda, C) != 0)
                numerical = true;
            if (numerical)  // no iteration was completed: the Rayleigh quotients x'Ax / x'Bx of the start vectors are all there is to report
                for (int j = 0; j < m; j++)
                    m_lambda[size_t(j)] = GB[size_t(j) * m + j] > 0.0 ? GA[size_t(j) * m + j] / GB[size_t(j) * m + j] : 0.0;
            else
            {
                m_be.vq(X, m, C.data(), m, m, X);
                m_be.vq(m_AS[m_cur], m, C.data(), m, m, m_AS[m_cur]);
                if (m_hasB)
                    m_be.vq(m_BS[m_cur], m, C.data(), m, m, m_BS[m_cur]);
            }
        }
        // ---- iterations
        std::vector<int> idx(static_cast<size_t>(m)), now;
        std::iota(idx.begin(), idx.end(), 0);
        std::vector<double> norms2(static_cast<size_t>(m)), Cprev, GA, GB, GAs, GBs, theta, C;
        int tail_prev = 0;  // columns of [R P] of the previous block (rows of Cprev)
        for (int64_t it = 0; !numerical; it++)
        {
            const int cur = m_cur, old = m_cur ^ 1;
            double* S = m_S[cur];
            double* AS = m_AS[cur];
            double* BS = m_BS[cur];
            double* R = col(S, m);
            double* Rdst = m_hasT ? m_W : R;
            // the list of the previous iteration is the prediction; a column that converged (or came back) costs a second launch
            for (int pass = 0; pass < 2; pass++)
            {
                m_be.resid(AS, BS, m, m_lambda.data(), idx.data(), int(idx.size()), m_jacobi, Rdst, norms2.data());
                now.clear();
                for (int j = 0; j < m; j++)
                {
                    m_norms[size_t(j)] = std::sqrt(norms2[size_t(j)]);
                    if (!(m_norms[size_t(j)] < tol))
                        now.push_back(j);
                }
                if (now == idx)
                    break;
                idx = now;
                if (idx.empty())
                    break;
            }
            const int a = int(idx.size());
            if (a == 0)
                break;
            if (it >= maxit)
                break;
            if (m_hasT)
                m_be.apply_T(m_W, a, R);
            if (m_c > 0)
                apply_constraints(R, a);
            double* BR = col(BS, m);
            if (m_hasB)
                m_be.apply_B(R, a, BR);
            if (!cholqr(R, BR, nullptr, a))
            {
                numerical = true;
                break;
            }
            m_be.apply_A(R, a, col(AS, m));
            m_nops += a;
            m_active_sum += a;
            bool hasP = tail_prev > 0;
            if (hasP)
            {
                // P = [R P]_old C_RP[:, active] and its images, from the block the last Rayleigh-Ritz step read
                std::vector<double> Cp(size_t(tail_prev) * a);
                for (int k = 0; k < a; k++)
                    std::copy(Cprev.begin() + size_t(idx[size_t(k)]) * tail_prev, Cprev.begin() + size_t(idx[size_t(k)] + 1) * tail_prev,
                              Cp.begin() + size_t(k) * tail_prev);
                m_be.vq(col(m_S[old], m), tail_prev, Cp.data(), tail_prev, a, col(S, m + a));
                m_be.vq(col(m_AS[old], m), tail_prev, Cp.data(), tail_prev, a, col(AS, m + a));
                if (m_hasB)
                    m_be.vq(col(m_BS[old], m), tail_prev, Cp.data(), tail_prev, a, col(BS, m + a));
                if (!cholqr(col(S, m + a), col(BS, m + a), col(AS, m + a), a))
                {
                    numerical = true;
                    break;
                }
            }
            int s = m + a + (hasP ? a : 0);
            GA.resize(size_t(s) * s);
            GB.resize(size_t(s) * s);
            m_be.gram(S, s, AS, s, true, GA.data());
            m_be.gram(S, s, BS, s, true, GB.data());
            int rc = lobpcg_rayleigh_ritz(s, GA, GB, largest, m, theta, C);
            if (rc == 1 && hasP)
            {
                // retry once without P: the leading blocks of the Gram matrices
                m_retries++;
                const int s2 = m + a;
                GAs.resize(size_t(s2) * s2);
                GBs.resize(size_t(s2) * s2);
                for (int j = 0; j < s2; j++)
                    for (int i = 0; i < s2; i++)
                    {
                        GAs[size_t(j) * s2 + i] = GA[size_t(j) * s + i];
                        GBs[size_t(j) * s2 + i] = GB[size_t(j) * s + i];
                    }
                s = s2;
                rc = lobpcg_rayleigh_ritz(s, GAs, GBs, largest, m, theta, C);
            }
            if (rc != 0)
            {
                numerical = true;
                break;
            }
            m_be.vq(S, s, C.data(), s, m, m_S[old]);
            m_be.vq(AS, s, C.data(), s, m, m_AS[old]);
            if (m_hasB)
                m_be.vq(BS, s, C.data(), s, m, m_BS[old]);
            m_lambda = theta;
            tail_prev = s - m;
            Cprev.resize(size_t(tail_prev) * m);
            for (int j = 0; j < m; j++)
                std::copy(C.begin() + size_t(j) * s + m, C.begin() + size_t(j + 1) * s, Cprev.begin() + size_t(j) * tail_prev);
            m_cur = old;
            m_niter = it + 1;
        }
        // ---- end: fresh products, the residuals and the info that are reported
        {
            double* X = m_S[m_cur];
            m_be.apply_A(X, m, m_AS[m_cur]);
            m_nops += m;
            if (m_hasB)
                m_be.apply_B(X, m, m_BS[m_cur]);
            std::vector<int> all(static_cast<size_t>(m));
            std::iota(all.begin(), all.end(), 0);
            m_be.resid(m_AS[m_cur], m_BS[m_cur], m, m_lambda.data(), all.data(), m, false, col(X, m), norms2.data());
            int nconv = 0;
            for (int j = 0; j < m; j++)
            {
                m_norms[size_t(j)] = std::sqrt(norms2[size_t(j)]);
                nconv += m_norms[size_t(j)] < tol ? 1 : 0;
            }
            m_info = numerical ? kLobpcgNumericalIssue : nconv == m ? kLobpcgSuccess : kLobpcgNoConvergence;
            m_computed = true;
            return nconv;
        }
    }
};

}  // namespace mispec
