// The dense symmetric eigenproblem the block solvers of libmispec_extras.so solve on the host (davidson.hip: the projected matrix
// V'AV; lobpcg_flow.hpp: the reduced pencil of the Rayleigh-Ritz step).  Host code only: the host-backend tests include it too.
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

#include <Spectra/internal/SmallDense.h>

namespace mispec {

// All eigenpairs of the symmetric s x s matrix G (column-major, destroyed): evals[s], evecs s x s column-major.
// Householder reduction to tridiagonal form with the transformation accumulated, then the implicit-shift QR of
// internal/SmallDense.h applied to that accumulated matrix.  Returns false if the QR iteration did not converge.
inline bool symmetric_eigen(int s, std::vector<double>& G, std::vector<double>& evals, std::vector<double>& evecs)
{
    auto g = [&](int i, int j) -> double& { return G[size_t(j) * s + i]; };
    evecs.assign(size_t(s) * s, 0.0);
    auto q = [&](int i, int j) -> double& { return evecs[size_t(j) * s + i]; };
    for (int i = 0; i < s; i++)
        q(i, i) = 1.0;
    std::vector<double> v(static_cast<size_t>(s)), w(static_cast<size_t>(s));
    for (int k = 0; k + 2 < s; k++)
    {
        double norm2 = 0.0;
        for (int i = k + 1; i < s; i++)
            norm2 += g(i, k) * g(i, k);
        const double x0 = g(k + 1, k);
        if (!(norm2 - x0 * x0 > 0.0))
            continue;  // already tridiagonal in this column
        const double alpha = x0 > 0.0 ? -std::sqrt(norm2) : std::sqrt(norm2);
        std::fill(v.begin(), v.end(), 0.0);
        for (int i = k + 1; i < s; i++)
            v[size_t(i)] = g(i, k);
        v[size_t(k) + 1] -= alpha;
        double vn = 0.0;
        for (int i = k + 1; i < s; i++)
            vn += v[size_t(i)] * v[size_t(i)];
        vn = std::sqrt(vn);
        if (!(vn > 0.0))
            continue;
        for (int i = k + 1; i < s; i++)
            v[size_t(i)] /= vn;
        // G <- H G H with H = I - 2 v v':  w = G v ; K = v'w ; G -= 2 (v w' + w v') - 4 K v v'
        for (int i = 0; i < s; i++)
        {
            double acc = 0.0;
            for (int j = k + 1; j < s; j++)
                acc += g(i, j) * v[size_t(j)];
            w[size_t(i)] = acc;
        }
        double K = 0.0;
        for (int i = k + 1; i < s; i++)
            K += v[size_t(i)] * w[size_t(i)];
        for (int j = 0; j < s; j++)
            for (int i = 0; i < s; i++)
                g(i, j) -= 2.0 * (v[size_t(i)] * w[size_t(j)] + w[size_t(i)] * v[size_t(j)]) - 4.0 * K * v[size_t(i)] * v[size_t(j)];
        // Q <- Q H
        for (int i = 0; i < s; i++)
        {
            double acc = 0.0;
            for (int j = k + 1; j < s; j++)
                acc += q(i, j) * v[size_t(j)];
            for (int j = k + 1; j < s; j++)
                q(i, j) -= 2.0 * acc * v[size_t(j)];
        }
    }
    evals.resize(static_cast<size_t>(s));
    std::vector<double> subd(static_cast<size_t>(std::max(s - 1, 1)), 0.0);
    for (int i = 0; i < s; i++)
        evals[size_t(i)] = g(i, i);
    for (int i = 0; i + 1 < s; i++)
        subd[size_t(i)] = 0.5 * (g(i + 1, i) + g(i, i + 1));
    return small::tridiag_eigen(s, evals.data(), subd.data(), evecs.data(), s, small::Lanes{0, 1}) == 0;
}

}  // namespace mispec
