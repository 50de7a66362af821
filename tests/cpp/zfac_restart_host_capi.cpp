// TEST INFRASTRUCTURE — not part of the library.  The entry points of tests/cpp/zfac_host_capi.cpp (the complex factorisation's
// control flow, spectra_amd/csrc/zfac_flow.hpp, over a plain host backend) plus the restart primitives of the Hermitian solver
// (mispec_zfac_set_H, mispec_zfac_compress_real, mispec_zfac_ritz_vectors), whose backend primitive `vq` is added here by a derived
// backend.  tests/test_host_hermeigs.py loads it to run the restart checks of tests/herm_checks.py where there is no GPU.
//   g++ -std=c++17 -O2 -shared -fPIC -I spectra_amd/csrc tests/cpp/zfac_restart_host_capi.cpp -o <tmp>/libzfac_restart_host.so
#include "zfac_host_backend.hpp"

struct HostBackendVQ : HostBackend
{
    // out[:, c] = V[:, :nnz] Q[:nnz, c], nnz = min(m, first_nnz + c); a row at a time, so that out may be V
    void vq(const cd* V, int64_t ldv, int m, const double* Q, int ldq, int ncols, int first_nnz, cd* out, int64_t ldo)
    {
        std::vector<cd> row(static_cast<size_t>(m)), res(static_cast<size_t>(ncols));
        for (int64_t i = 0; i < n; i++)
        {
            for (int j = 0; j < m; j++)
                row[size_t(j)] = V[j * ldv + i];
            for (int c = 0; c < ncols; c++)
            {
                const int nnz = std::min(m, first_nnz + c);
                cd acc(0.0);
                for (int j = 0; j < nnz; j++)
                    acc += row[size_t(j)] * Q[size_t(c) * ldq + j];
                res[size_t(c)] = acc;
            }
            for (int c = 0; c < ncols; c++)
                out[c * ldo + i] = res[size_t(c)];
        }
    }
};

// the same entry points over the extended backend
#define HostBackend HostBackendVQ
#include "zfac_host_capi.cpp"
#undef HostBackend

extern "C" {
int mispec_zfac_set_H(zfac* F, const double* H)
{
    return guarded([&] { F->flow->set_H(reinterpret_cast<const cd*>(H)); });
}
int mispec_zfac_compress_real(zfac* F, const double* Q, int k)
{
    return guarded([&] { F->flow->compress_real(Q, k); });
}
int mispec_zfac_ritz_vectors(zfac* F, const double* Y, int nvec, double* X)
{
    return guarded([&] { F->flow->ritz_vectors(Y, nvec, reinterpret_cast<cd*>(X)); });
}
}
