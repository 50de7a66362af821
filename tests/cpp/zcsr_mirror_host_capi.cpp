// TEST INFRASTRUCTURE — not part of the library.  The host ingest of the complex Hermitian sparse operator (zcsr_mirror,
// spectra_amd/csrc/zcsr.hpp: the source mispec_zcsr_upload runs before anything reaches the device) behind one C entry point, for
// tests/test_host_zcsr.py.  Returns 0, -1 for std::invalid_argument (MISPEC_EINVAL), -3 for anything else; the caller sizes
// col / val for `cap` entries (twice the stored entries of the input always suffices).
//   g++ -std=c++17 -O2 -shared -fPIC -I spectra_amd/csrc tests/cpp/zcsr_mirror_host_capi.cpp -o <tmp>/libzcsr_mirror_host.so
#include <zcsr.hpp>

#include <cstring>

extern "C" int zcsr_mirror_host(int64_t n, const void* outer, const void* inner, int index_bytes, const double* values, int row_major,
                                char uplo, int32_t* rowptr, int32_t* col, double* val, int64_t cap, int64_t* nnz)
{
    try
    {
        mispec::ZCsrHost H;
        const std::complex<double>* v = reinterpret_cast<const std::complex<double>*>(values);
        if (index_bytes == 4)
            mispec::zcsr_mirror(n, static_cast<const int32_t*>(outer), static_cast<const int32_t*>(inner), v, row_major != 0, uplo, H);
        else
            mispec::zcsr_mirror(n, static_cast<const int64_t*>(outer), static_cast<const int64_t*>(inner), v, row_major != 0, uplo, H);
        *nnz = int64_t(H.col.size());
        if (H.n != n || int64_t(H.rowptr.size()) != n + 1 || H.val.size() != H.col.size() || *nnz > cap)
            return -3;
        std::memcpy(rowptr, H.rowptr.data(), H.rowptr.size() * sizeof(int32_t));
        if (*nnz)
        {
            std::memcpy(col, H.col.data(), H.col.size() * sizeof(int32_t));
            std::memcpy(val, H.val.data(), H.val.size() * sizeof(std::complex<double>));
        }
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
