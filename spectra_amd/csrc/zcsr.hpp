// Complex Hermitian sparse operator (mispec_zcsr, include/mispec_extras.h): the host-side ingest — one triangle of a compressed
// complex matrix mirrored conjugated into full int32 CSR — and, for the HIP sources, the device product csrc/zcsr.hip launches.
// The ingest is plain C++ so that a host build (tests) can use the same source.
//
// What `mat.selfadjointView<Uplo>()` reads (reference MatOp/SparseHermMatProd.h): entries of the `uplo` triangle only, the other
// triangle ignored; an off-diagonal entry a(i, j) stands for itself and for a(j, i) = conj(a(i, j)); the diagonal is taken real (its
// imaginary part dropped, as zdense_expand does for the dense operator).  Duplicates of one position are summed in input order.
#pragma once

#include <algorithm>
#include <complex>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

namespace mispec {

struct ZCsrHost
{
    int64_t n = 0;
    std::vector<int32_t> rowptr;  // n + 1
    std::vector<int32_t> col;     // nnz, ascending within a row
    std::vector<std::complex<double>> val;
};

// outer[outer_size + 1] / inner[nnz] with index type I (any width; narrowed to int32 here, rejected if it does not fit);
// row_major: outer runs over rows (CSR), else over columns (CSC).
template <typename I>
inline void zcsr_mirror(int64_t n, const I* outer, const I* inner, const std::complex<double>* values, bool row_major, char uplo,
                        ZCsrHost& out)
{
    using cd = std::complex<double>;
    if (n < 0 || n > int64_t(std::numeric_limits<int32_t>::max()))
        throw std::invalid_argument("complex sparse matrix: the dimension does not fit int32 indices");
    if (uplo != 'L' && uplo != 'U')
        throw std::invalid_argument("complex sparse matrix: uplo must be 'L' or 'U'");
    const int64_t nnz_in = n ? int64_t(outer[n]) - int64_t(outer[0]) : 0;
    if (n && (int64_t(outer[0]) != 0 || nnz_in < 0))
        throw std::invalid_argument("complex sparse matrix: the outer index array must start at 0 and not decrease");
    // (row, col) of stored entry e of outer slot o
    auto at = [&](int64_t o, int64_t e, int64_t& i, int64_t& j) {
        const int64_t in = int64_t(inner[e]);
        if (in < 0 || in >= n)
            throw std::invalid_argument("complex sparse matrix: inner index out of range");
        i = row_major ? o : in;
        j = row_major ? in : o;
    };
    auto kept = [&](int64_t i, int64_t j) { return uplo == 'L' ? i >= j : i <= j; };
    // pass 1: entries per row of the full matrix
    std::vector<int64_t> count(size_t(n) + 1, 0);
    for (int64_t o = 0; o < n; o++)
    {
        if (int64_t(outer[o + 1]) < int64_t(outer[o]))
            throw std::invalid_argument("complex sparse matrix: the outer index array must not decrease");
        for (int64_t e = int64_t(outer[o]); e < int64_t(outer[o + 1]); e++)
        {
            int64_t i, j;
            at(o, e, i, j);
            if (!kept(i, j))
                continue;
            count[size_t(i)]++;
            if (i != j)
                count[size_t(j)]++;
        }
    }
    std::vector<int64_t> start(size_t(n) + 1, 0);
    for (int64_t r = 0; r < n; r++)
        start[size_t(r) + 1] = start[size_t(r)] + count[size_t(r)];
    const int64_t total = start[size_t(n)];
    std::vector<int64_t> tcol(static_cast<size_t>(total));
    std::vector<cd> tval(static_cast<size_t>(total));
    std::vector<int64_t> fill(start.begin(), start.end() - 1);
    for (int64_t o = 0; o < n; o++)
        for (int64_t e = int64_t(outer[o]); e < int64_t(outer[o + 1]); e++)
        {
            int64_t i, j;
            at(o, e, i, j);
            if (!kept(i, j))
                continue;
            const cd v = values[e];
            if (i == j)
            {
                tcol[size_t(fill[size_t(i)])] = j;
                tval[size_t(fill[size_t(i)]++)] = cd(v.real(), 0.0);
                continue;
            }
            tcol[size_t(fill[size_t(i)])] = j;
            tval[size_t(fill[size_t(i)]++)] = v;
            tcol[size_t(fill[size_t(j)])] = i;
            tval[size_t(fill[size_t(j)]++)] = std::conj(v);
        }
    // sort every row by column (stable: duplicates keep input order) and sum duplicates
    out.n = n;
    out.rowptr.assign(size_t(n) + 1, 0);
    out.col.clear();
    out.val.clear();
    out.col.reserve(size_t(total));
    out.val.reserve(size_t(total));
    std::vector<int64_t> perm;
    for (int64_t r = 0; r < n; r++)
    {
        const int64_t b = start[size_t(r)], e = start[size_t(r) + 1];
        perm.resize(size_t(e - b));
        for (int64_t k = 0; k < e - b; k++)
            perm[size_t(k)] = b + k;
        std::stable_sort(perm.begin(), perm.end(), [&](int64_t x, int64_t y) { return tcol[size_t(x)] < tcol[size_t(y)]; });
        for (size_t k = 0; k < perm.size(); k++)
        {
            const int64_t c = tcol[size_t(perm[k])];
            if (k > 0 && int64_t(out.col.back()) == c && int64_t(out.col.size()) > int64_t(out.rowptr[size_t(r)]))
                out.val.back() += tval[size_t(perm[k])];
            else
            {
                out.col.push_back(int32_t(c));
                out.val.push_back(tval[size_t(perm[k])]);
            }
        }
        if (int64_t(out.col.size()) > int64_t(std::numeric_limits<int32_t>::max()))
            throw std::invalid_argument("complex sparse matrix: the mirrored matrix has more than 2^31 - 1 entries (int32 row pointers)");
        out.rowptr[size_t(r) + 1] = int32_t(out.col.size());
    }
}

}  // namespace mispec

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

struct mispec_zcsr;
namespace mispec {
// y = A x on device pointers (n complex entries each), on `stream`
void zcsr_apply(const mispec_zcsr* A, const double2* x, double2* y, hipStream_t stream);
int64_t zcsr_rows(const mispec_zcsr* A);
}  // namespace mispec
#endif
