// diag[r] = A(row_begin + r, row_begin + r) of the STORED matrix (the permuted one when A is reordered): the diagonal preconditioners of
// the Davidson and LOBPCG solvers (davidson.hip, lobpcg.hip).
#pragma once

#include "csr.hpp"

namespace mispec {

constexpr int kCsrDiagThreads = 256;

static __global__ __launch_bounds__(kCsrDiagThreads) void k_csr_diag(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                        const double* __restrict__ val, int64_t row_begin, int64_t nloc,
                                                        double* __restrict__ diag)
{
    const int64_t r = int64_t(blockIdx.x) * kCsrDiagThreads + threadIdx.x;
    if (r >= nloc)
        return;
    double d = 0.0;
    for (int p = rowptr[r]; p < rowptr[r + 1]; p++)
        if (colind[p] == row_begin + r)
            d += val[p];
    diag[r] = d;
}

}  // namespace mispec
