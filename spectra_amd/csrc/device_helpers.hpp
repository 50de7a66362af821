// Device helpers shared by every kernel file: the fixed-order reductions over a wavefront and over a 256-thread workgroup, and the
// streamed 16-byte load of the basis passes.  One definition each, so every kernel sums in the same tree.  Internal.
#pragma once
#include <hip/hip_runtime.h>

namespace {

typedef double v2d __attribute__((ext_vector_type(2)));

// 16-byte load of two rows of a basis column with the non-temporal hint (streamed once per pass)
__device__ __forceinline__ double2 load_streamed(const double* p)
{
    const v2d t = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(p));  // (plain loads: round 4, profiles/r07b — the solve 1.7 % slower)
    double2 r;
    r.x = t.x;
    r.y = t.y;
    return r;
}

// sum / max over the 64 lanes of a wavefront in a fixed order; lane 0 holds the result
__device__ __forceinline__ double wave_reduce_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off, 64);
    return v;
}
__device__ __forceinline__ double wave_reduce_max(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = fmax(v, __shfl_down(v, off, 64));
    return v;
}

// Deterministic 256-thread sum; every thread returns the total.
__device__ __forceinline__ double block_reduce_sum(double v, double* red)
{
    v = wave_reduce_sum(v);
    if ((threadIdx.x & 63) == 0)
        red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace
