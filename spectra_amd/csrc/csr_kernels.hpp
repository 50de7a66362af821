// Device helpers shared by the SpMV kernels of csr.hip (CSR-stream), csr_win.hip (int32 CSR with x windows) and csr_dia.hip
// (diagonal storage): vector types, the LDS chunk sizes, the offset-code descriptor, the row-block map of a launch and the host's
// launch helpers; the fixed-order block sum comes from device_helpers.hpp.  Internal.
#pragma once
#include "csr.hpp"
#include "device_helpers.hpp"
#include "krylov.hpp"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <type_traits>
#include <utility>

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

// THREADS * 4 entries * 4 load steps = 16 * THREADS >= cap + 3 (k_spmv_csr_stream's ITERS = 4)
// products per LDS chunk for a THREADS-row workgroup: 256 -> (4080+4)*8 B + 32 B <= 32 KiB -> 5 workgroups / CU
constexpr int chunk_cap(int threads) { return threads * 16 - 16; }
// offset-coded variant: 1 KiB of the 32 KiB goes to the dictionary -> (3952+4)*8 + 1024 + 32 B, still 5 workgroups / CU
constexpr int chunk_cap_codes(int threads) { return threads * 16 - 144; }
constexpr int kMaxDict = 256;

struct SpmvCodes
{
    const uint8_t* codes;
    const int32_t* dict;
    int ndict;
    int col_max;       // n_cols - 1
    int64_t row_begin; // global index of local row 0
};

// XCD-aware row-block map of an SpMV launch over nblocks row-blocks: the grid is spmv_grid_blocks(nblocks) = 8 * per workgroups;
// hardware sends block b to XCD b % 8, so block b takes the (b / 8)-th row-block of that XCD's contiguous range of `per` and an
// XCD's private L2 sees one sliding window of x instead of eight interleaved ones.  Returns the row-block's index within the
// launch, or -1 for the blocks past the end.  Every storage format uses this same map over the same 256-row blocks: the alpha
// partials of the fused epilogue are identical records.
__device__ __forceinline__ int spmv_block_of_launch(int nblocks)
{
    const int per = (nblocks + 7) >> 3;
    const int lmap = (int(blockIdx.x) & 7) * per + (int(blockIdx.x) >> 3);
    return lmap < nblocks ? lmap : -1;
}
inline unsigned spmv_grid_blocks(int nblocks) { return unsigned(((nblocks + 7) / 8) * 8); }

// One launch path.  With an event pair the launch is timed through the dispatch's own completion signal (start/stop of the
// kernel itself, as a profiler sees it) instead of marker packets around it.
template <typename... Params, typename... Args>
void launch_kernel(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, hipEvent_t ev_start,
                   hipEvent_t ev_stop, const Args&... args)
{
    static_assert(sizeof...(Params) == sizeof...(Args), "launch_kernel: argument count");
    if (ev_start && ev_stop)
        hipExtLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, ev_start, ev_stop, 0, static_cast<Params>(args)...);
    else
        hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, static_cast<Params>(args)...);
}

// A run-time value as a compile-time constant for a generic lambda: f(std::integral_constant<int, C>{}) with the first listed
// constant C that is >= v, else the last; f(std::true_type / std::false_type{}) for a bool.  Only the listed constants are
// instantiated; a lambda excludes a combination with `if constexpr`.
template <int C0, int... Cs, typename F>
void with_tier(int v, F&& f)
{
    if constexpr (sizeof...(Cs) == 0)
        f(std::integral_constant<int, C0>{});
    else if (v <= C0)
        f(std::integral_constant<int, C0>{});
    else
        with_tier<Cs...>(v, std::forward<F>(f));
}
template <typename F>
void with_bool(bool v, F&& f)
{
    if (v)
        f(std::true_type{});
    else
        f(std::false_type{});
}

}  // namespace

namespace mispec {

// What launch_spmv_raw (csr.hip) hands to the per-format launchers: the grid over the row-blocks [first_block, first_block +
// nblocks) of the shard (XCD-aware block map inside the kernels), the epilogue with first_block filled in, the event pair of a
// timed launch (the dispatch's own completion signal), the operands.
struct SpmvLaunch
{
    dim3 grid, block;
    int64_t nloc;
    int nblocks;
    const SpmvEpilogue* epi;  // nullptr: plain product
    SpmvEpilogue e;
    hipEvent_t ev_start, ev_stop;
    const double* x_dev;
    double* y_dev;
};
// csr_dia.hip — diagonal storage (format 2): build at ingest, launch
void build_dia(mispec_csr& A, const std::vector<int32_t>& dict);
void launch_spmv_dia(const mispec_csr& A, const SpmvLaunch& L);
// csr_win.hip — int32 CSR with the x entries of a row-block staged through LDS windows (format 0 with a window table)
void build_windows(mispec_csr& A);
void launch_spmv_csr_win(const mispec_csr& A, const SpmvLaunch& L);

}  // namespace mispec
