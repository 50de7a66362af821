// Ingest from device memory: the front end that turns compressed arrays ALREADY in HBM (a torch.sparse_csr / sparse_csc tensor,
// or any arrays assembled on the device) into the mispec_csr the host entry points build — validation and narrowing of the
// indices, triangle -> full symmetric CSR (the device counterpart of csr.hip's mirror_triangle), general CSC -> CSR, the
// offset dictionary and codes (build_offset_codes), the far-gather statistic (far_fraction) — followed by the unchanged
// build_dia / build_windows.  The result cannot be told apart from the host path's: same arrays, same formats, same products.
//
// Shape of the mirror / transpose (k_count -> scan -> k_scatter -> k_rank):
//   * every input entry is one thread's work; its outer index is found by a binary search in the outer array that is narrowed
//     to the rows of the block's 4096-entry tile first (two full searches per block, ~8 steps per entry after that);
//   * k_count adds 1 to the length of every output row an entry goes to (integer atomics), an exclusive scan (k_scan_tile /
//     k_scan_add, 2048 entries per block, recursive over the block sums) turns the lengths into row pointers;
//   * k_scatter draws a slot from the row's cursor (integer atomic) and stores the 64-bit key (column << 32 | input position)
//     and the value's bits there: the ARRIVAL order inside a row is arbitrary, the key is not;
//   * k_rank gives every entry its place in the row: the number of entries of the row with a smaller key.  Keys are unique
//     inside a row (an input entry reaches a row at most once), so this is the stable sort by column the host does, for any
//     input: unsorted inner indices, duplicates, entries in the ignored triangle, empty rows.  It works out of global memory
//     (the keys of a short row sit in one or two cache lines; all lanes of a long row read the same key at a time), so a row of
//     any length takes the same path and nothing depends on what LDS holds.  Cost: (row length)^2 compares per row — 225 at the
//     15 entries per row of a band, 4.9e9 spread over 70 000 threads for one full row of n = 70 000.  A matrix with a row of more
//     than kLongRow = 2^20 entries is not ranked here at all: k_max_row finds it right after the scan, the validated input is
//     downloaded once and the host routine (which sorts such a row in milliseconds) builds the same bytes.
//   Values travel as 64-bit integers: -0.0, NaN payloads and denormals arrive bit for bit.  No floating-point atomics anywhere.
//   A triangle whose inner indices are sorted is NOT detected (the host skips its row sort then): the cursors hand out slots in
//   arrival order, so the rows are ranked either way.
//
// Peak device memory of the mirror, everything resident together, with E_in entries in, E_out <= 2 E_in entries out, n rows and
// index width w (4 or 8):   input  w (n + 1) + (w + 8) E_in     (the caller's, untouched)
//                         + output 4 (n + 1) + 12 (E_out + 12)  (rowptr, colind, val with their padding)
//                         + scratch 4 n + 16 E_out + 4 ceil((n + 1) / 2048) + ...   (cursors, keys, value bits, scan sums)
// i.e. about (w + 8) E_in + 28 E_out + (w + 8) n bytes; the scratch is freed before the index formats are built.
//
// Patterns that need host-built structures: reverse Cuthill-McKee, the staged image and the tiles are built by host code from
// host arrays (reorder.hip, staged.hip, tiles.hip).  They are wanted when more than a quarter of the entries are further than
// kFarWindow from the diagonal with n >= 2 kFarWindow, or when options reorder=rcm, spmv_staged=1 or spmv_tiles=1 ask for them.
// In those cases only, the full CSR built here is downloaded once and handed to the host path (csr_upload_host), whose
// decisions and result are then the operator; banded, stencil and mesh matrices never take this download.  Porting those
// three builders to the device is not part of this file.
#include "csr_kernels.hpp"
#include "ingest.hpp"

#include <algorithm>
#include <chrono>
#include <memory>

using namespace mispec;

namespace {

constexpr int kTile = 4096;          // input / output entries per 256-thread block
constexpr int kScanTile = 2048;      // row lengths per block of the scan
constexpr int kSlots = 1024;         // open-addressing table of the dictionary: <= 25 % full at kMaxDict diagonals
constexpr int kEmptyKey = INT32_MIN; // no diagonal: |col - row| < 2^31 - 1
typedef unsigned long long u64;

// status words the kernels raise (device flags, read by the host once per stage)
enum Status { kBadOuter = 0, kBigOuter, kBadInner, kDictFull, kDictCount, kFar, kOuterFirst, kOuterLast, kMaxRow, kStatusWords };

// an index array of 4- or 8-byte integers in device memory
struct Idx
{
    const void* p;
    int bytes;
    __device__ __forceinline__ int64_t operator()(int64_t i) const
    {
        return bytes == 8 ? int64_t(static_cast<const long long*>(p)[i]) : int64_t(static_cast<const int*>(p)[i]);
    }
};

// largest o in [lo, hi) with outer(o) <= p; requires outer(lo) <= p and a non-decreasing outer
__device__ __forceinline__ int64_t owner_of(const Idx& outer, int64_t lo, int64_t hi, int64_t p)
{
    while (hi - lo > 1)
    {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (outer(mid) <= p)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// The outer range that owns positions [p_first, p_last] of a block's tile, found by threads 0 and 64 and shared through LDS.
__device__ __forceinline__ void tile_owners(const Idx& outer, int64_t n_outer, int64_t p_first, int64_t p_last, int64_t* s_range)
{
    if (threadIdx.x == 0)
        s_range[0] = owner_of(outer, 0, n_outer, p_first);
    if (threadIdx.x == 64)
        s_range[1] = owner_of(outer, 0, n_outer, p_last) + 1;
    __syncthreads();
}

// outer must be non-decreasing, non-negative and below `limit` BEFORE anything indexes with it
__global__ __launch_bounds__(256) void k_check_outer(Idx outer, int64_t n_outer, int64_t limit, u64* __restrict__ st)
{
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i > n_outer)
        return;
    const int64_t v = outer(i);
    if (v < 0 || (i > 0 && v < outer(i - 1)))
        st[kBadOuter] = 1;
    if (v > limit)
        st[kBigOuter] = 1;
    if (i == 0)
        st[kOuterFirst] = u64(v);
    if (i == n_outer)
        st[kOuterLast] = u64(v);
}

// MIRROR: entry (r, c) of the requested triangle goes to row r and, off the diagonal, to row c; else (general CSC): to row `inner`
template <bool MIRROR>
__global__ __launch_bounds__(256) void k_count(Idx outer, Idx inner, int64_t n_outer, int64_t n_inner, int64_t first, int64_t nnz_in,
                                               int lower, int row_major, uint32_t* __restrict__ len, u64* __restrict__ st)
{
    __shared__ int64_t s_range[2];
    const int64_t k0 = int64_t(blockIdx.x) * kTile, k1 = min(k0 + kTile, nnz_in);
    tile_owners(outer, n_outer, first + k0, first + k1 - 1, s_range);
    const int64_t olo = s_range[0], ohi = s_range[1];
    bool bad = false;
    for (int64_t k = k0 + threadIdx.x; k < k1; k += 256)
    {
        const int64_t o = owner_of(outer, olo, ohi, first + k);
        const int64_t in = inner(first + k);
        if (in < 0 || in >= n_inner)
        {
            bad = true;
            continue;
        }
        if (MIRROR)
        {
            const int64_t r = row_major ? o : in, c = row_major ? in : o;
            if (!(lower ? (r >= c) : (r <= c)))
                continue;
            atomicAdd(&len[r], 1u);
            if (r != c)
                atomicAdd(&len[c], 1u);
        }
        else
            atomicAdd(&len[in], 1u);
    }
    if (bad)
        st[kBadInner] = 1;
}

template <bool MIRROR>
__global__ __launch_bounds__(256) void k_scatter(Idx outer, Idx inner, const u64* __restrict__ val, int64_t n_outer, int64_t first,
                                                 int64_t nnz_in, int lower, int row_major, uint32_t* __restrict__ cursor,
                                                 u64* __restrict__ key, u64* __restrict__ bits)
{
    __shared__ int64_t s_range[2];
    const int64_t k0 = int64_t(blockIdx.x) * kTile, k1 = min(k0 + kTile, nnz_in);
    tile_owners(outer, n_outer, first + k0, first + k1 - 1, s_range);
    const int64_t olo = s_range[0], ohi = s_range[1];
    for (int64_t k = k0 + threadIdx.x; k < k1; k += 256)
    {
        const int64_t o = owner_of(outer, olo, ohi, first + k);
        const int64_t in = inner(first + k);  // validated by k_count
        const u64 v = val[first + k];
        if (MIRROR)
        {
            const int64_t r = row_major ? o : in, c = row_major ? in : o;
            if (!(lower ? (r >= c) : (r <= c)))
                continue;
            const uint32_t q = atomicAdd(&cursor[r], 1u);
            key[q] = (u64(c) << 32) | u64(k);
            bits[q] = v;
            if (r != c)
            {
                const uint32_t q2 = atomicAdd(&cursor[c], 1u);
                key[q2] = (u64(r) << 32) | u64(k);
                bits[q2] = v;
            }
        }
        else
        {
            const uint32_t q = atomicAdd(&cursor[in], 1u);
            key[q] = (u64(o) << 32) | u64(k);
            bits[q] = v;
        }
    }
}

// entry q of row [rs, re) goes to rs + (number of the row's keys below its own)
__global__ __launch_bounds__(256) void k_rank(const int32_t* __restrict__ rowptr, int64_t n_rows, int64_t nnz, const u64* __restrict__ key,
                                              const u64* __restrict__ bits, int32_t* __restrict__ colind, u64* __restrict__ val)
{
    __shared__ int64_t s_range[2];
    const Idx rp{rowptr, 4};
    const int64_t q0 = int64_t(blockIdx.x) * kTile, q1 = min(q0 + kTile, nnz);
    tile_owners(rp, n_rows, q0, q1 - 1, s_range);
    const int64_t rlo = s_range[0], rhi = s_range[1];
    for (int64_t q = q0 + threadIdx.x; q < q1; q += 256)
    {
        const int64_t r = owner_of(rp, rlo, rhi, q);
        const int rs = rowptr[r], re = rowptr[r + 1];
        const u64 mine = key[q];
        int below = 0;
        for (int j = rs; j < re; j++)
            below += key[j] < mine;
        colind[rs + below] = int32_t(mine >> 32);
        val[rs + below] = bits[q];
    }
}

// general CSR taken as it is: narrow and validate the column indices (values and row pointers are copied by the caller)
__global__ __launch_bounds__(256) void k_narrow(Idx inner, int64_t first, int64_t nnz, int64_t n_inner, int32_t* __restrict__ colind,
                                                u64* __restrict__ st)
{
    const int64_t k = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (k >= nnz)
        return;
    const int64_t in = inner(first + k);
    if (in < 0 || in >= n_inner)
    {
        st[kBadInner] = 1;
        return;
    }
    colind[k] = int32_t(in);
}
__global__ __launch_bounds__(256) void k_rebase(Idx outer, int64_t n_outer, int64_t first, int32_t* __restrict__ rowptr)
{
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i <= n_outer)
        rowptr[i] = int32_t(outer(i) - first);
}

// st[kMaxRow] = the longest row (rows of more than kLongRow entries are not ranked on the device, see Transposer)
__global__ __launch_bounds__(256) void k_max_row(const uint32_t* __restrict__ rowptr, int64_t n_rows, u64* __restrict__ st)
{
    __shared__ unsigned s_max;
    if (threadIdx.x == 0)
        s_max = 0;
    __syncthreads();
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i < n_rows)
        atomicMax(&s_max, rowptr[i + 1] - rowptr[i]);
    __syncthreads();
    if (threadIdx.x == 0 && s_max)
        atomicMax(&st[kMaxRow], u64(s_max));
}

// ---- exclusive scan of uint32 (row lengths -> row pointers), in place -----------------------------------------------------
__global__ __launch_bounds__(256) void k_scan_tile(uint32_t* __restrict__ data, int64_t n, uint32_t* __restrict__ sums)
{
    __shared__ uint32_t wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t base = int64_t(blockIdx.x) * kScanTile + int64_t(tid) * 8;
    uint32_t v[8], t = 0;
#pragma unroll
    for (int j = 0; j < 8; j++)
    {
        v[j] = base + j < n ? data[base + j] : 0u;
        t += v[j];
    }
    uint32_t x = t;  // inclusive over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1)
    {
        const uint32_t y = __shfl_up(x, off, 64);
        if (lane >= off)
            x += y;
    }
    if (lane == 63)
        wsum[wave] = x;
    __syncthreads();
    uint32_t before = 0;
    for (int w = 0; w < wave; w++)
        before += wsum[w];
    uint32_t run = before + x - t;
#pragma unroll
    for (int j = 0; j < 8; j++)
    {
        if (base + j < n)
            data[base + j] = run;
        run += v[j];
    }
    if (tid == 255)
        sums[blockIdx.x] = before + x;
}
__global__ __launch_bounds__(256) void k_scan_add(uint32_t* __restrict__ data, int64_t n, const uint32_t* __restrict__ sums)
{
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i < n)
        data[i] += sums[i / kScanTile];
}

// ---- offset dictionary, codes, far statistic ------------------------------------------------------------------------------
__host__ __device__ __forceinline__ unsigned dict_slot(int d) { return (unsigned(d) * 0x9E3779B1u) >> 22; }  // 10 bits

// Insert diagonal d, seen at entry position pos, into an open-addressing table (key, smallest position); *count counts the
// distinct keys.  false: the table has no room or no match within kSlots probes.
__device__ __forceinline__ bool dict_insert(int* key, unsigned* minpos, unsigned* count, int d, unsigned pos)
{
    unsigned h = dict_slot(d);
    for (int probe = 0; probe < kSlots; probe++, h = (h + 1) & (kSlots - 1))
    {
        int cur = *static_cast<volatile int*>(&key[h]);
        if (cur == kEmptyKey)
        {
            cur = atomicCAS(&key[h], kEmptyKey, d);
            if (cur == kEmptyKey)
            {
                atomicAdd(count, 1u);
                cur = d;
            }
        }
        if (cur == d)
        {
            if (pos < *static_cast<volatile unsigned*>(&minpos[h]))
                atomicMin(&minpos[h], pos);
            return true;
        }
    }
    return false;
}

// Per tile: the distinct diagonals col - row with the smallest position each occurs at, first in LDS, then merged into the
// global table gkey / gpos (kSlots each); st[kDictFull] once more than kMaxDict are seen.  Ordering the table's entries by
// position on the host gives the dictionary a single scan in entry order builds.  Also st[kFar] += entries with
// |col - row| > far_window, counted whether or not the dictionary overflows.
__global__ __launch_bounds__(256) void k_dict_far(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind, int64_t n_rows,
                                                  int64_t nnz, int64_t far_window, int* __restrict__ gkey, unsigned* __restrict__ gpos,
                                                  u64* __restrict__ st)
{
    __shared__ int64_t s_range[2];
    __shared__ int skey[kSlots];
    __shared__ unsigned spos[kSlots];
    __shared__ unsigned s_count, s_far, s_full;
    const Idx rp{rowptr, 4};
    for (int s = threadIdx.x; s < kSlots; s += 256)
    {
        skey[s] = kEmptyKey;
        spos[s] = 0xFFFFFFFFu;
    }
    if (threadIdx.x == 128)
    {
        s_count = 0;
        s_far = 0;
        s_full = *static_cast<volatile u64*>(&st[kDictFull]) != 0;
    }
    const int64_t q0 = int64_t(blockIdx.x) * kTile, q1 = min(q0 + kTile, nnz);
    tile_owners(rp, n_rows, q0, q1 - 1, s_range);  // (barrier: the table is initialised)
    const int64_t rlo = s_range[0], rhi = s_range[1];
    unsigned far = 0;
    for (int64_t q = q0 + threadIdx.x; q < q1; q += 256)
    {
        const int64_t r = owner_of(rp, rlo, rhi, q);
        const int64_t d = int64_t(colind[q]) - r;
        far += (d > far_window || -d > far_window);
        if (*static_cast<volatile unsigned*>(&s_full) == 0)
            if (!dict_insert(skey, spos, &s_count, int(d), unsigned(q)) || *static_cast<volatile unsigned*>(&s_count) > unsigned(kMaxDict))
                s_full = 1;
    }
    if (far)
        atomicAdd(&s_far, far);
    __syncthreads();
    if (threadIdx.x == 0 && s_far)
        atomicAdd(&st[kFar], u64(s_far));
    if (s_full)
    {
        if (threadIdx.x == 0)
            st[kDictFull] = 1;
        return;
    }
    unsigned* gcount = reinterpret_cast<unsigned*>(&st[kDictCount]);  // the low word (little endian) of a zeroed 64-bit slot
    for (int s = threadIdx.x; s < kSlots; s += 256)
        if (skey[s] != kEmptyKey)
            if (!dict_insert(gkey, gpos, gcount, skey[s], spos[s]) || *static_cast<volatile unsigned*>(gcount) > unsigned(kMaxDict))
                st[kDictFull] = 1;
}

// codes[q] = position of (colind[q] - row) in the dictionary, through the host-built lookup table (key, code) of kSlots slots
__global__ __launch_bounds__(256) void k_encode(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind, int64_t n_rows,
                                                int64_t nnz, const int* __restrict__ tkey, const int* __restrict__ tcode,
                                                uint8_t* __restrict__ codes)
{
    __shared__ int64_t s_range[2];
    __shared__ int skey[kSlots], scode[kSlots];
    const Idx rp{rowptr, 4};
    for (int s = threadIdx.x; s < kSlots; s += 256)
    {
        skey[s] = tkey[s];
        scode[s] = tcode[s];
    }
    const int64_t q0 = int64_t(blockIdx.x) * kTile, q1 = min(q0 + kTile, nnz);
    tile_owners(rp, n_rows, q0, q1 - 1, s_range);
    const int64_t rlo = s_range[0], rhi = s_range[1];
    for (int64_t q = q0 + threadIdx.x; q < q1; q += 256)
    {
        const int64_t r = owner_of(rp, rlo, rhi, q);
        const int d = int(int64_t(colind[q]) - r);
        unsigned h = dict_slot(d);
        int code = 0;
        for (int probe = 0; probe < kSlots; probe++, h = (h + 1) & (kSlots - 1))
            if (skey[h] == d)
            {
                code = scode[h];
                break;
            }
        codes[q] = uint8_t(code);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
inline unsigned tiles_of(int64_t n, int per) { return unsigned((n + per - 1) / per); }

struct StageTimer
{
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    int slot;
    explicit StageTimer(int s) : slot(s) {}
    ~StageTimer() { ingest_seconds()[slot] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};

// the status words of one call
struct DevStatus
{
    DevBuf<u64> d;
    u64 h[kStatusWords];
    hipStream_t s;
    explicit DevStatus(hipStream_t stream) : s(stream)
    {
        d.alloc(kStatusWords);
        MISPEC_HIP(hipMemsetAsync(d.p, 0, kStatusWords * sizeof(u64), s));
    }
    void read()  // synchronises the stream
    {
        MISPEC_HIP(hipMemcpyAsync(h, d.p, sizeof(h), hipMemcpyDeviceToHost, s));
        MISPEC_HIP(hipStreamSynchronize(s));
    }
};

void scan_exclusive(hipStream_t s, uint32_t* data, int64_t n, std::vector<std::unique_ptr<DevBuf<uint32_t>>>& keep)
{
    const unsigned nb = tiles_of(n, kScanTile);
    std::unique_ptr<DevBuf<uint32_t>> sums(new DevBuf<uint32_t>());
    sums->alloc(nb);
    hipLaunchKernelGGL(k_scan_tile, dim3(nb), dim3(256), 0, s, data, n, sums->p);
    MISPEC_HIP(hipGetLastError());
    if (nb > 1)
    {
        scan_exclusive(s, sums->p, nb, keep);
        hipLaunchKernelGGL(k_scan_add, dim3(tiles_of(n, 256)), dim3(256), 0, s, data, n, sums->p);
        MISPEC_HIP(hipGetLastError());
    }
    keep.push_back(std::move(sums));
}

// What the caller handed over, checked on the device: outer is safe to index with afterwards.
struct DeviceInput
{
    Idx outer, inner;
    const u64* val;
    int64_t n_outer, n_inner;
    int64_t first = 0, nnz = 0;  // entries [first, first + nnz) of inner / val
};

DeviceInput check_input(const char* who, mispec_ctx* ctx, DevStatus& st, int64_t n_outer, int64_t n_inner, const void* outer,
                        const void* inner, int index_bytes, const double* val)
{
    DeviceInput in{Idx{outer, index_bytes}, Idx{inner, index_bytes}, reinterpret_cast<const u64*>(val), n_outer, n_inner};
    const int64_t limit = (int64_t(1) << 31) - 17;  // alloc_entries: nnz < 2^31 - 16
    hipLaunchKernelGGL(k_check_outer, dim3(tiles_of(n_outer + 1, 256)), dim3(256), 0, ctx->stream, in.outer, n_outer, limit, st.d.p);
    MISPEC_HIP(hipGetLastError());
    st.read();
    MISPEC_REQUIRE(!st.h[kBadOuter], std::string(who) + ": row pointers must be non-decreasing");
    MISPEC_REQUIRE(!st.h[kBigOuter], std::string(who) + ": matrix shard has too many non-zeros for int32 row pointers");
    in.first = int64_t(st.h[kOuterFirst]);
    in.nnz = int64_t(st.h[kOuterLast]) - in.first;
    return in;
}

// Triangle -> full symmetric CSR (mirror), or general CSC -> CSR (!mirror), in two steps: count() makes the row pointers and the
// entry count, fill() the entries.
struct Transposer
{
    mispec_ctx* ctx;
    const DeviceInput& in;
    bool mirror, lower, row_major;
    int64_t n_rows;
    DevBuf<uint32_t> cursor;
    DevBuf<u64> key, bits;
    std::vector<std::unique_ptr<DevBuf<uint32_t>>> keep;
    int64_t max_row = 0;  // longest output row, after count(); beyond kLongRow the caller hands the matrix to the host routine

    // rowptr: n_rows + 1 ints of device memory.  Returns the entry count; `who` prefixes the messages.
    int64_t count(const char* who, DevStatus& st, int32_t* rowptr)
    {
        hipStream_t s = ctx->stream;
        uint32_t* len = reinterpret_cast<uint32_t*>(rowptr);
        MISPEC_HIP(hipMemsetAsync(len, 0, size_t(n_rows + 1) * sizeof(uint32_t), s));
        if (in.nnz > 0)
        {
            const dim3 grid(tiles_of(in.nnz, kTile)), block(256);
            if (mirror)
                hipLaunchKernelGGL(k_count<true>, grid, block, 0, s, in.outer, in.inner, in.n_outer, in.n_inner, in.first, in.nnz,
                                   int(lower), int(row_major), len, st.d.p);
            else
                hipLaunchKernelGGL(k_count<false>, grid, block, 0, s, in.outer, in.inner, in.n_outer, in.n_inner, in.first, in.nnz, 0, 0,
                                   len, st.d.p);
            MISPEC_HIP(hipGetLastError());
        }
        scan_exclusive(s, len, n_rows + 1, keep);
        if (n_rows > 0)
        {
            hipLaunchKernelGGL(k_max_row, dim3(tiles_of(n_rows, 256)), dim3(256), 0, s, len, n_rows, st.d.p);
            MISPEC_HIP(hipGetLastError());
        }
        uint32_t total = 0;
        MISPEC_HIP(hipMemcpyAsync(&total, len + n_rows, sizeof(total), hipMemcpyDeviceToHost, s));
        st.read();
        keep.clear();
        MISPEC_REQUIRE(!st.h[kBadInner], std::string(who) + (mirror ? ": index out of range" : ": row index out of range"));
        MISPEC_REQUIRE(int64_t(total) <= INT32_MAX, std::string(who) + ": more than 2^31 - 1 entries");
        max_row = int64_t(st.h[kMaxRow]);
        return int64_t(total);
    }
    void fill(const int32_t* rowptr, int64_t nnz_out, int32_t* colind, double* val)
    {
        if (nnz_out == 0)
            return;
        hipStream_t s = ctx->stream;
        cursor.alloc(size_t(n_rows));
        key.alloc(size_t(nnz_out));
        bits.alloc(size_t(nnz_out));
        MISPEC_HIP(hipMemcpyAsync(cursor.p, rowptr, size_t(n_rows) * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        const dim3 grid(tiles_of(in.nnz, kTile)), block(256);
        if (mirror)
            hipLaunchKernelGGL(k_scatter<true>, grid, block, 0, s, in.outer, in.inner, in.val, in.n_outer, in.first, in.nnz, int(lower),
                               int(row_major), cursor.p, key.p, bits.p);
        else
            hipLaunchKernelGGL(k_scatter<false>, grid, block, 0, s, in.outer, in.inner, in.val, in.n_outer, in.first, in.nnz, 0, 0, cursor.p,
                               key.p, bits.p);
        MISPEC_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_rank, dim3(tiles_of(nnz_out, kTile)), block, 0, s, rowptr, n_rows, nnz_out, key.p, bits.p, colind,
                           reinterpret_cast<u64*>(val));
        MISPEC_HIP(hipGetLastError());
        MISPEC_HIP(hipStreamSynchronize(s));
        cursor.release();
        key.release();
        bits.release();
    }
};

// The long-row path.  k_rank costs (row length)^2 compares per row: nothing for the rows of a band or a mesh, 35 ms for one
// row of a million entries, minutes for one of ten million.  A matrix with a row beyond kLongRow is therefore not ranked on the
// device: its (validated) input is downloaded once and the host routine, which sorts such a row in milliseconds, builds the
// same bytes.  The capability and the result stay; only the copy to the host is paid, by these matrices alone.
constexpr int64_t kLongRow = int64_t(1) << 20;

struct HostInput
{
    std::vector<int32_t> outer;
    RawVec<int32_t> inner;
    RawVec<double> val;
};
template <typename I>
void download_narrowed(const void* dev, int64_t first, int64_t count, int64_t subtract, int32_t* dst)
{
    if (count == 0)
        return;
    RawVec<I> tmp;
    tmp.resize_uninitialized(size_t(count));
    MISPEC_HIP(hipMemcpy(tmp.data(), static_cast<const I*>(dev) + first, size_t(count) * sizeof(I), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < count; i++)
        dst[i] = int32_t(int64_t(tmp[size_t(i)]) - subtract);  // in range: checked on the device
}
void download_input(mispec_ctx* ctx, const DeviceInput& in, HostInput& H)
{
    MISPEC_HIP(hipStreamSynchronize(ctx->stream));
    H.outer.assign(size_t(in.n_outer) + 1, 0);
    H.inner.resize_uninitialized(size_t(std::max<int64_t>(in.nnz, 1)));
    H.val.resize_uninitialized(size_t(std::max<int64_t>(in.nnz, 1)));
    if (in.outer.bytes == 8)
    {
        download_narrowed<long long>(in.outer.p, 0, in.n_outer + 1, in.first, H.outer.data());
        download_narrowed<long long>(in.inner.p, in.first, in.nnz, 0, H.inner.data());
    }
    else
    {
        download_narrowed<int>(in.outer.p, 0, in.n_outer + 1, in.first, H.outer.data());
        download_narrowed<int>(in.inner.p, in.first, in.nnz, 0, H.inner.data());
    }
    if (in.nnz > 0)
        MISPEC_HIP(hipMemcpy(H.val.data(), in.val + in.first, size_t(in.nnz) * sizeof(double), hipMemcpyDeviceToHost));
}
void rethrow_host(int rc)
{
    if (rc != MISPEC_OK)
        throw Error(rc, std::string(mispec_last_error()));
}

void require_plain_context(const char* who, const mispec_ctx* ctx, int index_bytes)
{
    MISPEC_REQUIRE(index_bytes == 4 || index_bytes == 8, std::string(who) + ": index_bytes must be 4 (int32) or 8 (int64)");
    MISPEC_REQUIRE(ctx->world() == 1 && ctx->comm.allgather == nullptr,
                   std::string(who) + ": a sharded context, or one with a communicator attached, cannot ingest device arrays "
                                      "(row shards from device memory are not supported)");
}

// The index formats and the far statistic of a CSR matrix whose arrays are complete in HBM, then — for the patterns that need
// host-built structures only — the hand-over to the host path.  Takes A over; returns the operator.
mispec_csr* finish_formats(std::unique_ptr<mispec_csr> A, bool structurally_symmetric)
{
    mispec_ctx* ctx = A->ctx;
    hipStream_t s = ctx->stream;
    const int64_t n_rows = A->n_rows, n_cols = A->n_cols, nnz = A->nnz;
    A->structurally_symmetric = structurally_symmetric;
    if (nnz == 0)
    {
        MISPEC_HIP(hipStreamSynchronize(s));
        return A.release();
    }
    // one pass: the distinct diagonals with their first positions, and the far count
    DevStatus st(s);
    DevBuf<int> table;  // [kSlots] diagonals, [kSlots] smallest positions
    std::vector<int> init(2 * kSlots, kEmptyKey);
    {
        StageTimer timer(3);
        table.alloc(2 * kSlots);
        std::fill(init.begin() + kSlots, init.end(), -1);  // 0xFFFFFFFF
        MISPEC_HIP(hipMemcpyAsync(table.p, init.data(), init.size() * sizeof(int), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_dict_far, dim3(tiles_of(nnz, kTile)), dim3(256), 0, s, A->rowptr.p, A->colind.p, n_rows, nnz, kFarWindow,
                           table.p, reinterpret_cast<unsigned*>(table.p + kSlots), st.d.p);
        MISPEC_HIP(hipGetLastError());
        MISPEC_HIP(hipMemcpyAsync(init.data(), table.p, init.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        st.read();
    }
    const double far = double(int64_t(st.h[kFar])) / double(nnz);  // far_fraction, to the bit: both are exact integers
    A->far_before = far;
    // does the host path build something from host arrays for this matrix?  (the conditions of upload_rows)  Decided before the
    // formats are built: the host path builds its own.
    const Reorder reorder = option_choice(Opt::reorder, Reorder::automatic);
    const Tri staged = option_choice(Opt::spmv_staged, Tri::automatic), tiles = option_choice(Opt::spmv_tiles, Tri::automatic);
    const bool scattered = n_cols >= 2 * kFarWindow && far > 0.25;
    const bool wants_rcm = reorder != Reorder::none && n_rows == n_cols && (reorder == Reorder::rcm || (n_rows >= 2 * kFarWindow && far > 0.25));
    const bool wants_staged = staged != Tri::off && (staged == Tri::on || scattered);
    const bool wants_tiles = tiles != Tri::off && (tiles == Tri::on || scattered);
    if (!(wants_rcm || wants_staged || wants_tiles))
    {
        StageTimer timer(3);
        std::vector<std::pair<unsigned, int>> found;  // (first position, diagonal)
        for (int h = 0; h < kSlots; h++)
            if (init[size_t(h)] != kEmptyKey)
                found.emplace_back(unsigned(init[size_t(kSlots + h)]), init[size_t(h)]);
        if (!st.h[kDictFull] && !found.empty() && int(found.size()) <= kMaxDict)
        {
            std::sort(found.begin(), found.end());
            std::vector<int32_t> dict;
            std::vector<int> lookup(2 * kSlots, kEmptyKey);
            for (size_t k = 0; k < found.size(); k++)
            {
                const int d = found[k].second;
                dict.push_back(d);
                unsigned h = dict_slot(d);
                while (lookup[h] != kEmptyKey)
                    h = (h + 1) & (kSlots - 1);
                lookup[h] = d;
                lookup[size_t(kSlots) + h] = int(k);
            }
            csr_alloc_codes(*A);
            A->dict.alloc(dict.size());
            MISPEC_HIP(hipMemcpyAsync(A->dict.p, dict.data(), dict.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
            MISPEC_HIP(hipMemcpyAsync(table.p, lookup.data(), lookup.size() * sizeof(int), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_encode, dim3(tiles_of(nnz, kTile)), dim3(256), 0, s, A->rowptr.p, A->colind.p, n_rows, nnz, table.p,
                               table.p + kSlots, A->codes.p);
            MISPEC_HIP(hipGetLastError());
            MISPEC_HIP(hipStreamSynchronize(s));  // dict and lookup are locals
            A->ndict = int(dict.size());
            build_dia(*A, dict);
        }
        MISPEC_HIP(hipStreamSynchronize(s));
        build_windows(*A);
        return A.release();
    }
    std::vector<int32_t> rp(size_t(n_rows) + 1);
    RawVec<int32_t> ci;
    RawVec<double> v;
    ci.resize_uninitialized(size_t(nnz));
    v.resize_uninitialized(size_t(nnz));
    MISPEC_HIP(hipMemcpyAsync(rp.data(), A->rowptr.p, rp.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MISPEC_HIP(hipMemcpyAsync(ci.data(), A->colind.p, size_t(nnz) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MISPEC_HIP(hipMemcpyAsync(v.data(), A->val.p, size_t(nnz) * sizeof(double), hipMemcpyDeviceToHost, s));
    MISPEC_HIP(hipStreamSynchronize(s));
    A.reset();
    return csr_upload_host(ctx, n_rows, n_cols, rp.data(), ci.data(), v.data(), structurally_symmetric);
}

std::unique_ptr<mispec_csr> new_matrix(mispec_ctx* ctx, int64_t n_rows, int64_t n_cols)
{
    std::unique_ptr<mispec_csr> A(new mispec_csr());
    A->ctx = ctx;
    A->n_rows = n_rows;
    A->n_cols = n_cols;
    A->row_begin = 0;
    A->row_end = n_rows;
    A->rowptr.alloc(size_t(n_rows) + 1);
    return A;
}

bool is_uplo(char u) { return u == 'L' || u == 'U' || u == 'l' || u == 'u'; }

}  // namespace

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" int mispec_csr_from_device(mispec_ctx* ctx, int64_t n_rows, int64_t n_cols, const void* outer_dev, const void* inner_dev,
                                      int index_bytes, const double* val_dev, int row_major, mispec_csr** out)
{
    return guarded([&] {
        const char* who = "mispec_csr_from_device";
        MISPEC_REQUIRE(ctx && out && outer_dev && inner_dev && val_dev, "mispec_csr_from_device: NULL argument");
        MISPEC_REQUIRE(n_rows >= 0 && n_cols >= 0, "mispec_csr_from_device: bad argument");
        MISPEC_REQUIRE(n_rows < (int64_t(1) << 31) && n_cols < (int64_t(1) << 31), "mispec_csr_from_device: row or column count exceeds int32");
        require_plain_context(who, ctx, index_bytes);
        ctx->make_current();
        std::fill(ingest_seconds(), ingest_seconds() + 10, 0.0);
        StageTimer total(0);
        hipStream_t s = ctx->stream;
        std::unique_ptr<mispec_csr> A = new_matrix(ctx, n_rows, n_cols);
        HostInput long_rows;
        {
            StageTimer timer(2);
            DevStatus st(s);
            const DeviceInput in = check_input(who, ctx, st, row_major ? n_rows : n_cols, row_major ? n_cols : n_rows, outer_dev, inner_dev,
                                               index_bytes, val_dev);
            if (row_major)
            {
                csr_alloc_entries(*A, in.nnz);
                hipLaunchKernelGGL(k_rebase, dim3(tiles_of(n_rows + 1, 256)), dim3(256), 0, s, in.outer, n_rows, in.first, A->rowptr.p);
                MISPEC_HIP(hipGetLastError());
                if (in.nnz > 0)
                {
                    hipLaunchKernelGGL(k_narrow, dim3(tiles_of(in.nnz, 256)), dim3(256), 0, s, in.inner, in.first, in.nnz, n_cols,
                                       A->colind.p, st.d.p);
                    MISPEC_HIP(hipGetLastError());
                    MISPEC_HIP(hipMemcpyAsync(A->val.p, val_dev + in.first, size_t(in.nnz) * sizeof(double), hipMemcpyDeviceToDevice, s));
                }
                st.read();
                MISPEC_REQUIRE(!st.h[kBadInner], "mispec_csr_from_device: column index out of range");
            }
            else
            {
                Transposer T{ctx, in, false, false, false, n_rows};
                const int64_t nnz = T.count(who, st, A->rowptr.p);
                if (T.max_row > kLongRow)
                {
                    download_input(ctx, in, long_rows);
                    A.reset();
                }
                else
                {
                    csr_alloc_entries(*A, nnz);
                    T.fill(A->rowptr.p, nnz, A->colind.p, A->val.p);
                }
            }
        }
        if (!A)  // the long-row path: the host routine transposes (and resets and fills the stage timers)
        {
            rethrow_host(mispec_csr_from_csc(ctx, n_rows, n_cols, long_rows.outer.data(), long_rows.inner.data(), long_rows.val.data(), out));
            ingest_seconds()[0] = 0.0;  // `total` adds the whole call
            return;
        }
        *out = finish_formats(std::move(A), false);
    });
}

extern "C" int mispec_csr_from_triangle_device(mispec_ctx* ctx, int64_t n, const void* outer_dev, const void* inner_dev, int index_bytes,
                                               const double* val_dev, char uplo, int row_major, mispec_csr** out)
{
    return guarded([&] {
        const char* who = "mispec_csr_from_triangle_device";
        MISPEC_REQUIRE(ctx && out && outer_dev && inner_dev && val_dev, "mispec_csr_from_triangle_device: NULL argument");
        MISPEC_REQUIRE(is_uplo(uplo), "mispec_csr_from_triangle_device: uplo must be 'L' or 'U'");
        MISPEC_REQUIRE(n >= 0 && n < (int64_t(1) << 31), "mispec_csr_from_triangle_device: n must lie in [0, 2^31)");
        require_plain_context(who, ctx, index_bytes);
        ctx->make_current();
        std::fill(ingest_seconds(), ingest_seconds() + 10, 0.0);
        StageTimer total(0);
        std::unique_ptr<mispec_csr> A = new_matrix(ctx, n, n);
        HostInput long_rows;
        {
            StageTimer timer(1);
            DevStatus st(ctx->stream);
            const DeviceInput in = check_input(who, ctx, st, n, n, outer_dev, inner_dev, index_bytes, val_dev);
            Transposer T{ctx, in, true, uplo == 'L' || uplo == 'l', row_major != 0, n};
            const int64_t nnz = T.count(who, st, A->rowptr.p);
            if (T.max_row > kLongRow)
            {
                download_input(ctx, in, long_rows);
                A.reset();
            }
            else
            {
                csr_alloc_entries(*A, nnz);
                T.fill(A->rowptr.p, nnz, A->colind.p, A->val.p);
            }
        }
        if (!A)  // the long-row path: the host routine mirrors (and resets and fills the stage timers)
        {
            rethrow_host(mispec_csr_from_triangle(ctx, n, long_rows.outer.data(), long_rows.inner.data(), long_rows.val.data(), uplo,
                                                  row_major, out));
            ingest_seconds()[0] = 0.0;  // `total` adds the whole call
            return;
        }
        *out = finish_formats(std::move(A), true);
    });
}

extern "C" int mispec_mirror_triangle_device(mispec_ctx* ctx, int64_t n, const void* outer_dev, const void* inner_dev, int index_bytes,
                                             const double* val_dev, char uplo, int row_major, int32_t* rowptr_dev_out,
                                             int32_t* colind_dev_out, double* val_dev_out, int64_t capacity, int64_t* nnz_out)
{
    return guarded([&] {
        const char* who = "mispec_mirror_triangle_device";
        MISPEC_REQUIRE(ctx && outer_dev && inner_dev && val_dev && rowptr_dev_out && colind_dev_out && val_dev_out && nnz_out,
                       "mispec_mirror_triangle_device: NULL argument");
        MISPEC_REQUIRE(is_uplo(uplo), "mispec_mirror_triangle_device: uplo must be 'L' or 'U'");
        MISPEC_REQUIRE(n >= 0 && n < (int64_t(1) << 31), "mispec_mirror_triangle_device: n must lie in [0, 2^31)");
        require_plain_context(who, ctx, index_bytes);
        ctx->make_current();
        DevStatus st(ctx->stream);
        const DeviceInput in = check_input(who, ctx, st, n, n, outer_dev, inner_dev, index_bytes, val_dev);
        Transposer T{ctx, in, true, uplo == 'L' || uplo == 'l', row_major != 0, n};
        const int64_t nnz = T.count(who, st, rowptr_dev_out);
        MISPEC_REQUIRE(nnz <= capacity, "mispec_mirror_triangle_device: output capacity too small");
        if (T.max_row > kLongRow)  // the long-row path: mirrored by the host routine, copied back
        {
            HostInput H;
            download_input(ctx, in, H);
            std::vector<int32_t> rp(size_t(n) + 1);
            RawVec<int32_t> ci;
            RawVec<double> v;
            ci.resize_uninitialized(size_t(nnz));
            v.resize_uninitialized(size_t(nnz));
            int64_t host_nnz = 0;
            rethrow_host(mispec_mirror_triangle_host(n, H.outer.data(), H.inner.data(), H.val.data(), uplo, row_major, rp.data(), ci.data(),
                                                     v.data(), nnz, &host_nnz));
            MISPEC_HIP(hipMemcpy(rowptr_dev_out, rp.data(), rp.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            MISPEC_HIP(hipMemcpy(colind_dev_out, ci.data(), size_t(host_nnz) * sizeof(int32_t), hipMemcpyHostToDevice));
            MISPEC_HIP(hipMemcpy(val_dev_out, v.data(), size_t(host_nnz) * sizeof(double), hipMemcpyHostToDevice));
            *nnz_out = host_nnz;
            return;
        }
        T.fill(rowptr_dev_out, nnz, colind_dev_out, val_dev_out);
        MISPEC_HIP(hipStreamSynchronize(ctx->stream));
        *nnz_out = nnz;
    });
}
