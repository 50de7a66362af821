// Block-tridiagonal path of the shift-and-invert operator: bands of half-bandwidth 65 ... 512 beyond the dense limit
// (shiftsolve.hpp shift_path).  M = A - sigma B is cut into N = ceil(n / s) blocks of s = band_b rows; the diagonal blocks D_i are
// symmetric dense, the sub-diagonal blocks E_i upper triangular (the band ends on their diagonal).  The last block is padded to s
// rows with rows of the identity, so every block has one shape.
//
//   factor (set_shift):  S_0 = D_0;  L_i = E_i S_{i-1}^{-1},  S_i = D_i - L_i E_i'   — kept: S_i^{-1} and L_i, 16 n s bytes
//   solve:               y_i = x_i - L_i y_{i-1};   z_i = S_i^{-1} y_i (one batched launch);   w_i = z_i - L_{i+1}' w_{i+1}
//
// There is no pivoting across blocks: an interior shift loses digits where a leading block system is nearly singular, and the
// calibrated refinement of shiftsolve.hip (calibrate_refinement / refine_once) wins them back, as on the chunk path.
// Order between the steps comes from the stream alone: one launch per chain step, no workgroup waits for another one.  Every
// entry is summed in an order fixed by (s, row, column): two factorisations and two solves give the same bits.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "shiftsolve.hpp"

namespace mispec {
namespace {

constexpr int kTile = 64;       // output tile of the block products
constexpr int kTileK = 16;      // depth of one LDS stage
constexpr int kInvThreads = 1024;
constexpr int kGemvRows = 16;   // rows per workgroup of the row products: 4 waves x 4 rows
constexpr int kGemvTSlices = 8; // row slices per column of the transposed product

// entry (row, row - d) of A - sigma B from the resident band(s), d >= 0 (as k_band_resid forms it)
__device__ __forceinline__ double shifted_entry(const double* __restrict__ band, const double* __restrict__ bandB, double sigma,
                                                int64_t bw, int64_t row, int64_t d)
{
    const double a = band[row * bw + d];
    if (bandB)
        return a - sigma * bandB[row * bw + d];
    return d == 0 ? a - sigma : a;
}

// D_i -> D + i s^2 (both triangles), E_i -> E + i s^2 (zero below its diagonal and for block 0), all blocks in one launch.
// Rows and columns beyond n: identity in D, zero in E.
__global__ __launch_bounds__(256) void k_bt_assemble(int64_t n, int s, double sigma, const double* __restrict__ band,
                                                     const double* __restrict__ bandB, double* __restrict__ D, double* __restrict__ E)
{
    const int64_t i = blockIdx.x;
    const int e = int(blockIdx.y) * 256 + int(threadIdx.x);
    if (e >= s * s)
        return;
    const int r = e / s, c = e - r * s;
    const int64_t bw = int64_t(s) + 1, gr = i * s + r, gc = i * s + c;
    const size_t o = size_t(i) * size_t(s) * size_t(s) + size_t(e);
    double dv;
    if (gr >= n || gc >= n)
        dv = r == c ? 1.0 : 0.0;
    else
        dv = shifted_entry(band, bandB, sigma, bw, gr > gc ? gr : gc, r > c ? r - c : c - r);
    D[o] = dv;
    double ev = 0.0;
    if (i > 0 && c >= r && gr < n)  // column (i - 1) s + c: distance s + r - c <= s
        ev = shifted_entry(band, bandB, sigma, bw, gr, int64_t(s) + r - c);
    E[o] = ev;
}

// NT == false:  C = A B      for upper triangular A (A(r, k) = 0 for k < r): L_i = E_i S_{i-1}^{-1}
// NT == true:   C -= A B'    for upper triangular B (B(c, k) = 0 for k < c), lower triangle computed and mirrored: S_i = D_i - L_i E_i'
// s x s row-major blocks, 64 x 64 tiles of 4 x 4 entries per thread, k ascending from the tile's first nonzero column.
template <bool NT>
__global__ __launch_bounds__(256) void k_bt_gemm(int s, const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ C)
{
    __shared__ double As[kTileK][kTile + 4], Bs[kTileK][kTile + 4];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int r0 = int(blockIdx.y) * kTile, c0 = int(blockIdx.x) * kTile;
    if (NT && r0 < c0)
        return;
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++)
            acc[i][j] = 0.0;
    for (int k0 = NT ? c0 : r0; k0 < s; k0 += kTileK)
    {
#pragma unroll
        for (int j = 0; j < 4; j++)
        {
            const int e = t + j * 256;
            const int kk = e & 15, rr = e >> 4;
            const int gk = k0 + kk;
            As[kk][rr] = (r0 + rr < s && gk < s) ? A[size_t(r0 + rr) * s + gk] : 0.0;
            if (NT)
                Bs[kk][rr] = (c0 + rr < s && gk < s) ? B[size_t(c0 + rr) * s + gk] : 0.0;
            else
            {
                const int cc = e & 63, kb = e >> 6;
                Bs[kb][cc] = (k0 + kb < s && c0 + cc < s) ? B[size_t(k0 + kb) * s + c0 + cc] : 0.0;
            }
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kTileK; kk++)
        {
            double a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; i++)
            {
                a[i] = As[kk][ty * 4 + i];
                b[i] = Bs[kk][tx * 4 + i];
            }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[i][j] = fma(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++)
        {
            const int r = r0 + ty * 4 + i, c = c0 + tx * 4 + j;
            if (r >= s || c >= s)
                continue;
            if (!NT)
                C[size_t(r) * s + c] = acc[i][j];
            else if (r >= c)
            {
                const double v = C[size_t(r) * s + c] - acc[i][j];
                C[size_t(r) * s + c] = v;
                if (r > c)
                    C[size_t(c) * s + r] = v;  // exactly symmetric: the upper triangle is a copy
            }
        }
}

// In-place inverse of one s x s row-major block by Gauss-Jordan elimination with partial (row) pivoting: one workgroup, the block
// stays in the XCD's L2 between the s steps.  tx_n >= s threads span a row, kInvThreads / tx_n rows are updated at a time.
// record[0] counts pivot columns that are exactly zero (or not finite), record[1] keeps the bits of the smallest |pivot| / max |A|
// over the first `valid` steps (the rest are the identity rows that pad the last block).
__global__ __launch_bounds__(kInvThreads) void k_bt_inverse(int s, int valid, int tx_n, double* __restrict__ A,
                                                            unsigned long long* __restrict__ record)
{
    __shared__ double prow[kMaxBlockBandwidth], fcol[kMaxBlockBandwidth];
    __shared__ int pivots[kMaxBlockBandwidth];
    __shared__ double red_v[kInvThreads / 64];
    __shared__ int red_i[kInvThreads / 64];
    __shared__ double s_val;
    __shared__ int s_idx;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tx = t % tx_n, ty = t / tx_n, ty_n = kInvThreads / tx_n;

    // scale of the block: max |A|
    double m = 0.0;
    for (int e = t; e < s * s; e += kInvThreads)
        m = fmax(m, fabs(A[e]));
    for (int o = 32; o >= 1; o >>= 1)
        m = fmax(m, __shfl_xor(m, o));
    if (lane == 0)
        red_v[wave] = m;
    __syncthreads();
    if (t == 0)
    {
        double v = red_v[0];
        for (int q = 1; q < kInvThreads / 64; q++)
            v = fmax(v, red_v[q]);
        s_val = v;
    }
    __syncthreads();
    const double scale = s_val;
    double min_ratio = 1.0;  // thread 0
    int zero_pivots = 0;     // thread 0

    for (int k = 0; k < s; k++)
    {
        // the largest |A(r, k)|, r >= k; the smallest row among equals
        double bv = -1.0;
        int bi = s;
        if (k + t < s)
        {
            const double v = fabs(A[size_t(k + t) * s + k]);
            if (v > bv)  // a NaN is never chosen
            {
                bv = v;
                bi = k + t;
            }
        }
        for (int o = 32; o >= 1; o >>= 1)
        {
            const double ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (ov > bv || (ov == bv && oi < bi))
            {
                bv = ov;
                bi = oi;
            }
        }
        __syncthreads();  // the previous step's reads of red_* and s_* are done
        if (lane == 0)
        {
            red_v[wave] = bv;
            red_i[wave] = bi;
        }
        __syncthreads();
        if (t == 0)
        {
            double v = red_v[0];
            int p = red_i[0];
            for (int q = 1; q < kInvThreads / 64; q++)
                if (red_v[q] > v || (red_v[q] == v && red_i[q] < p))
                {
                    v = red_v[q];
                    p = red_i[q];
                }
            if (!(v > 0.0) || !(v <= 1.7976931348623157e308))
            {
                zero_pivots++;
                p = -1;  // no row exchange, the step divides by 1
            }
            else if (scale > 0.0 && k < valid)
                min_ratio = fmin(min_ratio, v / scale);
            s_idx = p;
            pivots[k] = p < 0 ? k : p;
        }
        __syncthreads();
        const bool singular = s_idx < 0;
        const int p = singular ? k : s_idx;
        // exchange rows k and p; the pivot row goes through registers
        double rp = 0.0;
        if (t < s)
        {
            rp = A[size_t(p) * s + t];
            if (p != k)
                A[size_t(p) * s + t] = A[size_t(k) * s + t];
            if (t == k)
                s_val = singular ? 1.0 : rp;
        }
        __syncthreads();
        if (t < s)
        {
            const double pr = (t == k ? 1.0 : rp) / s_val;
            prow[t] = pr;
            fcol[t] = t == k ? 0.0 : A[size_t(t) * s + k];
            A[size_t(k) * s + t] = pr;
        }
        __syncthreads();
        if (tx < s && ty < ty_n)
        {
            const double pc = prow[tx];
            for (int r = ty; r < s; r += ty_n)
                if (r != k)
                {
                    const double a = tx == k ? 0.0 : A[size_t(r) * s + tx];
                    A[size_t(r) * s + tx] = fma(-fcol[r], pc, a);
                }
        }
        __syncthreads();
    }
    // (P A)^{-1} is in place: A^{-1} = (P A)^{-1} P, the column exchanges in reverse order
    for (int k = s - 1; k >= 0; k--)
    {
        const int p = pivots[k];
        if (p != k)
        {
            if (t < s)
            {
                const double a = A[size_t(t) * s + k];
                A[size_t(t) * s + k] = A[size_t(t) * s + p];
                A[size_t(t) * s + p] = a;
            }
            __syncthreads();
        }
    }
    if (t == 0)
    {
        if (zero_pivots)
            atomicAdd(&record[0], (unsigned long long) zero_pivots);
        atomicMin(&record[1], (unsigned long long) __double_as_longlong(min_ratio));
    }
}

// out_b[r] = (SUB ? out_b[r] : 0) -/+ sum_c M_b(r, c) in_b[c] for the blocks b = blockIdx.x: M_b = M + b mstride (s x s row-major),
// in_b = in + b vstride, out_b = out + b vstride.  One wave per 4 rows; a lane adds its columns c = lane, lane + 64, ... in
// ascending order, then the 64 partial sums meet in a fixed butterfly.
template <bool SUB>
__global__ __launch_bounds__(64 * kGemvRows / 4) void k_bt_gemv(int s, const double* __restrict__ M, size_t mstride,
                                                                 const double* __restrict__ in, double* __restrict__ out, size_t vstride)
{
    __shared__ double xs[kMaxBlockBandwidth];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const double* Mb = M + size_t(blockIdx.x) * mstride;
    const double* inb = in + size_t(blockIdx.x) * vstride;
    double* outb = out + size_t(blockIdx.x) * vstride;
    for (int c = t; c < s; c += 64 * kGemvRows / 4)
        xs[c] = inb[c];
    __syncthreads();
    const int row0 = int(blockIdx.y) * kGemvRows + wave * 4;
    if (row0 >= s)
        return;
    const double* rowp[4];
    double acc[4];
#pragma unroll
    for (int q = 0; q < 4; q++)
    {
        rowp[q] = Mb + size_t(row0 + q < s ? row0 + q : s - 1) * s;
        acc[q] = 0.0;
    }
    for (int c = lane; c < s; c += 64)
    {
        const double x = xs[c];
#pragma unroll
        for (int q = 0; q < 4; q++)
            acc[q] = fma(rowp[q][c], x, acc[q]);
    }
#pragma unroll
    for (int q = 0; q < 4; q++)
        for (int o = 32; o >= 1; o >>= 1)
            acc[q] += __shfl_xor(acc[q], o);
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (row0 + q < s)
                outb[row0 + q] = SUB ? outb[row0 + q] - acc[q] : acc[q];
}

// out[c] -= sum_r M(r, c) in[r]: the transposed product of the backward chain.  A workgroup takes 64 columns; the rows are cut
// into kGemvTSlices contiguous slices, each summed in ascending order by one wave, and the slices are added in their order.
__global__ __launch_bounds__(64 * kGemvTSlices) void k_bt_gemv_t(int s, const double* __restrict__ M, const double* __restrict__ in,
                                                                 double* __restrict__ out)
{
    __shared__ double xs[kMaxBlockBandwidth];
    __shared__ double part[kGemvTSlices][64];
    const int t = threadIdx.x, lane = t & 63, q = t >> 6;
    for (int r = t; r < s; r += 64 * kGemvTSlices)
        xs[r] = in[r];
    __syncthreads();
    const int c = int(blockIdx.x) * 64 + lane;
    const int per = (s + kGemvTSlices - 1) / kGemvTSlices;
    const int r0 = q * per, r1 = r0 + per < s ? r0 + per : s;
    double acc = 0.0;
    if (c < s)
        for (int r = r0; r < r1; r++)
            acc = fma(M[size_t(r) * s + c], xs[r], acc);
    part[q][lane] = acc;
    __syncthreads();
    if (q == 0 && c < s)
    {
        double v = part[0][lane];
        for (int j = 1; j < kGemvTSlices; j++)
            v += part[j][lane];
        out[c] -= v;
    }
}

// dst[j] = src[j] for j < n, 0 for n <= j < total
__global__ __launch_bounds__(256) void k_bt_pad(int64_t n, int64_t total, const double* __restrict__ src, double* __restrict__ dst)
{
    const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (j < total)
        dst[j] = j < n ? src[j] : 0.0;
}

inline dim3 blocks_of(int64_t count, int per) { return dim3(unsigned((count + per - 1) / per)); }

}  // namespace

double blocktri_factor(mispec_symshift& S, double sigma)
{
    const int64_t n = S.n;
    const int s = S.band_b;
    MISPEC_REQUIRE(s >= 1 && s <= kMaxBlockBandwidth && S.band0_dev.p && (!S.pencil || S.bandB0_dev.p),
                   "internal: the block-tridiagonal path needs a resident band of half-bandwidth <= 512");
    const int64_t N = (n + s - 1) / s;
    const size_t ss = size_t(s) * size_t(s);
    hipStream_t st = S.ctx->stream;
    if (!S.blocktri)
    {
        auto F = std::make_unique<BlockTri>();
        F->s = s;
        F->N = N;
        // the whole footprint against the free device memory, before the first allocation
        const size_t need = F->factor_bytes() + (ss + 2 * size_t(N) * size_t(s)) * sizeof(double) + 2 * sizeof(unsigned long long);
        size_t free_bytes = 0, total_bytes = 0;
        MISPEC_HIP(hipMemGetInfo(&free_bytes, &total_bytes));
        if (need > free_bytes)
            throw Error(MISPEC_ERUNTIME, "SparseSymShiftSolve: out of memory: the block-tridiagonal factor of n = " + std::to_string(n) +
                                             ", half-bandwidth " + std::to_string(s) + " needs " + std::to_string(need) +
                                             " bytes of device memory, " + std::to_string(free_bytes) + " are free");
        F->sinv.alloc(size_t(N) * ss);
        F->l.alloc(size_t(N) * ss);
        F->w.alloc(ss);
        F->y.alloc(size_t(N) * size_t(s));
        F->z.alloc(size_t(N) * size_t(s));
        F->record.alloc(2);
        S.blocktri = std::move(F);
    }
    BlockTri& F = *S.blocktri;
    const double one = 1.0;
    unsigned long long rec[2] = {0ull, 0ull};
    std::memcpy(&rec[1], &one, sizeof(double));
    MISPEC_HIP(hipMemcpyAsync(F.record.p, rec, sizeof(rec), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_bt_assemble, dim3(unsigned(N), unsigned((ss + 255) / 256)), dim3(256), 0, st, n, s, sigma, S.band0_dev.p,
                       S.pencil ? S.bandB0_dev.p : nullptr, F.sinv.p, F.l.p);
    MISPEC_HIP(hipGetLastError());
    const int tx_n = int(round_up(s, 64));
    const dim3 tiles(unsigned((s + kTile - 1) / kTile), unsigned((s + kTile - 1) / kTile));
    for (int64_t i = 0; i < N; i++)
    {
        double* Si = F.sinv.p + size_t(i) * ss;
        if (i > 0)
        {
            double* Ei = F.l.p + size_t(i) * ss;
            hipLaunchKernelGGL(k_bt_gemm<false>, tiles, dim3(256), 0, st, s, Ei, Si - ss, F.w.p);  // L_i = E_i S_{i-1}^{-1}
            hipLaunchKernelGGL(k_bt_gemm<true>, tiles, dim3(256), 0, st, s, F.w.p, Ei, Si);        // S_i = D_i - L_i E_i'
            MISPEC_HIP(hipMemcpyAsync(Ei, F.w.p, ss * sizeof(double), hipMemcpyDeviceToDevice, st));
        }
        hipLaunchKernelGGL(k_bt_inverse, dim3(1), dim3(kInvThreads), 0, st, s, int(std::min<int64_t>(s, n - i * s)), tx_n, Si, F.record.p);
    }
    MISPEC_HIP(hipGetLastError());
    // the one host read of the chain
    MISPEC_HIP(hipMemcpyAsync(rec, F.record.p, sizeof(rec), hipMemcpyDeviceToHost, st));
    MISPEC_HIP(hipStreamSynchronize(st));
    if (rec[0] != 0)
        throw Error(MISPEC_EINVAL, "SparseSymShiftSolve: factorization failed with the given shift (" + std::to_string(rec[0]) +
                                       " pivot columns of the block-tridiagonal factorisation are exactly zero)");
    double ratio;
    std::memcpy(&ratio, &rec[1], sizeof(double));
    return ratio;
}

void blocktri_solve(const mispec_symshift& S, const double* x_dev, double* y_dev)
{
    const BlockTri& F = *S.blocktri;
    const int s = int(F.s);
    const int64_t N = F.N, total = N * s;
    const size_t ss = size_t(s) * size_t(s);
    hipStream_t st = S.ctx->stream;
    const dim3 wg(64 * kGemvRows / 4);
    const unsigned row_groups = unsigned((s + kGemvRows - 1) / kGemvRows);
    hipLaunchKernelGGL(k_bt_pad, blocks_of(total, 256), dim3(256), 0, st, S.n, total, x_dev, F.y.p);
    for (int64_t i = 1; i < N; i++)  // y_i = x_i - L_i y_{i-1}
        hipLaunchKernelGGL(k_bt_gemv<true>, dim3(1, row_groups), wg, 0, st, s, F.l.p + size_t(i) * ss, size_t(0), F.y.p + (i - 1) * s,
                           F.y.p + i * s, size_t(0));
    hipLaunchKernelGGL(k_bt_gemv<false>, dim3(unsigned(N), row_groups), wg, 0, st, s, F.sinv.p, ss, F.y.p, F.z.p, size_t(s));
    for (int64_t i = N - 2; i >= 0; i--)  // w_i = z_i - L_{i+1}' w_{i+1}
        hipLaunchKernelGGL(k_bt_gemv_t, dim3(unsigned((s + 63) / 64)), dim3(64 * kGemvTSlices), 0, st, s, F.l.p + size_t(i + 1) * ss,
                           F.z.p + (i + 1) * s, F.z.p + i * s);
    hipLaunchKernelGGL(k_bt_pad, blocks_of(S.n, 256), dim3(256), 0, st, S.n, S.n, F.z.p, y_dev);
    MISPEC_HIP(hipGetLastError());
}

}  // namespace mispec
