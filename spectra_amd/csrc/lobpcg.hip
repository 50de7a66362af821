// LOBPCG on the device (replaces contrib/LOBPCGSolver.h of the reference): the HIP backend of lobpcg_flow.hpp, its three block
// kernels and the C ABI (include/mispec_extras.h, mispec_lobpcg_*; include/mispec_lobpcg_pre.h for the solver preconditioner).
//
// What stays in HBM: S = [X | R | P], its images AS and BS (two buffers each, n x 3m), the constraints Y and BY, 1 / diag(A).  What the
// host does: see lobpcg_flow.hpp.  Products with A, B and the sparse preconditioner are block products (launch_spmm); the combinations
// X+ = S C and the CholQR updates are launch_vq on one <= 64-column panel.  New here, because no existing kernel does them as a block:
//   k_gram          G = U'W for two tall blocks of <= 64 columns (two stages, fixed summation order, no atomics)
//   k_lobpcg_resid  R = (AX - BX diag(lambda))[:, active] (* 1 / diag A) and |AX_j - lambda_j BX_j|^2 of every column in one pass
//   k_block_sub     Z -= Y C, the constraint projection
#include <cstring>
#include <memory>

#include "csr.hpp"
#include "csr_diag.hpp"
#include "device_helpers.hpp"
#include "krylov.hpp"
#include "lobpcg_flow.hpp"
#include "shiftsolve.hpp"
#include "../../include/mispec_lobpcg_pre.h"

using namespace mispec;

namespace {

constexpr int kThreads = 256;

// ---- k_gram.  A workgroup walks a contiguous chunk of row tiles; a tile (kGramTileRows rows of every column of U and W) is staged in
// LDS column by column, and thread (ti, tj) of the 16 x 16 grid keeps the register block G(ti + 16 a, tj + 16 b), a < PA, b < QB: per
// pair of rows PA + QB 16-byte LDS reads feed 2 PA QB FMAs.  Rows beyond n are staged as zeros (never read from memory), columns
// beyond p / q as zeros.  The workgroup's sums go to its record; k_gram_sum adds the records in a fixed order.
constexpr int kGramTileRows = 32;
constexpr int kGramTileLd = 34;      // doubles per staged column: 16-byte aligned, and 16 columns apart fall into distinct LDS banks
constexpr int kGramSlot = 16;        // columns per register slot
constexpr int kGramMaxGroups = 512;  // workgroups (= partial records) of a launch
constexpr int kGramRecord = 64 * 64;

__device__ __forceinline__ void gram_stage(double* __restrict__ lds, const double* __restrict__ U, int64_t ldu, int p, int slots, int64_t row0,
                                           int64_t n, int vec)
{
    for (int item = threadIdx.x; item < slots * kGramSlot * (kGramTileRows / 2); item += kThreads)
    {
        const int c = item / (kGramTileRows / 2), rp = item % (kGramTileRows / 2);
        const int64_t row = row0 + 2 * rp;
        double2 v = make_double2(0.0, 0.0);
        if (c < p && row < n)
        {
            const double* src = U + int64_t(c) * ldu + row;
            if (vec && row + 1 < n)
                v = *reinterpret_cast<const double2*>(src);
            else
            {
                v.x = src[0];
                if (row + 1 < n)
                    v.y = src[1];
            }
        }
        *reinterpret_cast<double2*>(lds + c * kGramTileLd + 2 * rp) = v;
    }
}

template <int PA, int QB, bool SYM>
__global__ __launch_bounds__(kThreads) void k_gram(const double* __restrict__ U, int64_t ldu, int p, const double* __restrict__ W, int64_t ldw,
                                                   int q, int64_t n, int64_t ntiles, int tiles_per_group, int same, int vec,
                                                   double* __restrict__ partials)
{
    __shared__ __attribute__((aligned(16))) double su[PA * kGramSlot * kGramTileLd];
    __shared__ __attribute__((aligned(16))) double sw[QB * kGramSlot * kGramTileLd];
    const double* swr = same ? su : sw;
    const int ti = threadIdx.x % kGramSlot, tj = threadIdx.x / kGramSlot;
    double acc[PA][QB];
#pragma unroll
    for (int a = 0; a < PA; a++)
#pragma unroll
        for (int b = 0; b < QB; b++)
            acc[a][b] = 0.0;
    const int64_t t0 = int64_t(blockIdx.x) * tiles_per_group;
    const int64_t t1 = t0 + tiles_per_group < ntiles ? t0 + tiles_per_group : ntiles;
    for (int64_t t = t0; t < t1; t++)
    {
        __syncthreads();
        gram_stage(su, U, ldu, p, PA, t * kGramTileRows, n, vec);
        if (!same)
            gram_stage(sw, W, ldw, q, QB, t * kGramTileRows, n, vec);
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < kGramTileRows; r += 2)
        {
            double2 u[PA], w[QB];
#pragma unroll
            for (int a = 0; a < PA; a++)
                u[a] = *reinterpret_cast<const double2*>(su + (ti + kGramSlot * a) * kGramTileLd + r);
#pragma unroll
            for (int b = 0; b < QB; b++)
                w[b] = *reinterpret_cast<const double2*>(swr + (tj + kGramSlot * b) * kGramTileLd + r);
#pragma unroll
            for (int a = 0; a < PA; a++)
#pragma unroll
                for (int b = 0; b < QB; b++)
                    if (!SYM || a <= b)
                    {
                        acc[a][b] = fma(u[a].x, w[b].x, acc[a][b]);
                        acc[a][b] = fma(u[a].y, w[b].y, acc[a][b]);
                    }
        }
    }
    double* rec = partials + size_t(blockIdx.x) * kGramRecord;
#pragma unroll
    for (int a = 0; a < PA; a++)
#pragma unroll
        for (int b = 0; b < QB; b++)
        {
            const int i = ti + kGramSlot * a, j = tj + kGramSlot * b;
            if ((!SYM || a <= b) && i < p && j < q)
                rec[j * 64 + i] = acc[a][b];
        }
}

// G[j * p + i] = sum over the records, in four runs of consecutive records that are added as (r0 + r1) + (r2 + r3).  With sym the
// 16 x 16 blocks below the diagonal were not computed: they are left to the launcher's mirroring.
__global__ __launch_bounds__(kThreads) void k_gram_sum(const double* __restrict__ partials, int nrec, int p, int q, int sym, double* __restrict__ G)
{
    __shared__ double part[4][64];
    const int lane = threadIdx.x % 64, run = threadIdx.x / 64;
    const int o = blockIdx.x * 64 + lane;
    const int per = (nrec + 3) / 4;
    double s = 0.0;
    const bool live = o < p * q && !(sym && (o % p) / kGramSlot > (o / p) / kGramSlot);
    if (live)
    {
        const int i = o % p, j = o / p;
        const int k1 = (run + 1) * per < nrec ? (run + 1) * per : nrec;
        for (int k = run * per; k < k1; k++)
            s += partials[size_t(k) * kGramRecord + j * 64 + i];
    }
    part[run][lane] = s;
    __syncthreads();
    if (run == 0 && o < p * q)
        G[o] = live ? (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]) : 0.0;
}

// ---- k_lobpcg_resid.  Two rows per thread and step (16-byte loads and stores), every column of AX and BX read once.  The residual is
// formed WITHOUT a fused multiply-add, r = fl(ax - fl(lambda bx)), and the Jacobi scaling is one more rounding, fl(r dinv): the test pins
// these bits.  The norms are of the unscaled residual; per-workgroup sums go to records that k_resid_sum adds in a fixed order.
constexpr int kResidMaxGroups = 1024;
struct ResidArgs
{
    double lambda[kLobpcgMaxBlock];
    int pos[kLobpcgMaxBlock];  // column of R that takes the residual of column j, -1: not active
};

// fl(ax - fl(lambda bx)): two roundings, never contracted into a fused multiply-add
__device__ __forceinline__ double resid_entry(double ax, double lam, double bx)
{
#pragma clang fp contract(off)
    const double t = lam * bx;
    return ax - t;
}

__global__ __launch_bounds__(kThreads) void k_lobpcg_resid(const double* __restrict__ AX, const double* __restrict__ BX, int64_t ld, int m, int64_t n,
                                                           ResidArgs args, const double* __restrict__ dinv, double* __restrict__ R, int64_t ldr,
                                                           int64_t pairs_per_group, int vec, double* __restrict__ partials)
{
    __shared__ double wsum[kThreads / 64][kLobpcgMaxBlock];
    double acc[kLobpcgMaxBlock];
#pragma unroll
    for (int j = 0; j < kLobpcgMaxBlock; j++)
        acc[j] = 0.0;
    const int64_t npairs = (n + 1) / 2;
    const int64_t p0 = int64_t(blockIdx.x) * pairs_per_group;
    const int64_t p1 = p0 + pairs_per_group < npairs ? p0 + pairs_per_group : npairs;
    for (int64_t pr = p0 + threadIdx.x; pr < p1; pr += kThreads)
    {
        const int64_t row = 2 * pr;
        const bool two = row + 1 < n;
        double2 d = make_double2(1.0, 1.0);
        if (dinv)
        {
            if (vec && two)
                d = *reinterpret_cast<const double2*>(dinv + row);
            else
            {
                d.x = dinv[row];
                if (two)
                    d.y = dinv[row + 1];
            }
        }
#pragma unroll
        for (int j = 0; j < kLobpcgMaxBlock; j++)
            if (j < m)
            {
                const double* a = AX + int64_t(j) * ld + row;
                const double* b = BX + int64_t(j) * ld + row;
                double2 av = make_double2(0.0, 0.0), bv = make_double2(0.0, 0.0);
                if (vec && two)
                {
                    av = *reinterpret_cast<const double2*>(a);
                    bv = *reinterpret_cast<const double2*>(b);
                }
                else
                {
                    av.x = a[0];
                    bv.x = b[0];
                    if (two)
                    {
                        av.y = a[1];
                        bv.y = b[1];
                    }
                }
                const double lam = args.lambda[j];
                double2 r;
                r.x = resid_entry(av.x, lam, bv.x);
                r.y = resid_entry(av.y, lam, bv.y);
                acc[j] = fma(r.x, r.x, acc[j]);
                acc[j] = fma(r.y, r.y, acc[j]);
                const int k = args.pos[j];
                if (k >= 0)
                {
                    if (dinv)
                    {
                        r.x *= d.x;
                        r.y *= d.y;
                    }
                    double* dst = R + int64_t(k) * ldr + row;
                    if (vec && two)
                        *reinterpret_cast<double2*>(dst) = r;
                    else
                    {
                        dst[0] = r.x;
                        if (two)
                            dst[1] = r.y;
                    }
                }
            }
    }
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
#pragma unroll
    for (int j = 0; j < kLobpcgMaxBlock; j++)
        if (j < m)
        {
            const double v = wave_reduce_sum(acc[j]);
            if (lane == 0)
                wsum[wave][j] = v;
        }
    __syncthreads();
    if (int(threadIdx.x) < m)
        partials[size_t(blockIdx.x) * kLobpcgMaxBlock + threadIdx.x] =
            (wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + (wsum[2][threadIdx.x] + wsum[3][threadIdx.x]);
}

// out[j] = sum of column j of the records: thread t adds records t, t + 256, ... in order, then a fixed tree over the threads
__global__ __launch_bounds__(kThreads) void k_resid_sum(const double* __restrict__ partials, int nrec, double* __restrict__ out)
{
    __shared__ double s[kThreads];
    const int j = blockIdx.x;
    double v = 0.0;
    for (int k = threadIdx.x; k < nrec; k += kThreads)
        v += partials[size_t(k) * kLobpcgMaxBlock + j];
    s[threadIdx.x] = v;
    __syncthreads();
    for (int half = kThreads / 2; half > 0; half >>= 1)
    {
        if (int(threadIdx.x) < half)
            s[threadIdx.x] += s[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        out[j] = s[0];
}

// ---- k_block_sub: Z[:, j] -= Y C[:, j], one row per thread, the row of Y in registers, one FMA per term (c roundings per entry).
// C is c x q with leading dimension kLobpcgMaxBlock in device memory: the unrolled loops read it at addresses the compiler knows.
__global__ __launch_bounds__(kThreads) void k_block_sub(double* __restrict__ Z, int64_t ldz, int q, const double* __restrict__ Y, int64_t ldy, int c,
                                                        const double* __restrict__ C, int64_t n)
{
    const int64_t row = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (row >= n)
        return;
    double y[kLobpcgMaxBlock];
#pragma unroll
    for (int k = 0; k < kLobpcgMaxBlock; k++)
        y[k] = k < c ? Y[int64_t(k) * ldy + row] : 0.0;
#pragma unroll
    for (int j = 0; j < kLobpcgMaxBlock; j++)
        if (j < q)
        {
            double z = Z[int64_t(j) * ldz + row];
#pragma unroll
            for (int k = 0; k < kLobpcgMaxBlock; k++)
                if (k < c)
                    z = fma(-y[k], C[j * kLobpcgMaxBlock + k], z);
            Z[int64_t(j) * ldz + row] = z;
        }
}

__global__ __launch_bounds__(kThreads) void k_reciprocal(const double* __restrict__ d, int64_t n, double* __restrict__ out)
{
    const int64_t r = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (r < n)
        out[r] = 1.0 / d[r];
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Device scratch of the three kernels: partial records, the small results, the coefficient matrices of V*Q and k_block_sub.
struct LobpcgWork
{
    const mispec_ctx* ctx = nullptr;
    DevBuf<double> gram_partials, gram_out, resid_partials, resid_out, coef, q_dev;
    PinnedBuf<double> h_out;
    std::vector<double> q_last;  // what q_dev holds
    int q_ld = 0, q_cols = 0;

    explicit LobpcgWork(const mispec_ctx* c) : ctx(c)
    {
        gram_partials.alloc(size_t(kGramMaxGroups) * kGramRecord);
        gram_out.alloc(kGramRecord);
        resid_partials.alloc(size_t(kResidMaxGroups) * kLobpcgMaxBlock);
        resid_out.alloc(kLobpcgMaxBlock);
        coef.alloc(size_t(kLobpcgMaxBlock) * kLobpcgMaxBlock);
        q_dev.alloc(kGramRecord);
        h_out.alloc(kGramRecord);
    }

    // both stages, enqueued: gram_out holds G afterwards
    void gram_enqueue(const double* U, int64_t ldu, int p, const double* W, int64_t ldw, int q, int64_t n, bool symmetric)
    {
        MISPEC_REQUIRE(U && W && p >= 1 && p <= 64 && q >= 1 && q <= 64 && n >= 1 && ldu >= n && ldw >= n,
                       "Gram kernel: needs 1 <= p, q <= 64 columns, n >= 1 rows and leading dimensions >= n");
        MISPEC_REQUIRE(!symmetric || p == q, "Gram kernel: the symmetric form needs p == q");
        const int64_t ntiles = (n + kGramTileRows - 1) / kGramTileRows;
        const int64_t want = std::min<int64_t>(ntiles, kGramMaxGroups);
        const int tiles_per_group = int((ntiles + want - 1) / want);
        const int groups = int((ntiles + tiles_per_group - 1) / tiles_per_group);
        const int same = (U == W && ldu == ldw && p == q) ? 1 : 0;
        const int vec = (aligned16(U) && aligned16(W) && ldu % 2 == 0 && ldw % 2 == 0) ? 1 : 0;
        const int PA = (p + kGramSlot - 1) / kGramSlot, QB = (q + kGramSlot - 1) / kGramSlot;
        hipStream_t st = ctx->stream;
        const dim3 g(static_cast<unsigned>(groups)), b(kThreads);
#define MISPEC_GRAM(A_, B_)                                                                                                        \
    do                                                                                                                             \
    {                                                                                                                              \
        if (symmetric)                                                                                                             \
            hipLaunchKernelGGL((k_gram<A_, B_, true>), g, b, 0, st, U, ldu, p, W, ldw, q, n, ntiles, tiles_per_group, same, vec,   \
                               gram_partials.p);                                                                                   \
        else                                                                                                                       \
            hipLaunchKernelGGL((k_gram<A_, B_, false>), g, b, 0, st, U, ldu, p, W, ldw, q, n, ntiles, tiles_per_group, same, vec,  \
                               gram_partials.p);                                                                                   \
    } while (0)
#define MISPEC_GRAM_ROW(A_)  \
    switch (QB)              \
    {                        \
    case 1:                  \
        MISPEC_GRAM(A_, 1);  \
        break;               \
    case 2:                  \
        MISPEC_GRAM(A_, 2);  \
        break;               \
    case 3:                  \
        MISPEC_GRAM(A_, 3);  \
        break;               \
    default:                 \
        MISPEC_GRAM(A_, 4);  \
        break;               \
    }
        switch (PA)
        {
        case 1:
            MISPEC_GRAM_ROW(1);
            break;
        case 2:
            MISPEC_GRAM_ROW(2);
            break;
        case 3:
            MISPEC_GRAM_ROW(3);
            break;
        default:
            MISPEC_GRAM_ROW(4);
            break;
        }
#undef MISPEC_GRAM_ROW
#undef MISPEC_GRAM
        MISPEC_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_gram_sum, dim3(unsigned((p * q + 63) / 64)), b, 0, st, gram_partials.p, groups, p, q, symmetric ? 1 : 0,
                           gram_out.p);
        MISPEC_HIP(hipGetLastError());
    }

    void gram(const double* U, int64_t ldu, int p, const double* W, int64_t ldw, int q, int64_t n, bool symmetric, double* G_host)
    {
        MISPEC_REQUIRE(G_host, "Gram kernel: NULL result");
        gram_enqueue(U, ldu, p, W, ldw, q, n, symmetric);
        hipStream_t st = ctx->stream;
        MISPEC_HIP(hipMemcpyAsync(h_out.p, gram_out.p, size_t(p) * q * sizeof(double), hipMemcpyDeviceToHost, st));
        MISPEC_HIP(hipStreamSynchronize(st));
        for (int j = 0; j < q; j++)
            for (int i = 0; i < p; i++)
                G_host[size_t(j) * p + i] = (symmetric && i > j) ? h_out.p[size_t(i) * p + j] : h_out.p[size_t(j) * p + i];
    }

    // both stages, enqueued: resid_out holds the m sums afterwards
    void resid_enqueue(const double* AX, const double* BX, int64_t ld, int m, int64_t n, const double* lambda, const int* idx, int a,
                       const double* dinv, double* R, int64_t ldr)
    {
        MISPEC_REQUIRE(AX && BX && lambda && m >= 1 && m <= kLobpcgMaxBlock && n >= 1 && ld >= n && a >= 0 && a <= m,
                       "residual kernel: needs 1 <= m <= 21 columns, n >= 1 rows, a leading dimension >= n and 0 <= a <= m");
        MISPEC_REQUIRE(a == 0 || (idx && R && ldr >= n), "residual kernel: active columns need their list and an output block");
        ResidArgs args;
        for (int j = 0; j < kLobpcgMaxBlock; j++)
        {
            args.lambda[j] = j < m ? lambda[j] : 0.0;
            args.pos[j] = -1;
        }
        for (int k = 0; k < a; k++)
        {
            MISPEC_REQUIRE(idx[k] >= 0 && idx[k] < m && args.pos[idx[k]] < 0, "residual kernel: the active list must name distinct columns");
            args.pos[idx[k]] = k;
        }
        const int64_t npairs = (n + 1) / 2;
        const int64_t want = std::min<int64_t>((npairs + kThreads - 1) / kThreads, kResidMaxGroups);
        const int64_t pairs_per_group = (npairs + want - 1) / want;
        const int groups = int((npairs + pairs_per_group - 1) / pairs_per_group);
        const int vec = (aligned16(AX) && aligned16(BX) && ld % 2 == 0 && (a == 0 || (aligned16(R) && ldr % 2 == 0)) && (!dinv || aligned16(dinv)))
                            ? 1
                            : 0;
        hipStream_t st = ctx->stream;
        hipLaunchKernelGGL(k_lobpcg_resid, dim3(unsigned(groups)), dim3(kThreads), 0, st, AX, BX, ld, m, n, args, dinv, R, ldr, pairs_per_group,
                           vec, resid_partials.p);
        MISPEC_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_resid_sum, dim3(unsigned(m)), dim3(kThreads), 0, st, resid_partials.p, groups, resid_out.p);
        MISPEC_HIP(hipGetLastError());
    }

    void resid(const double* AX, const double* BX, int64_t ld, int m, int64_t n, const double* lambda, const int* idx, int a, const double* dinv,
               double* R, int64_t ldr, double* norms2)
    {
        MISPEC_REQUIRE(norms2, "residual kernel: NULL result");
        resid_enqueue(AX, BX, ld, m, n, lambda, idx, a, dinv, R, ldr);
        hipStream_t st = ctx->stream;
        MISPEC_HIP(hipMemcpyAsync(h_out.p, resid_out.p, size_t(m) * sizeof(double), hipMemcpyDeviceToHost, st));
        MISPEC_HIP(hipStreamSynchronize(st));
        std::copy(h_out.p, h_out.p + m, norms2);
    }

    void block_sub(double* Z, int64_t ldz, int q, const double* Y, int64_t ldy, int c, const double* C_host, int64_t n)
    {
        MISPEC_REQUIRE(Z && Y && C_host && q >= 1 && q <= kLobpcgMaxBlock && c >= 1 && c <= kLobpcgMaxBlock && n >= 1 && ldz >= n && ldy >= n,
                       "block subtraction kernel: needs 1 <= q, c <= 21 columns, n >= 1 rows and leading dimensions >= n");
        double pad[kLobpcgMaxBlock * kLobpcgMaxBlock] = {};
        for (int j = 0; j < q; j++)
            for (int k = 0; k < c; k++)
                pad[j * kLobpcgMaxBlock + k] = C_host[size_t(j) * c + k];
        hipStream_t st = ctx->stream;
        MISPEC_HIP(hipMemcpyAsync(coef.p, pad, sizeof(pad), hipMemcpyHostToDevice, st));
        MISPEC_HIP(hipStreamSynchronize(st));  // pad is a local
        hipLaunchKernelGGL(k_block_sub, dim3(unsigned((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, Z, ldz, q, Y, ldy, c, coef.p, n);
        MISPEC_HIP(hipGetLastError());
    }

    // the coefficient matrix of a V*Q launch: uploaded unless it is what the device already holds
    const double* coefficients(const double* Q_host, int ldq, int cols)
    {
        const size_t count = size_t(ldq) * cols;
        MISPEC_REQUIRE(count <= size_t(kGramRecord), "V*Q coefficients: at most 64 x 64");
        if (q_ld != ldq || q_cols != cols || q_last.size() != count || std::memcmp(q_last.data(), Q_host, count * sizeof(double)) != 0)
        {
            q_last.assign(Q_host, Q_host + count);
            q_ld = ldq;
            q_cols = cols;
            MISPEC_HIP(hipMemcpyAsync(q_dev.p, q_last.data(), count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            MISPEC_HIP(hipStreamSynchronize(ctx->stream));
        }
        return q_dev.p;
    }
};

// The Backend of lobpcg_flow.hpp on the device.
struct HipBackend
{
    mispec_ctx* ctx = nullptr;
    const mispec_csr* A = nullptr;
    const mispec_csr* B = nullptr;
    const mispec_csr* T = nullptr;
    const mispec_symshift* F = nullptr;  // preconditioner given as a shift solve (replaces T)
    int64_t n = 0, ldv = 0;
    LobpcgWork work;
    DevBuf<double> dinv;

    HipBackend(mispec_ctx* c, const mispec_csr* a) : ctx(c), A(a), n(a->n_rows), ldv(round_up(std::max<int64_t>(a->n_rows, 1), 2)), work(c) {}

    int64_t ld() const { return ldv; }
    double* alloc(size_t count)
    {
        double* p = nullptr;
        MISPEC_HIP(hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(double)));
        MISPEC_HIP(hipMemsetAsync(p, 0, count * sizeof(double), ctx->stream));
        MISPEC_HIP(hipStreamSynchronize(ctx->stream));  // callers fill blocks with copies that are not ordered against this stream
        return p;
    }
    void release(double* p)
    {
        if (p)
            (void) hipFree(p);
    }
    void copy(double* dst, const double* src, size_t count)
    {
        MISPEC_HIP(hipMemcpyAsync(dst, src, count * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    }
    void random_col(double* col, uint64_t seed) { launch_simple_random(*ctx, col, 0, n, seed); }
    void apply_A(const double* X, int k, double* Y) { launch_spmm(*A, X, ldv, k, Y, ldv); }
    void apply_B(const double* X, int k, double* Y) { launch_spmm(*B, X, ldv, k, Y, ldv); }
    void apply_T(const double* X, int k, double* Y)
    {
        if (F)
            launch_shiftsolve_block(*F, X, ldv, k, Y, ldv);  // the factorisation of a nearby matrix, one pass over it per panel
        else
            launch_spmm(*T, X, ldv, k, Y, ldv);
    }
    void gram(const double* U, int p, const double* W, int q, bool symmetric, double* G) { work.gram(U, ldv, p, W, ldv, q, n, symmetric, G); }
    void vq(const double* V, int mm, const double* Q_host, int ldq, int p, double* X)
    {
        launch_vq(*ctx, V, ldv, mm, work.coefficients(Q_host, ldq, p), ldq, p, X, ldv, n);
    }
    void resid(const double* AX, const double* BX, int m, const double* lambda, const int* idx, int a, bool jacobi, double* R, double* norms2)
    {
        work.resid(AX, BX, ldv, m, n, lambda, idx, a, jacobi ? dinv.p : nullptr, R, ldv, norms2);
    }
    void block_sub(double* Z, int q, const double* Y, int c, const double* C) { work.block_sub(Z, ldv, q, Y, ldv, c, C, n); }
};

}  // namespace

struct mispec_lobpcg
{
    mispec_ctx* ctx = nullptr;
    HipBackend be;
    std::unique_ptr<LobpcgFlow<HipBackend>> flow;
    mispec_lobpcg(mispec_ctx* c, const mispec_csr* A) : ctx(c), be(c, A) {}
};

namespace {

bool whole_square(const mispec_csr* M) { return M->n_rows == M->n_cols && M->row_begin == 0 && M->row_end == M->n_rows && M->ctx->world() == 1; }

void require_operator(const mispec_lobpcg* S, const mispec_csr* M, const char* what)
{
    MISPEC_REQUIRE(M->ctx == S->ctx && whole_square(M) && M->n_rows == S->be.n, what);
}

// the context's stream is not ordered against the copy: whatever was enqueued on it (the zero fill of a new block, kernels that still
// read the old contents) is waited for first
void copy_in(const mispec_lobpcg& S, double* dev, const double* host, int64_t ld, int cols)
{
    MISPEC_HIP(hipStreamSynchronize(S.ctx->stream));
    MISPEC_HIP(hipMemcpy2D(dev, size_t(S.be.ldv) * sizeof(double), host, size_t(ld) * sizeof(double), size_t(S.be.n) * sizeof(double), size_t(cols),
                           hipMemcpyHostToDevice));
}

void copy_out(const mispec_lobpcg& S, double* host, int64_t ld, const double* dev, int cols)
{
    MISPEC_HIP(hipStreamSynchronize(S.ctx->stream));
    MISPEC_HIP(hipMemcpy2D(host, size_t(ld) * sizeof(double), dev, size_t(S.be.ldv) * sizeof(double), size_t(S.be.n) * sizeof(double), size_t(cols),
                           hipMemcpyDeviceToHost));
}

}  // namespace

extern "C" int mispec_lobpcg_create(mispec_ctx* ctx, const mispec_csr* A, int64_t m, mispec_lobpcg** out)
{
    return guarded([&] {
        MISPEC_REQUIRE(ctx && A && out, "mispec_lobpcg_create: NULL argument");
        MISPEC_REQUIRE(A->ctx == ctx && whole_square(A), "LOBPCGSolver: needs a square, unsharded matrix of this context");
        MISPEC_REQUIRE(m >= 1 && m <= kLobpcgMaxBlock, "LOBPCGSolver: the block size must satisfy 1 <= m <= 21 (3 m columns fit one 64-column panel)");
        ctx->make_current();
        auto S = std::make_unique<mispec_lobpcg>(ctx, A);
        S->flow = std::make_unique<LobpcgFlow<HipBackend>>(S->be, A->n_rows, int(m));
        *out = S.release();
    });
}

extern "C" int mispec_lobpcg_destroy(mispec_lobpcg* S)
{
    return guarded([&] {
        if (S)
        {
            S->ctx->make_current();
            (void) hipStreamSynchronize(S->ctx->stream);
            delete S;
        }
    });
}

extern "C" int mispec_lobpcg_set_B(mispec_lobpcg* S, const mispec_csr* B)
{
    return guarded([&] {
        MISPEC_REQUIRE(S, "mispec_lobpcg_set_B: NULL argument");
        if (B)
            require_operator(S, B, "LOBPCGSolver: B must be an unsharded matrix of A's shape and context");
        S->ctx->make_current();
        S->be.B = B;
        S->flow->set_B(B != nullptr);
    });
}

extern "C" int mispec_lobpcg_set_preconditioner(mispec_lobpcg* S, const mispec_csr* T)
{
    return guarded([&] {
        MISPEC_REQUIRE(S, "mispec_lobpcg_set_preconditioner: NULL argument");
        if (T)
            require_operator(S, T, "LOBPCGSolver: the preconditioner must be an unsharded matrix of A's shape and context");
        S->ctx->make_current();
        S->be.T = T;
        S->be.F = nullptr;
        S->flow->set_T(T != nullptr);
    });
}

// T = (K - sigma M)^{-1} as a factorisation held by F: applied to the active columns by launch_shiftsolve_block.  T has to be positive
// definite; a banded factorisation knows the signs of its pivots, on the dense path (n <= 4096) definiteness is the caller's duty.
extern "C" int mispec_lobpcg_set_preconditioner_solver(mispec_lobpcg* S, const mispec_symshift* F)
{
    return guarded([&] {
        MISPEC_REQUIRE(S, "mispec_lobpcg_set_preconditioner_solver: NULL argument");
        if (F)
        {
            MISPEC_REQUIRE(F->ctx == S->ctx && F->n == S->be.n, "LOBPCGSolver: the preconditioner must be a solver of A's size and context");
            MISPEC_REQUIRE(!F->general, "LOBPCGSolver: the preconditioner must be a symmetric solver");
            // deliberate limit: a truncated Krylov solve is not a fixed linear operator, and its definiteness is not known
            MISPEC_REQUIRE(F->path() != mispec::ShiftPath::iterative,
                           "LOBPCGSolver: an operator on the iterative shift-solve path cannot be the preconditioner (a truncated Krylov "
                           "solve is not a fixed linear operator); use a direct shift solve or the Jacobi preconditioner");
            MISPEC_REQUIRE(!F->factored || F->dense || F->negative_pivots == 0,
                           "LOBPCGSolver: the preconditioner must be positive definite (the factorisation met negative pivots)");
        }
        S->ctx->make_current();
        S->be.T = nullptr;
        S->be.F = F;
        S->flow->set_T(F != nullptr);
    });
}

extern "C" int mispec_lobpcg_set_jacobi(mispec_lobpcg* S, int on)
{
    return guarded([&] {
        MISPEC_REQUIRE(S, "mispec_lobpcg_set_jacobi: NULL argument");
        S->ctx->make_current();
        if (on && !S->be.dinv.p)
        {
            const mispec_csr& A = *S->be.A;
            const int64_t n = S->be.n;
            hipStream_t st = S->ctx->stream;
            const dim3 grid(unsigned((n + kCsrDiagThreads - 1) / kCsrDiagThreads));
            DevBuf<double> diag, tmp;
            diag.alloc(size_t(n) + 2);
            hipLaunchKernelGGL(k_csr_diag, grid, dim3(kCsrDiagThreads), 0, st, A.rowptr.p, A.colind.p, A.val.p, A.row_begin, n, diag.p);
            MISPEC_HIP(hipGetLastError());
            if (A.reordered())
            {
                // the stored matrix is P A P' (reorder.hip); the solver's blocks keep the caller's order, like its products
                tmp.alloc(size_t(n) + 2);
                launch_from_stored_order(A, diag.p, tmp.p);
                diag.swap(tmp);
            }
            std::vector<double> host(static_cast<size_t>(n));
            MISPEC_HIP(hipMemcpyAsync(host.data(), diag.p, size_t(n) * sizeof(double), hipMemcpyDeviceToHost, st));
            MISPEC_HIP(hipStreamSynchronize(st));
            for (double d : host)
                MISPEC_REQUIRE(d > 0.0 && std::isfinite(d), "LOBPCGSolver: the Jacobi preconditioner needs a positive diagonal of A");
            DevBuf<double> inv;
            inv.alloc(size_t(S->be.ldv));
            MISPEC_HIP(hipMemsetAsync(inv.p, 0, inv.n * sizeof(double), st));
            hipLaunchKernelGGL(k_reciprocal, grid, dim3(kThreads), 0, st, diag.p, n, inv.p);
            MISPEC_HIP(hipGetLastError());
            MISPEC_HIP(hipStreamSynchronize(st));
            S->be.dinv.swap(inv);
        }
        if (on)
            S->be.F = nullptr;  // Jacobi replaces a solver preconditioner (the flow drops T itself)
        S->flow->set_jacobi(on != 0);
    });
}

extern "C" int mispec_lobpcg_set_constraints(mispec_lobpcg* S, const double* Y_host, int64_t ld, int64_t c)
{
    return guarded([&] {
        MISPEC_REQUIRE(S && (Y_host || c == 0), "mispec_lobpcg_set_constraints: NULL argument");
        MISPEC_REQUIRE(c >= 0 && c <= kLobpcgMaxBlock && (c == 0 || ld >= S->be.n), "LOBPCGSolver: at most 21 constraint vectors, ld >= n");
        S->ctx->make_current();
        MISPEC_HIP(hipStreamSynchronize(S->ctx->stream));  // nothing enqueued may still read the old block
        double* Y = S->flow->constraints_buffer(int(c));
        if (c > 0)
            copy_in(*S, Y, Y_host, ld, int(c));
    });
}

extern "C" int mispec_lobpcg_set_initial(mispec_lobpcg* S, const double* X_host, int64_t ld)
{
    return guarded([&] {
        MISPEC_REQUIRE(S && X_host && ld >= S->be.n, "mispec_lobpcg_set_initial: NULL argument or ld < n");
        S->ctx->make_current();
        MISPEC_HIP(hipStreamSynchronize(S->ctx->stream));
        copy_in(*S, S->flow->initial_buffer(), X_host, ld, S->flow->block_size());
        S->flow->initial_set();
    });
}

extern "C" int mispec_lobpcg_compute(mispec_lobpcg* S, int selection, int64_t maxit, double tol_abs, int64_t* nconv)
{
    return guarded([&] {
        MISPEC_REQUIRE(S && nconv, "mispec_lobpcg_compute: NULL argument");
        // Util/SelectionRule.h: LargestAlge = 3, SmallestAlge = 7
        MISPEC_REQUIRE(selection == 3 || selection == 7, "LOBPCGSolver: the selection rule must be SmallestAlge or LargestAlge");
        MISPEC_REQUIRE(maxit >= 0 && tol_abs >= 0.0, "LOBPCGSolver: maxit and the tolerance cannot be negative");
        if (S->be.F)
        {
            if (!S->be.F->factored)
                throw Error(MISPEC_ELOGIC, "LOBPCGSolver: the preconditioner's set_shift() has not been called");
            // the shift may have been set again since the solver was given
            MISPEC_REQUIRE(S->be.F->dense || S->be.F->negative_pivots == 0,
                           "LOBPCGSolver: the preconditioner must be positive definite (the factorisation met negative pivots)");
        }
        S->ctx->make_current();
        *nconv = S->flow->compute(selection == 3, maxit, tol_abs);
    });
}

extern "C" int mispec_lobpcg_info(const mispec_lobpcg* S) { return S ? S->flow->info() : kLobpcgInvalidInput; }
extern "C" int64_t mispec_lobpcg_num_iterations(const mispec_lobpcg* S) { return S ? S->flow->num_iterations() : 0; }
extern "C" int64_t mispec_lobpcg_num_operations(const mispec_lobpcg* S) { return S ? S->flow->num_operations() : 0; }
extern "C" int64_t mispec_lobpcg_num_retries(const mispec_lobpcg* S) { return S ? S->flow->num_retries_without_p() : 0; }

extern "C" int mispec_lobpcg_eigenvalues(const mispec_lobpcg* S, double* out)
{
    return guarded([&] {
        MISPEC_REQUIRE(S && out, "mispec_lobpcg_eigenvalues: NULL argument");
        MISPEC_REQUIRE(S->flow->computed(), "LOBPCGSolver: compute() has not been called");
        std::copy(S->flow->eigenvalues().begin(), S->flow->eigenvalues().end(), out);
    });
}

extern "C" int mispec_lobpcg_residual_norms(const mispec_lobpcg* S, double* out)
{
    return guarded([&] {
        MISPEC_REQUIRE(S && out, "mispec_lobpcg_residual_norms: NULL argument");
        MISPEC_REQUIRE(S->flow->computed(), "LOBPCGSolver: compute() has not been called");
        std::copy(S->flow->residual_norms().begin(), S->flow->residual_norms().end(), out);
    });
}

extern "C" int mispec_lobpcg_eigenvectors(const mispec_lobpcg* S, double* out_host, int64_t ld)
{
    return guarded([&] {
        MISPEC_REQUIRE(S && out_host && ld >= S->be.n, "mispec_lobpcg_eigenvectors: NULL argument or ld < n");
        MISPEC_REQUIRE(S->flow->computed(), "LOBPCGSolver: compute() has not been called");
        S->ctx->make_current();
        copy_out(*S, out_host, ld, S->flow->vectors(), S->flow->block_size());
    });
}

extern "C" int mispec_lobpcg_residuals(const mispec_lobpcg* S, double* out_host, int64_t ld)
{
    return guarded([&] {
        MISPEC_REQUIRE(S && out_host && ld >= S->be.n, "mispec_lobpcg_residuals: NULL argument or ld < n");
        MISPEC_REQUIRE(S->flow->computed(), "LOBPCGSolver: compute() has not been called");
        S->ctx->make_current();
        copy_out(*S, out_host, ld, S->flow->residuals(), S->flow->block_size());
    });
}

// ---- the kernels alone, on device pointers (tests, the benchmark tool)
extern "C" int mispec_lobpcg_gram(mispec_ctx* ctx, const double* U_dev, int64_t ldu, int p, const double* W_dev, int64_t ldw, int q, int64_t n,
                                  int symmetric, double* G_host)
{
    return guarded([&] {
        MISPEC_REQUIRE(ctx, "mispec_lobpcg_gram: NULL context");
        ctx->make_current();
        LobpcgWork work(ctx);
        work.gram(U_dev, ldu, p, W_dev, ldw, q, n, symmetric != 0, G_host);
    });
}

extern "C" int mispec_lobpcg_resid(mispec_ctx* ctx, const double* AX_dev, const double* BX_dev, int64_t ld, int m, int64_t n,
                                   const double* lambda_host, const int* idx_host, int a, const double* dinv_dev_or_null, double* R_dev, int64_t ldr,
                                   double* norms2_host)
{
    return guarded([&] {
        MISPEC_REQUIRE(ctx, "mispec_lobpcg_resid: NULL context");
        ctx->make_current();
        LobpcgWork work(ctx);
        work.resid(AX_dev, BX_dev, ld, m, n, lambda_host, idx_host, a, dinv_dev_or_null, R_dev, ldr, norms2_host);
    });
}

extern "C" int mispec_lobpcg_block_sub(mispec_ctx* ctx, double* Z_dev, int64_t ldz, int q, const double* Y_dev, int64_t ldy, int c,
                                       const double* C_host, int64_t n)
{
    return guarded([&] {
        MISPEC_REQUIRE(ctx, "mispec_lobpcg_block_sub: NULL context");
        ctx->make_current();
        LobpcgWork work(ctx);
        work.block_sub(Z_dev, ldz, q, Y_dev, ldy, c, C_host, n);
        MISPEC_HIP(hipStreamSynchronize(ctx->stream));
    });
}

// average ms of `reps` back-to-back launches of which = 0: k_gram (both stages; p columns of U against q of W), 1: k_lobpcg_resid
// (p columns, the first q of them active, R_dev as output), 2: the combination R[:, :q] = U[:, :p] Q (launch_vq, as the Rayleigh-Ritz
// step calls it); benchmark helper, like mispec_spmm_time
extern "C" int mispec_lobpcg_kernel_time(mispec_ctx* ctx, int which, const double* U_dev, const double* W_dev, int64_t ld, int p, int q, int64_t n,
                                         double* R_dev, int reps, float* ms_per_launch)
{
    return guarded([&] {
        MISPEC_REQUIRE(ctx && ms_per_launch && reps >= 1 && which >= 0 && which <= 2, "mispec_lobpcg_kernel_time: bad argument");
        ctx->make_current();
        LobpcgWork work(ctx);
        std::vector<double> lambda(size_t(kLobpcgMaxBlock), 0.5);
        std::vector<int> idx(static_cast<size_t>(kLobpcgMaxBlock));
        for (int k = 0; k < kLobpcgMaxBlock; k++)
            idx[size_t(k)] = k;
        const double* Qdev = nullptr;
        if (which == 2)
        {
            MISPEC_REQUIRE(U_dev && R_dev && p >= 1 && p <= 64 && q >= 1 && q <= 64 && ld >= n, "mispec_lobpcg_kernel_time: V*Q needs 1 <= p, q <= 64");
            std::vector<double> Q(size_t(p) * q);
            for (size_t k = 0; k < Q.size(); k++)
                Q[k] = 1.0 / double(k + 1);
            Qdev = work.coefficients(Q.data(), p, q);
        }
        auto once = [&] {
            if (which == 0)
                work.gram_enqueue(U_dev, ld, p, W_dev, ld, q, n, p == q);
            else if (which == 2)
                launch_vq(*ctx, U_dev, ld, p, Qdev, p, q, R_dev, ld, n);
            else
                work.resid_enqueue(U_dev, W_dev, ld, p, n, lambda.data(), idx.data(), q, nullptr, R_dev, ld);
        };
        once();
        hipEvent_t e0, e1;
        MISPEC_HIP(hipEventCreate(&e0));
        MISPEC_HIP(hipEventCreate(&e1));
        MISPEC_HIP(hipEventRecord(e0, ctx->stream));
        for (int r = 0; r < reps; r++)
            once();
        MISPEC_HIP(hipEventRecord(e1, ctx->stream));
        MISPEC_HIP(hipEventSynchronize(e1));
        float ms = 0.0f;
        MISPEC_HIP(hipEventElapsedTime(&ms, e0, e1));
        (void) hipEventDestroy(e0);
        (void) hipEventDestroy(e1);
        *ms_per_launch = ms / float(reps);
    });
}
