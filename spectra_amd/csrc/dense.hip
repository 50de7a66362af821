// Dense matrices in HBM and y = M x for them (DenseSymMatProd.h:81-86, DenseGenMatProd.h:78-83 of the reference are
// `m_mat.selfadjointView<Uplo>() * x` and `m_mat * x` through Eigen).
//
// Layout: row-major, row stride rounded up to even so that every row starts on a 16-byte boundary; a symmetric input
// given by one triangle is mirrored at upload (the other triangle of the input is ignored, as selfadjointView does).
// Kernel: one wavefront per row.  A lane streams 16-byte pieces of the row (four in flight), x comes from the L2
// (it is read by every row), a shuffle tree finishes the dot product.  Bound: HBM, 8 bytes per matrix entry.
#include "dense.hpp"
#include "device_helpers.hpp"

#include <cstring>
#include <memory>
#include <vector>

using namespace mispec;

namespace {

constexpr int kGemvThreads = 256;  // four rows per workgroup
constexpr int64_t kSerialGemvEntries = 128 * 128;  // up to this many entries: storage-order row sums (k_row_gemv_serial)

// Small matrices: one lane per row, the row summed in STORAGE ORDER with the product rounded before it is added — the order
// of a plain CPU row-dot and of the sparse kernels (csr.hip), whose results this kernel therefore reproduces bit for bit on
// the same entries (an entry that is 0 adds +-0).  The wavefront tree of k_row_gemv rounds differently, which is harmless except
// where a test of the reference sits exactly on a rounding boundary: test/Example1.cpp (20, 5, 12) exhausts its Krylov space
// and the surviving noise (1e-15) lands on either side of the breakdown clamp (Lanczos.h:163-168) depending on that order.
// A launch this small is latency-bound either way.
__global__ __launch_bounds__(64) void k_row_gemv_serial(int64_t rows, int64_t cols, int64_t ld, const double* __restrict__ M,
                                                         const double* __restrict__ x, double* __restrict__ y)
{
#pragma clang fp contract(off)
    const int64_t r = int64_t(blockIdx.x) * 64 + threadIdx.x;
    if (r >= rows)
        return;
    const double* a = M + r * ld;
    double acc = 0.0;
    for (int64_t c = 0; c < cols; c++)
        acc += a[c] * x[c];
    y[r] = acc;
}

// One wavefront per row, for a panel of K vectors (the single product is K = 1): the row is read once and applied to every column.
// VEC: row stride even and every column 16-byte aligned -> double2 loads; else a scalar walk with the same reduction tree shape.
// Per column the operations and their order do not depend on K and are written out, not left to the compiler's contraction: per
// 16-byte piece t = m.y * v.y rounded, t = fma(m.x, v.x, t), acc += t, an fma for the odd last column, and an fma per entry
// without VEC — every column has the bits of a single product.
template <bool VEC, int K>
__global__ __launch_bounds__(kGemvThreads) void k_row_gemv(int64_t rows, int64_t cols, int64_t ld, const double* __restrict__ M,
                                                            const double* __restrict__ X, int64_t ldx, double* __restrict__ Y,
                                                            int64_t ldy)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = int64_t(blockIdx.x) * (kGemvThreads / 64) + (threadIdx.x >> 6);
    if (r >= rows)
        return;
    const double* a = M + r * ld;
    double acc[K][4];
#pragma unroll
    for (int c = 0; c < K; c++)
        acc[c][0] = acc[c][1] = acc[c][2] = acc[c][3] = 0.0;
    const auto piece = [](double s, const double2 m, const double2 v) { return __dadd_rn(s, fma(m.x, v.x, __dmul_rn(m.y, v.y))); };
    if (VEC)
    {
        const double2* a2 = reinterpret_cast<const double2*>(a);
        const int64_t pairs = cols >> 1;
        int64_t p = lane;
        for (; p + 192 < pairs; p += 256)
        {
            const double2 m0 = a2[p], m1 = a2[p + 64], m2 = a2[p + 128], m3 = a2[p + 192];
#pragma unroll
            for (int c = 0; c < K; c++)
            {
                const double2* x2 = reinterpret_cast<const double2*>(X + int64_t(c) * ldx);
                const double2 v0 = x2[p], v1 = x2[p + 64], v2 = x2[p + 128], v3 = x2[p + 192];
                acc[c][0] = piece(acc[c][0], m0, v0);
                acc[c][1] = piece(acc[c][1], m1, v1);
                acc[c][2] = piece(acc[c][2], m2, v2);
                acc[c][3] = piece(acc[c][3], m3, v3);
            }
        }
        for (; p < pairs; p += 64)
        {
            const double2 m0 = a2[p];
#pragma unroll
            for (int c = 0; c < K; c++)
                acc[c][0] = piece(acc[c][0], m0, reinterpret_cast<const double2*>(X + int64_t(c) * ldx)[p]);
        }
        if ((cols & 1) && lane == 0)
        {
#pragma unroll
            for (int c = 0; c < K; c++)
                acc[c][1] = fma(a[cols - 1], X[int64_t(c) * ldx + cols - 1], acc[c][1]);
        }
    }
    else
    {
        int64_t j = lane;
        for (; j + 192 < cols; j += 256)
        {
            const double m0 = a[j], m1 = a[j + 64], m2 = a[j + 128], m3 = a[j + 192];
#pragma unroll
            for (int c = 0; c < K; c++)
            {
                const double* x = X + int64_t(c) * ldx;
                acc[c][0] = fma(m0, x[j], acc[c][0]);
                acc[c][1] = fma(m1, x[j + 64], acc[c][1]);
                acc[c][2] = fma(m2, x[j + 128], acc[c][2]);
                acc[c][3] = fma(m3, x[j + 192], acc[c][3]);
            }
        }
        for (; j < cols; j += 64)
        {
            const double m0 = a[j];
#pragma unroll
            for (int c = 0; c < K; c++)
                acc[c][0] = fma(m0, X[int64_t(c) * ldx + j], acc[c][0]);
        }
    }
#pragma unroll
    for (int c = 0; c < K; c++)
    {
        const double s = wave_reduce_sum(__dadd_rn(__dadd_rn(acc[c][0], acc[c][1]), __dadd_rn(acc[c][2], acc[c][3])));
        if (lane == 0)
            Y[int64_t(c) * ldy + r] = s;
    }
}

void ensure_stage(const mispec_dense& D)
{
    if (D.stage_x.n < size_t(D.cols) + 2)
        D.stage_x.alloc(size_t(D.cols) + 2);
    if (D.stage_y.n < size_t(D.rows) + 2)
        D.stage_y.alloc(size_t(D.rows) + 2);
}

}  // namespace

namespace mispec {

void launch_row_gemv(const mispec_ctx& ctx, const double* M, int64_t ld, int64_t rows, int64_t cols, const double* x, double* y,
                     bool storage_order_if_small)
{
    launch_row_gemv_panel(ctx, M, ld, rows, cols, x, 0, 1, y, 0, storage_order_if_small);
}

void launch_row_gemv_panel(const mispec_ctx& ctx, const double* M, int64_t ld, int64_t rows, int64_t cols, const double* X, int64_t ldx,
                           int k, double* Y, int64_t ldy, bool storage_order_if_small)
{
    if (rows <= 0 || k <= 0)
        return;
    // a product picks its kernel per vector from the vector's alignment: a panel kernel runs only where every column makes the
    // same choice (an odd ldx makes every second column 8-byte aligned only), and never for the storage-order kernel
    const auto vec_of = [&](int c) {
        return (ld % 2 == 0) && (reinterpret_cast<uintptr_t>(X + int64_t(c) * ldx) % 16 == 0) && (reinterpret_cast<uintptr_t>(M) % 16 == 0);
    };
    const bool serial = storage_order_if_small && rows * cols <= kSerialGemvEntries;
    bool same = true;
    for (int c = 1; c < k; c++)
        same = same && vec_of(c) == vec_of(0);
    if (k != 1 && ((k != 2 && k != 4) || !same || serial))
    {
        for (int c = 0; c < k; c++)
            launch_row_gemv(ctx, M, ld, rows, cols, X + int64_t(c) * ldx, Y + int64_t(c) * ldy, storage_order_if_small);
        return;
    }
    if (serial)
    {
        hipLaunchKernelGGL(k_row_gemv_serial, dim3(unsigned((rows + 63) / 64)), dim3(64), 0, ctx.stream, rows, cols, ld, M, X, Y);
        MISPEC_HIP(hipGetLastError());
        return;
    }
    const dim3 grid(unsigned((rows + kGemvThreads / 64 - 1) / (kGemvThreads / 64))), block(kGemvThreads);
    const auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, ctx.stream, rows, cols, ld, M, X, ldx, Y, ldy); };
    if (vec_of(0))
        k == 4 ? launch(&k_row_gemv<true, 4>) : k == 2 ? launch(&k_row_gemv<true, 2>) : launch(&k_row_gemv<true, 1>);
    else
        k == 4 ? launch(&k_row_gemv<false, 4>) : k == 2 ? launch(&k_row_gemv<false, 2>) : launch(&k_row_gemv<false, 1>);
    MISPEC_HIP(hipGetLastError());
}

}  // namespace mispec

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" int mispec_dense_upload(mispec_ctx* ctx, int64_t rows, int64_t cols, const double* data_host, int64_t ld_host,
                                   int row_major, char uplo, mispec_dense** out)
{
    return guarded([&] {
        MISPEC_REQUIRE(ctx && out && rows >= 0 && cols >= 0, "mispec_dense_upload: bad argument");
        MISPEC_REQUIRE(data_host || rows * cols == 0, "mispec_dense_upload: NULL matrix");
        MISPEC_REQUIRE(ld_host >= (row_major ? cols : rows), "mispec_dense_upload: leading dimension too small");
        const bool sym = (uplo == 'L' || uplo == 'l' || uplo == 'U' || uplo == 'u');
        MISPEC_REQUIRE(sym || uplo == 0 || uplo == 'G' || uplo == 'g', "mispec_dense_upload: uplo must be 'L', 'U' or 0 (general)");
        MISPEC_REQUIRE(!sym || rows == cols, "mispec_dense_upload: a symmetric matrix must be square");
        MISPEC_REQUIRE(ctx->comm.allgather == nullptr, "mispec_dense_upload: dense operators cannot be row-sharded");
        const bool lower = (uplo == 'L' || uplo == 'l');
        ctx->make_current();
        auto D = std::make_unique<mispec_dense>();
        D->ctx = ctx;
        D->rows = rows;
        D->cols = cols;
        D->ld = round_up(std::max<int64_t>(cols, 1), 2);
        std::vector<double> rm(size_t(std::max<int64_t>(rows, 1)) * size_t(D->ld), 0.0);
        auto in = [&](int64_t i, int64_t j) { return row_major ? data_host[i * ld_host + j] : data_host[j * ld_host + i]; };
        for (int64_t i = 0; i < rows; i++)
            for (int64_t j = 0; j < cols; j++)
            {
                double v;
                if (!sym)
                    v = in(i, j);
                else if (lower)
                    v = i >= j ? in(i, j) : in(j, i);  // selfadjointView<Lower>: the strict upper triangle is never read
                else
                    v = i <= j ? in(i, j) : in(j, i);
                rm[size_t(i) * size_t(D->ld) + size_t(j)] = v;
            }
        D->a.alloc(rm.size());
        MISPEC_HIP(hipMemcpy(D->a.p, rm.data(), rm.size() * sizeof(double), hipMemcpyHostToDevice));
        *out = D.release();
    });
}

extern "C" int mispec_dense_destroy(mispec_dense* D)
{
    return guarded([&] {
        if (D)
        {
            D->ctx->make_current();
            delete D;
        }
    });
}
extern "C" int64_t mispec_dense_rows(const mispec_dense* D) { return D ? D->rows : 0; }
extern "C" int64_t mispec_dense_cols(const mispec_dense* D) { return D ? D->cols : 0; }

extern "C" int mispec_dense_gemv(const mispec_dense* D, const double* x_dev, double* y_dev)
{
    return guarded([&] {
        MISPEC_REQUIRE(D && x_dev && y_dev, "mispec_dense_gemv: NULL argument");
        D->ctx->make_current();
        launch_row_gemv(*D->ctx, D->a.p, D->ld, D->rows, D->cols, x_dev, y_dev, true);
    });
}

extern "C" int mispec_dense_gemm_host(const mispec_dense* D, const double* X_host, int64_t ldx, int k, double* Y_host, int64_t ldy)
{
    return guarded([&] {
        MISPEC_REQUIRE(D && X_host && Y_host && k >= 0, "mispec_dense_gemm_host: bad argument");
        MISPEC_REQUIRE(ldx >= D->cols && ldy >= D->rows, "mispec_dense_gemm_host: leading dimension too small");
        D->ctx->make_current();
        hipStream_t s = D->ctx->stream;
        ensure_stage(*D);
        for (int c = 0; c < k; c++)
        {
            MISPEC_HIP(hipMemcpyAsync(D->stage_x.p, X_host + int64_t(c) * ldx, size_t(D->cols) * sizeof(double), hipMemcpyHostToDevice, s));
            launch_row_gemv(*D->ctx, D->a.p, D->ld, D->rows, D->cols, D->stage_x.p, D->stage_y.p, true);
            MISPEC_HIP(hipMemcpyAsync(Y_host + int64_t(c) * ldy, D->stage_y.p, size_t(D->rows) * sizeof(double), hipMemcpyDeviceToHost, s));
            MISPEC_HIP(hipStreamSynchronize(s));
        }
    });
}

extern "C" int mispec_dense_gemv_host(const mispec_dense* D, const double* x_host, double* y_host)
{
    return mispec_dense_gemm_host(D, x_host, D ? D->cols : 0, 1, y_host, D ? D->rows : 0);
}

extern "C" int mispec_dense_coeff(const mispec_dense* D, int64_t i, int64_t j, double* out)
{
    return guarded([&] {
        MISPEC_REQUIRE(D && out, "mispec_dense_coeff: NULL argument");
        MISPEC_REQUIRE(i >= 0 && i < D->rows && j >= 0 && j < D->cols, "mispec_dense_coeff: index out of range");
        D->ctx->make_current();
        MISPEC_HIP(hipMemcpy(out, D->a.p + i * D->ld + j, sizeof(double), hipMemcpyDeviceToHost));
    });
}

extern "C" int mispec_dense_gemv_time(const mispec_dense* D, const double* x_dev, double* y_dev, int reps, float* ms_per_launch)
{
    return guarded([&] {
        MISPEC_REQUIRE(D && x_dev && y_dev && reps > 0 && ms_per_launch, "mispec_dense_gemv_time: bad argument");
        D->ctx->make_current();
        hipEvent_t e0, e1;
        MISPEC_HIP(hipEventCreate(&e0));
        MISPEC_HIP(hipEventCreate(&e1));
        MISPEC_HIP(hipEventRecord(e0, D->ctx->stream));
        for (int i = 0; i < reps; i++)
            launch_row_gemv(*D->ctx, D->a.p, D->ld, D->rows, D->cols, x_dev, y_dev, true);
        MISPEC_HIP(hipEventRecord(e1, D->ctx->stream));
        MISPEC_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        MISPEC_HIP(hipEventElapsedTime(&ms, e0, e1));
        (void) hipEventDestroy(e0);
        (void) hipEventDestroy(e1);
        *ms_per_launch = ms / float(reps);
    });
}
