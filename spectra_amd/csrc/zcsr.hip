// Complex Hermitian sparse operator on the device (mispec_zcsr, include/mispec_extras.h): y = A x for the operator of
// SparseHermMatProd<std::complex<double>>, full int32 CSR in HBM after the mirroring of zcsr.hpp.  It is the hot path of
// HermEigsSolver over a sparse matrix (one product per Lanczos step); the real CSR kernels (csr_kernels.hpp) are not touched.
//
// k_zspmv_csr: LPR consecutive lanes per row (LPR = 8 by default, DESIGN.md "Complex Hermitian solver" gives the measurement that
// chose it).  Lane l of a row's group sums the row's entries l, l + LPR, ... in order, then the group adds its partial sums by a
// fixed xor butterfly: every row sums in one fixed order, so results are bit-identical from run to run and independent of the
// grid.  Values are double2 (one 16-byte load per entry), the gathered x entries too; no atomics.
#include <complex>
#include <memory>
#include <vector>

#include "common.hpp"
#include "zcsr.hpp"

using namespace mispec;
using cd = std::complex<double>;

namespace {

constexpr int kThreads = 256;
constexpr int kDefaultLanesPerRow = 8;

template <int LPR>
__global__ __launch_bounds__(kThreads) void k_zspmv_csr(int64_t n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                         const double2* __restrict__ val, const double2* __restrict__ x,
                                                         double2* __restrict__ y)
{
    const int64_t t = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    const int64_t row = t / LPR;
    const int lane = int(threadIdx.x) % LPR;
    double re = 0.0, im = 0.0;
    if (row < n)
    {
        const int32_t e = rowptr[row + 1];
        for (int32_t k = rowptr[row] + lane; k < e; k += LPR)
        {
            const double2 a = val[k];
            const double2 v = x[col[k]];
            re = fma(a.x, v.x, re);
            re = fma(-a.y, v.y, re);
            im = fma(a.x, v.y, im);
            im = fma(a.y, v.x, im);
        }
    }
    // every lane of the group takes part (no early return above)
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1)
    {
        re += __shfl_xor(re, o, LPR);
        im += __shfl_xor(im, o, LPR);
    }
    if (row < n && lane == 0)
        y[row] = make_double2(re, im);
}

inline unsigned blocks_for(int64_t n, int lpr) { return unsigned((n * lpr + kThreads - 1) / kThreads); }

void launch_spmv(int lpr, int64_t n, const int32_t* rowptr, const int32_t* col, const double2* val, const double2* x, double2* y,
                 hipStream_t s)
{
    if (n <= 0)
        return;
    switch (lpr)
    {
    case 4: hipLaunchKernelGGL(k_zspmv_csr<4>, dim3(blocks_for(n, 4)), dim3(kThreads), 0, s, n, rowptr, col, val, x, y); break;
    case 8: hipLaunchKernelGGL(k_zspmv_csr<8>, dim3(blocks_for(n, 8)), dim3(kThreads), 0, s, n, rowptr, col, val, x, y); break;
    case 16: hipLaunchKernelGGL(k_zspmv_csr<16>, dim3(blocks_for(n, 16)), dim3(kThreads), 0, s, n, rowptr, col, val, x, y); break;
    default: throw Error(MISPEC_EINVAL, "complex sparse product: lanes per row must be 4, 8 or 16");
    }
    MISPEC_HIP(hipGetLastError());
}

}  // namespace

struct mispec_zcsr
{
    mispec_ctx* ctx = nullptr;
    int64_t n = 0, nnz = 0;
    DevBuf<int32_t> rowptr, col;
    DevBuf<double2> val;
    mutable DevBuf<double2> stage_x, stage_y;
};

namespace mispec {

void zcsr_apply(const mispec_zcsr* A, const double2* x, double2* y, hipStream_t stream)
{
    launch_spmv(kDefaultLanesPerRow, A->n, A->rowptr.p, A->col.p, A->val.p, x, y, stream);
}

int64_t zcsr_rows(const mispec_zcsr* A) { return A->n; }

}  // namespace mispec

// =================================================================================================
// C ABI (include/mispec_extras.h)
// =================================================================================================
extern "C" int mispec_zcsr_upload(mispec_ctx* ctx, int64_t rows, int64_t cols, const void* outer, const void* inner, int index_bytes,
                                  const double* values, int row_major, char uplo, mispec_zcsr** out)
{
    return guarded([&] {
        MISPEC_REQUIRE(ctx && out && rows >= 0, "mispec_zcsr_upload: bad argument");
        MISPEC_REQUIRE(rows == cols, "mispec_zcsr_upload: a Hermitian matrix must be square");
        MISPEC_REQUIRE(index_bytes == 4 || index_bytes == 8, "mispec_zcsr_upload: index_bytes must be 4 or 8");
        MISPEC_REQUIRE(uplo == 'L' || uplo == 'U', "mispec_zcsr_upload: uplo must be 'L' or 'U'");
        MISPEC_REQUIRE(outer || rows == 0, "mispec_zcsr_upload: NULL outer index array");
        ZCsrHost H;
        const cd* v = reinterpret_cast<const cd*>(values);
        if (index_bytes == 4)
            zcsr_mirror(rows, static_cast<const int32_t*>(outer), static_cast<const int32_t*>(inner), v, row_major != 0, uplo, H);
        else
            zcsr_mirror(rows, static_cast<const int64_t*>(outer), static_cast<const int64_t*>(inner), v, row_major != 0, uplo, H);
        MISPEC_HIP(hipSetDevice(ctx->device));
        std::unique_ptr<mispec_zcsr> Z(new mispec_zcsr);
        Z->ctx = ctx;
        Z->n = rows;
        Z->nnz = int64_t(H.col.size());
        Z->rowptr.alloc(H.rowptr.size());
        Z->col.alloc(H.col.size());
        Z->val.alloc(H.val.size());
        MISPEC_HIP(hipMemcpy(Z->rowptr.p, H.rowptr.data(), H.rowptr.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        if (Z->nnz)
        {
            MISPEC_HIP(hipMemcpy(Z->col.p, H.col.data(), H.col.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            MISPEC_HIP(hipMemcpy(Z->val.p, H.val.data(), H.val.size() * sizeof(double2), hipMemcpyHostToDevice));
        }
        *out = Z.release();
    });
}

extern "C" int mispec_zcsr_destroy(mispec_zcsr* A)
{
    return guarded([&] { delete A; });
}

extern "C" int64_t mispec_zcsr_rows(const mispec_zcsr* A) { return A ? A->n : 0; }
extern "C" int64_t mispec_zcsr_cols(const mispec_zcsr* A) { return A ? A->n : 0; }
extern "C" int64_t mispec_zcsr_nnz(const mispec_zcsr* A) { return A ? A->nnz : 0; }

namespace {

// y_host = A x_host through the staging buffers, with `lpr` lanes per row
void spmv_host(const mispec_zcsr* A, int lpr, const double* x_host, double* y_host)
{
    MISPEC_HIP(hipSetDevice(A->ctx->device));
    if (A->stage_x.n < size_t(A->n))
    {
        A->stage_x.alloc(size_t(A->n));
        A->stage_y.alloc(size_t(A->n));
    }
    hipStream_t s = A->ctx->stream;
    const size_t bytes = size_t(A->n) * sizeof(double2);
    MISPEC_HIP(hipMemcpyAsync(A->stage_x.p, x_host, bytes, hipMemcpyHostToDevice, s));
    launch_spmv(lpr, A->n, A->rowptr.p, A->col.p, A->val.p, A->stage_x.p, A->stage_y.p, s);
    MISPEC_HIP(hipMemcpyAsync(y_host, A->stage_y.p, bytes, hipMemcpyDeviceToHost, s));
    MISPEC_HIP(hipStreamSynchronize(s));
}

}  // namespace

extern "C" int mispec_zcsr_spmv_host(const mispec_zcsr* A, const double* x_host, double* y_host)
{
    return guarded([&] {
        MISPEC_REQUIRE(A && x_host && y_host, "mispec_zcsr_spmv_host: NULL argument");
        spmv_host(A, kDefaultLanesPerRow, x_host, y_host);
    });
}

extern "C" int mispec_zcsr_spmv_host_lanes(const mispec_zcsr* A, int lanes_per_row, const double* x_host, double* y_host)
{
    return guarded([&] {
        MISPEC_REQUIRE(A && x_host && y_host, "mispec_zcsr_spmv_host_lanes: NULL argument");
        MISPEC_REQUIRE(lanes_per_row == 4 || lanes_per_row == 8 || lanes_per_row == 16,
                       "mispec_zcsr_spmv_host_lanes: lanes per row must be 4, 8 or 16");
        spmv_host(A, lanes_per_row, x_host, y_host);
    });
}

extern "C" int mispec_zcsr_coeff(const mispec_zcsr* A, int64_t i, int64_t j, double* out_re_im)
{
    return guarded([&] {
        MISPEC_REQUIRE(A && out_re_im, "mispec_zcsr_coeff: NULL argument");
        MISPEC_REQUIRE(i >= 0 && i < A->n && j >= 0 && j < A->n, "mispec_zcsr_coeff: index out of range");
        MISPEC_HIP(hipSetDevice(A->ctx->device));
        int32_t range[2];
        MISPEC_HIP(hipMemcpy(range, A->rowptr.p + i, 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
        const size_t len = size_t(range[1] - range[0]);
        std::vector<int32_t> cols(len);
        out_re_im[0] = out_re_im[1] = 0.0;
        if (!len)
            return;
        MISPEC_HIP(hipMemcpy(cols.data(), A->col.p + range[0], len * sizeof(int32_t), hipMemcpyDeviceToHost));
        const auto it = std::lower_bound(cols.begin(), cols.end(), int32_t(j));
        if (it == cols.end() || *it != int32_t(j))
            return;
        double2 v;
        MISPEC_HIP(hipMemcpy(&v, A->val.p + range[0] + (it - cols.begin()), sizeof(double2), hipMemcpyDeviceToHost));
        out_re_im[0] = v.x;
        out_re_im[1] = v.y;
    });
}

extern "C" int mispec_zcsr_spmv_time(const mispec_zcsr* A, int lanes_per_row, int reps, float* ms_per_launch)
{
    return guarded([&] {
        MISPEC_REQUIRE(A && ms_per_launch && reps > 0, "mispec_zcsr_spmv_time: bad argument");
        const int lpr = lanes_per_row ? lanes_per_row : kDefaultLanesPerRow;
        MISPEC_HIP(hipSetDevice(A->ctx->device));
        if (A->stage_x.n < size_t(A->n))
        {
            A->stage_x.alloc(size_t(A->n));
            A->stage_y.alloc(size_t(A->n));
        }
        hipStream_t s = A->ctx->stream;
        MISPEC_HIP(hipMemsetAsync(A->stage_x.p, 0, size_t(A->n) * sizeof(double2), s));
        launch_spmv(lpr, A->n, A->rowptr.p, A->col.p, A->val.p, A->stage_x.p, A->stage_y.p, s);  // warm-up
        hipEvent_t e0, e1;
        MISPEC_HIP(hipEventCreate(&e0));
        MISPEC_HIP(hipEventCreate(&e1));
        MISPEC_HIP(hipEventRecord(e0, s));
        for (int r = 0; r < reps; r++)
            launch_spmv(lpr, A->n, A->rowptr.p, A->col.p, A->val.p, A->stage_x.p, A->stage_y.p, s);
        MISPEC_HIP(hipEventRecord(e1, s));
        MISPEC_HIP(hipEventSynchronize(e1));
        float ms = 0.0f;
        MISPEC_HIP(hipEventElapsedTime(&ms, e0, e1));
        (void) hipEventDestroy(e0);
        (void) hipEventDestroy(e1);
        *ms_per_launch = ms / float(reps);
    });
}
