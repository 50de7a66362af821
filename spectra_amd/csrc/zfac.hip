// Complex-scalar Arnoldi / Lanczos factorisation on the device: the HIP backend of zfac_flow.hpp and its C entry points
// (include/mispec_extras.h).  OUTSIDE the hot path of SURVEY.md section 8 — the configs are real fp64 — and deliberately plain:
// host-driven steps in the reference's order, one kernel per vector primitive, no fusion.  It exists so that the reference's
// factorisation templates keep their complex instantiations (LinAlg/Arnoldi.h, LinAlg/Lanczos.h over DenseGenMatProd<complex> /
// DenseHermMatProd<complex>; test/Arnoldi.cpp:122-158) with the basis in HBM rather than on a CPU fallback.
//
// Layout: complex numbers interleaved (re, im) = double2, 16-byte loads; V is n x m column-major with leading dimension n; a dense
// operator is stored column-major (one thread per row reads a column slice coalesced), a Hermitian input given by one triangle is
// mirrored at upload with the diagonal's imaginary part dropped, as selfadjointView reads it.
// Every primitive is HBM-bound at 16 bytes per entry touched.  Reductions (X^H y over up to ncv + 1 columns, the norm, max |x_i|)
// run in two stages that fill the device: stage 1 gives every fixed chunk of kChunk rows (x a group of kColGroup columns) to one
// workgroup, which sums its rows in a fixed order, its lanes by a fixed shuffle tree and its four waves in order; stage 2 adds the
// partial sums of one column in a fixed order.  The partition depends on n only, so results are deterministic and independent of
// the launch geometry.  The operator is a dense device matrix, a device complex CSR matrix (csrc/zcsr.hip) or a host callback.
// The restart primitives of the Hermitian solver (include/Spectra/internal/ComplexHermEigs.h): k_zvq forms V Q for a real Q in
// place, row tile by row tile, and the Ritz vectors V Y into a separate buffer.
#include <complex>
#include <memory>
#include <vector>

#include "common.hpp"
#include "device_helpers.hpp"
#include "zcsr.hpp"
#include "zfac_flow.hpp"

using namespace mispec;
using cd = std::complex<double>;

namespace {

constexpr int kThreads = 256;

__device__ inline double2 zmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ inline double2 zmulc(double2 a, double2 b) { return make_double2(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x); }  // conj(a) b

constexpr int kChunk = 2048;   // rows per stage-1 partial sum: the fixed partition of every reduction
constexpr int kColGroup = 8;   // columns per stage-1 workgroup (X^H y)
constexpr int kWaves = kThreads / 64;
constexpr int kVqBatch = 8;    // k_zvq: tile loads in flight per thread

inline int64_t chunks_for(int64_t n) { return (n + kChunk - 1) / kChunk; }

// stage 1 of out[j] = X[:, j]^H y: block (chunk b, column group g) writes part[j * nchunks + b] for its kColGroup columns
__global__ __launch_bounds__(kThreads) void k_zdotc_partial(int64_t n, const double2* __restrict__ X, int64_t ldx, int ncols,
                                                             const double2* __restrict__ y, double2* __restrict__ part, int64_t nchunks)
{
    __shared__ double red[kWaves][2 * kColGroup];
    const int64_t r0 = int64_t(blockIdx.x) * kChunk;
    const int64_t r1 = (r0 + kChunk < n) ? r0 + kChunk : n;
    const int c0 = int(blockIdx.y) * kColGroup;
    const int nc = (ncols - c0 < kColGroup) ? ncols - c0 : kColGroup;
    double re[kColGroup], im[kColGroup];
#pragma unroll
    for (int c = 0; c < kColGroup; c++)
        re[c] = im[c] = 0.0;
    for (int64_t i = r0 + threadIdx.x; i < r1; i += kThreads)
    {
        const double2 yi = y[i];
#pragma unroll
        for (int c = 0; c < kColGroup; c++)
            if (c < nc)
            {
                const double2 p = zmulc(X[i + int64_t(c0 + c) * ldx], yi);
                re[c] += p.x;
                im[c] += p.y;
            }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < kColGroup; c++)
    {
        const double a = wave_reduce_sum(re[c]), b = wave_reduce_sum(im[c]);
        if (lane == 0)
        {
            red[wave][2 * c] = a;
            red[wave][2 * c + 1] = b;
        }
    }
    __syncthreads();
    if (int(threadIdx.x) < 2 * nc)
    {
        double v = red[0][threadIdx.x];
        for (int w = 1; w < kWaves; w++)
            v += red[w][threadIdx.x];
        double* dst = reinterpret_cast<double*>(part + int64_t(c0 + int(threadIdx.x) / 2) * nchunks + blockIdx.x);
        dst[threadIdx.x & 1] = v;
    }
}

// stage 2: out[j] = sum_b part[j * nchunks + b], one workgroup per column, fixed order
__global__ __launch_bounds__(kThreads) void k_zdotc_final(const double2* __restrict__ part, int64_t nchunks, double2* __restrict__ out)
{
    __shared__ double red[kWaves][2];
    const double2* p = part + int64_t(blockIdx.x) * nchunks;
    double re = 0.0, im = 0.0;
    for (int64_t b = threadIdx.x; b < nchunks; b += kThreads)
    {
        re += p[b].x;
        im += p[b].y;
    }
    re = wave_reduce_sum(re);
    im = wave_reduce_sum(im);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
    {
        red[wave][0] = re;
        red[wave][1] = im;
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        double a = red[0][0], b = red[0][1];
        for (int w = 1; w < kWaves; w++)
        {
            a += red[w][0];
            b += red[w][1];
        }
        out[blockIdx.x] = make_double2(a, b);
    }
}

// f = w - V[:, :ncols] h  (w may alias f: each thread reads its own row before it writes it)
__global__ __launch_bounds__(kThreads) void k_zupdate(int64_t n, double2* f, const double2* w, const double2* __restrict__ V, int64_t ldv,
                                                       int ncols, const double2* __restrict__ h)
{
    const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= n)
        return;
    double2 acc = w[i];
    for (int j = 0; j < ncols; j++)
    {
        const double2 p = zmul(V[i + int64_t(j) * ldv], h[j]);
        acc.x -= p.x;
        acc.y -= p.y;
    }
    f[i] = acc;
}

// y = A x, A column-major rows x cols with leading dimension ld: one thread per row
__global__ __launch_bounds__(kThreads) void k_zgemv(int64_t rows, int64_t cols, const double2* __restrict__ A, int64_t ld,
                                                     const double2* __restrict__ x, double2* __restrict__ y)
{
    const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= rows)
        return;
    double2 acc = make_double2(0.0, 0.0);
    for (int64_t j = 0; j < cols; j++)
    {
        const double2 p = zmul(A[i + j * ld], x[j]);
        acc.x += p.x;
        acc.y += p.y;
    }
    y[i] = acc;
}

__global__ __launch_bounds__(kThreads) void k_zscale_copy(int64_t n, double2* dst, const double2* src, double alpha)
{
    const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (i < n)
    {
        const double2 v = src[i];
        dst[i] = make_double2(alpha * v.x, alpha * v.y);
    }
}

__global__ __launch_bounds__(kThreads) void k_zaxpy(int64_t n, double2* __restrict__ y, double2 a, const double2* __restrict__ x)
{
    const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (i < n)
    {
        const double2 p = zmul(a, x[i]);
        y[i] = make_double2(y[i].x + p.x, y[i].y + p.y);
    }
}

// max_i |x_i| in two stages: one partial per chunk, then one workgroup over the partials (max is exact in any order; the partition
// is the fixed one of the sums above all the same)
__global__ __launch_bounds__(kThreads) void k_zabsmax_partial(int64_t n, const double2* __restrict__ x, double* __restrict__ part)
{
    __shared__ double red[kWaves];
    const int64_t r0 = int64_t(blockIdx.x) * kChunk;
    const int64_t r1 = (r0 + kChunk < n) ? r0 + kChunk : n;
    double m = 0.0;
    for (int64_t i = r0 + threadIdx.x; i < r1; i += kThreads)
        m = fmax(m, hypot(x[i].x, x[i].y));
    m = wave_reduce_max(m);
    if ((threadIdx.x & 63) == 0)
        red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        for (int w = 1; w < kWaves; w++)
            m = fmax(m, red[w]);
        part[blockIdx.x] = m;
    }
}

__global__ __launch_bounds__(kThreads) void k_zabsmax_final(const double* __restrict__ part, int64_t nchunks, double* __restrict__ out)
{
    __shared__ double red[kWaves];
    double m = 0.0;
    for (int64_t b = threadIdx.x; b < nchunks; b += kThreads)
        m = fmax(m, part[b]);
    m = wave_reduce_max(m);
    if ((threadIdx.x & 63) == 0)
        red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        for (int w = 1; w < kWaves; w++)
            m = fmax(m, red[w]);
        out[0] = m;
    }
}

// out[:, c] = V[:, :nnz(c)] Q[:nnz(c), c] for c < ncols, nnz(c) = min(m, first_nnz + c) (Arnoldi.h:312-340 compress_V: column i of
// Q has m - k + i + 1 leading non-zeros; the Ritz vectors use all m).  Q is real, m x ncols, leading dimension ldq.  A block stages
// its tile of R rows x m columns of V in LDS, waits, then writes: `out` may be V itself (the blocks own disjoint rows).
// Thread (r, cl) of the block forms row r of columns cl, cl + 256 / R, ...; every entry sums over j in ascending order.
__global__ __launch_bounds__(kThreads) void k_zvq(int64_t n, const double2* V, int64_t ldv, int m, const double* __restrict__ Q, int ldq,
                                                   int ncols, int first_nnz, double2* out, int64_t ldo, int R)
{
    extern __shared__ double2 tile[];  // R x m, tile[j * R + r]
    const int64_t row0 = int64_t(blockIdx.x) * R;
    // kVqBatch loads in flight per thread before their LDS stores
    for (int base = threadIdx.x; base < R * m; base += kThreads * kVqBatch)
    {
        double2 v[kVqBatch];
#pragma unroll
        for (int u = 0; u < kVqBatch; u++)
        {
            const int idx = base + u * kThreads;
            const int64_t i = row0 + idx % R;
            v[u] = (idx < R * m && i < n) ? V[i + int64_t(idx / R) * ldv] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int u = 0; u < kVqBatch; u++)
            if (base + u * kThreads < R * m)
                tile[base + u * kThreads] = v[u];
    }
    __syncthreads();
    const int r = int(threadIdx.x) % R, cl = int(threadIdx.x) / R, CL = kThreads / R;
    const int64_t i = row0 + r;
    for (int c = cl; c < ncols; c += CL)
    {
        const int nnz = (first_nnz + c < m) ? first_nnz + c : m;
        const double* q = Q + int64_t(c) * ldq;
        double re = 0.0, im = 0.0;
        for (int j = 0; j < nnz; j++)
        {
            const double2 v = tile[j * R + r];
            re = fma(v.x, q[j], re);
            im = fma(v.y, q[j], im);
        }
        if (i < n)
            out[i + int64_t(c) * ldo] = make_double2(re, im);
    }
}

// rows per k_zvq tile: the tile (R x m complex) stays within 64 KiB of LDS
inline int vq_rows(int m)
{
    int R = 64;
    while (R > 1 && size_t(R) * size_t(m) * sizeof(double2) > 65536)
        R >>= 1;
    return R;
}
constexpr int kMaxVqCols = 4096;  // m <= 4096: R >= 1

inline unsigned blocks_for(int64_t n) { return unsigned((n + kThreads - 1) / kThreads); }
inline double2* z2(cd* p) { return reinterpret_cast<double2*>(p); }
inline const double2* z2(const cd* p) { return reinterpret_cast<const double2*>(p); }

}  // namespace

struct mispec_zdense
{
    mispec_ctx* ctx = nullptr;
    int64_t rows = 0, cols = 0;
    DevBuf<double2> a;  // column-major, leading dimension rows
    std::vector<cd> host;  // the same entries, for operator()
    mutable DevBuf<double2> stage_x, stage_y;
};

namespace {

// The primitives of zfac_flow.hpp on the context's stream.
struct HipBackend
{
    mispec_ctx* ctx = nullptr;
    int64_t n = 0;
    const mispec_zdense* dense = nullptr;
    const mispec_zcsr* csr = nullptr;
    mispec_zop_fn op = nullptr;
    void* op_user = nullptr;
    DevBuf<double2> small;           // reduction results / coefficient vectors on the device
    PinnedBuf<double2> small_host;   // their host images
    PinnedBuf<double2> stage_x, stage_y;  // host-pointer operator
    DevBuf<double> scalar;
    DevBuf<double2> part;      // stage-1 partial sums, (m + 1) columns x chunks_for(n)
    DevBuf<double> part_max;   // stage-1 partial maxima
    DevBuf<double> qmat;       // the real m x m matrix of k_zvq
    int64_t nchunks = 0;

    void setup(int m)
    {
        small.alloc(size_t(m) + 1);
        small_host.alloc(size_t(m) + 1);
        scalar.alloc(1);
        nchunks = chunks_for(n);
        part.alloc(size_t(nchunks) * (size_t(m) + 1));
        part_max.alloc(size_t(nchunks));
        if (op)
        {
            stage_x.alloc(size_t(n));
            stage_y.alloc(size_t(n));
        }
    }
    hipStream_t s() const { return ctx->stream; }

    cd* alloc(size_t count)
    {
        void* p = nullptr;
        MISPEC_HIP(hipMalloc(&p, count * sizeof(double2)));
        return static_cast<cd*>(p);
    }
    void release(cd* p)
    {
        if (p)
            (void) hipFree(p);
    }
    void upload(cd* dev, const cd* host, int64_t count)
    {
        MISPEC_HIP(hipMemcpyAsync(dev, host, size_t(count) * sizeof(double2), hipMemcpyHostToDevice, s()));
        MISPEC_HIP(hipStreamSynchronize(s()));
    }
    void download(cd* host, const cd* dev, int64_t count)
    {
        MISPEC_HIP(hipMemcpyAsync(host, dev, size_t(count) * sizeof(double2), hipMemcpyDeviceToHost, s()));
        MISPEC_HIP(hipStreamSynchronize(s()));
    }
    void apply(const cd* x, cd* y)
    {
        if (csr)
        {
            zcsr_apply(csr, z2(x), z2(y), s());
            return;
        }
        if (dense)
        {
            hipLaunchKernelGGL(k_zgemv, dim3(blocks_for(n)), dim3(kThreads), 0, s(), dense->rows, dense->cols, dense->a.p, dense->rows, z2(x),
                               z2(y));
            MISPEC_HIP(hipGetLastError());
            return;
        }
        // the reference's contract: perform_op(const Scalar* x_in, Scalar* y_out) on host pointers
        MISPEC_HIP(hipMemcpyAsync(stage_x.p, x, size_t(n) * sizeof(double2), hipMemcpyDeviceToHost, s()));
        MISPEC_HIP(hipStreamSynchronize(s()));
        if (op(op_user, reinterpret_cast<const double*>(stage_x.p), reinterpret_cast<double*>(stage_y.p)) != 0)
            throw Error(MISPEC_ERUNTIME, "complex factorisation: the user operator reported an error");
        MISPEC_HIP(hipMemcpyAsync(y, stage_y.p, size_t(n) * sizeof(double2), hipMemcpyHostToDevice, s()));
        MISPEC_HIP(hipStreamSynchronize(s()));
    }
    // the two stages of X^H y into small.p
    void launch_dotc(const cd* X, int64_t ldx, int ncols, const cd* y)
    {
        const unsigned groups = unsigned((ncols + kColGroup - 1) / kColGroup);
        hipLaunchKernelGGL(k_zdotc_partial, dim3(unsigned(nchunks), groups), dim3(kThreads), 0, s(), n, z2(X), ldx, ncols, z2(y), part.p,
                           nchunks);
        MISPEC_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_zdotc_final, dim3(unsigned(ncols)), dim3(kThreads), 0, s(), part.p, nchunks, small.p);
        MISPEC_HIP(hipGetLastError());
    }
    void dotc(const cd* X, int64_t ldx, int ncols, const cd* y, cd* out_host)
    {
        if (ncols <= 0)
            return;
        launch_dotc(X, ldx, ncols, y);
        MISPEC_HIP(hipMemcpyAsync(small_host.p, small.p, size_t(ncols) * sizeof(double2), hipMemcpyDeviceToHost, s()));
        MISPEC_HIP(hipStreamSynchronize(s()));
        for (int j = 0; j < ncols; j++)
            out_host[j] = cd(small_host.p[j].x, small_host.p[j].y);
    }
    void update(cd* f, const cd* w, const cd* V, int64_t ldv, int ncols, const cd* h_host)
    {
        for (int j = 0; j < ncols; j++)
            small_host.p[j] = make_double2(h_host[j].real(), h_host[j].imag());
        if (ncols > 0)
            MISPEC_HIP(hipMemcpyAsync(small.p, small_host.p, size_t(ncols) * sizeof(double2), hipMemcpyHostToDevice, s()));
        hipLaunchKernelGGL(k_zupdate, dim3(blocks_for(n)), dim3(kThreads), 0, s(), n, z2(f), z2(w), z2(V), ldv, ncols, small.p);
        MISPEC_HIP(hipGetLastError());
        MISPEC_HIP(hipStreamSynchronize(s()));  // small_host is rewritten by the next call
    }
    void scale_copy(cd* dst, const cd* src, double alpha)
    {
        hipLaunchKernelGGL(k_zscale_copy, dim3(blocks_for(n)), dim3(kThreads), 0, s(), n, z2(dst), z2(src), alpha);
        MISPEC_HIP(hipGetLastError());
    }
    void axpy(cd* y, cd a, const cd* x)
    {
        hipLaunchKernelGGL(k_zaxpy, dim3(blocks_for(n)), dim3(kThreads), 0, s(), n, z2(y), make_double2(a.real(), a.imag()), z2(x));
        MISPEC_HIP(hipGetLastError());
    }
    double norm(const cd* x)
    {
        cd r;
        dotc(x, n, 1, x, &r);
        return std::sqrt(r.real());
    }
    double absmax(const cd* x)
    {
        hipLaunchKernelGGL(k_zabsmax_partial, dim3(unsigned(nchunks)), dim3(kThreads), 0, s(), n, z2(x), part_max.p);
        MISPEC_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_zabsmax_final, dim3(1), dim3(kThreads), 0, s(), part_max.p, nchunks, scalar.p);
        MISPEC_HIP(hipGetLastError());
        double v = 0.0;
        MISPEC_HIP(hipMemcpyAsync(&v, scalar.p, sizeof(double), hipMemcpyDeviceToHost, s()));
        MISPEC_HIP(hipStreamSynchronize(s()));
        return v;
    }
    void zero(cd* x) { MISPEC_HIP(hipMemsetAsync(x, 0, size_t(n) * sizeof(double2), s())); }
    // out[:, c] = V[:, :nnz(c)] Q[:nnz(c), c], c < ncols, nnz(c) = min(m, first_nnz + c); Q real m x ncols on the host (ldq);
    // out may be V (in place)
    void vq(const cd* V, int64_t ldv, int m, const double* Q_host, int ldq, int ncols, int first_nnz, cd* out, int64_t ldo)
    {
        if (ncols <= 0)
            return;
        if (m > kMaxVqCols)
            throw Error(MISPEC_EINVAL, "complex factorisation: V Q needs ncv <= " + std::to_string(kMaxVqCols));
        if (qmat.n < size_t(m) * size_t(ncols))
            qmat.alloc(size_t(m) * size_t(ncols));
        MISPEC_HIP(hipMemcpy2DAsync(qmat.p, size_t(m) * sizeof(double), Q_host, size_t(ldq) * sizeof(double), size_t(m) * sizeof(double),
                                    size_t(ncols), hipMemcpyHostToDevice, s()));
        launch_vq(V, ldv, m, ncols, first_nnz, out, ldo);
        MISPEC_HIP(hipStreamSynchronize(s()));  // Q_host belongs to the caller
    }
    // k_zvq with the Q already in qmat (m x ncols, leading dimension m)
    void launch_vq(const cd* V, int64_t ldv, int m, int ncols, int first_nnz, cd* out, int64_t ldo)
    {
        const int R = vq_rows(m);
        const unsigned blocks = unsigned((n + R - 1) / R);
        hipLaunchKernelGGL(k_zvq, dim3(blocks), dim3(kThreads), size_t(R) * size_t(m) * sizeof(double2), s(), n, z2(V), ldv, m, qmat.p, m,
                           ncols, first_nnz, z2(out), ldo, R);
        MISPEC_HIP(hipGetLastError());
    }
};

}  // namespace

struct mispec_zfac
{
    HipBackend be;
    std::unique_ptr<ZFacFlow<HipBackend>> flow;
    DevBuf<double2> ritz;  // n x nvec, the last Ritz vectors
};

namespace {

mispec_zfac* make_zfac(mispec_ctx* ctx, int64_t n, int ncv, int hermitian, const mispec_zdense* D, mispec_zop_fn op, void* user,
                       const mispec_zcsr* Z = nullptr)
{
    MISPEC_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<mispec_zfac> F(new mispec_zfac);
    F->be.ctx = ctx;
    F->be.n = n;
    F->be.dense = D;
    F->be.csr = Z;
    F->be.op = op;
    F->be.op_user = user;
    F->be.setup(ncv);
    F->flow.reset(new ZFacFlow<HipBackend>(F->be, n, ncv, hermitian != 0));
    return F.release();
}

}  // namespace

// =================================================================================================
// C ABI (include/mispec_extras.h)
// =================================================================================================
extern "C" int mispec_zdense_upload(mispec_ctx* ctx, int64_t rows, int64_t cols, const double* data_host, int64_t ld_host,
                                    int row_major, char uplo, mispec_zdense** out)
{
    return guarded([&] {
        MISPEC_REQUIRE(ctx && out && rows >= 0 && cols >= 0, "mispec_zdense_upload: bad argument");
        MISPEC_REQUIRE(data_host || rows * cols == 0, "mispec_zdense_upload: NULL matrix");
        MISPEC_REQUIRE(ld_host >= (row_major ? cols : rows), "mispec_zdense_upload: leading dimension too small");
        MISPEC_REQUIRE(uplo == 0 || uplo == 'L' || uplo == 'U', "mispec_zdense_upload: uplo must be 0, 'L' or 'U'");
        MISPEC_REQUIRE(uplo == 0 || rows == cols, "mispec_zdense_upload: a Hermitian matrix must be square");
        MISPEC_HIP(hipSetDevice(ctx->device));
        std::unique_ptr<mispec_zdense> D(new mispec_zdense);
        D->ctx = ctx;
        D->rows = rows;
        D->cols = cols;
        D->host.resize(size_t(rows) * size_t(cols));
        zdense_expand(rows, cols, reinterpret_cast<const cd*>(data_host), ld_host, row_major != 0, uplo, D->host.data());
        D->a.alloc(D->host.size());
        if (!D->host.empty())
            MISPEC_HIP(hipMemcpy(D->a.p, D->host.data(), D->host.size() * sizeof(double2), hipMemcpyHostToDevice));
        *out = D.release();
    });
}

extern "C" int mispec_zdense_destroy(mispec_zdense* D)
{
    return guarded([&] { delete D; });
}

extern "C" int64_t mispec_zdense_rows(const mispec_zdense* D) { return D ? D->rows : 0; }
extern "C" int64_t mispec_zdense_cols(const mispec_zdense* D) { return D ? D->cols : 0; }

extern "C" int mispec_zdense_gemv_host(const mispec_zdense* D, const double* x_host, double* y_host)
{
    return guarded([&] {
        MISPEC_REQUIRE(D && x_host && y_host, "mispec_zdense_gemv_host: NULL argument");
        MISPEC_HIP(hipSetDevice(D->ctx->device));
        if (D->stage_x.n < size_t(D->cols))
            D->stage_x.alloc(size_t(D->cols));
        if (D->stage_y.n < size_t(D->rows))
            D->stage_y.alloc(size_t(D->rows));
        hipStream_t s = D->ctx->stream;
        MISPEC_HIP(hipMemcpyAsync(D->stage_x.p, x_host, size_t(D->cols) * sizeof(double2), hipMemcpyHostToDevice, s));
        if (D->rows > 0)
        {
            hipLaunchKernelGGL(k_zgemv, dim3(blocks_for(D->rows)), dim3(kThreads), 0, s, D->rows, D->cols, D->a.p, D->rows, D->stage_x.p,
                               D->stage_y.p);
            MISPEC_HIP(hipGetLastError());
        }
        MISPEC_HIP(hipMemcpyAsync(y_host, D->stage_y.p, size_t(D->rows) * sizeof(double2), hipMemcpyDeviceToHost, s));
        MISPEC_HIP(hipStreamSynchronize(s));
    });
}

extern "C" int mispec_zdense_coeff(const mispec_zdense* D, int64_t i, int64_t j, double* out_re_im)
{
    return guarded([&] {
        MISPEC_REQUIRE(D && out_re_im, "mispec_zdense_coeff: NULL argument");
        MISPEC_REQUIRE(i >= 0 && i < D->rows && j >= 0 && j < D->cols, "mispec_zdense_coeff: index out of range");
        const cd v = D->host[size_t(j) * size_t(D->rows) + size_t(i)];
        out_re_im[0] = v.real();
        out_re_im[1] = v.imag();
    });
}

extern "C" int mispec_zfac_create_dense(mispec_ctx* ctx, const mispec_zdense* D, int ncv, int hermitian, mispec_zfac** out)
{
    return guarded([&] {
        MISPEC_REQUIRE(ctx && D && out, "mispec_zfac_create_dense: NULL argument");
        MISPEC_REQUIRE(D->rows == D->cols, "mispec_zfac_create_dense: the matrix must be square");
        *out = make_zfac(ctx, D->rows, ncv, hermitian, D, nullptr, nullptr);
    });
}

extern "C" int mispec_zfac_create_op(mispec_ctx* ctx, mispec_zop_fn op, void* op_user, int64_t n, int ncv, int hermitian,
                                     mispec_zfac** out)
{
    return guarded([&] {
        MISPEC_REQUIRE(ctx && op && out, "mispec_zfac_create_op: NULL argument");
        *out = make_zfac(ctx, n, ncv, hermitian, nullptr, op, op_user);
    });
}

extern "C" int mispec_zfac_create_csr(mispec_ctx* ctx, const mispec_zcsr* A, int ncv, int hermitian, mispec_zfac** out)
{
    return guarded([&] {
        MISPEC_REQUIRE(ctx && A && out, "mispec_zfac_create_csr: NULL argument");
        *out = make_zfac(ctx, zcsr_rows(A), ncv, hermitian, nullptr, nullptr, nullptr, A);
    });
}

extern "C" int mispec_zfac_destroy(mispec_zfac* F)
{
    return guarded([&] { delete F; });
}

extern "C" int mispec_zfac_init(mispec_zfac* F, const double* v0_host, int64_t* op_counter)
{
    return guarded([&] {
        MISPEC_REQUIRE(F && v0_host && op_counter, "mispec_zfac_init: NULL argument");
        MISPEC_HIP(hipSetDevice(F->be.ctx->device));
        F->flow->init(reinterpret_cast<const cd*>(v0_host), *op_counter);
    });
}

extern "C" int mispec_zfac_factorize(mispec_zfac* F, int from_k, int to_m, int64_t* op_counter)
{
    return guarded([&] {
        MISPEC_REQUIRE(F && op_counter, "mispec_zfac_factorize: NULL argument");
        MISPEC_HIP(hipSetDevice(F->be.ctx->device));
        F->flow->factorize_from(from_k, to_m, *op_counter);
    });
}

extern "C" int mispec_zfac_subspace_dim(const mispec_zfac* F) { return F ? F->flow->subspace_dim() : 0; }

extern "C" int mispec_zfac_f_norm(const mispec_zfac* F, double* out)
{
    return guarded([&] {
        MISPEC_REQUIRE(F && out, "mispec_zfac_f_norm: NULL argument");
        *out = F->flow->f_norm();
    });
}

extern "C" int mispec_zfac_get_H(const mispec_zfac* F, double* H_host)
{
    return guarded([&] {
        MISPEC_REQUIRE(F && H_host, "mispec_zfac_get_H: NULL argument");
        const std::vector<cd>& H = F->flow->matrix_H();
        std::copy(H.begin(), H.end(), reinterpret_cast<cd*>(H_host));
    });
}

extern "C" int mispec_zfac_get_V(const mispec_zfac* F, int ncols, double* V_host)
{
    return guarded([&] {
        MISPEC_REQUIRE(F && V_host && ncols >= 0 && ncols <= F->flow->max_dim(), "mispec_zfac_get_V: bad argument");
        MISPEC_HIP(hipSetDevice(F->be.ctx->device));
        F->flow->get_V(reinterpret_cast<cd*>(V_host), ncols);
    });
}

extern "C" int mispec_zfac_get_f(const mispec_zfac* F, double* f_host)
{
    return guarded([&] {
        MISPEC_REQUIRE(F && f_host, "mispec_zfac_get_f: NULL argument");
        MISPEC_HIP(hipSetDevice(F->be.ctx->device));
        F->flow->get_f(reinterpret_cast<cd*>(f_host));
    });
}

extern "C" int mispec_zfac_set_H(mispec_zfac* F, const double* H_host)
{
    return guarded([&] {
        MISPEC_REQUIRE(F && H_host, "mispec_zfac_set_H: NULL argument");
        F->flow->set_H(reinterpret_cast<const cd*>(H_host));
    });
}

extern "C" int mispec_zfac_compress_real(mispec_zfac* F, const double* Q_host, int k)
{
    return guarded([&] {
        MISPEC_REQUIRE(F && Q_host, "mispec_zfac_compress_real: NULL argument");
        MISPEC_HIP(hipSetDevice(F->be.ctx->device));
        F->flow->compress_real(Q_host, k);
    });
}

extern "C" int mispec_zfac_ritz_vectors(mispec_zfac* F, const double* Y_host, int nvec, double* X_host)
{
    return guarded([&] {
        MISPEC_REQUIRE(F && (Y_host || nvec == 0) && (X_host || nvec == 0), "mispec_zfac_ritz_vectors: NULL argument");
        MISPEC_REQUIRE(nvec >= 0 && nvec <= F->flow->max_dim(), "mispec_zfac_ritz_vectors: need 0 <= nvec <= ncv");
        if (nvec == 0)
            return;
        MISPEC_HIP(hipSetDevice(F->be.ctx->device));
        const size_t count = size_t(F->flow->rows()) * size_t(nvec);
        if (F->ritz.n < count)
            F->ritz.alloc(count);
        cd* X = reinterpret_cast<cd*>(F->ritz.p);
        F->flow->ritz_vectors(Y_host, nvec, X);
        F->be.download(reinterpret_cast<cd*>(X_host), X, int64_t(count));
    });
}

extern "C" int mispec_zfac_kernel_time(mispec_zfac* F, int which, int ncols, int reps, float* ms_per_launch)
{
    return guarded([&] {
        MISPEC_REQUIRE(F && ms_per_launch && reps > 0, "mispec_zfac_kernel_time: bad argument");
        const int m = F->flow->max_dim();
        MISPEC_REQUIRE(which == 0 || which == 1, "mispec_zfac_kernel_time: which must be 0 (X^H y) or 1 (V Q)");
        MISPEC_REQUIRE(ncols >= (which == 0 ? 1 : 2) && ncols <= m, "mispec_zfac_kernel_time: bad column count");
        MISPEC_REQUIRE(F->flow->subspace_dim() == m, "mispec_zfac_kernel_time: needs a full m-step factorisation");
        MISPEC_HIP(hipSetDevice(F->be.ctx->device));
        HipBackend& be = F->be;
        cd* V = F->flow->basis();
        cd* y = F->flow->residual();
        if (which == 1)
        {
            // Q = I: V Q leaves V as it is (v * 1 + 0 * ..., exact), so the kernel can run in place any number of times
            std::vector<double> I(size_t(m) * size_t(ncols), 0.0);
            for (int c = 0; c < ncols; c++)
                I[size_t(c) * m + c] = 1.0;
            if (be.qmat.n < I.size())
                be.qmat.alloc(I.size());
            MISPEC_HIP(hipMemcpy(be.qmat.p, I.data(), I.size() * sizeof(double), hipMemcpyHostToDevice));
        }
        auto launch = [&] {
            if (which == 0)
                be.launch_dotc(V, be.n, ncols, y);
            else
                be.launch_vq(V, be.n, m, ncols, m - ncols + 2, V, be.n);
        };
        launch();  // warm-up
        hipEvent_t e0, e1;
        MISPEC_HIP(hipEventCreate(&e0));
        MISPEC_HIP(hipEventCreate(&e1));
        MISPEC_HIP(hipEventRecord(e0, be.s()));
        for (int r = 0; r < reps; r++)
            launch();
        MISPEC_HIP(hipEventRecord(e1, be.s()));
        MISPEC_HIP(hipEventSynchronize(e1));
        float ms = 0.0f;
        MISPEC_HIP(hipEventElapsedTime(&ms, e0, e1));
        (void) hipEventDestroy(e0);
        (void) hipEventDestroy(e1);
        *ms_per_launch = ms / float(reps);
    });
}
