// What the two Krylov methods of the iterative shift-solve path share (shift_minres.hip: MINRES for symmetric operators and pencils;
// shift_bicgstab.hip: BiCGStab for general ones) besides shift_iterative_state.hpp: the loop and the block reductions of a vector
// pass, the kernels of construction, set_shift and the explicit residual, the predicated product, and the acceptance rule with its
// failure wording.  For .hip translation units only.
#pragma once
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>

#include "common.hpp"
#include "csr.hpp"
#include "device_helpers.hpp"
#include "shift_iterative_state.hpp"

// the bits of every sum and update are those of the operations written here: products and sums are not contracted, fma is explicit
#pragma clang fp contract(off)

namespace mispec {

namespace shift_iter {

constexpr int kThreads = 256;
constexpr double kMargin = 0.25;

__device__ __forceinline__ double2 ld2(const double* p, int64_t i) { return *reinterpret_cast<const double2*>(p + i); }
__device__ __forceinline__ void st2(double* p, int64_t i, double2 v) { *reinterpret_cast<double2*>(p + i) = v; }
// a caller's vector may be only 8-byte aligned (a column of a block with an odd leading dimension): two 8-byte accesses then
template <bool AL>
__device__ __forceinline__ double2 ext_ld2(const double* p, int64_t i)
{
    if (AL)
        return ld2(p, i);
    double2 v;
    v.x = p[i];
    v.y = p[i + 1];
    return v;
}
template <bool AL>
__device__ __forceinline__ void ext_st2(double* p, int64_t i, double2 v)
{
    if (AL)
        st2(p, i, v);
    else
    {
        p[i] = v.x;
        p[i + 1] = v.y;
    }
}
__device__ __forceinline__ double nan_max(double m, double a) { return (a > m || a != a) ? a : m; }  // a NaN wins

// The loop of every vector pass: pairs of rows by 16-byte accesses in a grid-stride loop, then the last row of an odd n by the
// thread that follows the last pair's.  pair(i) handles rows i and i + 1, one(i) row i.
template <typename Pair, typename One>
__device__ __forceinline__ void for_rows(int64_t n, Pair&& pair, One&& one)
{
    const int64_t npair = n >> 1, stride = int64_t(gridDim.x) * kThreads;
    const int64_t first = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    for (int64_t j = first; j < npair; j += stride)
        pair(2 * j);
    if ((n & 1) && first == npair % stride)
        one(n - 1);
}

// max over the workgroup; every thread returns it
__device__ __forceinline__ double block_reduce_max(double v, double* red)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = nan_max(v, __shfl_down(v, off, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
        red[threadIdx.x >> 6] = v;
    __syncthreads();
    return nan_max(nan_max(red[0], red[1]), nan_max(red[2], red[3]));
}
__device__ __forceinline__ double block_sum(double v, double* red)
{
    __syncthreads();
    return block_reduce_sum(v, red);
}
// sum of the workgroups' records in a fixed order; every thread returns it
__device__ __forceinline__ double sum_partials(const double* __restrict__ partials, int nblocks, double* red)
{
    double a = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += kThreads)
        a += partials[i];
    return block_sum(a, red);
}

// ---- construction: diagonal and row sums of |.| of a CSR matrix (stored order) ------------------------------------------------
static __global__ __launch_bounds__(kThreads) void k_diag_rowsum(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                                  const double* __restrict__ val, int64_t n, double* __restrict__ diag,
                                                                  double* __restrict__ rowsum)
{
    const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= n)
        return;
    double d = 0.0, a = 0.0;
    for (int32_t p = rowptr[i]; p < rowptr[i + 1]; p++)
    {
        const double v = val[p];
        if (colind[p] == i)
            d += v;
        a += fabs(v);
    }
    diag[i] = d;
    rowsum[i] = a;
}

// ---- set_shift: max |d_i| and max_i (|A|_i + |sigma| |B|_i), then the preconditioner ------------------------------------------
static __global__ __launch_bounds__(kThreads) void k_shift_scan(int64_t n, double sigma, const double* __restrict__ dA,
                                                                 const double* __restrict__ dB, const double* __restrict__ aA,
                                                                 const double* __restrict__ aB, double* __restrict__ partials)
{
    __shared__ double red[4];
    double md = 0.0, mn = 0.0;
    for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += int64_t(gridDim.x) * kThreads)
    {
        md = nan_max(md, fabs(fma(-sigma, dB ? dB[i] : 1.0, dA[i])));
        mn = nan_max(mn, fma(fabs(sigma), aB ? aB[i] : 1.0, aA[i]));
    }
    md = block_reduce_max(md, red);
    mn = block_reduce_max(mn, red);
    if (threadIdx.x == 0)
    {
        partials[blockIdx.x] = md;
        partials[gridDim.x + blockIdx.x] = mn;
    }
}
// minv_i = 1 / |d_i| (Signed: 1 / d_i); an entry with |d_i| <= 2^-26 max |d| counts as max |d|.  Unsigned, the preconditioner
// stays positive definite, which MINRES needs; BiCGStab takes the signed one.
template <bool Signed>
static __global__ __launch_bounds__(kThreads) void k_precond(int64_t n, double sigma, const double* __restrict__ dA,
                                                              const double* __restrict__ dB, const double* __restrict__ norms,
                                                              double* __restrict__ minv)
{
    const double maxd = norms[0];
    const double floor_d = maxd * (1.0 / 67108864.0);
    for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += int64_t(gridDim.x) * kThreads)
    {
        const double ds = fma(-sigma, dB ? dB[i] : 1.0, dA[i]);
        const double d = fabs(ds);
        minv[i] = (d > floor_d) ? 1.0 / (Signed ? ds : d) : (maxd > 0.0 ? 1.0 / maxd : 1.0);
    }
}
// out[s] = max_b partials[s][b], s < nslots
static __global__ __launch_bounds__(kThreads) void k_max_slots(const double* __restrict__ partials, int nblocks, int nslots,
                                                                double* __restrict__ out)
{
    __shared__ double red[4];
    for (int s = 0; s < nslots; s++)
    {
        double m = 0.0;
        for (int i = threadIdx.x; i < nblocks; i += kThreads)
            m = nan_max(m, partials[s * nblocks + i]);
        m = block_reduce_max(m, red);
        if (threadIdx.x == 0)
            out[s] = m;
    }
}

// res = x - (p - sigma (q | y)) with p = A y, q = B y; records max |res|, max |y|, max |x|
template <bool AL>
static __global__ __launch_bounds__(kThreads) void k_residual(int64_t n, double sigma, const double* __restrict__ x,
                                                               const double* __restrict__ y, const double* __restrict__ p,
                                                               const double* __restrict__ q, double* __restrict__ res,
                                                               double* __restrict__ partials)
{
    __shared__ double red[4];
    double mr = 0.0, my = 0.0, mx = 0.0;
    const auto row = [&](double xv, double yv, double pv, double qv) {
        const double r = xv - fma(-sigma, qv, pv);
        mr = nan_max(mr, fabs(r));
        my = nan_max(my, fabs(yv));
        mx = nan_max(mx, fabs(xv));
        return r;
    };
    for_rows(
        n,
        [&](int64_t i) {
            const double2 xv = ext_ld2<AL>(x, i), yv = ld2(y, i), pv = ld2(p, i), qv = q ? ld2(q, i) : yv;
            double2 r;
            r.x = row(xv.x, yv.x, pv.x, qv.x);
            r.y = row(xv.y, yv.y, pv.y, qv.y);
            st2(res, i, r);
        },
        [&](int64_t i) { res[i] = row(x[i], y[i], p[i], q ? q[i] : y[i]); });
    mr = block_reduce_max(mr, red);
    my = block_reduce_max(my, red);
    mx = block_reduce_max(mx, red);
    if (threadIdx.x == 0)
    {
        partials[blockIdx.x] = mr;
        partials[gridDim.x + blockIdx.x] = my;
        partials[2 * gridDim.x + blockIdx.x] = mx;
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline std::string sci(double v)
{
    char buf[48];
    std::snprintf(buf, sizeof(buf), "%.3e", v);
    return buf;
}

// diag and row sums of |.| in the caller's index order
inline void diag_rowsum(const mispec_csr& A, int64_t n, DevBuf<double>& diag, DevBuf<double>& rowsum)
{
    diag.alloc(size_t(n) + 2);
    rowsum.alloc(size_t(n) + 2);
    hipStream_t st = A.ctx->stream;
    const dim3 grid(unsigned((n + kThreads - 1) / kThreads));
    if (!A.reordered())
    {
        hipLaunchKernelGGL(k_diag_rowsum, grid, dim3(kThreads), 0, st, A.rowptr.p, A.colind.p, A.val.p, n, diag.p, rowsum.p);
        MISPEC_HIP(hipGetLastError());
        return;
    }
    // the stored matrix is P A P': entry i of what the kernel computes belongs to row perm[i]
    DevBuf<double> d, r;
    d.alloc(size_t(n));
    r.alloc(size_t(n));
    hipLaunchKernelGGL(k_diag_rowsum, grid, dim3(kThreads), 0, st, A.rowptr.p, A.colind.p, A.val.p, n, d.p, r.p);
    MISPEC_HIP(hipGetLastError());
    launch_from_stored_order(A, d.p, diag.p);
    launch_from_stored_order(A, r.p, rowsum.p);
    MISPEC_HIP(hipStreamSynchronize(st));  // d and r are freed on return
}

// the grid of the vector passes and what both methods allocate at the first set_shift
inline void alloc_shared(ShiftIterative& M, const mispec_ctx& ctx, int64_t n)
{
    const size_t np = size_t(n) + 2;
    M.grid = int(std::max<int64_t>(1, std::min<int64_t>(((n + 1) / 2 + kThreads - 1) / kThreads, int64_t(ctx.num_cu) * 4)));
    M.minv.alloc(np);
    for (DevBuf<double>* v : {&M.p, &M.ycur, &M.res})
        v->alloc(np);
    M.partials.alloc(3 * size_t(M.grid));
    M.epi_partials.alloc(size_t(spmv_num_blocks(n)) + 1);
    M.norms.alloc(3);
    M.h_norms.alloc(3);
}

// set_shift's O(n) part: max |d|, the bound on |A - sigma B|_inf (kept in M.mnorm), the preconditioner
template <bool Signed>
inline void form_preconditioner(ShiftIterative& M, const mispec_ctx& ctx, int64_t n, double sigma, const double* dB, const double* aB)
{
    hipStream_t st = ctx.stream;
    const dim3 g(unsigned(M.grid)), b(kThreads);
    hipLaunchKernelGGL(k_shift_scan, g, b, 0, st, n, sigma, M.diagA.p, dB, M.absA.p, aB, M.partials.p);
    hipLaunchKernelGGL(k_max_slots, dim3(1), b, 0, st, M.partials.p, M.grid, 2, M.norms.p);
    hipLaunchKernelGGL(k_precond<Signed>, g, b, 0, st, n, sigma, M.diagA.p, dB, M.norms.p, M.minv.p);
    MISPEC_HIP(hipGetLastError());
    MISPEC_HIP(hipMemcpyAsync(M.h_norms.p, M.norms.p, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    MISPEC_HIP(hipStreamSynchronize(st));
    M.mnorm = M.h_norms.p[1];
    if (!(M.mnorm == M.mnorm) || !(sigma == sigma))
        throw Error(MISPEC_EINVAL, "SparseSymShiftSolve: the matrix or the shift is not finite");
}

// set_shift's probe: the probe right-hand side of the direct paths' calibration, solved by `solve` to the acceptance rule (which
// throws MISPEC_EINVAL for a shift it cannot solve)
template <typename Solve>
inline void solve_probe(mispec_symshift& S, ShiftIterative& M, double sigma, Solve&& solve)
{
    DevBuf<double> px, py;
    px.alloc(size_t(S.n) + 2);
    py.alloc(size_t(S.n) + 2);
    launch_probe_fill(*S.ctx, S.n, px.p);
    S.sigma = sigma;
    solve(px.p, py.p);
    MISPEC_HIP(hipStreamSynchronize(S.ctx->stream));
    S.refine_steps = 0;
    S.boosted_pivots = 0;
    S.min_pivot_ratio = 0.0;
    S.probe_backward_error = M.last_backward_error;
    M.probe_iterations = M.last_iterations;
}

// p = Op v where the pass still iterates (status: the record's done flag; the stop predicate rides on the product's epilogue,
// whose records nobody reads), or unconditionally (status == nullptr)
inline void product(const ShiftIterative& M, const mispec_csr& Op, const double* v, double* out, const int* status)
{
    if (!status)
    {
        launch_spmv(Op, v, out, nullptr);
        return;
    }
    SpmvEpilogue epi;
    epi.v_rows = v;
    epi.partials = M.epi_partials.p;
    epi.status = status;
    launch_spmv(Op, v, out, &epi);
}

// The explicit residual res = x - (A - sigma B) y with p = A y (q = B y) at hand, and the backward error
// omega = |res|_inf / (|M|_inf |y|_inf + |x|_inf).  Synchronises the stream.
inline double backward_error(ShiftIterative& M, const mispec_ctx& ctx, int64_t n, double sigma, const double* x_dev, const double* q)
{
    hipStream_t st = ctx.stream;
    const dim3 g(unsigned(M.grid)), b(kThreads);
    if (aligned16(x_dev))
        hipLaunchKernelGGL(k_residual<true>, g, b, 0, st, n, sigma, x_dev, M.ycur.p, M.p.p, q, M.res.p, M.partials.p);
    else
        hipLaunchKernelGGL(k_residual<false>, g, b, 0, st, n, sigma, x_dev, M.ycur.p, M.p.p, q, M.res.p, M.partials.p);
    hipLaunchKernelGGL(k_max_slots, dim3(1), b, 0, st, M.partials.p, M.grid, 3, M.norms.p);
    MISPEC_HIP(hipGetLastError());
    MISPEC_HIP(hipMemcpyAsync(M.h_norms.p, M.norms.p, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    MISPEC_HIP(hipStreamSynchronize(st));
    const double nr = M.h_norms.p[0], ny = M.h_norms.p[1], nx = M.h_norms.p[2];
    return nr / (M.mnorm * ny + nx);
}

// The acceptance rule of a solve of up to 1 + kMinresRestarts passes, its counters and its failure wording.
struct SolveRecord
{
    ShiftIterative& M;
    bool probe;
    int64_t used = 0;
    int passes = 0;
    double omega = 1.0, prev = std::numeric_limits<double>::infinity();

    void close()
    {
        M.last_iterations = used;
        M.last_passes = passes;
        M.last_backward_error = omega;
        M.total_iterations += used;
        M.solves += 1;
    }
    [[noreturn]] void fail(const std::string& why)
    {
        close();
        throw Error(probe ? MISPEC_EINVAL : MISPEC_ERUNTIME,
                    "SparseSymShiftSolve: the iterative solve with the given shift did not converge in " + std::to_string(used) +
                        " iterations (backward error " + sci(omega) + why + ")");
    }
    // what the next pass has to reduce its residual by, and the iterations it may take
    double need() const { return kMargin * std::min(1.0, M.tol / omega); }
    int cap() const { return int(std::max<int64_t>(0, int64_t(M.max_iterations) - used)); }
    void not_finite()
    {
        omega = std::numeric_limits<double>::quiet_NaN();
        fail("; the recurrence is not finite");
    }
    // after pass `pass` with the backward error `w` of its result: true = accepted, false = restart on the residual
    bool accepted(int pass, double w)
    {
        omega = w;
        if (!(omega == omega))
            fail("; the solution is not finite");
        if (omega <= M.tol)
            return true;
        const bool capped = used >= M.max_iterations;
        if (pass == kMinresRestarts || capped || (pass >= 1 && omega > 0.9 * prev))
        {
            if (omega <= std::max(M.tol, kMinresStagnation))  // stagnation at a backward error below the eigensolvers' tolerances
                return true;
            fail(capped ? "" : "; stagnating after " + std::to_string(passes) + " passes");
        }
        prev = omega;
        return false;
    }
};

}  // namespace shift_iter
}  // namespace mispec
