// Block product Y = A X for a panel of k vectors in one pass over A (launch_spmm, mispec_spmm*), gfx950.
//
// The k columns are cut into panels of KB = 8, 4 or 2 columns (spmm_plan below: 8s, then a 4, then a 2 as far as option spmm
// allows the width; remaining single columns are ordinary launch_spmv calls).  Per panel:
//   * k_spmm_pack<KB> interleaves the panel of X: Xp[j * KB + c] = X[j + c * ldx] (X[perm[j] + c * ldx] for a reordered matrix,
//     so the gather into the stored order costs no pass of its own).  One stored entry then needs KB * 8 contiguous bytes of
//     Xp, fetched with 16-byte loads, instead of KB scattered 8-byte loads;
//   * k_spmm_csr<KB> works on the plain int32 CSR arrays that every mispec_csr keeps, whatever format its SpMV uses: a
//     workgroup of 256 threads owns 256 consecutive rows (the XCD-aware block map of k_spmv_csr_stream), streams its run of
//     val / colind once with coalesced 16-byte loads into LDS, and thread r then walks row r's entries in storage order with KB
//     accumulators in registers.  Rows longer than a chunk are summed across chunks.
// Arithmetic: one accumulator per (row, column) starting at 0.0, entries added in storage order, every product rounded
// before it is added (add_rounded_product below: no contraction into an fma) — the order and the roundings of every SpMV
// format and of the CPU row-dot, so the block product is bit-identical to k single products.  No atomics; the result does not
// depend on the launch geometry; nothing outside the padded arrays is read.
// Bound: HBM.  Algorithmic bytes of a panel: 12 nnz + 4 (rows + 1) + 8 KB (cols + rows), plus the pack's 16 KB cols.
#include "csr_kernels.hpp"

#include <algorithm>

using namespace mispec;

namespace {

constexpr int kSpmmThreads = 256;  // rows per workgroup, one thread per row in the summation phase
constexpr int kSpmmIters = 2;      // 16-byte load groups per thread and chunk
// entries per LDS chunk: kSpmmIters * 4 * 256 >= cap + 3 (the chunk starts at a multiple of 4 at most 3 entries early)
constexpr int kSpmmCap = kSpmmThreads * 4 * kSpmmIters - 16;
constexpr int kSpmmLdsBytes = (kSpmmCap + 4) * int(sizeof(double) + sizeof(int32_t));
constexpr int kLdsPerCu = 160 * 1024;
static_assert(kSpmmThreads * 4 * kSpmmIters >= kSpmmCap + 3, "the load steps of a chunk cover it");
static_assert(4 * kSpmmLdsBytes <= kLdsPerCu, "at least four workgroups of k_spmm_csr fit in the LDS of a CU");

// acc + round(v * x).  hipcc contracts a product and a sum into an fma unless told otherwise (-ffp-contract=fast-honor-pragmas is its
// default) and this ROCm's __dmul_rn / __dadd_rn are the plain operators, which contract as well: the pragma is what keeps the
// product rounded, as it is in every SpMV kernel (they round it through LDS) and in the CPU row-dot.
__device__ __forceinline__ double add_rounded_product(double acc, double v, double x)
{
#pragma clang fp contract(off)
    const double p = v * x;
    return acc + p;
}

template <int KB>
__global__ __launch_bounds__(256) void k_spmm_pack(int64_t ncols, const int32_t* __restrict__ perm, const double* __restrict__ X,
                                                    int64_t ldx, double* __restrict__ Xp)
{
    const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (j >= ncols)
        return;
    const int64_t src = perm ? int64_t(perm[j]) : j;
    double2* out = reinterpret_cast<double2*>(Xp + j * KB);
#pragma unroll
    for (int c = 0; c < KB; c += 2)
        out[c >> 1] = make_double2(X[src + int64_t(c) * ldx], X[src + int64_t(c + 1) * ldx]);
}

template <int KB>
__global__ __launch_bounds__(kSpmmThreads) void k_spmm_csr(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colind,
                                                            const double* __restrict__ val, const double* __restrict__ Xp,
                                                            const int32_t* __restrict__ perm, double* __restrict__ Y, int64_t ldy,
                                                            int64_t nrows, int nblocks)
{
    __shared__ __attribute__((aligned(16))) double s_val[kSpmmCap + 4];
    __shared__ __attribute__((aligned(16))) int32_t s_col[kSpmmCap + 4];

    const int lb = spmv_block_of_launch(nblocks);
    if (lb < 0)
        return;

    const int tid = threadIdx.x;
    const int64_t row0 = int64_t(lb) * kSpmmThreads;
    const int nr = int(min(int64_t(kSpmmThreads), nrows - row0));
    const int bs = rowptr[row0];
    const int be = rowptr[row0 + nr];
    int rs = 0, re = 0;
    if (tid < nr)
    {
        rs = rowptr[row0 + tid];
        re = rowptr[row0 + tid + 1];
    }

    double acc[KB];
#pragma unroll
    for (int c = 0; c < KB; c++)
        acc[c] = 0.0;

    for (int cs = bs; cs < be;)
    {
        const int a0 = cs & ~3;  // 32-byte aligned start for the vector loads
        const int ce = min(be, a0 + kSpmmCap);
        // the chunk's values and column indices -> LDS.  Lanes past the end of the chunk re-read its last aligned group (inside
        // the padded arrays) and store nothing.
        const int last = (ce - 1) & ~3;
        double2 va[kSpmmIters][2];
        int4 ci[kSpmmIters];
#pragma unroll
        for (int it = 0; it < kSpmmIters; it++)
        {
            const int base = min(a0 + tid * 4 + it * (kSpmmThreads * 4), last);
            va[it][0] = *reinterpret_cast<const double2*>(val + base);
            va[it][1] = *reinterpret_cast<const double2*>(val + base + 2);
            ci[it] = *reinterpret_cast<const int4*>(colind + base);
        }
#pragma unroll
        for (int it = 0; it < kSpmmIters; it++)
        {
            const int base = a0 + tid * 4 + it * (kSpmmThreads * 4);
            if (base < ce)
            {
                *reinterpret_cast<double2*>(&s_val[base - a0]) = va[it][0];
                *reinterpret_cast<double2*>(&s_val[base - a0 + 2]) = va[it][1];
                *reinterpret_cast<int4*>(&s_col[base - a0]) = ci[it];
            }
        }
        __syncthreads();
        // thread r: the part of row r inside [cs, ce), in storage order; two entries' panel rows in flight
        const int lo = max(rs, cs), hi = min(re, ce);
        int k = lo;
        for (; k + 2 <= hi; k += 2)
        {
            const double v0 = s_val[k - a0], v1 = s_val[k - a0 + 1];
            const double2* x0 = reinterpret_cast<const double2*>(Xp + int64_t(s_col[k - a0]) * KB);
            const double2* x1 = reinterpret_cast<const double2*>(Xp + int64_t(s_col[k - a0 + 1]) * KB);
            double2 a[KB / 2], b[KB / 2];
#pragma unroll
            for (int c = 0; c < KB / 2; c++)
            {
                a[c] = x0[c];
                b[c] = x1[c];
            }
#pragma unroll
            for (int c = 0; c < KB / 2; c++)
            {
                acc[2 * c] = add_rounded_product(acc[2 * c], v0, a[c].x);
                acc[2 * c + 1] = add_rounded_product(acc[2 * c + 1], v0, a[c].y);
            }
#pragma unroll
            for (int c = 0; c < KB / 2; c++)
            {
                acc[2 * c] = add_rounded_product(acc[2 * c], v1, b[c].x);
                acc[2 * c + 1] = add_rounded_product(acc[2 * c + 1], v1, b[c].y);
            }
        }
        if (k < hi)
        {
            const double v0 = s_val[k - a0];
            const double2* x0 = reinterpret_cast<const double2*>(Xp + int64_t(s_col[k - a0]) * KB);
#pragma unroll
            for (int c = 0; c < KB / 2; c++)
            {
                const double2 a = x0[c];
                acc[2 * c] = add_rounded_product(acc[2 * c], v0, a.x);
                acc[2 * c + 1] = add_rounded_product(acc[2 * c + 1], v0, a.y);
            }
        }
        cs = ce;
        if (cs < be)
            __syncthreads();  // the next chunk overwrites the LDS arrays
    }

    if (tid < nr)
    {
        // column-major, coalesced per column; a reordered matrix writes the caller's row
        const int64_t row = perm ? int64_t(perm[row0 + tid]) : row0 + tid;
#pragma unroll
        for (int c = 0; c < KB; c++)
            Y[row + int64_t(c) * ldy] = acc[c];
    }
}

template <int KB>
void launch_panel(const mispec_csr& A, const double* X, int64_t ldx, double* Y, int64_t ldy)
{
    const int64_t nloc = A.local_rows();
    const int nblocks = spmv_num_blocks(nloc);
    hipStream_t st = A.ctx->stream;
    if (A.n_cols > 0)
        hipLaunchKernelGGL((k_spmm_pack<KB>), dim3(unsigned((A.n_cols + 255) / 256)), dim3(256), 0, st, A.n_cols, A.perm.p, X, ldx,
                           A.spmm_x.p);
    MISPEC_HIP(hipGetLastError());
    hipLaunchKernelGGL((k_spmm_csr<KB>), dim3(spmv_grid_blocks(nblocks)), dim3(kSpmmThreads), 0, st, A.rowptr.p, A.colind.p, A.val.p,
                       A.spmm_x.p, A.perm.p, Y, ldy, nloc, nblocks);
    MISPEC_HIP(hipGetLastError());
}

// Panel widths that `auto` uses, widest first.  A width stays here only while one panel of it measures faster than as many
// single products in the matrix's automatic SpMV format on both benchmark matrices (tools/bench_spmm.py).
// Width 2 lost on M-band, whose single product runs on diagonal storage (8 instead of 12 bytes per entry): 0.535 against
// 2 x 0.226 ms; it stays available as option spmm=2 and as the tail of spmm=4 / 8.
constexpr int kAutoWidths[] = {8, 4};

// The cut of k columns into panels: for every width allowed, widest first, as many panels as fit; what remains is single columns.
// forced: 0 follow option spmm, 1 single columns only, 2 | 4 | 8 the widest panel.
std::vector<int> spmm_plan(int k, int forced)
{
    MISPEC_REQUIRE(k >= 0, "mispec_spmm_plan: k < 0");
    MISPEC_REQUIRE(forced == 0 || forced == 1 || forced == 2 || forced == 4 || forced == 8,
                   "mispec_spmm_plan: forced_panel is one of 0 (option spmm), 1, 2, 4, 8");
    int allowed[3] = {0, 0, 0}, na = 0;
    const Spmm opt = forced == 0 ? option_choice(Opt::spmm, Spmm::automatic) : Spmm::automatic;
    if (forced == 0 && opt == Spmm::automatic)
        for (const int w : kAutoWidths)
            allowed[na++] = w;
    else
    {
        const int cap = forced ? forced : (opt == Spmm::off ? 1 : opt == Spmm::w2 ? 2 : opt == Spmm::w4 ? 4 : 8);
        for (int w = 8; w >= 2; w >>= 1)
            if (w <= cap)
                allowed[na++] = w;
    }
    std::vector<int> widths;
    for (int i = 0; i < na; i++)
        for (; k >= allowed[i]; k -= allowed[i])
            widths.push_back(allowed[i]);
    widths.insert(widths.end(), size_t(k), 1);
    return widths;
}

void require_spmm_args(const mispec_csr& A, const double* X_dev, int64_t ldx, int k, double* Y_dev, int64_t ldy)
{
    MISPEC_REQUIRE(X_dev && Y_dev, "mispec_spmm: NULL argument");
    MISPEC_REQUIRE(k >= 0, "mispec_spmm: k < 0");
    MISPEC_REQUIRE(ldx >= A.n_cols && ldy >= A.n_rows, "mispec_spmm: leading dimension too small");
    MISPEC_REQUIRE(A.ctx->world() == 1, "mispec_spmm: block products need an unsharded matrix");
}

}  // namespace

namespace mispec {

void launch_spmm(const mispec_csr& A, const double* X_dev, int64_t ldx, int k, double* Y_dev, int64_t ldy)
{
    require_spmm_args(A, X_dev, ldx, k, Y_dev, ldy);
    if (k == 0 || A.local_rows() == 0)
        return;
    const std::vector<int> widths = spmm_plan(k, 0);
    int c = 0;
    for (const int w : widths)
    {
        const double* X = X_dev + int64_t(c) * ldx;
        double* Y = Y_dev + int64_t(c) * ldy;
        if (w == 1)
            launch_spmv(A, X, Y, nullptr);
        else
        {
            if (A.spmm_x.n < size_t(A.n_cols) * size_t(widths[0]))
                A.spmm_x.alloc(size_t(A.n_cols) * size_t(widths[0]));  // the plan's widest panel comes first
            if (w == 8)
                launch_panel<8>(A, X, ldx, Y, ldy);
            else if (w == 4)
                launch_panel<4>(A, X, ldx, Y, ldy);
            else
                launch_panel<2>(A, X, ldx, Y, ldy);
        }
        c += w;
    }
}

}  // namespace mispec

extern "C" int mispec_spmm_plan(int k, int forced_panel, int* widths_out, int cap, int* count)
{
    return guarded([&] {
        MISPEC_REQUIRE(count != nullptr, "mispec_spmm_plan: count is NULL");
        const std::vector<int> widths = spmm_plan(k, forced_panel);
        MISPEC_REQUIRE(int64_t(widths.size()) <= int64_t(cap < 0 ? 0 : cap) && (widths.empty() || widths_out),
                       "mispec_spmm_plan: widths_out holds fewer than the " + std::to_string(widths.size()) + " panels of the plan");
        std::copy(widths.begin(), widths.end(), widths_out);
        *count = int(widths.size());
    });
}

extern "C" int mispec_spmm(const mispec_csr* A, const double* X_dev, int64_t ldx, int k, double* Y_dev, int64_t ldy)
{
    return guarded([&] {
        MISPEC_REQUIRE(A, "mispec_spmm: NULL argument");
        A->ctx->make_current();
        launch_spmm(*A, X_dev, ldx, k, Y_dev, ldy);
    });
}

extern "C" int mispec_spmm_time(const mispec_csr* A, const double* X_dev, int64_t ldx, int k, double* Y_dev, int64_t ldy, int reps,
                                float* ms_per_launch)
{
    return guarded([&] {
        MISPEC_REQUIRE(A && reps > 0 && ms_per_launch, "mispec_spmm_time: bad argument");
        require_spmm_args(*A, X_dev, ldx, k, Y_dev, ldy);
        A->ctx->make_current();
        hipEvent_t e0, e1;
        MISPEC_HIP(hipEventCreate(&e0));
        MISPEC_HIP(hipEventCreate(&e1));
        MISPEC_HIP(hipEventRecord(e0, A->ctx->stream));
        for (int i = 0; i < reps; i++)
            launch_spmm(*A, X_dev, ldx, k, Y_dev, ldy);  // the whole block product: packs, panels, single columns
        MISPEC_HIP(hipEventRecord(e1, A->ctx->stream));
        MISPEC_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        MISPEC_HIP(hipEventElapsedTime(&ms, e0, e1));
        (void) hipEventDestroy(e0);
        (void) hipEventDestroy(e1);
        *ms_per_launch = ms / float(reps);
    });
}
