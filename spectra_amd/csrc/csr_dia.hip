// Diagonal storage of a banded / stencil matrix (SpMV format 2) — the automatic choice for BASELINE.json's matrices: the values
// of a 256-row block as one contiguous [nd][256] piece, y[r] = sum_k dia[k][r] * x[r + off_k] in ascending offset order (the CSR
// row sum's products in its order; absent entries add 0: bit-identical to it), no index, no gather.  k_spmv_dia_win2 — the
// headline kernel — handles two rows per thread with 16-byte loads and takes x from LDS windows; k_spmv_dia_win: one row per thread
// (unaligned operands); k_spmv_dia: direct x loads (offsets in more than 8 clusters).  Replaces SparseSymMatProd::perform_op /
// SparseGenMatProd::perform_op (MatOp/SparseSymMatProd.h:85-90) for such matrices.  Bound: HBM, 8 nstored n + 16 n bytes per product.
// Mirrored diagonals (option dia_sym): a diagonal -k whose values equal +k's bit for bit on every local row is not stored; the two
// windowed kernels read A(r, r - k) as the +k array's entry of row r - k — the same bits in the same place of the same sum — which
// the workgroup of that row streamed from HBM shortly before on the same XCD (lmap gives an XCD consecutive row blocks).
#include "csr_kernels.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

using namespace mispec;

namespace {

// ---- diagonal storage -----------------------------------------------------------------------------------------------
constexpr int kMaxDia = 32;      // diagonals of the diagonal format
constexpr int kDiaGroup = 8;     // loads issued together per thread: 8 values + 8 x entries
// dia_sym = auto mirrors the diagonals -k with k <= kDiaSymReach.  Measured on M-band at n = 1e7 (profiles/r15a): with
// the five near diagonals (k <= 1001, the partner's rows at most 4 row blocks back: L2) the product takes 0.200 ms, with the two far
// ones as well (k = 100001: 391 blocks, 8.6 MB of this XCD's traffic back — beyond L2, inside the Infinity Cache) 0.182 ms, against
// 0.238 ms with every diagonal stored.  Nothing further out has been measured: the reach ends at 1 MiB of x (csr.hpp kFarWindow).
constexpr int64_t kDiaSymReach = 131072;
// The windowed kernels' template parameter NG is the number of groups of eight diagonals, plus kDiaMir in the instantiations that
// read the mirror plan.  A matrix with nothing mirrored (dia_sym = 0, a non-symmetric band, diagonals that differ) runs the plain
// instantiations: every value at vrow + k * 256, nontemporal, no plan.
// (the encoding stays: bench.py and tests/test_host_profiles.py parse the demangled <EPI, NG, NCW, POST> by position)
constexpr int kDiaMir = 8;

// One thread per row: scatter the row's values into the [nd][256] piece of its 256-row block.  `pos_of_code` maps a dictionary
// code to the rank of its offset.  Within a row the ranks must increase strictly (columns sorted, no duplicates), else the diagonal
// sum would not be the CSR row sum bit for bit: such matrices raise *bad and keep the CSR kernels.
__global__ __launch_bounds__(256) void k_build_dia(const int32_t* __restrict__ rowptr, const uint8_t* __restrict__ codes,
                                                   const double* __restrict__ val, const int32_t* __restrict__ pos_of_code,
                                                   int64_t nloc, int nd, double* __restrict__ dia, int* __restrict__ bad)
{
    const int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (r >= nloc)
        return;
    int last = -1;
    for (int p = rowptr[r]; p < rowptr[r + 1]; p++)
    {
        const int pos = pos_of_code[codes[p]];
        if (pos <= last)
            *bad = 1;
        last = pos;
        dia[(int64_t(blockIdx.x) * nd + pos) * 256 + threadIdx.x] = val[p];
    }
}

// Candidate pairs of the mirror plan: diagonal lo (offset -k) against diagonal hi (offset +k), positions in the full array.
struct DiaPairs
{
    int count = 0;
    int lo[kMaxDia / 2], hi[kMaxDia / 2], k[kMaxDia / 2];
};
// bad[p] = 1 unless A(r, r - k) and A(r - k, r) hold the same 64 bits for every local row r with r - k local (absent entries are
// the +0.0 of the zeroed array on both sides; -0.0 and NaN payloads differ from it as integers)
__global__ __launch_bounds__(256) void k_dia_sym_check(const double* __restrict__ full, int nd, int64_t nloc, DiaPairs pairs,
                                                       int* __restrict__ bad)
{
    const int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (r >= nloc)
        return;
    const unsigned long long* bits = reinterpret_cast<const unsigned long long*>(full);
    for (int p = 0; p < pairs.count; p++)
    {
        const int64_t s = r - pairs.k[p];
        if (s < 0)
            continue;
        const unsigned long long a = bits[(int64_t(blockIdx.x) * nd + pairs.lo[p]) * 256 + threadIdx.x];
        const unsigned long long b = bits[((s >> 8) * nd + pairs.hi[p]) * 256 + (s & 255)];
        if (a != b)
            bad[p] = 1;
    }
}
// full [nd][256] blocks -> the plan's layout: the stored diagonals of every block behind plan.lead zeroed blocks, and in the lead
// what a mirrored read of the first local rows reaches: A(s, s + k) for s < 0 (local), taken from the local rows' own lower
// entries A(s + k, s).  On an unsharded matrix those columns do not exist and the lead stays zero.
__global__ __launch_bounds__(256) void k_dia_compact(const double* __restrict__ full, int nd, int64_t nloc, mispec_dia_plan plan,
                                                     double* __restrict__ out)
{
    const int64_t lb = blockIdx.x;
    const int t = threadIdx.x;
    const double* src = full + lb * nd * 256 + t;
    double* dst = out + (lb + plan.lead) * plan.nstored * 256 + t;
    const int64_t r = lb * 256 + t;
    for (int k = 0; k < nd; k++)
    {
        const double a = src[int64_t(k) * 256];
        const int sh = plan.shift[k];
        if (sh == 0)
            dst[int64_t(plan.slot(k)) * 256] = a;
        else if (r < sh && r < nloc)
        {
            const int64_t e = int64_t(plan.lead) * 256 + r - sh;
            out[((e >> 8) * plan.nstored + plan.slot(k)) * 256 + (e & 255)] = a;
        }
    }
}

// acc + a*b with the product rounded before the sum, as the CSR kernels do it (their products pass through LDS)
__device__ __forceinline__ double add_rounded_product(double acc, double a, double b)
{
#pragma clang fp contract(off)
    const double p = a * b;
    return acc + p;
}

struct DiaArgs
{
    const double* dia;  // block layout: dia[(block * nd + k) * 256 + r % 256] without a plan
    const int32_t* off;
    int nd;
    int col_max;
    int64_t row_begin;
    mispec_dia_plan plan;  // where each diagonal's values are: src[] / shift[] per diagonal (read by the NG >= kDiaMir
                           // instantiations only), [plan.nstored][256] per block, plan.lead blocks in front of block 0
};
// The plan's entries of the diagonals a thread keeps, read from the kernel arguments in one go at the top of a kernel (read where
// they are used, each value load would wait for a scalar load of its own).  Entries past nd repeat the last diagonal.
template <int N>
struct PlanRegs
{
    int src[N], shift[N];
    __device__ __forceinline__ explicit PlanRegs(const mispec_dia_plan& pl)
    {
#pragma unroll
        for (int k = 0; k < N; k++)
        {
            src[k] = pl.src[k];
            shift[k] = pl.shift[k];
        }
    }
};
// entry e (a row of the lead-extended block layout) of stored array src
__device__ __forceinline__ const double* dia_src(const DiaArgs& da, int src, int64_t e)
{
    return da.dia + ((e >> 8) * da.plan.nstored + (src & (mispec_dia_plan::kStream - 1))) * 256 + (e & 255);
}
// value of a diagonal for row e of the lead-extended layout (e >= 256 lead): a stored diagonal's own entry, a mirrored one's
// partner entry `shift` rows higher (never below entry 0: lead = ceil(largest shift / 256))
__device__ __forceinline__ double dia_load1(const DiaArgs& da, int src, int shift, int64_t e)
{
    const double* q = dia_src(da, src, e - shift);
    return (src & mispec_dia_plan::kStream) ? __builtin_nontemporal_load(q) : *q;
}
// rows e, e + 1 (e even).  Even shift: one aligned 16-byte load inside one block.  Odd shift: the two entries straddle two
// aligned pairs and, once per block, two blocks, which are nstored * 256 entries apart: two 8-byte loads (they hit L2).  The
// alternative — the aligned pair (e - shift + 1, e - shift + 2), the neighbour lane's second entry through a lane shuffle and the
// wave's missing entry loaded by its last lane, same register count — measured 0.271 ms per product on M-band against 0.182 ms
// with the two 8-byte loads (profiles/r15b_bench_dia_sym_ab.jsonl) and is gone.
__device__ __forceinline__ double2 dia_load2(const DiaArgs& da, int src, int shift, int64_t e)
{
    const bool nt = (src & mispec_dia_plan::kStream) != 0;
    if (shift & 1)
    {
        const double* q0 = dia_src(da, src, e - shift);
        const double* q1 = dia_src(da, src, e - shift + 1);
        if (nt)
            return make_double2(__builtin_nontemporal_load(q0), __builtin_nontemporal_load(q1));
        return make_double2(*q0, *q1);
    }
    const v2d* q = reinterpret_cast<const v2d*>(dia_src(da, src, e - shift));
    const v2d t2 = nt ? __builtin_nontemporal_load(q) : *q;
    return make_double2(t2.x, t2.y);
}

// The post-scaled step start (POST instantiations of the windowed kernels): reads beta = |f| from the step state, takes the
// beta < sqrt(eps) stop and records H(i,i-1) = beta.  Every block takes the same decision from the same beta; one thread (`first`)
// records it (Lanczos.h:99-128 without the restart branch).  Returns whether the block goes on.
__device__ __forceinline__ bool post_scaled_step_start(const SpmvEpilogue& epi, bool first, double& beta)
{
    StepState* st = static_cast<StepState*>(epi.post_scale_state);
    beta = st->beta;
    if (beta < epi.post_scale_eps_sqrt)
    {
        if (first)
        {
            st->status = kStepSmallBeta;
            st->stop_step = epi.post_scale_step;
            st->stop_count = 0;
        }
        return false;
    }
    if (first)
        st->subd[epi.post_scale_step - 1] = beta;
    return true;
}

template <bool EPI>
__global__ __launch_bounds__(256) void k_spmv_dia(DiaArgs da, const double* __restrict__ x, double* __restrict__ y, int64_t nrows,
                                                  int nblocks, SpmvEpilogue epi)
{
    __shared__ int off_s[kMaxDia];
    __shared__ double red[4];
    const int lmap = spmv_block_of_launch(nblocks);
    if (lmap < 0)
        return;
    const int lb = epi.first_block + lmap;  // a launch may cover a sub-range of the row-blocks (comm / compute overlap)
    if (EPI && epi.status && *epi.status != 0)
        return;
    const int tid = threadIdx.x;
    if (tid < da.nd)
        off_s[tid] = da.off[tid];
    __syncthreads();
    const int64_t row0 = int64_t(lb) * 256;
    const int nr = int(min(int64_t(256), nrows - row0));
    const int64_t r = row0 + min(tid, nr - 1);  // threads past the last row repeat it (their result is dropped)
    const double* vrow = da.dia + int64_t(lb) * da.nd * 256 + min(tid, nr - 1);
    const int64_t grow = da.row_begin + r;
    double acc = 0.0;
    for (int g = 0; g < da.nd; g += kDiaGroup)
    {
        double v[kDiaGroup], xv[kDiaGroup];
#pragma unroll
        for (int u = 0; u < kDiaGroup; u++)
        {
            const int d = min(g + u, da.nd - 1);
            v[u] = __builtin_nontemporal_load(vrow + int64_t(d) * 256);  // read once per SpMV
            const int64_t c = grow + off_s[d];
            xv[u] = x[min(max(c, int64_t(0)), int64_t(da.col_max))];  // out of range only where the value is a padding zero
        }
#pragma unroll
        for (int u = 0; u < kDiaGroup; u++)
            if (g + u < da.nd)
                acc = add_rounded_product(acc, v[u], xv[u]);  // no FMA: bit-identical to the CSR row sum
    }
    if (EPI)
    {
        double contrib = 0.0;
        if (tid < nr)
        {
            const int64_t row = row0 + tid;
            double yv = acc;
            if (epi.v_prev)
                yv -= (epi.h_prev_dev ? *epi.h_prev_dev : epi.h_prev) * epi.v_prev[row];  // Lanczos.h:139
            y[row] = yv;
            contrib = epi.v_rows[row] * yv;  // Lanczos.h:142 partial <v, w>
        }
        const double total = block_reduce_sum(contrib, red);
        if (tid == 0)
            epi.partials[lb] = total;
    }
    else if (tid < nr)
        y[row0 + tid] = acc;
}

// The same product with the x entries of a row-block staged through LDS: the offsets cluster, so a block of 256 rows reads
// a few contiguous windows of x (coalesced, once) instead of one 8-byte load per row and diagonal through the L1.
// NG = groups of eight diagonals whose values a thread keeps in registers.
// POST (one-sweep Lanczos steps only, fac.hip lanczos_step_lagged): the input is the UN-normalised residual f and the division
// by beta = |f| (read from the step state) is applied to the row sums and to the epilogue's v instead of to every window entry —
// w = (A f)/beta - beta v_prev, alpha partial = (f/beta) w — together with the step start that k_scale_step otherwise does
// (H(i,i-1) = beta, the beta < sqrt(eps) stop): no scaling pass and no scaled copy of f, two divisions per row.
template <bool EPI, int NG, int NCW = 8, bool POST = false>  // NCW: registers for window entries (>= number of windows)
__global__ __launch_bounds__(256) void k_spmv_dia_win(DiaArgs da, mispec_dia_windows w, const double* __restrict__ x,
                                                      double* __restrict__ y, int64_t nrows, int nblocks, SpmvEpilogue epi)
{
    extern __shared__ double xs[];
    __shared__ double red[4];
    constexpr bool MIR = NG >= kDiaMir;
    constexpr int NV = (NG % kDiaMir) * kDiaGroup;
    const PlanRegs<MIR ? NV : 1> pl(da.plan);
    const int lmap = spmv_block_of_launch(nblocks);
    if (lmap < 0)
        return;
    const int lb = epi.first_block + lmap;  // a launch may cover a sub-range of the row-blocks (comm / compute overlap)
    if (EPI && epi.status && *epi.status != 0)
        return;
    const int tid = threadIdx.x;
    double beta = 1.0;
    if (POST && !post_scaled_step_start(epi, lmap == 0 && tid == 0, beta))
        return;
    const int64_t row0 = int64_t(lb) * 256;
    const int nr = int(min(int64_t(256), nrows - row0));
    double v[NV];
    if constexpr (MIR)
    {
        const int64_t erow = (int64_t(da.plan.lead) + lb) * 256 + min(tid, nr - 1);  // threads past the last row repeat it
#pragma unroll
        for (int k = 0; k < NV; k++)
            v[k] = dia_load1(da, pl.src[k], pl.shift[k], erow);
    }
    else
    {
        const double* vrow = da.dia + int64_t(lb) * da.nd * 256 + min(tid, nr - 1);
#pragma unroll
        for (int k = 0; k < NV; k++)
            v[k] = __builtin_nontemporal_load(vrow + int64_t(min(k, da.nd - 1)) * 256);
    }
    // The epilogue's operands travel with the matrix values: issued here, they are in flight during the window staging and
    // the barrier instead of costing the block a second round trip to HBM after its row sums (the kernel is bound by the
    // number of resident blocks, i.e. by latency per block: profiles/rounds_1_2/r02r_*, r03q_*).
    double vprev_early = 0.0, vrow_early = 0.0, hprev_early = 0.0;
    const bool early = EPI && tid < nr;
    if (early)
    {
        if (epi.v_prev)
        {
            vprev_early = epi.v_prev[row0 + tid];
            hprev_early = POST ? beta : (epi.h_prev_dev ? *epi.h_prev_dev : epi.h_prev);
        }
        vrow_early = epi.v_rows[row0 + tid];
        if (POST)
            vrow_early = vrow_early / beta;  // Lanczos.h:106
    }
    const int64_t g0 = da.row_begin + row0;
    // x windows -> LDS.  A window is 256 + span entries: two per thread, ALL loaded before the first LDS write.  (Written as
    // a loop over windows and pieces, each piece was a load, a wait and a write: ten dependent round trips per block on the
    // five clusters of M-band, the latency the occupancy experiments of profiles/rounds_1_2/r02r_* were measuring.)
    const auto xat = [&](int64_t col) { return x[min(max(col, int64_t(0)), int64_t(da.col_max))]; };
    // entry tid of every window in a register of its own; the entries past 256 (the spans: 10 in all for M-band) one per
    // thread, thread t taking the t-th of them — 64 VGPRs in total, i.e. eight workgroups per CU as before
    double xw[NCW], xtail = 0.0;
    int tail_pos = -1;  // LDS slot of this thread's tail entry
    const int tails = w.total - 256 * w.nc;
    {
        int before = 0;
#pragma unroll
        for (int c = 0; c < NCW; c++)
        {
            xw[c] = 0.0;
            if (c < w.nc)
            {
                xw[c] = xat(g0 + w.start[c] + tid);
                const int span = w.len[c] - 256;
                if (tid >= before && tid < before + span)
                {
                    tail_pos = w.base[c] + 256 + (tid - before);
                    xtail = xat(g0 + w.start[c] + 256 + (tid - before));
                }
                before += span;
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < NCW; c++)
        if (c < w.nc)
            xs[w.base[c] + tid] = xw[c];
    if (tail_pos >= 0)
        xs[tail_pos] = xtail;
    if (tails > 256)  // more tail entries than threads (very wide clusters): the rest the slow way
    {
        int before = 0;
        for (int c = 0; c < w.nc; c++)
        {
            const int span = w.len[c] - 256;
            for (int t = tid + 256; t < before + span; t += 256)
                if (t >= before)
                {
                    const double xv = xat(g0 + w.start[c] + 256 + (t - before));
                    xs[w.base[c] + 256 + (t - before)] = xv;
                }
            before += span;
        }
    }
    __syncthreads();
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < NV; k++)
        if (k < da.nd)
            acc = add_rounded_product(acc, v[k], xs[w.idx[k] + tid]);
    if (EPI)
    {
        double contrib = 0.0;
        if (tid < nr)
        {
            const int64_t row = row0 + tid;
            double yv = POST ? acc / beta : acc;
            if (epi.v_prev)
                yv -= (early ? hprev_early : (epi.h_prev_dev ? *epi.h_prev_dev : epi.h_prev)) *
                      (early ? vprev_early : epi.v_prev[row]);  // Lanczos.h:139
            y[row] = yv;
            contrib = (early ? vrow_early : epi.v_rows[row]) * yv;  // Lanczos.h:142 partial <v, w>
        }
        const double total = block_reduce_sum(contrib, red);
        if (tid == 0)
            epi.partials[lb] = total;
    }
    else if (tid < nr)
        y[row0 + tid] = acc;
}

// Two rows per thread (round 5): the values of a 256-row block are read with 16-byte loads by 128 threads — half the load
// instructions per byte (the one-row-per-thread kernel above issues 8-byte loads, which the memory pipeline serves at 0.54-0.70 of
// the 16-byte rate: it moved 1.38 GB at 5.5 TB/s where the 16-byte kernels of this library reach 5.8-6.3) — rows 2t and 2t + 1,
// y / v_prev / v as 16-byte accesses too.  Same products in the same order, and the alpha record of the block is formed by the
// same tree as everywhere else (per-row contributions through LDS, then the four 64-row shuffle trees and (w0 + w1) + (w2 + w3)):
// bit-identical results and records.  Needs 16-byte aligned y / v vectors.
template <bool EPI, int NG, int NCW = 8, bool POST = false>
__global__ __launch_bounds__(128) void k_spmv_dia_win2(DiaArgs da, mispec_dia_windows w, const double* __restrict__ x,
                                                       double* __restrict__ y, int64_t nrows, int nblocks, SpmvEpilogue epi)
{
    extern __shared__ double xs[];  // windows, then 256 per-row contributions of the epilogue
    __shared__ double red[4];
    constexpr bool MIR = NG >= kDiaMir;
    constexpr int NV = (NG % kDiaMir) * kDiaGroup;
    const PlanRegs<MIR ? NV : 1> pl(da.plan);
    const int lmap = spmv_block_of_launch(nblocks);
    if (lmap < 0)
        return;
    const int lb = epi.first_block + lmap;
    if (EPI && epi.status && *epi.status != 0)
        return;
    const int tid = threadIdx.x;
    double beta = 1.0;
    if (POST && !post_scaled_step_start(epi, lmap == 0 && tid == 0, beta))
        return;
    const int64_t row0 = int64_t(lb) * 256;
    const int nr = int(min(int64_t(256), nrows - row0));
    const int r0 = 2 * tid;  // rows r0, r0 + 1 of the block (the value array is zero-padded to whole blocks)
    double2 v[NV];
    if constexpr (MIR)
    {
        const int64_t erow = (int64_t(da.plan.lead) + lb) * 256 + r0;
#pragma unroll
        for (int k = 0; k < NV; k++)
            v[k] = dia_load2(da, pl.src[k], pl.shift[k], erow);
    }
    else
    {
        const double* vrow = da.dia + int64_t(lb) * da.nd * 256 + r0;
#pragma unroll
        for (int k = 0; k < NV; k++)
        {
            const v2d t2 = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(vrow + int64_t(min(k, da.nd - 1)) * 256));
            v[k] = make_double2(t2.x, t2.y);
        }
    }
    double2 vprev_e = make_double2(0.0, 0.0), vrow_e = make_double2(0.0, 0.0);
    double hprev_e = 0.0;
    const bool have0 = r0 < nr, have1 = r0 + 1 < nr;
    if (EPI && have0)
    {
        if (epi.v_prev)
        {
            if (have1)
                vprev_e = *reinterpret_cast<const double2*>(epi.v_prev + row0 + r0);
            else
                vprev_e.x = epi.v_prev[row0 + r0];
            hprev_e = POST ? beta : (epi.h_prev_dev ? *epi.h_prev_dev : epi.h_prev);
        }
        if (have1)
            vrow_e = *reinterpret_cast<const double2*>(epi.v_rows + row0 + r0);
        else
            vrow_e.x = epi.v_rows[row0 + r0];
        if (POST)
        {
            vrow_e.x = vrow_e.x / beta;  // Lanczos.h:106
            vrow_e.y = vrow_e.y / beta;
        }
    }
    const int64_t g0 = da.row_begin + row0;
    const auto xat = [&](int64_t col) { return x[min(max(col, int64_t(0)), int64_t(da.col_max))]; };
    // windows -> LDS: entries tid and tid + 128 of every window, the entries past 256 (the spans) two per thread
    double xw[NCW][2], xtail[2] = {0.0, 0.0};
    int tail_pos[2] = {-1, -1};
    const int tails = w.total - 256 * w.nc;
    {
        int before = 0;
#pragma unroll
        for (int c = 0; c < NCW; c++)
        {
            xw[c][0] = xw[c][1] = 0.0;
            if (c < w.nc)
            {
                xw[c][0] = xat(g0 + w.start[c] + tid);
                xw[c][1] = xat(g0 + w.start[c] + tid + 128);
                const int span = w.len[c] - 256;
#pragma unroll
                for (int h = 0; h < 2; h++)
                {
                    const int t = tid + 128 * h;
                    if (t >= before && t < before + span)
                    {
                        tail_pos[h] = w.base[c] + 256 + (t - before);
                        xtail[h] = xat(g0 + w.start[c] + 256 + (t - before));
                    }
                }
                before += span;
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < NCW; c++)
        if (c < w.nc)
        {
            xs[w.base[c] + tid] = xw[c][0];
            xs[w.base[c] + tid + 128] = xw[c][1];
        }
#pragma unroll
    for (int h = 0; h < 2; h++)
        if (tail_pos[h] >= 0)
            xs[tail_pos[h]] = xtail[h];
    if (tails > 256)
    {
        int before = 0;
        for (int c = 0; c < w.nc; c++)
        {
            const int span = w.len[c] - 256;
            for (int t = tid + 256; t < before + span; t += 128)
                if (t >= before)
                    xs[w.base[c] + 256 + (t - before)] = xat(g0 + w.start[c] + 256 + (t - before));
            before += span;
        }
    }
    __syncthreads();
    double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
    for (int k = 0; k < NV; k++)
        if (k < da.nd)
        {
            acc0 = add_rounded_product(acc0, v[k].x, xs[w.idx[k] + r0]);
            acc1 = add_rounded_product(acc1, v[k].y, xs[w.idx[k] + r0 + 1]);
        }
    if (EPI)
    {
        double* cbuf = xs + w.total;  // per-row contributions of the block
        double c0 = 0.0, c1 = 0.0;
        double2 yv;
        yv.x = POST ? acc0 / beta : acc0;
        yv.y = POST ? acc1 / beta : acc1;
        if (epi.v_prev)
        {
            yv.x -= hprev_e * vprev_e.x;  // Lanczos.h:139
            yv.y -= hprev_e * vprev_e.y;
        }
        if (have1)
            *reinterpret_cast<double2*>(y + row0 + r0) = yv;
        else if (have0)
            y[row0 + r0] = yv.x;
        if (have0)
            c0 = vrow_e.x * yv.x;  // Lanczos.h:142 partial <v, w>
        if (have1)
            c1 = vrow_e.y * yv.y;
        cbuf[r0] = c0;
        cbuf[r0 + 1] = c1;
        __syncthreads();
        // the record's tree: wave k of a 256-thread block sums rows 64 k .. 64 k + 63 by shuffles, then (w0 + w1) + (w2 + w3)
        const int wv = tid >> 6, lane = tid & 63;
#pragma unroll
        for (int h = 0; h < 2; h++)
        {
            const int k = 2 * wv + h;
            const double s = wave_reduce_sum(cbuf[64 * k + lane]);
            if (lane == 0)
                red[k] = s;
        }
        __syncthreads();
        if (tid == 0)
            epi.partials[lb] = (red[0] + red[1]) + (red[2] + red[3]);
    }
    else
    {
        if (have1)
            *reinterpret_cast<double2*>(y + row0 + r0) = make_double2(acc0, acc1);
        else if (have0)
            y[row0 + r0] = acc0;
    }
}

// The rule of option dia_sym (host only): flags[i] = 1 where diagonal i has a negative offset -k, +k is in the dictionary and
// k <= reach (reach < 0: no limit).  Returns ceil(largest such k / 256), the lead blocks a plan of these diagonals needs.
int dia_sym_rule(const int32_t* offs, int nd, int64_t reach, int32_t* flags)
{
    int64_t kmax = 0;
    for (int i = 0; i < nd; i++)
    {
        flags[i] = 0;
        const int64_t k = -int64_t(offs[i]);
        if (k <= 0 || (reach >= 0 && k > reach))
            continue;
        for (int j = 0; j < nd; j++)
            if (int64_t(offs[j]) == k)
                flags[i] = 1;
        if (flags[i])
            kmax = std::max(kmax, k);
    }
    return int((kmax + 255) / 256);
}

// plan from the flags of the diagonals that are mirrored (offsets ascending): slots in ascending order of the stored ones
mispec_dia_plan make_plan(const int32_t* offs, int nd, const int32_t* mirrored)
{
    mispec_dia_plan pl;
    int64_t kmax = 0;
    for (int i = 0; i < nd; i++)
    {
        pl.shift[i] = mirrored[i] ? -offs[i] : 0;
        if (!mirrored[i])
            pl.src[i] = pl.nstored++ + mispec_dia_plan::kStream;
        else
            kmax = std::max<int64_t>(kmax, -int64_t(offs[i]));
    }
    pl.lead = int((kmax + 255) / 256);
    for (int i = 0; i < nd; i++)
        if (mirrored[i])
            for (int j = 0; j < nd; j++)
                if (offs[j] == -offs[i])
                {
                    pl.src[j] = pl.slot(j);  // read again by the mirrored diagonal: not nontemporal, its lines stay in L2
                    // mirrored reads, and the stored loads they come back to, are plain loads: nontemporal ones measured as a loss
                    // on data that is read again, and nontemporal mirrored reads made no difference where they were tried (on the
                    // 16-byte variant of dia_load2's odd case, profiles/r15b_bench_dia_sym_ab.jsonl)
                    pl.src[i] = pl.slot(j);
                }
    for (int i = nd; i < 32; i++)  // the kernels load whole groups of eight: the rest repeat the last diagonal
    {
        pl.src[i] = pl.src[nd - 1];
        pl.shift[i] = pl.shift[nd - 1];
    }
    return pl;
}

}  // namespace

extern "C" int mispec_dia_sym_plan(const int32_t* offsets, int nd, int64_t reach, int32_t* out_flags, int* lead_blocks)
{
    return guarded([&] {
        MISPEC_REQUIRE(nd >= 0 && nd <= kMaxDia && (nd == 0 || (offsets && out_flags)), "mispec_dia_sym_plan: bad argument");
        const int lead = dia_sym_rule(offsets, nd, reach, out_flags);
        if (lead_blocks)
            *lead_blocks = lead;
    });
}

extern "C" int mispec_csr_dia_info(const mispec_csr* A, int* ndia, int* nstored, int* nmirrored, int* lead_blocks)
{
    return guarded([&] {
        MISPEC_REQUIRE(A, "mispec_csr_dia_info: NULL argument");
        if (ndia)
            *ndia = A->ndia;
        if (nstored)
            *nstored = A->ndia ? A->dia_plan.nstored : 0;
        if (nmirrored)
            *nmirrored = A->ndia ? A->ndia - A->dia_plan.nstored : 0;
        if (lead_blocks)
            *lead_blocks = A->ndia ? A->dia_plan.lead : 0;
    });
}

namespace mispec {

// Diagonal storage from the offset codes (device): only for small, well-filled dictionaries whose rows are sorted and free
// of duplicates; anything else keeps the CSR kernels (mispec_csr_set_spmv_format selects among the formats a matrix has).
void build_dia(mispec_csr& A, const std::vector<int32_t>& dict)
{
    const int64_t nloc = A.local_rows();
    const int nd = int(dict.size());
    if (nd == 0 || nd > kMaxDia || nloc == 0 || double(A.nnz) < 0.75 * double(nd) * double(nloc))
        return;
    std::vector<int32_t> order(static_cast<size_t>(nd)), pos(static_cast<size_t>(nd)), offs(static_cast<size_t>(nd));
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return dict[size_t(a)] < dict[size_t(b)]; });
    for (int k = 0; k < nd; k++)
    {
        pos[size_t(order[size_t(k)])] = k;
        offs[size_t(k)] = dict[size_t(order[size_t(k)])];
    }
    // the values of a 256-row block are stored as one contiguous [nd][256] piece, so a workgroup streams ONE 30 KB run instead
    // of nd runs of 2 KB that are 80 MB apart (the diagonal-major layout dia[k][row] of round 1 measured 1.5 % slower and is gone)
    const int64_t ld = round_up(nloc, 256);
    DevBuf<int32_t> d_pos;
    DevBuf<int> d_bad;
    d_pos.alloc(size_t(nd));
    d_bad.alloc(1);
    A.dia.alloc(size_t(ld) * size_t(nd));
    A.dia_off.alloc(size_t(nd));
    hipStream_t st = A.ctx->stream;
    MISPEC_HIP(hipMemsetAsync(A.dia.p, 0, A.dia.n * sizeof(double), st));
    MISPEC_HIP(hipMemsetAsync(d_bad.p, 0, sizeof(int), st));
    MISPEC_HIP(hipMemcpyAsync(d_pos.p, pos.data(), pos.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    MISPEC_HIP(hipMemcpyAsync(A.dia_off.p, offs.data(), offs.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_build_dia, dim3(unsigned((nloc + 255) / 256)), dim3(256), 0, st, A.rowptr.p, A.codes.p, A.val.p, d_pos.p, nloc, nd,
                       A.dia.p, d_bad.p);
    MISPEC_HIP(hipGetLastError());
    int bad = 0;
    MISPEC_HIP(hipMemcpyAsync(&bad, d_bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
    MISPEC_HIP(hipStreamSynchronize(st));
    if (bad)
    {
        A.dia.release();
        A.dia_off.release();
        return;
    }
    A.ndia = nd;
    // x windows: consecutive sorted offsets share a window while it stays within 256 + 256 entries
    mispec_dia_windows w;
    int first = 0;
    bool ok = true;
    for (int k = 0; k <= nd && ok; k++)
        if (k == nd || int64_t(offs[size_t(k)]) - int64_t(offs[size_t(first)]) > 256)
        {
            if (w.nc == 8)
            {
                ok = false;
                break;
            }
            const int c = w.nc++;
            w.start[c] = offs[size_t(first)];
            w.len[c] = 256 + (offs[size_t(k) - 1] - offs[size_t(first)]);
            w.base[c] = w.total;
            for (int d = first; d < k; d++)
                w.idx[d] = w.total + (offs[size_t(d)] - offs[size_t(first)]);
            w.total += w.len[c];
            first = k;
        }
    if (ok)
        A.dia_win = w;
    // Mirror plan (option dia_sym).  The direct kernel k_spmv_dia (no windows) keeps every diagonal.
    const std::vector<int32_t> none(static_cast<size_t>(nd), 0);
    A.dia_plan = make_plan(offs.data(), nd, none.data());
    const DiaSym sym = option_choice(Opt::dia_sym, DiaSym::automatic);
    if (!ok || sym == DiaSym::off)
        return;
    std::vector<int32_t> flags(static_cast<size_t>(nd), 0);
    dia_sym_rule(offs.data(), nd, sym == DiaSym::all ? int64_t(-1) : kDiaSymReach, flags.data());
    DiaPairs pairs;
    int which[kMaxDia / 2];
    for (int i = 0; i < nd; i++)
        if (flags[size_t(i)])
        {
            const int p = pairs.count++;
            which[p] = i;
            pairs.lo[p] = i;
            pairs.hi[p] = int(std::find(offs.begin(), offs.end(), -offs[size_t(i)]) - offs.begin());
            pairs.k[p] = -offs[size_t(i)];
        }
    if (pairs.count == 0)
        return;
    DevBuf<int> d_asym;
    d_asym.alloc(size_t(pairs.count));
    MISPEC_HIP(hipMemsetAsync(d_asym.p, 0, size_t(pairs.count) * sizeof(int), st));
    const unsigned nblk = unsigned(ld / 256);
    hipLaunchKernelGGL(k_dia_sym_check, dim3(nblk), dim3(256), 0, st, A.dia.p, nd, nloc, pairs, d_asym.p);
    MISPEC_HIP(hipGetLastError());
    int asym[kMaxDia / 2] = {};
    MISPEC_HIP(hipMemcpyAsync(asym, d_asym.p, size_t(pairs.count) * sizeof(int), hipMemcpyDeviceToHost, st));
    MISPEC_HIP(hipStreamSynchronize(st));
    int nmir = 0;
    for (int p = 0; p < pairs.count; p++)
    {
        if (asym[p])
            flags[size_t(which[p])] = 0;  // differs somewhere: stays stored
        nmir += flags[size_t(which[p])];
    }
    if (nmir == 0)
        return;
    const mispec_dia_plan plan = make_plan(offs.data(), nd, flags.data());
    DevBuf<double> packed;
    packed.alloc(size_t(ld + 256 * int64_t(plan.lead)) * size_t(plan.nstored));
    MISPEC_HIP(hipMemsetAsync(packed.p, 0, packed.n * sizeof(double), st));
    hipLaunchKernelGGL(k_dia_compact, dim3(nblk), dim3(256), 0, st, A.dia.p, nd, nloc, plan, packed.p);
    MISPEC_HIP(hipGetLastError());
    MISPEC_HIP(hipStreamSynchronize(st));
    A.dia.swap(packed);
    A.dia_plan = plan;
}

void launch_spmv_dia(const mispec_csr& A, const SpmvLaunch& L)
{
    const DiaArgs da{A.dia.p, A.dia_off.p, A.ndia, int(A.n_cols - 1), A.row_begin, A.dia_plan};
    // with mirrored diagonals the instantiations that read the plan (NG + kDiaMir)
    const bool mir = A.dia_plan.nstored != A.ndia;
    MISPEC_REQUIRE(!mir || A.dia_win.nc > 0, "diagonal storage: a mirror plan needs x windows");
    const int ng = (A.ndia + kDiaGroup - 1) / kDiaGroup + (mir ? kDiaMir : 0);
    const bool post = L.epi && L.e.post_scale_state;
    const auto launch = [&](auto kernel, dim3 block, size_t lds, const auto&... operands) {
        launch_kernel(kernel, L.grid, block, lds, A.ctx->stream, L.ev_start, L.ev_stop, da, operands..., L.x_dev, L.y_dev, L.nloc,
                      L.nblocks, L.e);
        MISPEC_HIP(hipGetLastError());
    };
    // x staged through LDS windows when the offsets form at most 8 clusters, else direct loads (k_spmv_dia)
    if (A.dia_win.nc == 0)
    {
        with_bool(L.epi != nullptr, [&](auto E) { launch(k_spmv_dia<E()>, L.block, 0); });
        return;
    }
    // two rows per thread with 16-byte loads (k_spmv_dia_win2) when the number of diagonals and the alignment allow
    const auto aligned16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool dia2 = A.ndia <= 2 * kDiaGroup && aligned16(L.y_dev) && (!L.epi || (aligned16(L.e.v_rows) && aligned16(L.e.v_prev)));
    with_bool(L.epi != nullptr, [&](auto E) {
        with_bool(post, [&](auto P) {
            with_tier<4, 6, 8>(A.dia_win.nc, [&](auto W) {
                if constexpr (E() || !P())  // POST only with EPI
                {
                    if (dia2)
                        with_tier<1, 2, kDiaMir + 1, kDiaMir + 2>(ng, [&](auto G) {
                            launch(k_spmv_dia_win2<E(), G(), W(), P()>, dim3(128), size_t(A.dia_win.total + 256) * sizeof(double), A.dia_win);
                        });
                    else
                        with_tier<1, 2, 3, 4, kDiaMir + 1, kDiaMir + 2, kDiaMir + 3, kDiaMir + 4>(ng, [&](auto G) {
                            launch(k_spmv_dia_win<E(), G(), W(), P()>, L.block, size_t(A.dia_win.total) * sizeof(double), A.dia_win);
                        });
                }
            });
        });
    });
}

}  // namespace mispec
