// The one-sweep orthogonalisation pass (krylov.hip k_orth_lagged, ORTH_LAGGED) with the basis streamed through an LDS ring by
// LDS-DMA (`global_load_lds_dwordx4`) instead of through registers — round 6, VERDICT r05 item 2.  Why, and the ordering rules the
// loop below follows: orth_ring.hpp.  Here a wave reads its own columns after its own wait, and f, u = src and column i-1
// (regions of waves 0, 1 and (i-1) % 4) after the exchange barrier of the tile.
//
// Arithmetic, record layout and the device-side step decisions are those of k_orth_lagged (same expressions per element; the
// partial sums are grouped by 256 workgroups x 128-row tiles instead of 1024 x 256, so the reduced sums differ from the
// register kernel's by rounding — as they do between any two grid sizes of that kernel).
// Replaces Lanczos.h:171 of step i-1 + :106, :139, :145-152 of step i, as k_orth_lagged does.
#include "device_helpers.hpp"
#include "krylov.hpp"
#include "orth_ring.hpp"
#include "orth_step.hpp"

using namespace mispec;

namespace {

constexpr int kThreads = 256;
constexpr int kNW = 4;
constexpr int kRows = 128;  // rows of a tile: one 16-byte DMA element per lane and column covers two rows
typedef __attribute__((address_space(3))) char lds_char;

template <int MAXS, int DEPTH, bool ONERED>
__global__ __launch_bounds__(kThreads, 1) void k_orth_lagged_dma(OrthArgs a)
{
    constexpr int NL = MAXS + 1;                  // DMA instructions per wavefront and tile: its columns + one of {f, src}
    constexpr int kRegion = kRows;                // doubles per (wave, column slot) region = 1 KiB
    constexpr int kSlotDoubles = kNW * NL * kRegion;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* ring = reinterpret_cast<double*>(smem);            // [DEPTH][kNW][NL][128]
    double* psum = ring + DEPTH * kSlotDoubles;                 // [2][kNW][128]
    double* cs = psum + 2 * kNW * kRows;                        // [64]
    static_assert((DEPTH * kSlotDoubles + 2 * kNW * kRows + 64) * sizeof(double) == ring_lds_bytes<MAXS, DEPTH>(), "carve-up and launcher disagree");

    if (a.status && *a.status != kStepOk)
        return;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool pending = *a.pending != 0;
    const double alpha = *a.alpha_dev;
    const double beta = *a.beta_dev;
    if (tid < 64)
        cs[tid] = (pending && tid < a.ncol) ? a.c_in[tid] : 0.0;
    __syncthreads();  // (also retires every compiler-visible load above: nothing of the compiler's is in flight below)

    const double* colp[MAXS];
    double cw[MAXS], acc[MAXS], chk[MAXS];
#pragma unroll
    for (int jj = 0; jj < MAXS; jj++)
    {
        const int j = w + kNW * jj;
        colp[jj] = a.V + int64_t(j < a.ncol ? j : 0) * a.ldv;  // surplus slots re-read column 0 with coefficient 0
        cw[jj] = cs[j];
        acc[jj] = 0.0;
        chk[jj] = 0.0;
    }
    const double* extra = (w & 1) ? a.src : a.vi;  // wave 0: f, wave 1: u (waves 2, 3 repeat them: equal DMA counts per wave)
    double b2 = 0.0, mx = 0.0, dvi = 0.0;

    const unsigned lds0 = static_cast<unsigned>(reinterpret_cast<uintptr_t>((lds_char*) smem));  // LDS byte offset of the ring
    const int64_t ntiles = (a.n + kRows - 1) / kRows;
    const int64_t G = gridDim.x;

    auto issue = [&](int64_t t, int slot) {
        const int64_t r = t * kRows + 2 * lane;
        const int64_t rc = r < a.n ? r : 0;
        const unsigned base = __builtin_amdgcn_readfirstlane(lds0 + unsigned((slot * kNW + w) * NL) * 1024u);
#pragma unroll
        for (int jj = 0; jj < MAXS; jj++)
            dma16<true>(colp[jj] + rc, base + unsigned(jj) * 1024u);
        dma16<false>(extra + rc, base + unsigned(MAXS) * 1024u);
    };

    // tiles of this workgroup: b, b + G, b + 2G, ... (neighbouring workgroups read neighbouring KiB of a column at about the same
    // time; one contiguous run of tiles per workgroup measured slower, profiles/r11d)
    int64_t t = blockIdx.x;
    if (t < ntiles)
        issue(t, 0);
    if (DEPTH == 3 && t + G < ntiles)
        issue(t + G, 1);
    int slot = 0, buf = 0;
    const int jp = a.ncol - 1;  // ONERED: column i-1 = slot jp / 4 of wavefront jp % 4 (a.ncol = i >= 1)
    for (; t < ntiles; t += G)
    {
        // ---- tile t of this wave's columns has landed ----
        if (DEPTH == 3 && t + G < ntiles)
            asm volatile("s_waitcnt vmcnt(%0)" ::"i"(NL) : "memory");
        else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const double* mine = ring + (slot * kNW + w) * NL * kRegion + 2 * lane;
        double2 vv[MAXS];
#pragma unroll
        for (int jj = 0; jj < MAXS; jj++)
            vv[jj] = *reinterpret_cast<const double2*>(mine + jj * kRegion);
        double2 p;
        p.x = 0.0;
        p.y = 0.0;
#pragma unroll
        for (int jj = 0; jj < MAXS; jj++)
        {
            p.x += vv[jj].x * cw[jj];
            p.y += vv[jj].y * cw[jj];
        }
        *reinterpret_cast<double2*>(&psum[(buf * kNW + w) * kRows + 2 * lane]) = p;
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        // ---- every wave has left tile t-1's slot: refill it (DEPTH 3: tile t+2G; DEPTH 2: tile t+G) ----
        if (DEPTH == 3)
        {
            if (t + 2 * G < ntiles)
                issue(t + 2 * G, slot == 0 ? 2 : slot - 1);
        }
        else if (t + G < ntiles)
            issue(t + G, slot ^ 1);
        const int64_t r = t * kRows + 2 * lane;
        const bool valid = r < a.n;  // rows come in even pairs; vectors are zero-padded to an even length
        const double* tile = ring + slot * kSlotDoubles + 2 * lane;
        double2 fv = *reinterpret_cast<const double2*>(tile + (0 * NL + MAXS) * kRegion);
        double2 wv = *reinterpret_cast<const double2*>(tile + (1 * NL + MAXS) * kRegion);
        if (!valid)
        {
            fv.x = fv.y = 0.0;
            wv.x = wv.y = 0.0;
        }
        if (ONERED)
        {
            const double2 vp = *reinterpret_cast<const double2*>(tile + ((jp % kNW) * NL + jp / kNW) * kRegion);
            wv.x = wv.x / beta - beta * vp.x;  // Lanczos.h:106 and :139 applied after the product
            wv.y = wv.y / beta - beta * vp.y;
            if (!valid)
            {
                wv.x = 0.0;
                wv.y = 0.0;
            }
        }
        const double* ps = psum + buf * kNW * kRows + 2 * lane;
        const double2 p0 = *reinterpret_cast<const double2*>(ps);
        const double2 p1 = *reinterpret_cast<const double2*>(ps + kRows);
        const double2 p2 = *reinterpret_cast<const double2*>(ps + 2 * kRows);
        const double2 p3 = *reinterpret_cast<const double2*>(ps + 3 * kRows);
        const double px = (p0.x + p1.x) + (p2.x + p3.x), py = (p0.y + p1.y) + (p2.y + p3.y);
        double2 vi, fn;
        vi.x = (fv.x - px) / beta;  // Lanczos.h:171 then :106 (true division)
        vi.y = (fv.y - py) / beta;
        if (!valid)  // rows past the end were loaded from row 0 (clamped address): they must not reach the sums
        {
            vi.x = 0.0;
            vi.y = 0.0;
        }
        fn.x = wv.x - alpha * vi.x;  // Lanczos.h:145
        fn.y = wv.y - alpha * vi.y;
        if (w == 0)
        {
            if (valid)
            {
                *reinterpret_cast<double2*>(a.vout + r) = vi;  // cacheable: the next product reads column i and f
                *reinterpret_cast<double2*>(a.dst + r) = fn;
            }
            b2 += fn.x * fn.x + fn.y * fn.y;
            dvi += vi.x * fn.x + vi.y * fn.y;
            mx = fmax(mx, fmax(fabs(fn.x), fabs(fn.y)));
        }
#pragma unroll
        for (int jj = 0; jj < MAXS; jj++)
        {
            acc[jj] += vv[jj].x * fn.x + vv[jj].y * fn.y;
            chk[jj] += vv[jj].x * vi.x + vv[jj].y * vi.y;
        }
        buf ^= 1;
        slot = (DEPTH == 3) ? (slot == 2 ? 0 : slot + 1) : (slot ^ 1);
    }

    lagged_record<kNW>(a, 0, a.ncol, w, lane, acc, chk, b2, dvi, mx);
}

template <int MAXS, int DEPTH>
void launch_one(const mispec_ctx& ctx, const OrthArgs& a, int grid)
{
    const dim3 g(static_cast<unsigned>(grid)), b(kThreads);
    if (a.onered)
        launch_with_dynamic_lds<k_orth_lagged_dma<MAXS, DEPTH, true>>(ctx, g, b, ring_lds_bytes<MAXS, DEPTH>(), a);
    else
        launch_with_dynamic_lds<k_orth_lagged_dma<MAXS, DEPTH, false>>(ctx, g, b, ring_lds_bytes<MAXS, DEPTH>(), a);
}

}  // namespace

namespace mispec {

// ring slots by columns per wavefront: three while 3 x 4 x (S + 1) KiB + 8.5 KiB fit the CU's 160 KiB (S <= 11), else two
bool orth_lagged_dma_eligible(const OrthArgs& a)
{
    const int slots = (a.ncol + 3) / 4;
    return a.ncol >= 1 && a.ncol < kPanelCols && slots <= 16 && a.n >= 1;
}

int launch_orth_lagged_dma(const mispec_ctx& ctx, const OrthArgs& a, int depth_override)
{
    const int64_t ntiles = (a.n + kRows - 1) / kRows;
    const int grid = int(std::min<int64_t>(ntiles, ctx.num_cu));  // one workgroup per CU (the ring does not leave room for two)
    MISPEC_REQUIRE(a.pstride >= grid, "one-sweep orth kernel (LDS-DMA): partial-record stride smaller than the grid");
    const int slots = (a.ncol + 3) / 4;
    const bool three = slots <= 11 && depth_override != 2;
    const bool ok = dispatch_slots<1, 11>(slots, [&](auto slots_c) {
                        constexpr int S = decltype(slots_c)::value;
                        if (three)
                            launch_one<S, 3>(ctx, a, grid);
                        else
                            launch_one<S, 2>(ctx, a, grid);
                    }) ||
                    dispatch_slots<12, 16>(slots, [&](auto slots_c) { launch_one<decltype(slots_c)::value, 2>(ctx, a, grid); });
    if (!ok)
        throw Error(MISPEC_EINVAL, "one-sweep orth kernel (LDS-DMA): needs 1 <= columns <= 63");
    MISPEC_HIP(hipGetLastError());
    return grid;
}

}  // namespace mispec
