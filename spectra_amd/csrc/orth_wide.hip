// One-sweep Lanczos step (ORTH_LAGGED, krylov.hip k_orth_lagged) on bases of 129 to 512 columns: the step in column panels
// (opt-in: MISPEC_ORTH_WIDE).  With i >= 128 finished columns v_i = (f - V c_in) / beta needs every panel's part
// of V c_in before a dot product with it can be formed, so launch_orth (krylov.hip) enqueues three groups over panels of
// kPanelCols columns, all on one grid and all into the same partial records:
//   subtract   panels 0 .. npan-2: column i <- f - sum_q V_q c_q, un-normalised (k_orth's CORRECT_ONLY; f stays intact, the
//              launches are no-ops while no correction is pending)
//   finish     the last panel (k_lagged_last_panel below) does what the one-panel kernel does: running vector - V_q c_q, / beta
//              -> column i ; w (one-reduction form: u / beta - beta v_{i-1}, column i-1 is in this panel) ; dst = w - alpha v_i
//              -> f ; its own c_j / chk_j, <v_i, dst>, |dst|^2, max |dst|
//   dots       panels 0 .. npan-2 (k_lagged_dots below): c_j = <V_j, dst> and chk_j = <V_j, v_i> from ONE read of the panel
// Record slots as the one-panel kernel's: [0, i) c ; i <v_i, dst> ; [i+1, 2i+1) chk ; kSlotBeta2 / kSlotMaxAbs of dst — the
// reduction and its scalar tail (k_reduce_partials, kFinishLagged) serve the step unchanged.  Per step about 2 i - i_last basis
// columns are read (i_last: width of the last panel) where the reference flow reads about (3 - 1/npan) i.
// Tiling, load pattern and the fixed-order cross-wave sums are k_orth's (krylov.hip): 256 threads, 128-row tiles, lane l owns
// rows (2l, 2l+1), wavefront w owns the panel's columns w, w + 4, ...; no floating-point atomics.
#include "device_helpers.hpp"
#include "krylov.hpp"
#include "orth_launch.hpp"
#include "orth_step.hpp"

using namespace mispec;

namespace {

constexpr int kThreads = 256;
constexpr int kTileRows = 128;
constexpr int kNW = 4;

// The last panel of a panelled one-sweep step: columns [a.col0, a.col0 + a.ncol), a.ncol in 1..64, step i = a.col0 + a.ncol.
// The running vector f - sum of the earlier panels is in column i (a.vout) when a correction is pending, else it is f itself.
template <int MAXS, bool ONERED>
__global__ __launch_bounds__(kThreads) void k_lagged_last_panel(OrthArgs a)
{
    __shared__ double cs[kPanelCols];
    __shared__ __attribute__((aligned(16))) double psum[2][kNW][kTileRows];
    __shared__ __attribute__((aligned(16))) double vprev_s[ONERED ? 2 : 1][ONERED ? kTileRows : 2];

    if (a.status && *a.status != kStepOk)
        return;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool pending = *a.pending != 0;
    if (tid < kPanelCols)
        cs[tid] = (pending && tid < a.ncol) ? a.c_in[a.col0 + tid] : 0.0;
    __syncthreads();
    const double alpha = *a.alpha_dev;
    const double beta = *a.beta_dev;
    const double* run = pending ? a.vout : a.vi;
    const int step = a.col0 + a.ncol;

    const double* colp[MAXS];
    double cw[MAXS], acc[MAXS], chk[MAXS];
#pragma unroll
    for (int jj = 0; jj < MAXS; jj++)
    {
        const int j = w + kNW * jj;
        colp[jj] = a.V + int64_t(a.col0 + (j < a.ncol ? j : 0)) * a.ldv;
        cw[jj] = (j < kPanelCols) ? cs[j] : 0.0;
        acc[jj] = 0.0;
        chk[jj] = 0.0;
    }
    double b2 = 0.0, mx = 0.0, dvi = 0.0;

    const int64_t ntiles = (a.n + kTileRows - 1) / kTileRows;
    int buf = 0;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x)
    {
        const int64_t r = t * kTileRows + 2 * lane;
        const bool valid = r < a.n;  // rows come in even pairs; vectors are zero-padded to an even length
        const int64_t rc = valid ? r : 0;
        double2 vv[MAXS];
#pragma unroll
        for (int jj = 0; jj < MAXS; jj++)
            vv[jj] = load_streamed(colp[jj] + rc);
        double2 fv = *reinterpret_cast<const double2*>(run + rc);
        double2 wv = *reinterpret_cast<const double2*>(a.src + rc);
        if (!valid)
        {
            fv.x = fv.y = 0.0;
            wv.x = wv.y = 0.0;
        }
        double2 p;
        p.x = 0.0;
        p.y = 0.0;
#pragma unroll
        for (int jj = 0; jj < MAXS; jj++)
        {
            p.x += vv[jj].x * cw[jj];
            p.y += vv[jj].y * cw[jj];
        }
        *reinterpret_cast<double2*>(&psum[buf][w][2 * lane]) = p;
        if (ONERED)
        {
            // column i-1 = slot (ncol - 1) / 4 of wavefront (ncol - 1) % 4 of this panel
            const int jp = a.ncol - 1;
            if (w == jp % kNW)
            {
#pragma unroll
                for (int jj = 0; jj < MAXS; jj++)
                    if (jj == jp / kNW)
                        *reinterpret_cast<double2*>(&vprev_s[buf][2 * lane]) = vv[jj];
            }
        }
        __syncthreads();
        if (ONERED)
        {
            const double2 vp = *reinterpret_cast<const double2*>(&vprev_s[buf][2 * lane]);
            wv.x = wv.x / beta - beta * vp.x;
            wv.y = wv.y / beta - beta * vp.y;
            if (!valid)
            {
                wv.x = 0.0;
                wv.y = 0.0;
            }
        }
        const double2 p0 = *reinterpret_cast<const double2*>(&psum[buf][0][2 * lane]);
        const double2 p1 = *reinterpret_cast<const double2*>(&psum[buf][1][2 * lane]);
        const double2 p2 = *reinterpret_cast<const double2*>(&psum[buf][2][2 * lane]);
        const double2 p3 = *reinterpret_cast<const double2*>(&psum[buf][3][2 * lane]);
        double2 vi, fn;
        vi.x = (fv.x - ((p0.x + p1.x) + (p2.x + p3.x))) / beta;  // Lanczos.h:171 then :106 (true division)
        vi.y = (fv.y - ((p0.y + p1.y) + (p2.y + p3.y))) / beta;
        if (!valid)  // rows past the end were loaded from row 0 (clamped address): they must not reach the sums
        {
            vi.x = 0.0;
            vi.y = 0.0;
        }
        fn.x = wv.x - alpha * vi.x;  // Lanczos.h:145
        fn.y = wv.y - alpha * vi.y;
        buf ^= 1;
        if (w == 0)
        {
            if (valid)
            {
                *reinterpret_cast<double2*>(a.vout + r) = vi;
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
    }

    lagged_record<kNW>(a, a.col0, step, w, lane, acc, chk, b2, dvi, mx);
}

// A full panel (kPanelCols columns from a.col0) against the finished step `step`: c_j = <V_j, f> (a.dst) and chk_j = <V_j, v_i>
// (a.vout) from one read of the panel.
__global__ __launch_bounds__(kThreads) void k_lagged_dots(OrthArgs a, int step)
{
    constexpr int MAXS = kPanelCols / kNW;
    if (a.status && *a.status != kStepOk)
        return;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);

    const double* colp[MAXS];
    double acc[MAXS], chk[MAXS];
#pragma unroll
    for (int jj = 0; jj < MAXS; jj++)
    {
        colp[jj] = a.V + int64_t(a.col0 + w + kNW * jj) * a.ldv;
        acc[jj] = 0.0;
        chk[jj] = 0.0;
    }
    const int64_t ntiles = (a.n + kTileRows - 1) / kTileRows;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x)
    {
        const int64_t r = t * kTileRows + 2 * lane;
        const bool valid = r < a.n;
        const int64_t rc = valid ? r : 0;
        double2 vv[MAXS];
#pragma unroll
        for (int jj = 0; jj < MAXS; jj++)
            vv[jj] = load_streamed(colp[jj] + rc);
        double2 fn = *reinterpret_cast<const double2*>(a.dst + rc);
        double2 vi = *reinterpret_cast<const double2*>(a.vout + rc);
        if (!valid)
        {
            fn.x = fn.y = 0.0;
            vi.x = vi.y = 0.0;
        }
#pragma unroll
        for (int jj = 0; jj < MAXS; jj++)
        {
            acc[jj] += vv[jj].x * fn.x + vv[jj].y * fn.y;
            chk[jj] += vv[jj].x * vi.x + vv[jj].y * vi.y;
        }
    }
    double* rec = a.partials + blockIdx.x;
#pragma unroll
    for (int jj = 0; jj < MAXS; jj++)
    {
        const double s = wave_reduce_sum(acc[jj]);
        const double c = wave_reduce_sum(chk[jj]);
        const int j = a.col0 + w + kNW * jj;
        if (lane == 0)
        {
            rec[int64_t(j) * a.pstride] = s;
            rec[int64_t(step + 1 + j) * a.pstride] = c;
        }
    }
}

}  // namespace

namespace mispec {

void launch_orth_lagged_wide(const mispec_ctx& ctx, const OrthArgs& a, int grid)
{
    const int step = a.ncol;
    MISPEC_REQUIRE(step >= 2 * kPanelCols && 2 * step + 1 <= kMaxCols, "panelled one-sweep step: needs 128 <= columns <= 511");
    MISPEC_REQUIRE(grid >= 1 && a.pstride >= grid, "panelled one-sweep step: partial-record stride smaller than the grid");
    const int npan = (step + kPanelCols - 1) / kPanelCols;
    const dim3 g(static_cast<unsigned>(grid)), b(kThreads);
    OrthArgs last = a;
    last.col0 = (npan - 1) * kPanelCols;
    last.ncol = step - last.col0;
    const bool ok = dispatch_slots<1, 16>((last.ncol + kNW - 1) / kNW, [&](auto slots_c) {
        constexpr int S = decltype(slots_c)::value;
        if (a.onered)
            hipLaunchKernelGGL((k_lagged_last_panel<S, true>), g, b, 0, ctx.stream, last);
        else
            hipLaunchKernelGGL((k_lagged_last_panel<S, false>), g, b, 0, ctx.stream, last);
    });
    if (!ok)
        throw Error(MISPEC_EINVAL, "panelled one-sweep step: last panel wider than 64 columns");
    MISPEC_HIP(hipGetLastError());
    for (int q = 0; q + 1 < npan; q++)
    {
        OrthArgs d = a;
        d.col0 = q * kPanelCols;
        d.ncol = kPanelCols;
        hipLaunchKernelGGL(k_lagged_dots, g, b, 0, ctx.stream, d, step);
    }
    MISPEC_HIP(hipGetLastError());
}

}  // namespace mispec
