// Device code that the one-sweep orthogonalisation passes share (k_orth_lagged in krylov.hip, k_orth_lagged_dma in orth_dma.hip,
// k_lagged_last_panel in orth_wide.hip): the record epilogue.  Wavefront w of NW owns the columns w + NW * jj of its
// panel ("slot" jj < MAXS); slot j of a workgroup's record is rec[j * pstride].  Internal.
#pragma once
#include "device_helpers.hpp"
#include "krylov.hpp"

namespace {

// One-sweep step `step` for the panel whose first column is col0 (one panel: col0 = 0, step = ncol):
// [0, step) c_j = <V_j, dst> ; step <v_i, dst> ; [step + 1, 2 step + 1) chk_j = <V_j, v_i> ; kSlotBeta2 / kSlotMaxAbs of dst
template <int NW, int MAXS>
__device__ __forceinline__ void lagged_record(const mispec::OrthArgs& a, int col0, int step, int w, int lane, const double (&acc)[MAXS],
                                              const double (&chk)[MAXS], double b2, double dvi, double mx)
{
    double* rec = a.partials + blockIdx.x;
#pragma unroll
    for (int jj = 0; jj < MAXS; jj++)
    {
        const double s = wave_reduce_sum(acc[jj]);
        const double c = wave_reduce_sum(chk[jj]);
        const int j = w + NW * jj;
        if (lane == 0 && j < a.ncol)
        {
            rec[int64_t(col0 + j) * a.pstride] = s;
            rec[int64_t(step + 1 + col0 + j) * a.pstride] = c;
        }
    }
    if (w == 0)
    {
        b2 = wave_reduce_sum(b2);
        dvi = wave_reduce_sum(dvi);
        mx = wave_reduce_max(mx);
        if (lane == 0)
        {
            rec[int64_t(step) * a.pstride] = dvi;
            rec[mispec::kSlotBeta2 * a.pstride] = b2;
            rec[mispec::kSlotMaxAbs * a.pstride] = mx;
        }
    }
}

}  // namespace
