// The LDS ring through which the orthogonalisation passes stream the basis by LDS-DMA (`global_load_lds_dwordx4`) instead of
// through registers: k_orth_lagged_dma (orth_dma.hip, the one-sweep step) and k_orth_dma (orth_dma_modes.hip, the reference flow and
// the Arnoldi process) — round 6, VERDICT r05 item 2.
//
// Why: the register version issues a tile's 20 x 16-byte loads per lane, waits for all of them, computes, and only then issues
// the next tile's loads; its SQ / TCC counters (profiles/r11a_pmc_sq_tcc_tcp_onesweep_c2_round5_tree.txt) show 90 128-byte requests in flight
// per CU on average at 1214 cycles per request — the memory system is asked for 5.8 TB/s, not saturated.  Holding a second
// tile in flight costs 80 more VGPRs per lane in registers and nothing in LDS: here every wavefront keeps DEPTH - 1 tiles of its
// own columns in flight (wave-private regions of a DEPTH-slot ring, 1 KiB per column and tile = one DMA instruction), waits
// with a COUNTED `s_waitcnt vmcnt(N)` — never 0 inside the loop —, and the per-tile barrier of the row-sum exchange is a bare
// `s_barrier` that does not drain VMEM.  One 256-thread workgroup per CU (the ring is 3 x 44 KiB at 40 columns), grid-stride
// over 128-row tiles; 256 partial records instead of 1024, so the record reduction behind the pass reads a quarter.
//
// Ordering rules used (MI355X_MICROARCH.md "Two waves per SIMD" item 7, cdna_hip_programming.md 5.7):
//   * LDS-DMA data is ordered for a ds_read only by the ISSUING wave's covering vmcnt; other waves read it after a barrier the
//     issuer reached behind that wait: a wave reads its own columns after its own wait, and the vectors and columns in other
//     waves' regions after the exchange barrier of the tile;
//   * the asm DMA is invisible to hipcc's waitcnt bookkeeping: every wait for it is an explicit statement; the loop holds no
//     compiler-visible VMEM load, and wave 0's stores per tile only make the counted wait conservative (vmcnt counts them
//     too; loads complete in order among themselves, so "at most NL outstanding" still means tile t has landed);
//   * a ring slot is refilled only behind the barrier that follows the last cross-wave read of it (slot of tile t-1 behind the
//     barrier of tile t; every wave's LDS reads are retired by the lgkmcnt(0) in front of that barrier).
// What the two files share is here: these rules, the DMA instruction and the ring's LDS size.  Each kernel keeps its loop — waits,
// barrier and refill as statements of its own — because hipcc's register allocation and its choice of which product of
// x * x + y * y to contract follow the shape of the whole kernel: the same loop written through shared inline functions moved the
// VGPR counts across occupancy steps and the last bits of the results (profiles/r19a_orth_refactor_parent_vs_tree.txt).  Internal.
#pragma once
#include "orth_launch.hpp"

namespace {

// one wave-wide LDS-DMA: lane l's 16 bytes at gsrc land at LDS byte lds_dst + 16 l (lds_dst wave-uniform)
template <bool NT>
__device__ __forceinline__ void dma16(const double* gsrc, unsigned lds_dst)
{
    unsigned keep;
    if (NT)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(gsrc), "s"(lds_dst)
                     : "memory");
    else
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(gsrc), "s"(lds_dst)
                     : "memory");
}

// Dynamic LDS of a ring kernel in bytes: ring[DEPTH][4][MAXS + 1][128] ; psum[2][4][128] (the row-sum exchange) ; cs[64] (c_in).
// The kernels carve the three arrays up in this order and assert that their sizes add up to this.
// Three slots while 3 x 4 x (MAXS + 1) KiB + 8.5 KiB fit the CU's 160 KiB (MAXS <= 11), else two.
template <int MAXS, int DEPTH>
constexpr size_t ring_lds_bytes()
{
    return (size_t(DEPTH) * 4 * (MAXS + 1) * 128 + 2 * 4 * 128 + 64) * sizeof(double);
}

}  // namespace
