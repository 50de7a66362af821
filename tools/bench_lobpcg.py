"""LOBPCG benchmark (spectra_amd.LOBPCGSolver): the headline M-band (SparseSymMatProd.synth_band) at n = 1e7, shifted by a multiple of
the identity so that it is positive definite (Gershgorin: shift = max(0, 1 - min_i(a_ii - sum_j |a_ij|)), printed), block size m = 8,
Jacobi preconditioner, tol = 1e-8 (absolute), maxit = 200, SmallestAlge.  Prints one JSON line: iterations, seconds per solve and per
iteration, products with A, and HIP-event times of the solver's kernels, each as a fraction of 8 TB/s on its algorithmic bytes:
  k_gram          s = 24 and s = 63 columns against themselves' images: 8 n (p + q)
  k_lobpcg_resid  m = 8 columns, all active: 8 n (2 m + a)
  V*Q combine     X+ = S C from s = 24 to m = 8 columns (launch_vq): 8 n (s + m)
  block product   A X on m = 8 columns (mispec_spmm_time), bytes of one pass over A plus 16 n m
For orientation it also runs SymEigsSolver(nev = 8, ncv = 40, SmallestAlge) on the same operator to the same residual.
Yardsticks: the X^H y pass of section 7.1 (0.69 of peak) and the real orthogonalisation pass (0.79 of peak).

--preconditioner near-band replaces Jacobi by the factorisation of the matrix's diagonals at offsets <= 3 (SparseSymShiftSolve at
sigma = 0), applied to the active columns by the block shift solve.

    python tools/bench_lobpcg.py [--n N] [--m M] [--no-lanczos] [--no-kernels] [--preconditioner jacobi|near-band] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp

import spectra_amd as sa

PEAK = 8.0e12


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--m", type=int, default=8)
    ap.add_argument("--maxit", type=int, default=200)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--no-lanczos", action="store_true")
    ap.add_argument("--no-kernels", action="store_true", help="the solve alone")
    ap.add_argument("--preconditioner", choices=("jacobi", "near-band"), default="jacobi",
                    help="near-band: the factorisation of the matrix's diagonals at offsets <= 3 (SparseSymShiftSolve at sigma = 0), "
                         "applied by the block shift solve")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, m = a.n, a.m
    ctx = sa.default_context()
    lib = sa.lib()

    t0 = time.perf_counter()
    rp, ci, v = sa.SparseSymMatProd.synth_band(n, ctx=ctx).to_host_csr()
    A = sp.csr_matrix((v, ci, rp), shape=(n, n))
    d = A.diagonal()
    radius = np.asarray(abs(A).sum(axis=1)).ravel() - np.abs(d)
    shift = max(0.0, 1.0 - float((d - radius).min()))
    A = (A + shift * sp.identity(n, format="csr")).tocsr()
    op = sa.SparseSymMatProd(sp.tril(A).tocsc(), ctx=ctx)
    res = {"workload": "M-band + shift", "n": n, "m": m, "shift": shift, "tol": a.tol, "maxit": a.maxit, "nnz": op.nnz(),
           "seconds_setup": round(time.perf_counter() - t0, 2)}

    # kernels alone (HIP events, back to back, no read-back)
    ms = C.c_float()
    for s in (() if a.no_kernels else (24, 63)):
        U = torch.rand((s, n), dtype=torch.float64, device="cuda")
        W = torch.rand((s, n), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        sa.check(lib.mispec_lobpcg_kernel_time(ctx.h, 0, C.c_void_p(U.data_ptr()), C.c_void_p(W.data_ptr()), n, s, s, n, None, 10, C.byref(ms)))
        b = 8.0 * n * 2 * s
        res["k_gram_s%d" % s] = {"ms": round(ms.value, 4), "bytes": b, "frac_8TBps": round(b / (ms.value * 1e-3) / PEAK, 3)}
        del U, W
    if not a.no_kernels:
        kernel_times(torch, lib, ctx, op, n, m, ms, res)

    # the solve
    pre = "jacobi"
    if a.preconditioner == "near-band":
        t0 = time.perf_counter()
        near = (sp.tril(A, 0) - sp.tril(A, -4)).tocsc()  # the diagonals at offsets 0 ... 3: diagonally dominant like A, so SPD
        pre = sa.SparseSymShiftSolve(near, ctx=ctx)
        pre.set_shift(0.0)
        res["seconds_preconditioner_setup"] = round(time.perf_counter() - t0, 2)
    res["preconditioner"] = a.preconditioner
    eigs = sa.LOBPCGSolver(op, nev=m, preconditioner=pre)
    solve(ctx, a, eigs, op, m, res)


def kernel_times(torch, lib, ctx, op, n, m, ms, res):
    AX = torch.rand((m, n), dtype=torch.float64, device="cuda")
    BX = torch.rand((m, n), dtype=torch.float64, device="cuda")
    R = torch.empty((m, n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    sa.check(lib.mispec_lobpcg_kernel_time(ctx.h, 1, C.c_void_p(AX.data_ptr()), C.c_void_p(BX.data_ptr()), n, m, m, n, C.c_void_p(R.data_ptr()), 10,
                                           C.byref(ms)))
    b = 8.0 * n * 3 * m
    res["k_lobpcg_resid"] = {"ms": round(ms.value, 4), "bytes": b, "frac_8TBps": round(b / (ms.value * 1e-3) / PEAK, 3)}
    S = torch.rand((24, n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    sa.check(lib.mispec_lobpcg_kernel_time(ctx.h, 2, C.c_void_p(S.data_ptr()), None, n, 24, m, n, C.c_void_p(R.data_ptr()), 10, C.byref(ms)))
    b = 8.0 * n * (24 + m)
    res["vq_combine_s24"] = {"ms": round(ms.value, 4), "bytes": b, "frac_8TBps": round(b / (ms.value * 1e-3) / PEAK, 3)}
    del S
    t = op.spmm_time(AX.data_ptr(), n, m, R.data_ptr(), n, 10)
    b = op.algorithmic_bytes() + 16.0 * n * (m - 1)
    res["block_product"] = {"ms": round(t, 4), "bytes": b, "frac_8TBps": round(b / (t * 1e-3) / PEAK, 3)}
    del AX, BX, R


def solve(ctx, a, eigs, op, m, res):
    ctx.sync()
    t0 = time.perf_counter()
    nconv = eigs.compute(sa.SortRule.SmallestAlge, a.maxit, a.tol)
    dt = time.perf_counter() - t0
    it = eigs.num_iterations()
    res["lobpcg"] = {"nconv": nconv, "info": eigs.info().name, "iterations": it, "products_with_A": eigs.num_operations(),
                     "retries_without_P": eigs.num_retries(), "seconds": round(dt, 4), "seconds_per_iteration": round(dt / max(it, 1), 5),
                     "max_residual_norm": float(eigs.residual_norms().max()), "lambda": eigs.eigenvalues().tolist()}
    if not a.no_lanczos:
        lan = sa.SymEigsSolver(op, m, 40)
        lan.init()
        ctx.sync()
        t0 = time.perf_counter()
        nc = lan.compute(sa.SortRule.SmallestAlge, 1000, a.tol / max(abs(eigs.eigenvalues()).max(), 1.0))
        dt = time.perf_counter() - t0
        res["lanczos_for_orientation"] = {"nconv": nc, "info": lan.info().name, "restarts": lan.num_iterations(),
                                          "products_with_A": lan.num_operations(), "seconds": round(dt, 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
