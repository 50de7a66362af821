"""Iterative shift-solve benchmark (csrc/shift_minres.hip): matrices no direct path takes.

  * the 7-point Laplacian of a 128^3 and of a 200^3 grid, sigma = 0;
  * the headline M-band (15 entries per row on fixed offsets, U(-0.5, 0.5); its SpMV is the diagonal kernel) at
    n = 10^7, shifted below its spectrum (sigma = -8: every row sum of |A| is below 7.5).

Per matrix and run: set_shift (host wall clock: O(n) work and the probe solve), then a solve of a random right-hand side — HIP events
around `reps` back-to-back solves after one that is not timed (mispec_symshift_solve_block_time with one column) — with its iterations
and passes, hence ms per iteration; the bytes the two vector passes move by count (pass A: 7 reads and 3 writes of n doubles, 8 and 3
for a pencil; pass B: 3 reads, 2 writes) against 8 TB/s and the 6.3 TB/s copy rate of DESIGN.md 3.2.3; one SymEigsShiftSolver(8, 24,
sigma = 0) solve with its solve and iteration counts (Laplacians only).  The split of an iteration into product, pass A, pass B and the
two reduction tails comes from a kernel trace of one solve:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/bench_shift_minres.py --trace-only lap128
    python tools/bench_shift_minres.py --summarize DIR/.../t_kernel_stats.csv

scipy's eigsh(sigma=0) with SuperLU at 128^3 is for orientation only (--splu; it takes minutes and gigabytes).

    timeout 1100 python tools/bench_shift_minres.py [--runs 2] [--reps 3] [--which lap128,lap200,mband] [--out FILE]
"""
import argparse
import ctypes as C
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import spectra_amd as sa
from spectra_amd import workloads

COPY_RATE, PEAK = 6.3e12, 8.0e12  # bytes per second: DESIGN.md 3.2.3, the data sheet
PASS_A_VECTORS, PASS_B_VECTORS = 10, 5  # n doubles read or written per iteration, B = I


def lap3_lower(m):
    T = lambda k: sp.diags([2 * np.ones(k), -np.ones(k - 1)], [0, -1])  # noqa: E731  (lower triangle of the 1-D Laplacian)
    I = sp.identity(m)
    D = sp.diags([2 * np.ones(m)], [0])
    # lower triangle of kron sums: the diagonal counted once per direction
    L1 = sp.kron(sp.kron(I, I), T(m)) + sp.kron(sp.kron(I, T(m) - D), I) + sp.kron(sp.kron(T(m) - D, I), I)
    return (L1 + 4 * sp.identity(m ** 3)).tocsc()


def mband_lower(n, seed=sa.SYNTH_SEED):
    """lower triangle (CSR) of the real M-band: entry (r, r - off) = h(seed, r - off, r), diagonal h(seed, r, r)"""
    r_all = np.arange(n, dtype=np.uint64)
    indptr = np.zeros(n + 1, dtype=np.int64)
    offs = [o for o in sorted(workloads.BAND_OFFSETS, reverse=True) if o < n]
    counts = np.ones(n, dtype=np.int64)
    for off in offs:
        counts[off:] += 1
    indptr[1:] = np.cumsum(counts)
    cols = np.empty(indptr[-1], dtype=np.int32)
    vals = np.empty(indptr[-1])
    pos = indptr[:-1].copy()
    for off in offs:  # ascending columns: the largest offset first
        r = r_all[off:]
        c = r - np.uint64(off)
        p = pos[off:]
        cols[p] = c.astype(np.int32)
        vals[p] = workloads.hash_value(seed, c, r)
        pos[off:] += 1
    cols[pos] = r_all.astype(np.int32)
    vals[pos] = workloads.hash_value(seed, r_all, r_all)
    return sp.csr_matrix((vals, cols, indptr.astype(np.int32)), shape=(n, n))


MATRICES = {
    "lap128": lambda: (lap3_lower(128), 0.0, True),
    "lap200": lambda: (lap3_lower(200), 0.0, True),
    "mband": lambda: (mband_lower(10_000_000), -8.0, False),
    "lap32": lambda: (lap3_lower(32), 0.0, True),  # a quick check of the tool
}


def summarize(path):
    classes = {"product": 0.0, "pass_a": 0.0, "pass_b": 0.0, "tails": 0.0, "per_pass": 0.0, "other": 0.0}
    calls = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name, ns = row["Name"], float(row["TotalDurationNs"])
            key = ("pass_a" if "k_pass_a" in name else "pass_b" if "k_pass_b" in name else
                   "tails" if "k_tail_a" in name or "k_tail_b" in name else
                   "per_pass" if any(k in name for k in ("k_start", "k_tail_start", "k_finish", "k_residual", "k_max_slots")) else
                   "product" if "spmv" in name or "k_perm_" in name or "k_epilogue_blocks" in name else "other")
            classes[key] += ns
            calls[key] = calls.get(key, 0) + int(row["Calls"])
    it = max(calls.get("pass_a", 0), 1)
    print(json.dumps({"iterations_traced": it, "ms_per_iteration": {k: round(v / it * 1e-6, 5) for k, v in classes.items() if k != "other"},
                      "calls": calls}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--which", default="lap128,lap200,mband")
    ap.add_argument("--trace-only", default=None, help="one matrix: set_shift and one solve, nothing timed (to run under a kernel trace)")
    ap.add_argument("--summarize", default=None, help="a kernel stats csv of such a trace: ms per iteration by kernel class")
    ap.add_argument("--splu", action="store_true", help="scipy eigsh(sigma=0) with SuperLU on lap128, for orientation")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    import torch

    ctx = sa.default_context()
    lib = sa.lib()
    ms = C.c_float()
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    for name in ([a.trace_only] if a.trace_only else a.which.split(",")):
        t0 = time.perf_counter()
        Lo, sigma, eigs_too = MATRICES[name]()
        n = Lo.shape[0]
        t_build = time.perf_counter() - t0
        t0 = time.perf_counter()
        op = sa.SparseSymShiftSolve(Lo, ctx=ctx, solver="auto")
        t_create = time.perf_counter() - t0
        assert op.path_info()["path"] == 3, op.path_info()
        X = torch.rand(n, dtype=torch.float64, device="cuda") - 0.5
        Y = torch.empty(n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        emit({"matrix": name, "n": n, "nnz_lower": int(Lo.nnz), "sigma": sigma, "host_build_s": round(t_build, 2), "create_s": round(t_create, 2),
              "bandwidth": op.bandwidth_info()})
        op.set_shift(sigma)  # warm-up
        op.solve_device(X.data_ptr(), Y.data_ptr())
        torch.cuda.synchronize()
        if a.trace_only:
            return
        for run in range(a.runs):
            t0 = time.perf_counter()
            op.set_shift(sigma)
            t_shift = time.perf_counter() - t0
            probe = op.iterative_info()
            sa.check(lib.mispec_symshift_solve_block_time(op.h, C.c_void_p(X.data_ptr()), n, 1, C.c_void_p(Y.data_ptr()), n, a.reps, C.byref(ms)))
            info = op.iterative_info()
            per_it = ms.value / max(info["last_iterations"], 1)
            bytes_a, bytes_b = 8 * n * PASS_A_VECTORS, 8 * n * PASS_B_VECTORS
            emit({"matrix": name, "run": run, "set_shift_s": round(t_shift, 4), "probe_iterations": probe["probe_iterations"],
                  "iterations": info["last_iterations"], "passes": info["last_passes"], "backward_error": info["last_backward_error"],
                  "ms_per_solve": round(ms.value, 3), "ms_per_iteration_all_kernels": round(per_it, 5),
                  "pass_a_bytes": bytes_a, "pass_b_bytes": bytes_b,
                  "pass_a_ms_at_8TBs": round(1e3 * bytes_a / PEAK, 5), "pass_a_ms_at_copy_rate": round(1e3 * bytes_a / COPY_RATE, 5),
                  "pass_b_ms_at_8TBs": round(1e3 * bytes_b / PEAK, 5), "pass_b_ms_at_copy_rate": round(1e3 * bytes_b / COPY_RATE, 5)})
        if eigs_too:
            before = op.iterative_info()
            t0 = time.perf_counter()
            eigs = sa.SymEigsShiftSolver(op, 8, 24, sigma)
            eigs.init()
            nconv = eigs.compute(sa.SortRule.LargestMagn, 1000, 1e-10)
            t_eigs = time.perf_counter() - t0
            after = op.iterative_info()
            emit({"matrix": name, "symeigs_shift_8_24": {"nconv": int(nconv), "seconds": round(t_eigs, 3), "solves": after["solves"] - before["solves"],
                                                        "iterations": after["total_iterations"] - before["total_iterations"],
                                                        "eigenvalues": [float(v) for v in np.sort(eigs.eigenvalues())]}})
        if a.splu and name == "lap128":
            A = (Lo + sp.tril(Lo, -1).T).tocsc()
            t0 = time.perf_counter()
            ev = spla.eigsh(A, k=8, ncv=24, sigma=0.0, which="LM", return_eigenvectors=False)
            emit({"matrix": name, "scipy_eigsh_superlu_s": round(time.perf_counter() - t0, 2), "eigenvalues": [float(v) for v in np.sort(ev)]})
        del op, X, Y
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
