"""Iterative shift-solve benchmark of the general operator (csrc/shift_bicgstab.hip): convection-diffusion on a 128^3 and on a 200^3
grid (the Kronecker sum of tridiag(lower -1 - c, 2, upper -1 + c) over the three axes, c = 0.1), sigma = 0.

Per matrix and run: set_shift (host wall clock: O(n) work and the probe solve), then a solve of a random right-hand side — HIP events
around `reps` back-to-back solves after one that is not timed (mispec_symshift_solve_block_time with one column) — with its iterations
and passes, hence ms per iteration (one BiCGStab iteration: two products, five vector passes, three reduction tails); the bytes each
vector pass moves by count (PASS_VECTORS below, n doubles each) against 8 TB/s and the 6.3 TB/s copy rate of DESIGN.md
3.2.3; one GenEigsRealShiftSolver(8, 24, sigma = 0) solve with its solve and iteration counts.  The split of an iteration into products,
passes and tails comes from a kernel trace of one solve:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/bench_shift_bicgstab.py --trace-only cd128
    python tools/bench_shift_bicgstab.py --summarize DIR/.../t_kernel_stats.csv

    timeout 1100 python tools/bench_shift_bicgstab.py [--runs 2] [--reps 3] [--which cd128,cd200] [--out FILE]
"""
import argparse
import ctypes as C
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import shift_gen_checks as G
import spectra_amd as sa

COPY_RATE, PEAK = 6.3e12, 8.0e12  # bytes per second: DESIGN.md 3.2.3, the data sheet
# n doubles read + written per iteration by each vector pass (csrc/shift_bicgstab.hip)
PASS_VECTORS = {"pass_d": 4 + 2, "pass_v": 3 + 1, "pass_s": 3 + 2, "pass_t": 3 + 1, "pass_x": 6 + 2}

MATRICES = {
    "cd128": lambda: (G.cd3(128, 128, 128, 0.1)[0], 0.0),
    "cd200": lambda: (G.cd3(200, 200, 200, 0.1)[0], 0.0),
    "cd32": lambda: (G.cd3(32, 32, 32, 0.1)[0], 0.0),  # a quick check of the tool
}


def summarize(path):
    classes = dict.fromkeys(list(PASS_VECTORS) + ["product", "tails", "per_pass", "other"], 0.0)
    calls = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name, ns = row["Name"], float(row["TotalDurationNs"])
            key = next((k for k in PASS_VECTORS if "k_" + k in name), None)
            if key is None:
                key = ("tails" if any(k in name for k in ("k_tail_v", "k_tail_t", "k_tail_x")) else
                       "per_pass" if any(k in name for k in ("k_start", "k_tail_start", "k_finish", "k_residual", "k_max_slots")) else
                       "product" if "spmv" in name or "k_perm_" in name or "k_epilogue_blocks" in name else "other")
            classes[key] += ns
            calls[key] = calls.get(key, 0) + int(row["Calls"])
    it = max(calls.get("pass_x", 0), 1)
    print(json.dumps({"iterations_traced": it, "ms_per_iteration": {k: round(v / it * 1e-6, 5) for k, v in classes.items() if k != "other"},
                      "calls": calls}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--which", default="cd128,cd200")
    ap.add_argument("--trace-only", default=None, help="one matrix: set_shift and one solve, nothing timed (to run under a kernel trace)")
    ap.add_argument("--summarize", default=None, help="a kernel stats csv of such a trace: ms per iteration by kernel class")
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
        A, sigma = MATRICES[name]()
        n = A.shape[0]
        t_build = time.perf_counter() - t0
        t0 = time.perf_counter()
        op = sa.SparseGenRealShiftSolve(A, ctx=ctx, solver="auto" if n > 4096 else "iterative")
        t_create = time.perf_counter() - t0
        assert op.path_info()["path"] == 3, op.path_info()
        X = torch.rand(n, dtype=torch.float64, device="cuda") - 0.5
        Y = torch.empty(n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        emit({"matrix": name, "n": n, "nnz": int(A.nnz), "sigma": sigma, "host_build_s": round(t_build, 2), "create_s": round(t_create, 2)})
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
            line = {"matrix": name, "run": run, "set_shift_s": round(t_shift, 4), "probe_iterations": probe["probe_iterations"],
                    "iterations": info["last_iterations"], "products": 2 * info["last_iterations"] + info["last_passes"],
                    "passes": info["last_passes"], "backward_error": info["last_backward_error"],
                    "ms_per_solve": round(ms.value, 3), "ms_per_iteration_all_kernels": round(per_it, 5)}
            for k, vectors in PASS_VECTORS.items():
                b = 8 * n * vectors
                line[k] = {"bytes": b, "ms_at_8TBs": round(1e3 * b / PEAK, 5), "ms_at_copy_rate": round(1e3 * b / COPY_RATE, 5)}
            emit(line)
        before = op.iterative_info()
        t0 = time.perf_counter()
        eigs = sa.GenEigsRealShiftSolver(op, 8, 24, sigma)
        eigs.init()
        nconv = eigs.compute(sa.SortRule.LargestMagn, 1000, 1e-10)
        t_eigs = time.perf_counter() - t0
        after = op.iterative_info()
        ev = eigs.eigenvalues()
        emit({"matrix": name, "geneigs_real_shift_8_24": {"nconv": int(nconv), "seconds": round(t_eigs, 3), "solves": after["solves"] - before["solves"],
                                                          "iterations": after["total_iterations"] - before["total_iterations"],
                                                          "eigenvalues": [float(v) for v in np.sort(ev.real)],
                                                          "max_imag": float(np.abs(ev.imag).max()) if len(ev) else 0.0}})
        del op, X, Y
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
