"""Complex-shift iterative shift-solve benchmark of the general operator (csrc/shift_zbicgstab.hip): the normal non-symmetric matrix
shift_cplx_checks.rot3 on a 64^3 and on a 100^3 grid (g = 0.5), sigma = 1.5 + 1i, beside the real method (csrc/shift_bicgstab.hip) on
the same operator — the same handle — at sigma = 1.5.

Per matrix and run, for the complex and for the real shift: set_shift (host wall clock: O(n) work and the probe solve), then a solve of
a random right-hand side — HIP events around `reps` back-to-back solves after one that is not timed
(mispec_symshift_solve_block_time with one column) — with its iterations and passes, hence microseconds per iteration (one complex
BiCGStab iteration: four real products, five vector passes over complex vectors, three reduction tails), and the ratio of the two
per-iteration times.  The split of a complex iteration into products, passes and tails comes from a kernel trace of one solve, in a
run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/bench_shift_zbicgstab.py --trace-only rot100
    python tools/bench_shift_zbicgstab.py --summarize DIR/.../t_kernel_stats.csv

    timeout 900 python tools/bench_shift_zbicgstab.py [--runs 2] [--reps 3] [--which rot64,rot100] [--out FILE]
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

import shift_cplx_checks as Z
import spectra_amd as sa

PASSES = ["zpass_d", "zpass_v", "zpass_s", "zpass_t", "zpass_x"]
SIGMA = (1.5, 1.0)

MATRICES = {
    "rot64": lambda: Z.rot3(64, 64, 64, 0.5)[0],
    "rot100": lambda: Z.rot3(100, 100, 100, 0.5)[0],
    "rot24": lambda: Z.rot3(24, 24, 24, 0.5)[0],  # a quick check of the tool
}


def summarize(path):
    classes = dict.fromkeys(PASSES + ["product", "tails", "per_pass", "other"], 0.0)
    calls = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name, ns = row["Name"], float(row["TotalDurationNs"])
            key = next((k for k in PASSES if "k_" + k in name), None)
            if key is None:
                key = ("tails" if any(k in name for k in ("k_ztail_v", "k_ztail_t", "k_ztail_x")) else
                       "per_pass" if any(k in name for k in ("k_zstart", "k_ztail_start", "k_zfinish", "k_zresidual", "k_max_slots")) else
                       "product" if "spmv" in name or "k_perm_" in name or "k_epilogue_blocks" in name else "other")
            classes[key] += ns
            calls[key] = calls.get(key, 0) + int(row["Calls"])
    it = max(calls.get("zpass_x", 0), 1)
    print(json.dumps({"iterations_traced": it, "ms_per_iteration": {k: round(v / it * 1e-6, 5) for k, v in classes.items() if k != "other"},
                      "calls": calls}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--which", default="rot64,rot100")
    ap.add_argument("--trace-only", default=None, help="one matrix: a complex set_shift and one solve, nothing timed (to run under a kernel trace)")
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
        A = MATRICES[name]()
        n = A.shape[0]
        t_build = time.perf_counter() - t0
        t0 = time.perf_counter()
        op = sa.SparseGenComplexShiftSolve(A, ctx=ctx, complex_solver="iterative")
        t_create = time.perf_counter() - t0
        assert op.path_info()["path"] == 3, op.path_info()
        X = torch.rand(n, dtype=torch.float64, device="cuda") - 0.5
        Y = torch.empty(n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        emit({"matrix": name, "n": n, "nnz": int(A.nnz), "sigma": list(SIGMA), "host_build_s": round(t_build, 2), "create_s": round(t_create, 2)})
        op.set_shift(*SIGMA)  # warm-up
        op.solve_device(X.data_ptr(), Y.data_ptr())
        torch.cuda.synchronize()
        if a.trace_only:
            return
        for run in range(a.runs):
            line = {"matrix": name, "run": run}
            for kind, shift in (("complex", SIGMA), ("real", (SIGMA[0], 0.0))):
                t0 = time.perf_counter()
                op.set_shift(*shift)
                t_shift = time.perf_counter() - t0
                probe = op.iterative_info()
                sa.check(lib.mispec_symshift_solve_block_time(op.h, C.c_void_p(X.data_ptr()), n, 1, C.c_void_p(Y.data_ptr()), n, a.reps, C.byref(ms)))
                info = op.iterative_info()
                line[kind] = {"sigma": list(shift), "set_shift_s": round(t_shift, 4), "probe_iterations": probe["probe_iterations"],
                              "iterations": info["last_iterations"], "passes": info["last_passes"],
                              "real_products": (4 if kind == "complex" else 2) * info["last_iterations"] +
                                               (2 if kind == "complex" else 1) * info["last_passes"],
                              "backward_error": info["last_backward_error"], "ms_per_solve": round(ms.value, 3),
                              "us_per_iteration_all_kernels": round(1e3 * ms.value / max(info["last_iterations"], 1), 2)}
            line["complex_over_real_per_iteration"] = round(line["complex"]["us_per_iteration_all_kernels"] /
                                                            line["real"]["us_per_iteration_all_kernels"], 3)
            emit(line)
        del op, X, Y
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
