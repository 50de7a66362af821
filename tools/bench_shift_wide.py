"""Block-tridiagonal shift solve benchmark (csrc/shift_blocktri.hip): the 5-point Laplacians of a 256 x 1024 grid (n = 262 144,
half-bandwidth 256) and of a 512 x 2048 grid (n = 1 048 576, half-bandwidth 512), numbered along the short side.

Per shape and run: set_shift at sigma = 0 and at an interior sigma (host wall clock around the call, which ends with the one read of
the factorisation's record and the calibration of the refinement), then the single solve and a block solve of 8 columns (HIP events
around `reps` back-to-back calls after one that is not timed, mispec_symshift_solve_block_time), the two alternating in one process.
The whole run is repeated (--runs) to show the spread.  Beside each solve figure: the launches it enqueues ((2 N + 1) per factor
solve, N blocks; a refinement step adds a residual, a factor solve and an update) and the time its 24 n s bytes take at the device's
copy rate.  scipy's SuperLU (splu) on the same box gives the context: factor and solve time on the host.

    timeout 1100 python tools/bench_shift_wide.py [--runs 2] [--reps 5] [--out FILE] [--small] [--splu-max-n N]
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
import scipy.sparse.linalg as spla

import spectra_amd as sa

SHAPES = [(256, 1024), (512, 2048)]
INTERIOR_SIGMA = 1.0
COPY_RATE = 6.3e12  # bytes per second, DESIGN.md 3.2.3
COLUMNS = 8


def grid_laplacian(p, q):
    T = lambda m: sp.diags([2 * np.ones(m), -np.ones(m - 1), -np.ones(m - 1)], [0, 1, -1])  # noqa: E731
    return (sp.kron(T(q), sp.identity(p)) + sp.kron(sp.identity(q), T(p))).tocsc()


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="the long side divided by 16 (a quick check of the tool)")
    ap.add_argument("--splu-max-n", type=int, default=300_000, help="SuperLU runs for shapes up to this n (it takes minutes beyond)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sa.default_context()
    lib = sa.lib()
    ms = C.c_float()
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    def timed(op, X, Y, n, k, reps):
        sa.check(lib.mispec_symshift_solve_block_time(op.h, C.c_void_p(X.data_ptr()), n, k, C.c_void_p(Y.data_ptr()), n, reps, C.byref(ms)))
        return ms.value

    for p, q in SHAPES:
        if a.small:
            q //= 16
        A = grid_laplacian(p, q)
        n = A.shape[0]
        t0 = time.perf_counter()
        op = sa.SparseSymShiftSolve(sp.tril(A).tocsc(), ctx=ctx)
        t_create = time.perf_counter() - t0
        path = op.path_info()
        s, N = path["block_rows"], path["blocks"]
        assert path["path"] == 2, path
        X = torch.rand((COLUMNS, n), dtype=torch.float64, device="cuda")
        Y = torch.empty((COLUMNS, n), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        emit({"shape": [p, q], "n": n, "b": s, "blocks": N, "factor_bytes": path["factor_bytes"], "create_s": round(t_create, 3),
              "bandwidth": op.bandwidth_info()})
        op.set_shift(0.0)  # warm-up of the factorisation and of both solves
        timed(op, X, Y, n, 1, 1)
        timed(op, X, Y, n, COLUMNS, 1)
        for run in range(a.runs):
            for sigma in (0.0, INTERIOR_SIGMA):
                t0 = time.perf_counter()
                try:
                    op.set_shift(sigma)
                except ValueError as e:  # a shift too close to an eigenvalue of a leading block system: recorded, not hidden
                    emit({"run": run, "n": n, "b": s, "sigma": sigma, "set_shift_s": round(time.perf_counter() - t0, 4), "refused": str(e)})
                    continue
                t_shift = time.perf_counter() - t0
                info = op.refinement_info()
                t = {1: [], COLUMNS: []}
                for _ in range(3):  # alternating
                    for k in (1, COLUMNS):
                        t[k].append(timed(op, X, Y, n, k, a.reps))
                best = {k: min(t[k]) for k in t}
                per_factor_solve = 2 * N + 1
                launches = per_factor_solve + info["refine_steps"] * (per_factor_solve + 2)
                x = X[0].cpu().numpy()
                y = op.perform_op(x)
                M = A - sigma * sp.identity(n)
                emit({"run": run, "n": n, "b": s, "sigma": sigma, "set_shift_s": round(t_shift, 4), "refine_steps": info["refine_steps"],
                      "probe_backward_error": info["probe_backward_error"], "min_pivot_ratio": info["min_pivot_ratio"],
                      "ms_single": round(best[1], 4), "ms_block8": round(best[COLUMNS], 4),
                      "ms_per_column_block8": round(best[COLUMNS] / COLUMNS, 4), "launches_per_solve": launches,
                      "us_per_launch": round(1e3 * best[1] / launches, 3),
                      "factor_read_bytes": 24 * n * s * (1 + info["refine_steps"]),
                      "ms_at_copy_rate": round(1e3 * 24 * n * s * (1 + info["refine_steps"]) / COPY_RATE, 4),
                      "relative_residual": float(np.linalg.norm(M @ y - x) / np.linalg.norm(x)),
                      "all_ms": {str(k): [round(v, 4) for v in t[k]] for k in t}})
        if n <= a.splu_max_n:
            for sigma in (0.0, INTERIOR_SIGMA):
                M = (A - sigma * sp.identity(n)).tocsc()
                t0 = time.perf_counter()
                lu = spla.splu(M)
                t_factor = time.perf_counter() - t0
                x = np.random.default_rng(1).uniform(-1, 1, n)
                t0 = time.perf_counter()
                lu.solve(x)
                t_solve = time.perf_counter() - t0
                emit({"n": n, "b": s, "sigma": sigma, "splu_factor_s": round(t_factor, 3), "splu_solve_ms": round(1e3 * t_solve, 3),
                      "splu_fill_nnz": int(lu.L.nnz + lu.U.nnz)})
        del op, X, Y
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
