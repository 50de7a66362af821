"""Block shift solve benchmark (mispec_symshift_solve_block): for every shape below, a block solve of k columns under shift_block = 4
and = 2 against the same k columns under shift_block = 0 — k single solves, the only way to do this work without the panel kernels.
HIP events around `reps` back-to-back calls (mispec_symshift_solve_block_time), after a warm-up of every shape and variant, the
variants alternating in one process; the whole run is repeated (--runs) to show the spread.

  shape                      path
  n = 2e6, b = 3 (C5)        sweep kernels (15625 chunks: no explicit chunk inverses)
  n = 1e6, b = 8             sweep kernels; the second level (band 15) is wide and loops over the columns
  n = 2e5, b = 3             explicit chunk inverses
  n = 4096, b = 16           dense inverse
  n = 1e6, b = 32            wide band: one wavefront per chunk, every step loops over the columns (the panel variants guard
                             nothing here; the single solves time the widest separator kernel and the wide back substitution)

One JSON line per (run, shape, k): ms per call and per column of each variant, the ratio to the single solves, and the bytes per
second on the algorithmic bytes of the TOP level of a panel (factor once + 16 n K; the deeper levels hold 1/32 of the rows):
sweeps 8 n (b + 1) for the factor and its pivots + 16 n b for the spikes; chunk inverses 8 P m^2 + 16 n b; dense 8 n^2.

    timeout 900 python tools/bench_shift_block.py [--runs 2] [--reps 20] [--out FILE] [--small]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp

import spectra_amd as sa

SHAPES = [(2_000_000, 3, "sweeps"), (1_000_000, 8, "sweeps"), (200_000, 3, "chunk inverses"), (4096, 16, "dense inverse"),
          (1_000_000, 32, "wide band")]
COLUMNS = (2, 4, 8, 21)


def banded_spd(n, b, seed=0):
    rng = np.random.default_rng(seed)
    diags = [rng.uniform(-0.5, 0.5, n - d) for d in range(1, b + 1)]
    return sp.diags([rng.uniform(-0.5, 0.5, n) + b + 0.5] + diags + diags, [0] + list(range(1, b + 1)) + [-d for d in range(1, b + 1)],
                    format="csc")


def panel_bytes(n, b, path, width):
    if path == "dense inverse":
        factor = 8.0 * n * n
    elif path == "chunk inverses":
        chunks, m = n // 128, 128 - b
        factor = 8.0 * chunks * m * m + 16.0 * n * b
    else:
        factor = 8.0 * n * (b + 1) + 16.0 * n * b
    return factor + 16.0 * n * width


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="shapes divided by 20 (a quick check of the tool)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sa.default_context()
    lib = sa.lib()
    ms = C.c_float()
    kmax = max(COLUMNS)
    ops = []
    for n, b, path in SHAPES:
        if a.small and path != "dense inverse":
            n //= 20
        op = sa.SparseSymShiftSolve(sp.tril(banded_spd(n, b, seed=b)).tocsc(), ctx=ctx)
        op.set_shift(-1.0)
        X = torch.rand((kmax, n), dtype=torch.float64, device="cuda")
        Y = torch.empty((kmax, n), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ops.append((n, b, path, op, X, Y))

    def timed(op, X, Y, n, k, variant, reps):
        sa.set_option("shift_block", variant)
        try:
            sa.check(lib.mispec_symshift_solve_block_time(op.h, C.c_void_p(X.data_ptr()), n, k, C.c_void_p(Y.data_ptr()), n, reps, C.byref(ms)))
        finally:
            sa.set_option("shift_block", None)
        return ms.value

    for n, b, path, op, X, Y in ops:  # warm-up of every shape and variant
        for variant in ("0", "2", "4"):
            timed(op, X, Y, n, kmax, variant, 2)
    lines = []
    for run in range(a.runs):
        for n, b, path, op, X, Y in ops:
            for k in COLUMNS:
                t = {v: [] for v in ("0", "2", "4")}
                for _ in range(3):  # alternating
                    for v in ("0", "2", "4"):
                        t[v].append(timed(op, X, Y, n, k, v, a.reps))
                best = {v: min(t[v]) for v in t}
                line = {"run": run, "n": n, "b": b, "path": path, "k": k, "reps": a.reps,
                        "ms_singles": round(best["0"], 4), "ms_panel2": round(best["2"], 4), "ms_panel4": round(best["4"], 4),
                        "ms_per_column_singles": round(best["0"] / k, 4), "ms_per_column_panel2": round(best["2"] / k, 4),
                        "ms_per_column_panel4": round(best["4"] / k, 4),
                        "panel2_over_singles": round(best["2"] / best["0"], 3), "panel4_over_singles": round(best["4"] / best["0"], 3),
                        "all_ms": {v: [round(x, 4) for x in t[v]] for v in t}}
                if k in (2, 4):  # one panel exactly: bytes per second on its algorithmic bytes
                    line["panel_TBps"] = round(panel_bytes(n, b, path, k) / (best[str(k)] * 1e-3) / 1e12, 3)
                    line["single_TBps"] = round(panel_bytes(n, b, path, 1) / (best["0"] / k * 1e-3) / 1e12, 3)
                print(json.dumps(line), flush=True)
                lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
