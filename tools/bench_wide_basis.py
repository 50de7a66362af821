"""Wide bases (ncv > 128) on the headline matrix: the reference's two-pass flow — what such solves get today, with "onesweep" as
well, which falls back to it — against the opt-in panelled one-sweep steps ("onesweep-wide").  One matrix, one
solver per mode, the modes timed in turn so that clock and box drift hit all of them alike; then one more solve per mode with
every kernel family bracketed (profile level 1, as bench.py's split) for the time in the passes over the basis.

    python tools/bench_wide_basis.py [--size N] [--solves S] [--configs k:ncv,k:ncv,...] [--out FILE.jsonl]

One JSON line per (config, mode): ms per solve (all, min, median), operations, restarts, ms_vtf + ms_gemv of the profiled solve,
panel_steps; and per config the spread of the reference mode over its timed solves, the yardstick's own noise.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spectra_amd as sa

MODES = ("reference", "onesweep", "onesweep-wide")

p = argparse.ArgumentParser()
p.add_argument("--size", type=int, default=10_000_000)
p.add_argument("--solves", type=int, default=3)
p.add_argument("--configs", default="64:129,100:200,200:400")
p.add_argument("--tol", type=float, default=1e-11)
p.add_argument("--out", default=None)
a = p.parse_args()
ctx = sa.default_context()
op = sa.SparseSymMatProd.synth_band(a.size, ctx=ctx)
out = open(a.out, "a") if a.out else None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def solve(e):
    e.init()
    nconv = e.compute(sa.SortRule.LargestAlge, 1000, a.tol)
    ctx.sync()
    return nconv


for cfg in a.configs.split(","):
    k, m = (int(x) for x in cfg.split(":"))
    solvers = {}
    for mode in MODES:
        e = sa.SymEigsSolver(op, k, m)
        e.set_orth_mode(mode)
        solvers[mode] = e
        solve(e)  # warm-up
    times = {mode: [] for mode in MODES}
    nconv = {}
    for rep in range(a.solves):
        for mode, e in solvers.items():
            ctx.sync()
            t0 = time.perf_counter()
            nconv[mode] = solve(e)
            times[mode].append(time.perf_counter() - t0)
    for mode, e in solvers.items():
        ts = sorted(times[mode])
        rec = {"n": a.size, "k": k, "ncv": m, "mode": mode, "nconv": nconv[mode],
               "ms_per_solve_all": [round(1e3 * t, 1) for t in times[mode]], "ms_per_solve_min": round(1e3 * ts[0], 1),
               "ms_per_solve_median": round(1e3 * ts[len(ts) // 2], 1), "spread_ms": round(1e3 * (ts[-1] - ts[0]), 1),
               "num_operations": e.num_operations(), "num_iterations": e.num_iterations(),
               "max_residual": float(e.residuals().max())}
        info = e.orth_info()
        rec.update({"mode_in_effect": info["mode"], "wide": info["wide"], "panel_steps_per_solve": info["panel_steps"] // (a.solves + 1),
                    "lagged_steps_per_solve": info["lagged_steps"] // (a.solves + 1)})
        e.profile(1)
        p0 = e.get_profile()
        solve(e)
        p1 = e.get_profile()
        e.profile(0)
        rec.update({"profiled_ms_vtf": round(p1["ms_vtf"] - p0["ms_vtf"], 1), "profiled_ms_gemv": round(p1["ms_gemv"] - p0["ms_gemv"], 1),
                    "profiled_ms_spmv": round(p1["ms_spmv"] - p0["ms_spmv"], 1),
                    "profiled_ms_compress": round(p1["ms_compress"] - p0["ms_compress"], 1)})
        rec["profiled_ms_vtf_plus_gemv"] = round(rec["profiled_ms_vtf"] + rec["profiled_ms_gemv"], 1)
        emit(rec)
    del solvers, e
if out:
    out.close()
