"""Block product (mispec_spmm, spectra_amd/csrc/spmm.hip) against as many single products, stand-alone, on M-band (synthetic, n
= argv[1], default 1e7) and on the jittered band of spectra_amd/workloads.py (n = argv[2], default = argv[1]).  One JSON line
per case to the file argv[3] (default profiles/bench_spmm.jsonl) and to stdout.

Per matrix, in ONE process and interleaved over ROUNDS rounds (same box, same clocks): mispec_spmv_time in the automatic format
and with format 0 forced, and mispec_spmm_time for k in {2, 4, 8, 16} under option spmm = auto, 2, 4, 8.  Reported: the median
of the rounds (min and max next to it), k x the single product, the algorithmic bytes and their fraction of 8 TB/s.
BYTES: a panel of KB columns moves 12 nnz + 4 (rows + 1) + 8 KB (cols + rows), plus the pack's 16 KB cols (read X, write the
interleaved copy); a single column is the SpMV's 12 nnz + 4 (rows + 1) + 8 cols + 8 rows.
RULE for `auto` (spmm.hip kAutoWidths): a width stays only if the block product of exactly that many columns is faster than as
many single products in the matrix's automatic format on BOTH matrices; the last lines give the verdict per width."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import scipy.sparse as sp
import torch

import spectra_amd as sa
from spectra_amd import workloads

HBM = 8e12
KS = (2, 4, 8, 16)
OPTIONS = ("auto", "2", "4", "8")
ROUNDS, WARM, REPS = 3, 3, 20
FORMULA = "panel: 12 nnz + 4 (rows + 1) + 8 KB (cols + rows) + pack 16 KB cols; single column: 12 nnz + 4 (rows + 1) + 8 cols + 8 rows"


def plan_bytes(op, widths):
    nnz, rows, cols = op.nnz(), op.rows(), op.cols()
    total = 0.0
    for w in widths:
        total += 12.0 * nnz + 4.0 * (rows + 1) + 8.0 * w * (cols + rows) + (16.0 * w * cols if w > 1 else 0.0)
    return total


def med(v):
    return {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)}


def run(name, op, emit):
    n = op.rows()
    ld = n + (n & 1)
    kmax = max(KS)
    X = torch.rand((kmax, ld), dtype=torch.float64, device="cuda") - 0.5
    Y = torch.empty((kmax, ld), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    x, y = X.data_ptr(), Y.data_ptr()
    auto_format = op.spmv_format()
    spmv = {"auto": [], "format0": []}
    spmm = {(k, o): [] for k in KS for o in OPTIONS}
    try:
        for r in range(ROUNDS):
            for key, fmt in (("auto", -1), ("format0", 0)):
                op.set_spmv_format(fmt)
                op.spmv_time(x, y, WARM)
                spmv[key].append(op.spmv_time(x, y, REPS))
            op.set_spmv_format(-1)
            for o in OPTIONS:
                sa.set_option("spmm", o)
                for k in KS:
                    op.spmm_time(x, ld, k, y, ld, WARM)
                    spmm[(k, o)].append(op.spmm_time(x, ld, k, y, ld, REPS))
    finally:
        sa.set_option("spmm", None)
        op.set_spmv_format(-1)
    base = {"matrix": name, "n": n, "nnz": op.nnz(), "automatic_spmv_format": auto_format, "rounds": ROUNDS, "reps": REPS}
    single, single0 = statistics.median(spmv["auto"]), statistics.median(spmv["format0"])
    emit(dict(base, case="spmv", automatic=med(spmv["auto"]), format0=med(spmv["format0"]),
              frac_8TBs_on_csr_bytes=round(plan_bytes(op, [1]) / (single * 1e-3) / HBM, 4)))
    verdict = {}
    for o in OPTIONS:
        sa.set_option("spmm", o)
        try:
            plans = {k: sa.spmm_plan(k) for k in KS}
        finally:
            sa.set_option("spmm", None)
        for k in KS:
            t = statistics.median(spmm[(k, o)])
            b = plan_bytes(op, plans[k])
            emit(dict(base, case="spmm", k=k, option=o, panels=plans[k], spmm=med(spmm[(k, o)]), k_spmv_automatic_ms=round(k * single, 5),
                      k_spmv_format0_ms=round(k * single0, 5), speedup_vs_automatic=round(k * single / t, 4),
                      speedup_vs_format0=round(k * single0 / t, 4), bytes=b, bytes_formula=FORMULA,
                      frac_8TBs=round(b / (t * 1e-3) / HBM, 4)))
            if o != "auto" and int(o) == k:   # exactly one panel of the forced width
                verdict[k] = {"spmm_ms": round(t, 5), "k_spmv_automatic_ms": round(k * single, 5), "faster": bool(t < k * single)}
    return verdict


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    nj = int(float(sys.argv[2])) if len(sys.argv) > 2 else n
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "bench_spmm.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    ctx = sa.default_context()
    with open(path, "a") as f:
        def emit(d):
            line = json.dumps(d)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        verdicts = {}
        op = sa.SparseSymMatProd.synth_band(n, ctx=ctx)
        verdicts["m_band"] = run("m_band", op, emit)
        del op
        A = workloads.jitter_band(nj)
        tri = sp.tril(A).tocsc()
        del A
        op = sa.SparseSymMatProd(tri, ctx=ctx)
        del tri
        verdicts["jitter_band"] = run("jitter_band", op, emit)
        del op
        keep = [w for w in (8, 4, 2) if all(v[w]["faster"] for v in verdicts.values())]
        emit({"case": "auto_rule", "rule": "a width stays in auto only if one panel of it beats as many single products in the automatic "
              "format on both matrices", "per_width": verdicts, "widths_kept": keep})


if __name__ == "__main__":
    main()
