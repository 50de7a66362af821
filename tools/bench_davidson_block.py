"""Wall time of the Davidson solve of tests/test_gpu_davidson.py::test_at_scale_band_matrix (n = 4e5 band, nev = 6, maxit 200, tol
1e-8), for comparing two trees on the same box:

    python tools/bench_davidson_block.py                          one JSON line for the tree this file lies in
    python tools/bench_davidson_block.py --compare OTHER OUT      alternates fresh processes of OTHER (a checkout of the commit to
                                                                  compare with, built) and of this tree, ROUNDS each; every line is
                                                                  appended to OUT and a summary line follows
    --option NAME=VALUE                                           set a library option before the solves (e.g. spmm=0)
Each process builds the matrix once and solves SOLVES times; the first solve is the warm-up and is reported apart."""
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS, SOLVES = 3, 4


def one(root, option):
    sys.path.insert(0, root)
    import numpy as np
    import scipy.sparse as sp

    import spectra_amd as sa

    if option:
        name, value = option.split("=", 1)
        sa.set_option(name, value)
    n, k = 400_000, 6
    rng = np.random.default_rng(2)
    diags = [0.01 * rng.uniform(-1, 1, n - o) for o in (1, 2, 1000)]
    L = sp.diags([np.arange(1.0, n + 1.0)] + diags, [0, -1, -2, -1000], format="csc")
    ctx = sa.default_context()
    op = sa.SparseSymMatProd(L, ctx=ctx)
    times, res = [], None
    for _ in range(SOLVES):
        eigs = sa.DavidsonSymEigsSolver(op, k)
        ctx.sync()
        t0 = time.perf_counter()
        nconv = eigs.compute(sa.SortRule.LargestAlge, maxit=200, tol=1e-8)
        ctx.sync()
        times.append(time.perf_counter() - t0)
        res = (int(nconv), int(eigs.num_iterations()), int(eigs.num_operations()), float(np.sum(eigs.eigenvalues())))
    print(json.dumps({"case": "davidson_at_scale", "root": os.path.basename(os.path.abspath(root)), "option": option, "n": n, "nev": k,
                      "first_solve_s": round(times[0], 4), "solve_s": [round(t, 4) for t in times[1:]], "nconv": res[0],
                      "num_iterations": res[1], "num_operations": res[2], "eigenvalue_sum": res[3]}), flush=True)


def compare(other, out):
    lines = []
    for r in range(ROUNDS):
        for label, root in (("parent", other), ("tree", HERE)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root], stdout=subprocess.PIPE, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit("the %s process failed with status %d" % (label, p.returncode))
            d = json.loads(p.stdout.strip().splitlines()[-1])
            d.update(which=label, round=r)
            lines.append(d)
    summary = {"case": "davidson_at_scale_summary"}
    for label in ("parent", "tree"):
        t = [x for d in lines if d["which"] == label for x in d["solve_s"]]
        summary[label] = {"median_s": round(statistics.median(t), 4), "min_s": min(t), "max_s": max(t), "solves": len(t)}
    first = lines[0]
    summary["same_results"] = all((d["nconv"], d["num_iterations"], d["num_operations"], d["eigenvalue_sum"]) ==
                                  (first["nconv"], first["num_iterations"], first["num_operations"], first["eigenvalue_sum"]) for d in lines)
    with open(out, "a") as f:
        for d in lines + [summary]:
            f.write(json.dumps(d) + "\n")
            print(json.dumps(d), flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--compare":
        compare(a[1], a[2])
    else:
        root = a[a.index("--root") + 1] if "--root" in a else HERE
        one(root, a[a.index("--option") + 1] if "--option" in a else None)
