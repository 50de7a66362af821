"""Ingest of the headline matrix (the lower triangle of M-band, CSC, n = argv[1], default 1e7) from HOST arrays against the same
arrays already RESIDENT on the GPU, in one process on one box.  One JSON line per path to the file argv[2] (default
profiles/bench_ingest.jsonl) and to stdout, then a line with the bit-for-bit check of the two operators.

  host:    sa.SparseSymMatProd(scipy CSC)            -> mispec_csr_from_triangle, stages of mispec_last_ingest_info
  device:  sa.SparseSymMatProd.from_torch(sparse_csc) -> mispec_csr_from_triangle_device, stages, and the peak device memory:
           torch.cuda.max_memory_allocated (the input tensors and what torch allocates during the call) + the library's own
           allocations by the formula of include/mispec.h (output 12 (E_out + 12) + 4 (n + 1), scratch 16 E_out + 4 n + scan sums;
           the library allocates with hipMalloc, which torch's counters do not see) — and, measured, the device memory the finished
           operator keeps (hipMemGetInfo before / after).
Timed: the constructor call only, median of REPS after WARM warm-ups; the operator of every repetition is released before the next.
The yardstick is the host path measured here, not a number from another run."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scipy.sparse as sp
import torch

import spectra_amd as sa

WARM, REPS = 1, 5


def timed(make):
    runs = []
    for i in range(WARM + REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        op = make()
        dt = time.perf_counter() - t0
        st = sa.last_ingest_info()
        if i >= WARM:
            runs.append((dt, st))
        if i + 1 < WARM + REPS:
            del op
    secs = [r[0] for r in runs]
    mid = sorted(runs, key=lambda r: r[0])[len(runs) // 2]
    return op, {"median_seconds": round(statistics.median(secs), 4), "min_seconds": round(min(secs), 4), "max_seconds": round(max(secs), 4),
                "stages_of_the_median_run": {k: round(v, 4) for k, v in mid[1].items()}}


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10 ** 7
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "bench_ingest.jsonl")
    ctx = sa.default_context()
    gen = sa.SparseSymMatProd.synth_band(n, ctx=ctx)
    rp, ci, v = gen.to_host_csr()
    del gen
    tri = sp.tril(sp.csr_matrix((v, ci, rp), shape=(n, n))).tocsc()
    tri.sort_indices()
    del rp, ci, v
    lines = []

    def emit(rec):
        rec = dict(rec, n=n, nnz_triangle=int(tri.nnz), host_threads=int(sa.lib().mispec_ingest_threads()))
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))

    host, rec = timed(lambda: sa.SparseSymMatProd(tri, ctx=ctx))
    emit(dict(rec, path="host arrays: mispec_csr_from_triangle"))

    for idx in (torch.int64, torch.int32):
        t = torch.sparse_csc_tensor(torch.from_numpy(tri.indptr).to("cuda", idx), torch.from_numpy(tri.indices).to("cuda", idx),
                                    torch.from_numpy(tri.data).cuda(), size=(n, n))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        free0 = torch.cuda.mem_get_info()[0]
        dev, rec = timed(lambda: sa.SparseSymMatProd.from_torch(t, ctx=ctx))
        torch.cuda.synchronize()
        kept = free0 - torch.cuda.mem_get_info()[0]
        e_out = dev.nnz()
        library_peak = 12 * (e_out + 12) + 4 * (n + 1) + 16 * e_out + 4 * n + 4 * ((n + 1 + 2047) // 2048)
        emit(dict(rec, path="device arrays (%s indices): mispec_csr_from_triangle_device" % str(idx).split(".")[-1],
                  torch_max_memory_allocated_bytes=int(torch.cuda.max_memory_allocated()),
                  library_peak_bytes_by_formula=int(library_peak), peak_bytes=int(torch.cuda.max_memory_allocated() + library_peak),
                  operator_keeps_bytes_measured=int(kept)))
        x = np.random.default_rng(1).uniform(-1.0, 1.0, n)
        same = all(np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b)
                   for a, b in zip(dev.to_host_csr(), host.to_host_csr()))
        same_y = np.array_equal(dev.perform_op(x).view(np.uint64), host.perform_op(x).view(np.uint64))
        emit({"check": "device-built operator against the host-built one, bit for bit", "indices": str(idx).split(".")[-1],
              "to_host_csr_equal": bool(same), "product_equal": bool(same_y), "spmv_format": [dev.spmv_format(), host.spmv_format()],
              "dia_info_equal": dev.dia_info() == host.dia_info(), "windows_info_equal": dev.windows_info() == host.windows_info()})
        del dev, t
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
