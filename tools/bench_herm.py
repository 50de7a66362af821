"""Complex Hermitian solver benchmark (HermEigsSolver over SparseHermMatProd<std::complex<double>>): the complex M-band
(spectra_amd/workloads.herm_band: M-band's offsets, independent counter-hash real and imaginary parts, real diagonal) at n = 1e7,
nev = 20, ncv = 40, LargestMagn.  Prints one JSON line: seconds per solve, eigenpairs/s, operation and restart counts, the residual
max|AU - U Lambda| computed by scipy on the host, and HIP-event times of the three kernels of the complex path with their share of
8 TB/s on the bytes the algorithm must move:
  k_zspmv_csr  20 B per stored entry (16-byte value + 4-byte column) + 4 B per row pointer + x and y once (16 B per row each),
               for 4, 8 and 16 lanes per row (the default is 8: DESIGN.md "Complex Hermitian solver");
  X^H y        (k_zdotc_partial + k_zdotc_final) ncv columns of V and y, 16 B per entry;
  k_zvq        in place, V Q writing k + 1 = nev + 1 columns: reads ncv columns, writes k + 1.
Kernel times for the solve itself come from a separate `rocprofv3 --kernel-trace --stats` run of this script (--no-resid).

    python tools/bench_herm.py [--n N] [--nev K] [--ncv M] [--reps R] [--no-resid] [--out FILE]
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
from spectra_amd import workloads

PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--nev", type=int, default=20)
    ap.add_argument("--ncv", type=int, default=40)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--no-resid", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, k, m = a.n, a.nev, a.ncv
    ctx = sa.default_context()
    t0 = time.perf_counter()
    L = workloads.herm_band(n)
    t_gen = time.perf_counter() - t0
    t0 = time.perf_counter()
    op = sa.SparseHermMatProd(L, "L", ctx)
    t_up = time.perf_counter() - t0
    res = {"workload": "complex M-band", "n": n, "nev": k, "ncv": m, "rule": "LargestMagn", "nnz": op.nnz(),
           "seconds_generate_host": round(t_gen, 3), "seconds_ingest": round(t_up, 3)}

    # kernels on their own (HIP events, back to back)
    bytes_spmv = op.algorithmic_bytes()
    spmv = {}
    for lpr in (4, 8, 16):
        ms = op.spmv_time(20, lpr)
        spmv[str(lpr)] = {"ms": round(ms, 4), "TBps": round(bytes_spmv / (ms * 1e-3) / 1e12, 3),
                          "frac_8TBps": round(bytes_spmv / (ms * 1e-3) / PEAK, 3)}
    res["k_zspmv_csr"] = {"bytes": bytes_spmv, "lanes_per_row": spmv}
    lib = sa.lib()
    fac = C.c_void_p()
    sa.check(lib.mispec_zfac_create_csr(ctx.h, op.h, m, 1, C.byref(fac)))
    try:
        rng = np.random.default_rng(0)
        v0 = np.ascontiguousarray(rng.uniform(-0.5, 0.5, n) + 1j * rng.uniform(-0.5, 0.5, n))
        cnt = C.c_int64(0)
        dp = v0.ctypes.data_as(C.POINTER(C.c_double))
        sa.check(lib.mispec_zfac_init(fac, dp, C.byref(cnt)))
        sa.check(lib.mispec_zfac_factorize(fac, 1, m, C.byref(cnt)))
        ms = C.c_float()
        sa.check(lib.mispec_zfac_kernel_time(fac, 0, m, 20, C.byref(ms)))
        b = 16.0 * n * (m + 1)
        res["XHy"] = {"ncols": m, "ms": round(ms.value, 4), "bytes": b, "frac_8TBps": round(b / (ms.value * 1e-3) / PEAK, 3)}
        sa.check(lib.mispec_zfac_kernel_time(fac, 1, k + 1, 10, C.byref(ms)))
        b = 16.0 * n * (m + k + 1)
        res["k_zvq"] = {"ncols_out": k + 1, "ms": round(ms.value, 4), "bytes": b, "frac_8TBps": round(b / (ms.value * 1e-3) / PEAK, 3)}
    finally:
        lib.mispec_zfac_destroy(fac)

    # the solve
    times = []
    for _ in range(a.reps):
        eigs = sa.HermEigsSolver(op, k, m)
        t0 = time.perf_counter()
        eigs.init()
        nconv = eigs.compute(sa.SortRule.LargestMagn)
        U = eigs.eigenvectors()
        times.append(time.perf_counter() - t0)
        assert eigs.info() == sa.CompInfo.Successful and nconv == k, (eigs.info(), nconv)
    secs = min(times)
    evals = eigs.eigenvalues()
    res.update({"seconds_per_solve": round(secs, 3), "all_solves": [round(t, 3) for t in times], "eigenpairs_per_s": round(k / secs, 3),
                "num_operations": eigs.num_operations(), "num_restarts": eigs.num_iterations(),
                "eigenvalues_head": [float(x) for x in evals[:3]]})
    if not a.no_resid:
        full = (L + sp.tril(L, -1).conj().T).tocsr()
        res["resid_max_abs"] = float(np.abs(full @ U - U * evals).max())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
