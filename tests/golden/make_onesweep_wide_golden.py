"""Records what the CPU oracle gives on the wide-basis shapes of tests/test_gpu_onesweep_panels.py whose oracle run takes minutes
(n = 30 001; ncv = 193, 400, 512): the reference algorithm (oracle.SymEigsSolver) and the oracle's restatement of the one-sweep
variant in both reduction forms (set_onesweep(True, fused=False, one_reduction=...)).  The GPU test compares against these records
instead of running the oracle for a minute per case; the n = 1000 shapes are run live there.

    python tests/golden/make_onesweep_wide_golden.py      ->  tests/golden/onesweep_wide_oracle.json

The oracle by itself has to meet the gates the device is held to, otherwise the shape is no yardstick: nconv == k, info 0, relative
residual <= 1e-10, X'X - I <= 1e-10, variant against reference: eigenvalues to 1e-9, operations within ncv - k.  The script asserts
that and prints the figures."""
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import oracle as O  # noqa: E402

OFFSETS = (1, 2, 3, 100, 101, 2000, 2001)
SHAPES = [(30_001, 90, 193), (30_001, 150, 400), (30_001, 200, 512)]
RULES = ("LargestAlge", "BothEnds")
FLAVOURS = {"reference": None, "two-reductions": False, "one-reduction": True}


def main():
    out, bad = {}, []
    for n, k, m in SHAPES:
        rp, ci, v = O.synth_band_csr(n, offsets=OFFSETS)
        S = sp.csr_matrix((v, ci, rp), shape=(n, n))
        for rule in RULES:
            ref = None
            for flavour, one_reduction in FLAVOURS.items():
                t0 = time.time()
                o = O.SymEigsSolver(O.Op.csr(n, n, rp, ci, v), k, m)
                if one_reduction is not None:
                    o.set_onesweep(True, fused=False, one_reduction=one_reduction)
                o.init()
                nconv = o.compute(getattr(O, rule), 1000, 1e-11)
                ev, X = o.eigenvalues(), o.eigenvectors()
                resid = (np.linalg.norm(S @ X - X * ev, axis=0) / np.linalg.norm(X, axis=0)).max()
                orth = np.abs(X.T @ X - np.eye(k)).max()
                rec = {"nconv": int(nconv), "info": int(o.info()), "num_operations": int(o.num_operations()),
                       "num_iterations": int(o.num_iterations()), "eigenvalues": [float(x) for x in ev],
                       "max_rel_residual": float(resid), "max_orth_defect": float(orth)}
                if ref is None:
                    ref = rec
                dlam = np.abs(np.sort(ev) - np.sort(ref["eigenvalues"])).max()
                dops = rec["num_operations"] - ref["num_operations"]
                print(n, k, m, rule, flavour, "nconv", nconv, "ops", rec["num_operations"], "resid %.2e orth %.2e dlam %.2e dops %d"
                      % (resid, orth, dlam, dops), "%.0f s" % (time.time() - t0), flush=True)
                if not (nconv == k and rec["info"] == 0 and resid <= 1e-10 and orth <= 1e-10 and dlam < 1e-9 and abs(dops) <= m - k):
                    bad.append((n, k, m, rule, flavour))
                out["%d_%d_%d_%s_%s" % (n, k, m, rule, flavour)] = rec
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "onesweep_wide_oracle.json"), "w") as f:
        json.dump(out, f, indent=0)
    assert not bad, "the oracle itself misses the gates on %r: replace these shapes" % bad


if __name__ == "__main__":
    main()
