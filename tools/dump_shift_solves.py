"""Digests of what the shift solve computes, to compare two builds of the library bit for bit: per case one line with the SHA-256
of the bytes of a single solve (mispec_symshift_solve on a seeded right-hand side) and of a 5-column block solve under
shift_block = 4 (a panel of 4 and a single column).  The cases are those of tests/test_gpu_shift_block.py (narrow and deep shapes
with and without the explicit chunk inverses, the dense inverse and wide top levels, indefinite shifts with refinement, a reordered
matrix) plus a half-bandwidth of 40, the banded Cholesky solves and two dense products, which share the kernels.

Run it in two trees and compare the outputs; equal lines mean equal bits.  The digests also depend on how the compiler contracts
the factorisation kernels, so they are a comparison between two builds made by one compiler, not golden values.

    timeout 600 python tools/dump_shift_solves.py [--out FILE]
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import numpy as np
import scipy.sparse as sp

import shift_block_checks as SB
import spectra_amd as sa

DENSE_AND_WIDE = [(50, 16), (51, 16), (1500, 3), (3000, 16), (6000, 16)]   # test_dense_inverse_and_wide_top_level
INDEFINITE = [(3000, 2, 0.3), (5000, 3, 1.0), (100_000, 3, 0.1234)]          # test_indefinite_shifts_refine_every_column
K = 5


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def solves(op, n):
    """digests of a single solve of column 0 and of the block solve of all K columns, on the device"""
    import torch

    Xd = torch.from_numpy(np.ascontiguousarray(SB.rhs_block(n, K).T)).cuda()  # (K, n) row-major = n x K column-major
    y = torch.zeros(n, dtype=torch.float64, device="cuda")
    Y = torch.zeros((K, n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    op.solve_device(Xd.data_ptr(), y.data_ptr())
    try:
        sa.set_option("shift_block", "4")
        op.solve_block_device(Xd.data_ptr(), n, K, Y.data_ptr(), n)
    finally:
        sa.set_option("shift_block", None)
    torch.cuda.synchronize()
    return "single " + sha(y.cpu().numpy()) + " block5 " + sha(Y.cpu().numpy())


def shift_op(A, sigma, ctx, shift_option=None):
    op = sa.SparseSymShiftSolve(sp.tril(A).tocsc(), ctx=ctx)
    try:
        if shift_option:
            sa.set_option("shift", shift_option)  # read when the levels are factored
        op.set_shift(sigma)
    finally:
        sa.set_option("shift", None)
    return op


def cases(ctx):
    for n, b in SB.NARROW_SHAPES + SB.DEEP_SHAPES:
        A = SB.banded_spd(n, b, seed=n)
        for option in (None, "block_inverse=0"):
            yield f"spd n={n} b={b} sigma=-1.5 shift={option}", solves(shift_op(A, -1.5, ctx, option), n)
    for n, b in DENSE_AND_WIDE + [(20_000, 40)]:
        yield f"spd n={n} b={b} sigma=0", solves(shift_op(SB.banded_spd(n, b, seed=n), 0.0, ctx), n)
    for n, b, sigma in INDEFINITE:
        op = shift_op(SB.banded_indefinite(n, b, seed=n + b), sigma, ctx)
        yield f"indefinite n={n} b={b} sigma={sigma} refine_steps={op.refinement_info()['refine_steps']}", solves(op, n)
    n = 50_000  # test_reordered_band
    q = np.random.default_rng(11).permutation(n)
    op = shift_op(SB.banded_spd(n, 3, seed=7)[q][:, q].tocsc(), -1.0, ctx)
    yield f"reordered n={n} b=3 sigma=-1 reordered={op.bandwidth_info()['reordered']}", solves(op, n)
    n = 6000
    chol = sa.SparseCholesky(sp.tril(SB.banded_spd(n, 3, seed=n)).tocsc(), ctx=ctx)
    x = SB.rhs_block(n, 1)[:, 0]
    yield (f"cholesky n={n} b=3 info={chol.info().name}",
           "lower " + sha(chol.lower_triangular_solve(x)) + " upper " + sha(chol.upper_triangular_solve(x)))
    for n in (300, 301):
        M = np.random.default_rng(n).uniform(-1, 1, (n, n))
        yield f"dense product n={n}", "y " + sha(sa.DenseSymMatProd(M + M.T, ctx=ctx).perform_op(SB.rhs_block(n, 1)[:, 0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for name, digests in cases(sa.default_context()):
        lines.append(f"{name}: {digests}")
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
