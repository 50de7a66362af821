"""The Davidson solver's A V for the new columns is one block product (launch_spmm, spectra_amd/csrc/spmm.hip) instead of one
SpMV per column.  The block product is bit-identical to the column loop, so a solve under option spmm=0 (the column loop) and
one under spmm=auto must agree in everything: eigenvalues and eigenvectors to the bit, iterations, operator applications, info."""
import numpy as np
import pytest

import spectra_amd as sa
from test_oracle_davidson import davidson_sparse_fixture

pytestmark = pytest.mark.gpu


def solve(op, nev, spmm):
    sa.set_option("spmm", spmm)
    try:
        eigs = sa.DavidsonSymEigsSolver(op, nev)
        nconv = eigs.compute(sa.SortRule.LargestAlge)
        return nconv, eigs.eigenvalues(), eigs.eigenvectors(), eigs.num_iterations(), eigs.num_operations(), int(eigs.info())
    finally:
        sa.set_option("spmm", None)


@pytest.mark.parametrize("reorder", ["none", "rcm"])
def test_block_product_leaves_the_solve_unchanged(ctx, reorder):
    n, nev = 1000, 5
    A, S = davidson_sparse_fixture(n)
    op = sa.SparseSymMatProd(A, ctx=ctx, reorder=reorder)
    assert op.reordering() == reorder
    # the start block of 2 nev columns and every extension by nev columns hold at least one panel: the block kernel runs
    assert max(sa.spmm_plan(2 * nev)) > 1 and max(sa.spmm_plan(nev)) > 1
    old = solve(op, nev, "0")
    new = solve(op, nev, "auto")
    assert old[0] == nev and old[5] == int(sa.CompInfo.Successful)
    assert new[0] == old[0]
    assert np.array_equal(new[1], old[1])          # eigenvalues
    assert np.array_equal(new[2], old[2])          # eigenvectors, bit for bit
    assert new[3:] == old[3:], (new[3:], old[3:])  # num_iterations, num_operations, info
    assert old[4] > 2 * nev                        # more products than the start block: extensions went through the block path too
    evals, evecs = new[1], new[2]
    assert np.abs(S @ evecs - evecs * evals).max() < 1e-10  # the reference's bar (test/DavidsonSymEigs.cpp)
