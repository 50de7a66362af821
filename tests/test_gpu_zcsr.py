"""The complex Hermitian sparse operator on the device (csrc/zcsr.hip, mispec_zcsr: one triangle mirrored conjugated into full int32
CSR, k_zspmv_csr) and the restart primitives of the complex factorisation over it (k_zvq in place and into a buffer, the new
residual; tests/herm_checks.py, also run on a host backend by tests/test_host_hermeigs.py)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import spectra_amd as sa

import herm_checks as HC
import zfac_checks as Z

pytestmark = pytest.mark.gpu


def random_lower(n, density, seed, empty_rows=()):
    """Lower triangle (with a real diagonal) of a random complex Hermitian sparse matrix, and the full matrix it stands for."""
    rng = np.random.default_rng(seed)
    M = sp.random(n, n, density=density, format="coo", random_state=rng, data_rvs=lambda k: rng.uniform(-0.5, 0.5, k))
    M = M + 1j * sp.random(n, n, density=density, format="coo", random_state=rng, data_rvs=lambda k: rng.uniform(-0.5, 0.5, k))
    L = sp.tril(M, -1) + sp.diags(rng.uniform(-0.5, 0.5, n))
    L = L.tocsr()
    for r in empty_rows:
        L[r, :] = 0
        L[:, r] = 0
    L.eliminate_zeros()
    full = (L + sp.tril(L, -1).conj().T).tocsr()
    return L, full


def x_for(n, seed=3):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)


def rel_err(y, ref, full, x):
    bound = np.abs(full) @ np.abs(x)
    return np.abs(y - ref).max() / max(bound.max(), 1e-300)


@pytest.mark.parametrize("n,density", [(1, 1.0), (10, 0.5), (1001, 0.01), (4099, 0.002)])
def test_spmv_matches_scipy(ctx, n, density):
    L, full = random_lower(n, density, seed=n)
    op = sa.SparseHermMatProd(L.tocsc(), "L", ctx)
    assert op.rows() == n and op.cols() == n and op.nnz() == full.nnz
    x = x_for(n)
    assert rel_err(op.perform_op(x), full @ x, full, x) <= 1e-14


def test_spmv_bit_identical_runs_and_layouts(ctx):
    n = 3000
    L, full = random_lower(n, 0.003, seed=11)
    x = x_for(n)
    a = sa.SparseHermMatProd(L.tocsc(), "L", ctx)
    y1, y2 = a.perform_op(x), a.perform_op(x)
    assert np.array_equal(y1, y2)
    U = L.conj().T  # the same operator stored as its upper triangle
    for mat, uplo in ((L.tocsr(), "L"), (U.tocsr(), "U"), (U.tocsc(), "U")):
        assert np.array_equal(sa.SparseHermMatProd(mat, uplo, ctx).perform_op(x), y1)
    # garbage in the triangle that is not read changes nothing
    G = (L + sp.triu(sp.random(n, n, density=0.003, random_state=5), 1) * (3 + 2j)).tocsc()
    assert np.array_equal(sa.SparseHermMatProd(G, "L", ctx).perform_op(x), y1)
    # and the diagonal's imaginary part is dropped
    D = (L + sp.diags(np.full(n, 0.25j))).tocsc()
    assert np.array_equal(sa.SparseHermMatProd(D, "L", ctx).perform_op(x), y1)
    assert a(5, 5).imag == 0.0 and a(0, 1) == np.conj(a(1, 0))


def test_spmv_empty_rows_int64_indices_and_zero_matrix(ctx):
    n = 777  # not a multiple of any tile size
    L, full = random_lower(n, 0.01, seed=2, empty_rows=(0, 13, 776))
    x = x_for(n)
    y = sa.SparseHermMatProd(L.tocsc(), "L", ctx).perform_op(x)
    assert y[0] == 0 and y[13] == 0 and y[776] == 0
    assert rel_err(y, full @ x, full, x) <= 1e-14
    L64 = L.tocsc()
    L64.indptr, L64.indices = L64.indptr.astype(np.int64), L64.indices.astype(np.int64)
    assert np.array_equal(sa.SparseHermMatProd(L64, "L", ctx).perform_op(x), y)
    Zm = sp.csc_matrix((n, n), dtype=np.complex128)
    z = sa.SparseHermMatProd(Zm, "L", ctx)
    assert z.nnz() == 0 and np.array_equal(z.perform_op(x), np.zeros(n, dtype=np.complex128))


def test_spmv_rejects_bad_input(ctx):
    with pytest.raises(ValueError):
        sa.SparseHermMatProd(sp.csc_matrix((3, 4), dtype=np.complex128), "L", ctx)
    with pytest.raises(ValueError):
        sa.SparseHermMatProd(sp.identity(4, dtype=np.complex128, format="csc"), "X", ctx)


@pytest.mark.parametrize("n,m,k", [(300, 20, 8), (5000, 40, 20)])
def test_restart_primitives_on_the_device_csr_operator(ctx, n, m, k):
    L, full = random_lower(n, 8.0 / n, seed=n)
    op = sa.SparseHermMatProd(L.tocsc(), "L", ctx)
    lib = sa.lib()
    fac = C.c_void_p()
    Z.ok(lib.mispec_zfac_create_csr(ctx.h, op.h, m, 1, C.byref(fac)))
    try:
        HC.restart_checks(lib, fac, full.toarray() if n <= 300 else full, m, k)
    finally:
        lib.mispec_zfac_destroy(fac)
