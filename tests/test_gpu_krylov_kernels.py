"""The real orthogonalisation and V*Q kernels one step at a time (tests/krylov_checks.py: scripted operators, long-double
references, bounds counted from the kernels' source), at the smallest shapes at which each branch of csrc/krylov.hip,
csrc/orth_dma_modes.hip (launchers: csrc/orth_launch.hpp) and the step code of csrc/fac.hip exists.  The sizes that depend on
the device are derived from its CU count; the figures in the comments are for 256 CUs.  tests/test_host_krylov_checks.py shows, without a GPU, that an honest
float64 implementation meets these bounds and that each targeted defect exceeds them at least 100 times."""
import numpy as np
import pytest
import torch

import krylov_checks as K
import spectra_amd as sa

pytestmark = pytest.mark.gpu


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def scripted(ctx, n, m, symmetric, device, forced=False):
    """A fresh (factorisation, script, v0) over the script W(n, m): host operator or sa.DeviceOp."""
    W = K.script_matrix(n, m, 100 + n + m)
    if device:
        script = K.DeviceScript(W)
        fac = sa.Factorization(sa.DeviceOp(n, script, ctx=ctx), m, symmetric)
    else:
        script = K.HostScript(W, forced=forced, seed=n, record=n <= K.LD_ALL_ROWS)
        fac = sa.Factorization(script, m, symmetric, ctx=ctx)
    if symmetric:
        fac.set_orth_mode("reference")
    return fac, script, np.random.default_rng(n).uniform(-1.0, 1.0, n)


def run_steps(ctx, n, m, symmetric, device=False, forced=False, model=None, at_once=True):
    model = model or K.HipModel(cus())
    fac, script, v0 = scripted(ctx, n, m, symmetric, device, forced)
    run = K.collect(fac, script, m, v0, symmetric)
    if at_once and m > 1:  # the same steps enqueued in one factorize_from(1, m): bit for bit the same factorisation
        fac2, script2, _ = scripted(ctx, n, m, symmetric, device, forced)
        result, syncs = K.collect_at_once(fac2, script2, m, v0)
        K.assert_same_factorisation(run, result)
        assert np.array_equal(script2.W, run.W)
        if device and m >= 8:  # ... and it was a device-driven run: fewer host synchronisations than steps
            assert syncs < m - 1, (syncs, m)
    what = f"{'lanczos' if symmetric else 'arnoldi'} {n} x {m} ({'DeviceOp' if device else 'host operator'}{', forced' if forced else ''})"
    (K.check_lanczos if symmetric else K.check_arnoldi)(run, model).assert_ok(what)
    return run


# k_orth<MODE, S, R>: one row pair (1, 2, 3 rows: the zero-padded odd last row), one tile and its edges (127, 128, 129 rows with
# R = 2: 255, 256, 257), every slot count S = 1 ... 16 and the switch of the tile height at 40 | 41 columns (1000 x 64), column
# panels with col0 = 64, 128, 256 (65, 129, 257 columns).  Host-driven steps: ORTH_VTF, then ORTH_CORRECT_VTF.
@pytest.mark.parametrize("n,m", [(1, 1), (2, 2), (3, 3), (127, 8), (128, 8), (129, 9), (255, 41), (256, 41), (257, 44), (1000, 64),
                                 (1000, 65), (1000, 129), (1030, 257)])
def test_arnoldi_steps_host_driven(ctx, n, m):
    run_steps(ctx, n, m, False)


# the same passes enqueued by arnoldi_step_device, with kFinishArnoldiH / kFinishArnoldiF as the scalar tails
@pytest.mark.parametrize("n,m", [(257, 44), (1000, 65)])
def test_arnoldi_steps_device_driven(ctx, n, m):
    run_steps(ctx, n, m, False, device=True)


# w = V c + 1e-3 r: the 0.717 test fails in every step and the correction loop (ORTH_CORRECT_VTF in place) runs
@pytest.mark.parametrize("n,m", [(257, 44), (1000, 65)])
def test_arnoldi_steps_with_the_correction_loop(ctx, n, m):
    run_steps(ctx, n, m, False, forced=True)


# Lanczos, reference flow: k_lanczos_epilogue, ORTH_RESID_VTF, ORTH_CORRECT_VTF with full-sized coefficients (the script is not
# symmetric: V'f0 is of order one); lanczos_step_host, and lanczos_step_device with kFinishStepFirst / kFinishStepCorr
@pytest.mark.parametrize("device", [False, True], ids=["host-operator", "device-operator"])
@pytest.mark.parametrize("n,m", [(3, 3), (257, 44), (1000, 65), (1000, 129)])
def test_lanczos_steps(ctx, n, m, device):
    run_steps(ctx, n, m, True, device=device)


# the switch to k_orth_dma at 1024 tiles of 128 rows: the last size of the register kernel, exactly 1024 full tiles, and 1025
# tiles, ragged and odd, with every MAXS = 2 ... 16 and both ring depths (four or five tiles per workgroup)
@pytest.mark.parametrize("n,m", [(131_071, 8), (131_072, 8), (131_075, 64)])
def test_arnoldi_steps_across_the_switch_to_the_lds_dma_kernels(ctx, n, m):
    model = K.HipModel(cus())
    assert model.orth_launches(n, m)[0]["kernel"] == ("k_orth" if n < 131_072 else "k_orth_dma")
    run_steps(ctx, n, m, False, model=model)


def test_lanczos_steps_on_the_lds_dma_kernels(ctx):
    run_steps(ctx, 131_075, 64, True, device=True)


# the register kernels with several tiles per workgroup (the psum[buf] double buffer alternates): more than 2 x 4 CUs tiles of
# 256 rows — some workgroups take three tiles at R = 2 (up to 40 columns) and five at R = 1 (41 ... 44)
def test_arnoldi_steps_on_register_kernels_with_several_tiles_per_workgroup(ctx):
    n, m = 2 * (4 * cus() * 256) + 259, 44  # 524 547
    model = K.HipModel(cus(), force_reg=True)
    assert model.orth_launches(n, 40)[0]["T"] == 3 and model.orth_launches(n, 41)[0]["T"] == 5
    try:
        sa.set_option("orth_kernel", "reg")
        run_steps(ctx, n, m, False, model=model, at_once=False)
    finally:
        sa.set_option("orth_kernel", None)


# ---- V * Q ----------------------------------------------------------------------------------------------------------------
def n_prefetch():
    return 3 * cus() * 128 + 1699  # 100 003: more tiles of 128 rows than 3 CUs workgroups — some prefetch a second tile


def factorised(ctx, n, m):
    fac, script, v0 = scripted(ctx, n, m, False, device=False)
    fac.init(v0)
    fac.factorize_from(1, m)
    assert script.calls == fac.num_operations() == m + 1
    return fac, np.asfortranarray(fac.matrix_V()), fac.vector_f()


# k_vq<4 | 8 | 12 | 16> at its last and first output-column counts, one tile per workgroup and with the prefetch of a second
@pytest.mark.parametrize("big", [False, True], ids=["1000-rows", "prefetch"])
def test_ritz_vectors_one_panel(ctx, big):
    n, m = (n_prefetch() if big else 1000), 64
    fac, V, _ = factorised(ctx, n, m)
    model, out = K.HipModel(cus()), K.Ratios()
    for p in (1, 4, 5, 16, 17, 32, 33, 48, 49, 64):
        K.check_ritz(fac, V, p, model, out)
    assert np.array_equal(fac.matrix_V(), V)  # the basis itself is left alone
    out.assert_ok(f"ritz vectors {n} x {m}")


# accumulation over panels of input columns, panels of output columns
@pytest.mark.parametrize("m,p", [(65, 64), (129, 65), (257, 1)])
def test_ritz_vectors_in_panels(ctx, m, p):
    fac, V, _ = factorised(ctx, 1000, m)
    out = K.Ratios()
    K.check_ritz(fac, V, p, K.HipModel(cus()), out)
    assert np.array_equal(fac.matrix_V(), V)
    out.assert_ok(f"ritz vectors 1000 x {m}, {p} columns")


# compress_V: in place (up to 64 columns) and through the workspace (129), then k_axpby and its norm
@pytest.mark.parametrize("big,m,k", [(False, 20, 12), (False, 64, 63), (False, 64, 1), (False, 129, 70), (True, 20, 12),
                                     (True, 64, 63), (True, 64, 1)])
def test_compress_v(ctx, m, k, big):
    n = n_prefetch() if big else 1000
    fac, V, f = factorised(ctx, n, m)
    out = K.Ratios()
    K.check_compress(fac, V, f, k, K.HipModel(cus()), out)
    out.assert_ok(f"compress_V {n} x {m} -> {k}")
