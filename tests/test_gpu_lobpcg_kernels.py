"""The three kernels of the LOBPCG solver (spectra_amd/csrc/lobpcg.hip), each alone through its hook, against numpy.longdouble.

k_gram: a workgroup walks a chunk of 32-row tiles, thread (ti, tj) holds G(ti + 16 a, tj + 16 b): the row counts are the tile, the
chunk boundary and ragged sizes (lobpcg_checks.kernel_row_counts), the column counts every slot boundary (16, 32, 48) -1/0/+1.  Its
second stage sums at most 512 records in one pass: there is no further branch.  The bound holds for ANY summation order.
k_lobpcg_resid forms r = fl(ax - fl(lambda bx)) WITHOUT a fused multiply-add and the Jacobi scaling as one more rounding: the bits are
fixed and compared exactly.  k_block_sub uses one fused multiply-add per term: c roundings per entry, inside the (c + 1) 2^-53 bound."""
import numpy as np
import pytest

import lobpcg_checks as L
import spectra_amd as sa

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
LD = np.longdouble

GRAM_SHAPES = [(1, 1, False), (1, 64, False), (64, 1, False), (3, 5, False), (24, 24, True), (47, 47, True), (63, 63, True),
               (64, 64, False), (64, 64, True),
               # register-slot boundaries
               (15, 17, False), (16, 16, True), (17, 15, False), (17, 17, True), (31, 33, False), (32, 32, True), (33, 31, False),
               (33, 33, True), (47, 49, False), (48, 48, True), (49, 47, False), (49, 49, True)]


def torch_block(host, ld, fill=np.nan):
    """host (n, cols) -> CUDA tensor (cols, ld), column j of the block in row j, the rows between n and ld filled with `fill`"""
    import torch

    n, cols = host.shape
    t = torch.full((cols, ld), fill, dtype=torch.float64, device="cuda")
    t[:, :n] = torch.from_numpy(np.ascontiguousarray(host.T)).cuda()
    return t


def asymmetric(rng, n, cols):
    """uniform(-1, 1) scaled per column by 2^j: a transposed or column-swapped result cannot pass"""
    return rng.uniform(-1, 1, (n, cols)) * (2.0 ** (np.arange(cols) % 24))


def leading_dimensions(n):
    even = n + 2 + (n % 2)
    return [even, even + 1]  # 16-byte loads / the 8-byte path of a block that is not 16-byte aligned column by column


@pytest.mark.parametrize("n", L.kernel_row_counts())
def test_gram(ctx, n):
    rng = np.random.default_rng(n)
    cols = 72
    H1, H2 = asymmetric(rng, n, cols), asymmetric(rng, n, 64)
    # every product the cases below need, once: H1'H1 and H1[:, :64]'H2, laid out as blocks of [H1 | H2]' [H1 | H2]
    L1, L2 = H1.astype(LD), H2.astype(LD)
    ref, refabs = np.zeros((cols + 64, cols + 64), dtype=LD), np.zeros((cols + 64, cols + 64), dtype=LD)
    ref[:cols, :cols], refabs[:cols, :cols] = L1.T @ L1, np.abs(L1).T @ np.abs(L1)
    ref[:64, cols:], refabs[:64, cols:] = L1[:, :64].T @ L2, np.abs(L1[:, :64]).T @ np.abs(L2)
    gamma = LD((n + 1) * U53) / (1 - LD((n + 1) * U53))
    for ld in leading_dimensions(n):
        T1, T2 = torch_block(H1, ld), torch_block(H2, ld)
        for p, q, sym in GRAM_SHAPES:
            cases = []
            if sym:
                cases.append((T1[5:5 + p], T1[5:5 + p], 5, 5))                      # U is W
                T2[:p] = T1[5:5 + p]
                cases.append((T1[5:5 + p], T2[:p], 5, 5))                           # equal blocks in two buffers
            else:
                cases.append((T1[:p], T2[:q], 0, cols))                             # two buffers
                cases.append((T1[2:2 + p], T1[7:7 + q] if q <= cols - 7 else T1[:q], 2, 7 if q <= cols - 7 else 0))  # overlapping
            for U, W, iu, iw in cases:
                G = sa.lobpcg_gram(U, W, n, symmetric=sym, ctx=ctx)
                G2 = sa.lobpcg_gram(U, W, n, symmetric=sym, ctx=ctx)
                what = "n=%d ld=%d p=%d q=%d sym=%s u0=%d w0=%d" % (n, ld, p, q, sym, iu, iw)
                assert G.shape == (p, q) and np.all(np.isfinite(G)), what     # the NaN padding rows did not reach it
                assert np.array_equal(G, G2), what                            # two calls, identical bits
                r = ref[iu:iu + p, iw:iw + q]
                bound = gamma * refabs[iu:iu + p, iw:iw + q]
                err = np.abs(G.astype(LD) - r)
                assert np.all(err <= bound), (what, float((err / np.maximum(bound, LD(1e-300))).max()))
                if sym:
                    assert np.array_equal(G, G.T), what
            if sym:
                T2[:p] = torch_block(H2[:, :p], ld)  # restore


ACTIVE_LISTS = {"all": lambda m: list(range(m)), "none": lambda m: [], "one": lambda m: [m - 1], "every other": lambda m: list(range(0, m, 2))}


@pytest.mark.parametrize("n", L.kernel_row_counts() + [L.RESID_GROUP_ROWS * L.RESID_MAX_GROUPS + 3])
def test_resid(ctx, n):
    import torch

    rng = np.random.default_rng(n + 1)
    big = n > 100000  # beyond 1024 workgroups' chunks a workgroup sweeps twice
    gamma = LD((n + 1) * U53) / (1 - LD((n + 1) * U53))
    for m in ([8] if big else [1, 8, 21]):
        AX, BX = asymmetric(rng, n, m), asymmetric(rng, n, m)
        lam = rng.uniform(-2, 2, m)
        dinv = rng.uniform(0.5, 2, n)
        for ld in (leading_dimensions(n)[:1] if big else leading_dimensions(n)):
            tA, tB = torch_block(AX, ld), torch_block(BX, ld)
            tD = torch.full((ld,), float("nan"), dtype=torch.float64, device="cuda")
            tD[:n] = torch.from_numpy(dinv).cuda()
            for name, make in ACTIVE_LISTS.items():
                idx = make(m)
                for use_dinv in (False, True):
                    ldr = ld + 2
                    tR = torch.full((m, ldr), 777.0, dtype=torch.float64, device="cuda")
                    norms2 = sa.lobpcg_resid(tA, tB, n, lam, idx, R=tR, dinv=tD if use_dinv else None, ctx=ctx)
                    what = "n=%d m=%d ld=%d active=%s dinv=%s" % (n, m, ld, name, use_dinv)
                    r = AX - lam * BX  # numpy rounds the product, then the difference: the kernel's form
                    R = tR.cpu().numpy()
                    for k, j in enumerate(idx):
                        want = r[:, j] * dinv if use_dinv else r[:, j]
                        assert np.array_equal(R[k, :n], want), (what, k, j)
                    assert np.all(R[len(idx):] == 777.0) and np.all(R[:, n:] == 777.0), what  # canaries: inactive columns, padding
                    s = (r.astype(LD) ** 2).sum(axis=0)
                    assert np.all(np.abs(norms2.astype(LD) - s) <= gamma * s), what
                    assert np.array_equal(norms2, sa.lobpcg_resid(tA, tB, n, lam, idx, R=tR, dinv=tD if use_dinv else None, ctx=ctx)), what


@pytest.mark.parametrize("n", L.kernel_row_counts())
def test_block_sub(ctx, n):
    rng = np.random.default_rng(n + 2)
    for q, c in [(1, 1), (8, 3), (21, 21)]:
        Z, Y = asymmetric(rng, n, q), asymmetric(rng, n, c)
        Cm = rng.uniform(-1, 1, (c, q))
        for ld in leading_dimensions(n):
            tZ, tY = torch_block(Z, ld, fill=777.0), torch_block(Y, ld + 1)
            sa.lobpcg_block_sub(tZ, tY, Cm, n, ctx=ctx)
            out = tZ.cpu().numpy()
            what = "n=%d q=%d c=%d ld=%d" % (n, q, c, ld)
            assert np.all(out[:, n:] == 777.0), what
            ref = Z.astype(LD) - Y.astype(LD) @ Cm.astype(LD)
            bound = LD((c + 1) * U53) * (np.abs(Z).astype(LD) + np.abs(Y).astype(LD) @ np.abs(Cm).astype(LD))
            assert np.all(np.abs(out[:, :n].T.astype(LD) - ref) <= bound), what


def test_kernel_arguments_are_checked(ctx):
    import torch

    t = torch.zeros((65, 8), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        sa.lobpcg_gram(t, t[:3], 8, ctx=ctx)            # 65 columns
    with pytest.raises(ValueError):
        sa.lobpcg_gram(t[:3], t[:4], 8, symmetric=True, ctx=ctx)
    with pytest.raises(ValueError):
        sa.lobpcg_gram(t[:3], t[:3], 9, ctx=ctx)        # ld < n
    with pytest.raises(ValueError):
        sa.lobpcg_resid(t[:22], t[:22], 8, np.zeros(22), [], ctx=ctx)
    with pytest.raises(ValueError):
        sa.lobpcg_resid(t[:3], t[3:6], 8, np.zeros(3), [1, 1], R=t[6:9], ctx=ctx)
    with pytest.raises(ValueError):
        sa.lobpcg_block_sub(t[:22], t[22:23], np.zeros((1, 22)), 8, ctx=ctx)
