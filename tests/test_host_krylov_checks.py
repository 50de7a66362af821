"""tests/krylov_checks.py without a GPU: the checks that tests/test_gpu_krylov_kernels.py runs on the kernels, run here on a float64
numpy stand-in of the same interface (plain Arnoldi.h / Lanczos.h control flow, every sum one BLAS call: HostModel's roundings).
Twice: honest — the stand-in must stay inside every bound at every shape — and with each defect the checks are aimed at built
into the stand-in's primitives (persistently, as a wrong kernel would have it), where the bound must be exceeded 100 times."""
import numpy as np
import pytest

import krylov_checks as K

EPS = 2.0 ** -52


class NumpyFactorization:
    """init / factorize_from / matrix_V / matrix_H / vector_f / f_norm / num_operations / ritz_vectors / compress_V in float64."""

    def __init__(self, op, m, symmetric, defect=None):
        self.op, self.m, self.n, self.symmetric, self.defect = op, m, op.rows(), symmetric, defect
        self.V = np.zeros((self.n, m), order="F")
        self.H = np.zeros((m, m), order="F")
        self.f, self.beta, self.k, self.ops = np.zeros(self.n), 0.0, 0, 0

    # ---- the three primitives the kernels implement, with the targeted defects ----
    def _vtf(self, x, ncol):
        V = self.V[:, :ncol]
        c = V.T @ x
        if self.defect == "dot_last_row":  # the last row left out of one column's dot product
            c[0] -= V[-1, 0] * x[-1]
        if self.defect == "dot_last_tile":  # the last 128-row tile left out
            t0 = ((self.n - 1) // 128) * 128
            c -= V[t0:].T @ x[t0:]
        return c

    def _sub(self, x, c, ncol):
        c = c.copy()
        if self.defect == "sub_skip_col" and ncol > 1:  # one column skipped in the subtraction
            c[1] = 0.0
        if self.defect == "panel_coeffs" and ncol > K.PANEL:  # the second panel's coefficients taken from panel 0
            hi = min(ncol, 2 * K.PANEL)
            c[K.PANEL: hi] = c[: hi - K.PANEL]
        return x - self.V[:, :ncol] @ c

    def _vq(self, V, Q):
        Q = Q.copy()
        if self.defect == "q_zero_col":  # one column of Q zeroed
            Q[:, Q.shape[1] - 1] = 0.0
        return V @ Q

    def _apply(self, x):
        self.ops += 1
        return np.array(self.op.perform_op(x), dtype=np.float64)

    # ---- Arnoldi.h:145-195 ----
    def init(self, v0):
        v = self._apply(np.asarray(v0, dtype=np.float64))
        v = v / np.linalg.norm(v)
        w = self._apply(v)
        self.V[:, 0] = v
        self.H[0, 0] = v @ w
        self.f = w - v * self.H[0, 0]
        if np.abs(self.f).max() < EPS * abs(self.H[0, 0]):
            self.f[:] = 0.0
        self.beta, self.k = float(np.linalg.norm(self.f)), 1

    def factorize_from(self, from_k, to_m):
        n, V, H = self.n, self.V, self.H
        for i in range(from_k, to_m):
            assert self.beta > 0.0, "the restart branch (Arnoldi.h:228) is not part of the stand-in: the script must not reach it"
            V[:, i] = self.f / self.beta
            H[i, i - 1] = self.beta
            w = self._apply(V[:, i])
            i1 = i + 1
            if self.symmetric:  # Lanczos.h:127-182
                H[i - 1, i] = self.beta
                w = w - self.beta * V[:, i - 1]
                H[i, i] = V[:, i] @ w
                f = w - H[i, i] * V[:, i]
            else:  # Arnoldi.h:242-291
                h = self._vtf(w, i1)
                f = self._sub(w, h, i1)
            beta = float(np.linalg.norm(f))
            if self.symmetric or beta <= 0.717 * np.linalg.norm(h):
                Vf = self._vtf(f, i1)
                count = 0
                while count < 5 and np.abs(Vf).max() > EPS * beta:
                    if beta < EPS * np.sqrt(n):
                        f, beta = np.zeros(n), 0.0
                        break
                    f = self._sub(f, Vf, i1)
                    if self.symmetric:
                        H[i - 1, i] += Vf[i - 1]
                        H[i, i - 1] = H[i - 1, i]
                        H[i, i] += Vf[i]
                    else:
                        h = h + Vf
                    beta = float(np.linalg.norm(f))
                    Vf = self._vtf(f, i1)
                    count += 1
            if not self.symmetric:
                H[:i1, i] = h
            self.f, self.beta = f, beta
        self.k = to_m

    def matrix_V(self):
        return self.V.copy(order="F")

    def matrix_H(self):
        return self.H.copy(order="F")

    def vector_f(self):
        return self.f.copy()

    def f_norm(self):
        return self.beta

    def num_operations(self):
        return self.ops

    def ritz_vectors(self, Y):
        return self._vq(self.V, Y)

    def compress_V(self, Q, H, k):  # Arnoldi.h:326-339
        X = self._vq(self.V, Q[:, : k + 1])
        self.f = self.f * Q[self.m - 1, k - 1] + X[:, k] * H[k, k - 1]
        self.V[:, : k + 1] = X
        self.H, self.beta, self.k = np.array(H, order="F"), float(np.linalg.norm(self.f)), k


MODEL = K.HostModel()
ARNOLDI_SHAPES = [(1, 1), (2, 2), (3, 3), (127, 8), (128, 8), (129, 9), (255, 41), (256, 41), (257, 44), (1000, 64), (1000, 65),
                  (1000, 129), (4099, 44), (131_075, 16)]
LANCZOS_SHAPES = [(3, 3), (257, 44), (1000, 65), (1000, 129), (4099, 44), (131_075, 16)]


def run(n, m, symmetric, defect=None, forced=False):
    W = K.script_matrix(n, m, 100 + n + m)
    script = K.HostScript(W, forced=forced, seed=n)
    fac = NumpyFactorization(script, m, symmetric, defect)
    v0 = np.random.default_rng(n).uniform(-1.0, 1.0, n)
    return K.collect(fac, script, m, v0, symmetric), fac


@pytest.mark.parametrize("n,m", ARNOLDI_SHAPES)
def test_the_honest_arnoldi_stand_in_meets_every_bound(n, m):
    r, _ = run(n, m, False)
    K.check_arnoldi(r, MODEL).assert_ok(f"arnoldi {n} x {m}")
    if m > 1:  # one factorize_from(1, m) is the same factorisation as m - 1 single steps
        script = K.HostScript(r.W)
        result, _ = K.collect_at_once(NumpyFactorization(script, m, False), script, m, r.v0)
        K.assert_same_factorisation(r, result)


@pytest.mark.parametrize("n,m", [(257, 44), (1000, 65)])
def test_the_honest_arnoldi_stand_in_meets_every_bound_where_the_correction_loop_runs(n, m):
    r, _ = run(n, m, False, forced=True)
    K.check_arnoldi(r, MODEL).assert_ok(f"arnoldi, forced corrections, {n} x {m}")


@pytest.mark.parametrize("n,m", LANCZOS_SHAPES)
def test_the_honest_lanczos_stand_in_meets_every_bound(n, m):
    r, _ = run(n, m, True)
    K.check_lanczos(r, MODEL).assert_ok(f"lanczos {n} x {m}")


@pytest.mark.parametrize("n,m,p", [(1000, 64, 1), (1000, 64, 33), (1000, 64, 64), (1000, 129, 65), (1000, 257, 1), (100_003, 64, 17)])
def test_the_honest_stand_in_meets_the_product_bounds(n, m, p):
    r, fac = run(n, m, False)
    out = K.Ratios()
    K.check_ritz(fac, r.V, p, MODEL, out)
    K.check_compress(fac, r.V, r.fs[-1], min(p, m - 1), MODEL, out)
    out.assert_ok(f"V*Q {n} x {m}, p = {p}")


# every defect, at the smallest shape that has the branch it lives in, must exceed the bound of the check aimed at it 100 times —
# with the HIP model's (smaller) k the margin is larger still
@pytest.mark.parametrize("symmetric,keys", [(False, ("h",)), (True, ("r", "alpha", "subd"))])
@pytest.mark.parametrize("defect,n,m", [("dot_last_row", 129, 9), ("dot_last_row", 4099, 44), ("dot_last_row", 131_075, 16),
                                        ("dot_last_tile", 129, 9), ("dot_last_tile", 4099, 44), ("dot_last_tile", 131_075, 16)])
def test_a_dot_product_that_drops_rows_is_seen(symmetric, keys, defect, n, m):
    r, _ = run(n, m, symmetric, defect)
    out = (K.check_lanczos if symmetric else K.check_arnoldi)(r, MODEL)
    seen = max(out[k][0] for k in keys if k in out)
    print(defect, n, m, {k: out[k] for k in out})
    assert seen >= 100.0, (defect, seen)


@pytest.mark.parametrize("symmetric,keys", [(False, ("inv", "inv64")), (True, ("r", "r64"))])
@pytest.mark.parametrize("defect,n,m", [("sub_skip_col", 129, 9), ("sub_skip_col", 4099, 44), ("sub_skip_col", 131_075, 16),
                                        ("panel_coeffs", 1000, 65), ("panel_coeffs", 1000, 129)])
def test_a_subtraction_with_a_wrong_coefficient_is_seen(symmetric, keys, defect, n, m):
    r, _ = run(n, m, symmetric, defect)
    out = (K.check_lanczos if symmetric else K.check_arnoldi)(r, MODEL)
    seen = max(out[k][0] for k in keys if k in out)
    print(defect, n, m, {k: out[k] for k in out})
    assert seen >= 100.0, (defect, seen)


@pytest.mark.parametrize("n,m,p", [(1000, 64, 1), (1000, 64, 33), (1000, 129, 65), (100_003, 64, 17)])
def test_a_zeroed_column_of_q_is_seen(n, m, p):
    r, _ = run(n, m, False)
    script = K.HostScript(r.W)
    fac = NumpyFactorization(script, m, False, "q_zero_col")
    K.collect(fac, script, m, r.v0, False)
    out = K.Ratios()
    K.check_ritz(fac, r.V, p, MODEL, out)
    assert out["ritz"][0] >= 100.0
    out = K.Ratios()
    K.check_compress(fac, r.V, r.fs[-1], min(p, m - 1), MODEL, out)
    assert out["compress"][0] >= 100.0


def test_the_roundings_counted_for_the_kernels():
    """The instantiations the sizes of tests/test_gpu_krylov_kernels.py reach on 256 CUs, from the launch code (HipModel)."""
    M = K.HipModel(256)
    assert [L["S"] for ncol in range(1, 65) for L in M.orth_launches(1000, ncol)] == [K.cdiv(c, 4) for c in range(1, 65)]
    assert M.orth_launches(1000, 40)[0]["R"] == 2 and M.orth_launches(1000, 41)[0]["R"] == 1
    assert [L["col0"] for L in M.orth_launches(1030, 257)] == [0, 64, 128, 192, 256]
    assert M.orth_launches(131_071, 8)[0]["kernel"] == "k_orth" and M.orth_launches(131_072, 8)[0]["kernel"] == "k_orth_dma"
    assert {M.orth_launches(131_075, c)[0]["S"] for c in range(1, 65)} == {2, 4, 6, 8, 10, 12, 14, 16}
    assert {M.orth_launches(131_075, c)[0]["T"] for c in range(1, 65)} == {5}  # 1025 tiles on 256 workgroups: four or five each
    reg = K.HipModel(256, force_reg=True)
    assert reg.orth_launches(524_547, 40)[0]["T"] == 3 and reg.orth_launches(524_547, 41)[0]["T"] == 5
    assert M.k_dot(1000, 8) == 1 + 4 + 6 + 1 + 6 and M.k_upd(1000, 65) == (16 + 4) + (1 + 4)
