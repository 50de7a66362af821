"""spectra_amd — MI355X-native implicitly-restarted Lanczos eigensolver (drop-in for the Spectra hot path).

Python mirror of the reference's operator / solver interface for the path this repository implements
(yixuan/spectra v1.2.0, include/Spectra/): `SparseSymMatProd`, `SparseGenMatProd`, `SymEigsSolver`,
`SortRule`, `CompInfo` — same names, argument meaning and error behaviour — on top of the C ABI of
`libmispec.so` (include/mispec.h, HIP kernels for gfx950).  The C++ users' entry point is the header-only
API in include/Spectra/; this module exists for tests, the benchmark and Python callers.

There is NO CPU fallback: constructing a `Context` without a visible HIP device raises.
"""
import ctypes as C
import enum
import os

import numpy as np

from . import _capi
from ._capi import MispecError, Profile, build_library, check, lib

__all__ = ["SortRule", "CompInfo", "Context", "SparseSymMatProd", "SparseGenMatProd", "SparseSymShiftSolve", "SymEigsSolver",
           "SymEigsShiftSolver", "GenEigsSolver", "SVDMatOp", "PartialSVDSolver", "SparseRegularInverse", "SparseCholesky", "SymGEigsSolver", "SymShiftInvert", "SymGEigsShiftSolver", "SparseGenRealShiftSolve", "GenEigsRealShiftSolver", "shard_block",
           "Factorization", "tridiag_qr", "tridiag_eigen", "hess_qr", "double_shift_qr", "hess_schur", "hess_eigen", "MispecError", "build_library", "shard_range", "BAND_OFFSETS", "SYNTH_SEED",
           "SparseHermMatProd", "DenseHermMatProd", "HermEigsSolver", "spmm_plan", "shift_block_plan", "dia_sym_plan", "mirror_triangle_device",
           "LOBPCGSolver", "LOBPCGInfo", "lobpcg_gram", "lobpcg_resid", "lobpcg_block_sub", "shift_solver_path",
           "general_shift_solver_path", "general_complex_shift_solver_path"]

BAND_OFFSETS = (1, 2, 3, 1000, 1001, 100000, 100001)  # SURVEY.md §8(d) "M-band": 15 nnz/row with the diagonal
SYNTH_SEED = 20240607


# include/mispec.h MISPEC_ORTH_*: the reference's control flow, or the opt-in one-sweep steps; "onesweep-eager" applies the
# last correction of every sweep at once instead of letting it ride on the restart's V*Q pass, "onesweep-recorrect" is the test
# hook that lets one more correction follow every such fused restart
# "onesweep-restart-check" is the test hook of the restart without a host turn: its device-side test always reports a failure
# "onesweep-onered" / "onesweep-twored": one reduction per lagged step (include/mispec.h MISPEC_ORTH_ONE_REDUCTION) or the separate
# alpha reduction, whatever the library default is
# "onesweep-wide" (opt-in, MISPEC_ORTH_WIDE): the one-sweep steps on bases of 129 to 512 columns too, in column panels from step 128 on
ORTH_MODES = {"reference": 0, "onesweep": 1, "onesweep-eager": 1 | 0x100, "onesweep-recorrect": 1 | 0x200, "onesweep-restart-check": 1 | 0x400,
              "onesweep-onered": 1 | 0x800, "onesweep-twored": 1 | 0x1000, "onesweep-onered-eager": 1 | 0x800 | 0x100,
              "onesweep-wide": 1 | 0x2000, "onesweep-wide-onered": 1 | 0x2000 | 0x800, "onesweep-wide-twored": 1 | 0x2000 | 0x1000}


def _orth_mode_value(mode):
    """Name or integer of an orthogonalisation mode -> the integer of include/mispec.h; anything else is a ValueError that
    lists the names."""
    if isinstance(mode, str):
        if mode not in ORTH_MODES:
            raise ValueError("unknown orthogonalisation mode %r: one of %s" % (mode, ", ".join(sorted(ORTH_MODES))))
        return ORTH_MODES[mode]
    if isinstance(mode, int) and mode in ORTH_MODES.values():
        return mode
    raise ValueError("unknown orthogonalisation mode %r: one of %s" % (mode, ", ".join(sorted(ORTH_MODES))))



class SortRule(enum.IntEnum):
    """Util/SelectionRule.h:33-58 (same order as the C++ enum)."""
    LargestMagn = 0
    LargestReal = 1
    LargestImag = 2
    LargestAlge = 3
    SmallestMagn = 4
    SmallestReal = 5
    SmallestImag = 6
    SmallestAlge = 7
    BothEnds = 8


class CompInfo(enum.IntEnum):
    """Util/CompInfo.h:17-32."""
    Successful = 0
    NotComputed = 1
    NotConverging = 2
    NumericalIssue = 3


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None


def tiles_spmv_host(mat, x):
    """y = A x through the HOST image of the column-blocked tile format, in the kernel's summation order (mispec_tiles_spmv_host;
    no device needed).  mat: scipy CSR with sorted rows.  Returns (y or None when the format does not apply, stats dict)."""
    rp, ci, v = _i32(mat.indptr), _i32(mat.indices), _f64(mat.data)
    x = _f64(x)
    y = np.zeros(mat.shape[0])
    built = C.c_int(0)
    st = (C.c_int64 * 3)()
    check(lib().mispec_tiles_spmv_host(mat.shape[0], mat.shape[1], _ip(rp), _ip(ci), _dp(v), _dp(x), _dp(y), C.byref(built), st))
    return (y if built.value else None), {"entries": st[0], "padding": st[1], "chunks": st[2]}


def windows_host(mat, row_begin=0):
    """The x-window table of a CSR matrix (scipy, sorted rows) built on the HOST by the code the device builder runs
    (mispec_csr_windows_host; no device needed): (blocks x 32) int32, see include/mispec.h mispec_csr_windows_table."""
    rp, ci = _i32(mat.indptr), _i32(mat.indices)
    out = np.zeros(((mat.shape[0] + 255) // 256, 32), dtype=np.int32)
    check(lib().mispec_csr_windows_host(mat.shape[0], mat.shape[1], int(row_begin), _ip(rp), _ip(ci), _ip(out)))
    return out


def staged_spmv_host(mat, x):
    """y = A x through the HOST image of the staged format, in the order of its two kernels (mispec_staged_spmv_host; no device
    needed).  mat: scipy CSR with sorted rows.  Returns (y or None when the format does not apply, stats dict)."""
    rp, ci, v = _i32(mat.indptr), _i32(mat.indices), _f64(mat.data)
    x = _f64(x)
    y = np.zeros(mat.shape[0])
    built = C.c_int(0)
    st = (C.c_int64 * 5)()
    check(lib().mispec_staged_spmv_host(mat.shape[0], mat.shape[1], _ip(rp), _ip(ci), _dp(v), _dp(x), _dp(y), C.byref(built), st))
    return (y if built.value else None), {"bins": st[0], "slots": st[1], "batches": st[2], "chunks": st[3], "max_rounds": st[4],
                                          "well_filled": built.value == 1}


def last_ingest_info():
    """Seconds the host stages of the last matrix ingest on this thread took (mispec_last_ingest_info)."""
    out = np.zeros(10)
    check(lib().mispec_last_ingest_info(_dp(out), 10))
    keys = ("total", "mirror_triangle", "validate", "index_formats_and_h2d", "far_statistics_and_reordering", "tiles_build", "tiles_upload",
            "unused", "staged_build", "staged_upload")
    d = dict(zip(keys, out.tolist()))
    d.pop("unused")
    return d


def mirror_triangle_host(mat, uplo="L"):
    """The full symmetric CSR matrix that mispec_csr_from_triangle derives from the `uplo` triangle of a compressed scipy matrix
    (CSC or CSR; the other triangle is ignored) — host only, no device needed (mispec_mirror_triangle_host)."""
    import scipy.sparse as sp

    n, nc, outer, inner, val, row_major = _compressed(mat)
    cap = 2 * len(val) + 1
    rp = np.zeros(n + 1, dtype=np.int32)
    ci = np.zeros(cap, dtype=np.int32)
    v = np.zeros(cap)
    nnz = C.c_int64(0)
    check(lib().mispec_mirror_triangle_host(n, _ip(outer), _ip(inner), _dp(val), uplo.encode()[0:1], int(row_major), _ip(rp), _ip(ci), _dp(v),
                                           cap, C.byref(nnz)))
    return sp.csr_matrix((v[:nnz.value], ci[:nnz.value], rp), shape=(n, n))


def rcm_order(rowptr, colind, symmetric_pattern=True):
    """Reverse Cuthill-McKee ordering of an n x n CSR pattern on the host (mispec_rcm_order; no device needed).
    Returns (perm with perm[new] = old, gave_up, widest_level)."""
    rp, ci = _i32(rowptr), _i32(colind)
    n = len(rp) - 1
    perm = np.empty(n, dtype=np.int32)
    gave_up, widest = C.c_int(0), C.c_int64(0)
    check(lib().mispec_rcm_order(n, _ip(rp), _ip(ci), int(symmetric_pattern), _ip(perm), C.byref(gave_up), C.byref(widest)))
    return perm, bool(gave_up.value), int(widest.value)


def shard_block(n, world):
    """Rows per rank of the equal-block row partition (mispec_shard_block)."""
    return int(lib().mispec_shard_block(n, world))


def shard_range(n, world, rank):
    """Rows [begin, end) owned by `rank` (equal even-sized blocks, see mispec_shard_range)."""
    b, e = C.c_int64(), C.c_int64()
    check(lib().mispec_shard_range(n, world, rank, C.byref(b), C.byref(e)))
    return b.value, e.value


class Context:
    """One device + one HIP stream (+ the communicator of a row-sharded run)."""

    def __init__(self, device=0, stream=None):
        h = C.c_void_p()
        check(lib().mispec_ctx_create(int(device), C.c_void_p(stream) if stream else None, C.byref(h)))
        self.h = h
        self.device = int(device)
        self.rank, self.world = 0, 1
        self._keep = []

    def sync(self):
        check(lib().mispec_ctx_sync(self.h))

    @property
    def stream(self):
        return lib().mispec_ctx_stream(self.h)

    def set_comm_rccl(self, rank, world, unique_id):
        check(lib().mispec_ctx_set_comm_rccl(self.h, rank, world, unique_id))
        self.rank, self.world = rank, world

    def set_comm_callbacks(self, rank, world, allgather, allreduce_sum, exchange=None):
        """allgather(send_ptr, recv_ptr, count_per_rank, stream) / allreduce_sum(buf_ptr, count, stream) -> 0 on success;
        optional exchange(send_ptr, send_off[], send_count[], recv_ptr, recv_off[], recv_count[], stream) (mispec_comm.exchange)."""
        ag = _capi.allgather_fn(lambda user, s, r, cnt, st: int(allgather(s, r, cnt, st) or 0))
        ar = _capi.allreduce_fn(lambda user, b, cnt, st: int(allreduce_sum(b, cnt, st) or 0))
        comm = _capi.Comm(rank, world, ag, ar, None)
        if exchange is not None:
            def ex_tramp(user, s, so, sc, r, ro, rc, st):
                lst = lambda a: [int(a[i]) for i in range(world)]
                return int(exchange(int(s or 0), lst(so), lst(sc), int(r or 0), lst(ro), lst(rc), st) or 0)
            ex = _capi.exchange_fn(ex_tramp)
            comm.exchange = ex
            self._keep.append(ex)
        self._keep += [ag, ar, comm]
        check(lib().mispec_ctx_set_comm(self.h, C.byref(comm)))
        self.rank, self.world = rank, world

    @staticmethod
    def rccl_unique_id():
        buf = C.create_string_buffer(128)
        check(lib().mispec_rccl_unique_id(buf))
        return buf.raw

    def __del__(self):
        try:
            lib().mispec_ctx_destroy(self.h)
        except Exception:
            pass


_default_ctx = None


def set_option(name, value=None):
    """mispec_set_option: a tuning switch / test hook by name (include/mispec.h lists them); value None restores the default."""
    check(lib().mispec_set_option(name.encode(), None if value is None else str(value).encode()))


def get_option(name):
    v = lib().mispec_get_option(name.encode())
    return None if v is None else v.decode()


def spmm_plan(k, panel=0):
    """The panel widths a block product of k columns runs, in order (mispec_spmm_plan; host only): each 8, 4, 2 or 1.
    panel: 0 what option `spmm` says, 1 single columns only, 2 | 4 | 8 the widest panel."""
    cap = max(int(k), 1)
    out = (C.c_int * cap)()
    count = C.c_int(0)
    check(lib().mispec_spmm_plan(int(k), int(panel), out, cap, C.byref(count)))
    return [out[i] for i in range(count.value)]


def shift_block_plan(k, panel=0):
    """The panel widths a block shift solve of k columns runs, in order (mispec_symshift_block_plan; host only): each 4, 2 or 1.
    panel: 0 what option `shift_block` says, 1 single columns only, 2 | 4 the widest panel."""
    cap = max(int(k), 1)
    out = (C.c_int * cap)()
    count = C.c_int(0)
    check(lib().mispec_symshift_block_plan(int(k), int(panel), out, cap, C.byref(count)))
    return [out[i] for i in range(count.value)]


class _ShiftBlock:
    """Block solves of the shift-and-invert operators (mispec_symshift_solve_block): k right-hand sides, panels of 4 and 2 columns
    per pass over the factor, every column with the bits of perform_op on it alone."""

    def perform_op_block(self, X_in):
        X = np.asfortranarray(X_in, dtype=np.float64)
        if X.ndim != 2 or X.shape[0] != self.n:
            raise ValueError("perform_op_block: X must be an n x k array")
        Y = np.empty(X.shape, order="F")
        check(lib().mispec_symshift_solve_block_host(self.h, _dp(X), max(self.n, 1), X.shape[1], _dp(Y), max(self.n, 1)))
        return Y

    def solve_block_device(self, x_ptr, ldx, k, y_ptr, ldy):
        """Y[:, :k] = (A - sigma B)^{-1} X[:, :k] on device pointers (column-major, ldx, ldy >= n), enqueued on the context's stream."""
        check(lib().mispec_symshift_solve_block(self.h, C.c_void_p(int(x_ptr)), int(ldx), int(k), C.c_void_p(int(y_ptr)), int(ldy)))

    def path_info(self):
        """{path, block_rows, blocks, factor_bytes} (mispec_symshift_path_info): path 0 = explicit inverse, 1 = chunk path, 2 = the
        block-tridiagonal path with its block layout and the bytes of its factor (zeros on the other paths), 3 = the iterative path,
        -1 = unsupported."""
        p, s, nb, fb = C.c_int(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib().mispec_symshift_path_info(self.h, C.byref(p), C.byref(s), C.byref(nb), C.byref(fb)))
        return {"path": p.value, "block_rows": s.value, "blocks": nb.value, "factor_bytes": fb.value}

    def refinement_info(self):
        """Banded path: {refine_steps, boosted_pivots, min_pivot_ratio, probe_backward_error} of the last set_shift()."""
        st, bo, mr, om = C.c_int(0), C.c_int64(0), C.c_double(0.0), C.c_double(0.0)
        check(lib().mispec_symshift_refinement_info(self.h, C.byref(st), C.byref(bo), C.byref(mr), C.byref(om)))
        return {"refine_steps": st.value, "boosted_pivots": bo.value, "min_pivot_ratio": mr.value, "probe_backward_error": om.value}

    def set_iterative(self, tol=0.0, max_iterations=0):
        """Iterative path: tolerance on a solve's backward error and iteration cap per solve; a value <= 0 restores the default
        (4e-15, 20000).  mispec_symshift_set_iterative.  An iteration is one product on a symmetric operator (MINRES), two on a
        general one (BiCGStab)."""
        check(lib().mispec_symshift_set_iterative(self.h, float(tol), int(max_iterations)))

    def iterative_info(self):
        """Iterative path: {last_iterations, total_iterations, solves, last_passes, last_backward_error, probe_iterations}
        (mispec_symshift_iterative_info); zeros on a direct path."""
        li, ti, so, pi = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        lp, om = C.c_int(0), C.c_double(0.0)
        check(lib().mispec_symshift_iterative_info(self.h, C.byref(li), C.byref(ti), C.byref(so), C.byref(lp), C.byref(om), C.byref(pi)))
        return {"last_iterations": li.value, "total_iterations": ti.value, "solves": so.value, "last_passes": lp.value,
                "last_backward_error": om.value, "probe_iterations": pi.value}


SHIFT_SOLVERS = {"direct": 0, "auto": 1, "iterative": 2}


def _shift_solver_kind(solver):
    """None (what option shift_solver says) or one of direct | auto | iterative -> the solver kind of include/mispec.h."""
    if solver is None:
        return -1
    if solver not in SHIFT_SOLVERS:
        raise ValueError("unknown shift solver %r: one of %s" % (solver, ", ".join(SHIFT_SOLVERS)))
    return SHIFT_SOLVERS[solver]


def shift_solver_path(n, half_bandwidth, solver=None):
    """The path a shift-and-invert operator of this size and half-bandwidth takes under a solver kind (mispec_symshift_solver_path;
    host only): 0 inverse, 1 chunk, 2 block-tridiagonal, 3 iterative; ValueError where construction would refuse."""
    rc = lib().mispec_symshift_solver_path(int(n), int(half_bandwidth), _shift_solver_kind(solver))
    if rc < 0:
        check(rc)
    return rc


def general_shift_solver_path(n, solver=None):
    """The path a general (non-symmetric) shift-and-invert operator of this size takes under a solver kind
    (mispec_symshift_general_solver_path; host only): 0 inverse, 3 iterative; ValueError where construction would refuse."""
    rc = lib().mispec_symshift_general_solver_path(int(n), _shift_solver_kind(solver))
    if rc < 0:
        check(rc)
    return rc


def general_complex_shift_solver_path(n, solver):
    """The path SparseGenComplexShiftSolve(complex_solver=solver) takes at this size (mispec_symshift_general_complex_solver_path;
    host only): 0 inverse, 3 iterative (BiCGStab in complex arithmetic); ValueError where construction would refuse.  solver is
    one of direct | auto | iterative: option shift_solver is not read."""
    if solver is None:
        raise ValueError("unknown shift solver None: one of %s" % ", ".join(SHIFT_SOLVERS))
    rc = lib().mispec_symshift_general_complex_solver_path(int(n), _shift_solver_kind(solver))
    if rc < 0:
        check(rc)
    return rc


def dia_sym_plan(offsets, reach=-1):
    """The rule of option `dia_sym` (mispec_dia_sym_plan; host only): for the diagonal offsets given, (flags, lead_blocks) —
    flags[i] is True where diagonal i = -k may be mirrored (+k present, k <= reach; reach < 0: no limit), lead_blocks =
    ceil(largest such k / 256).  The ingest keeps, of these, the diagonals whose bits equal their partner's."""
    offs = np.ascontiguousarray(offsets, dtype=np.int32)
    flags = np.zeros(offs.size, dtype=np.int32)
    lead = C.c_int(0)
    check(lib().mispec_dia_sym_plan(_ip(offs), int(offs.size), int(reach), _ip(flags), C.byref(lead)))
    return [bool(f) for f in flags], lead.value


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class _DeviceMatrix:
    """A CSR row shard in HBM (mispec_csr)."""

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self.h = handle

    def rows(self):
        return lib().mispec_csr_rows(self.h)

    def cols(self):
        return lib().mispec_csr_cols(self.h)

    def local_rows(self):
        return lib().mispec_csr_local_rows(self.h)

    def nnz(self):
        return lib().mispec_csr_local_nnz(self.h)

    def perform_op(self, x_in, y_out=None):
        """y_out = A * x_in with HOST arrays (the reference's perform_op contract)."""
        x = _f64(x_in)
        if x.shape != (self.cols(),):
            raise ValueError("perform_op: x_in must have cols() entries")
        y = np.empty(self.rows()) if y_out is None else y_out
        check(lib().mispec_spmv_host(self.h, _dp(x), _dp(y)))
        return y

    def __matmul__(self, X):
        """operator*: A @ X for a dense block (SparseSymMatProd.h:93-96)."""
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            return self.perform_op(X)
        Xf = np.asfortranarray(X)
        Y = np.empty((self.rows(), X.shape[1]), order="F")
        check(lib().mispec_spmm_host(self.h, _dp(Xf), Xf.shape[0], X.shape[1], _dp(Y), Y.shape[0]))
        return Y

    def __call__(self, i, j):
        """operator()(i, j): coefficient of the (mirrored) operator."""
        v = C.c_double()
        check(lib().mispec_csr_coeff(self.h, int(i), int(j), C.byref(v)))
        return v.value

    def spmv_device(self, x_ptr, y_ptr):
        """y = A x with raw DEVICE pointers (x: cols() doubles, y: local_rows())."""
        check(lib().mispec_spmv(self.h, C.c_void_p(x_ptr), C.c_void_p(y_ptr)))

    def spmv_time(self, x_ptr, y_ptr, reps):
        ms = C.c_float()
        check(lib().mispec_spmv_time(self.h, C.c_void_p(x_ptr), C.c_void_p(y_ptr), reps, C.byref(ms)))
        return ms.value

    def spmm_device(self, x_ptr, ldx, k, y_ptr, ldy):
        """Y[:, :k] = A X[:, :k] with raw DEVICE pointers to column-major blocks (ldx >= cols(), ldy >= rows(); X and Y must not
        overlap), enqueued on the context's stream: mispec_spmm, bit-identical to k spmv_device calls."""
        check(lib().mispec_spmm(self.h, C.c_void_p(x_ptr), int(ldx), int(k), C.c_void_p(y_ptr), int(ldy)))

    def spmm_time(self, x_ptr, ldx, k, y_ptr, ldy, reps):
        ms = C.c_float()
        check(lib().mispec_spmm_time(self.h, C.c_void_p(x_ptr), int(ldx), int(k), C.c_void_p(y_ptr), int(ldy), int(reps), C.byref(ms)))
        return ms.value

    def algorithmic_bytes(self):
        return 12.0 * self.nnz() + 4.0 * (self.local_rows() + 1) + 8.0 * self.cols() + 8.0 * self.local_rows()

    def offset_codes(self):
        """0: the SpMV reads int32 column indices; d > 0: one-byte codes into a dictionary of d diagonals."""
        return int(lib().mispec_csr_offset_codes(self.h))

    def use_offset_codes(self, enable=True):
        check(lib().mispec_csr_use_offset_codes(self.h, 1 if enable else 0))

    def use_windows(self, enable=True):
        """Per-matrix switch of the int32 CSR kernel: x staged through LDS windows (True) or gathered entry by entry (False);
        None: automatic (windows when the table was adopted at ingest and the rows hold at least 9 entries on average)."""
        check(lib().mispec_csr_use_windows(self.h, -1 if enable is None else (1 if enable else 0)))

    def windows_info(self):
        """{blocks, covered_entries, lds_doubles} of the x windows of the int32 CSR kernel (lds_doubles = 0: not adopted)."""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib().mispec_csr_windows_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"blocks": a.value, "covered_entries": b.value, "lds_doubles": c.value}

    def dia_info(self):
        """{ndia, nstored, nmirrored, lead_blocks} of the diagonal storage (mispec_csr_dia_info; all 0: not built): nmirrored of the
        ndia diagonals are read from their partner +k instead of being stored (option dia_sym)."""
        a, b, c, d = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().mispec_csr_dia_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return {"ndia": a.value, "nstored": b.value, "nmirrored": c.value, "lead_blocks": d.value}

    def windows_in_use(self):
        """True when format 0 of this matrix runs the kernel with x windows (per-matrix switch and automatic rule applied)."""
        return bool(lib().mispec_csr_windows_in_use(self.h))

    def windows_table(self):
        """The per-block window records (blocks x 32 int32; include/mispec.h mispec_csr_windows_table)."""
        nb = (self.local_rows() + 255) // 256
        out = np.empty((nb, 32), dtype=np.int32)
        check(lib().mispec_csr_windows_table(self.h, _ip(out), out.size))
        return out

    def spmv_format(self):
        """0: CSR with int32 column indices, 1: CSR with offset codes, 2: diagonal storage — what the SpMV uses."""
        return int(lib().mispec_csr_spmv_format(self.h))

    def set_spmv_format(self, fmt=-1):
        """Force a storage format for this matrix (-1: automatic); all formats give bit-identical products."""
        check(lib().mispec_csr_set_spmv_format(self.h, int(fmt)))

    def stored_bytes(self):
        """Compulsory SpMV traffic with the index format in use (9 instead of 12 bytes per entry with offset codes)."""
        return float(lib().mispec_csr_spmv_bytes(self.h, 1))

    def staged_info(self):
        """{bins, slots, batches, chunks} of the staged format (two streaming phases with x and y in LDS; bins = 0: not built)."""
        a, b, c, d = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib().mispec_csr_staged_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return {"bins": a.value, "slots": b.value, "batches": c.value, "chunks": d.value}

    def tiles_info(self):
        """{segments, entries, padding, chunks} of the column-blocked tile format (segments = 0: not built)."""
        a, b, c, d = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib().mispec_csr_tiles_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return {"segments": a.value, "entries": b.value, "padding": c.value, "chunks": d.value}

    def reorder(self, method="rcm"):
        """Symmetric reordering of the stored matrix (mispec_csr_reorder): "rcm" always, "auto" only when it pays.  Returns
        True when the matrix is reordered afterwards.  Products and results keep the caller's index order."""
        applied = C.c_int(0)
        check(lib().mispec_csr_reorder(self.h, {"rcm": 1, "auto": -1}[method], C.byref(applied)))
        return bool(applied.value)

    def reordering(self):
        """"none" or "rcm"."""
        return {0: "none", 1: "rcm"}[int(lib().mispec_csr_reordering(self.h, None, None))]

    def reordering_info(self):
        fb, fa = C.c_double(0.0), C.c_double(0.0)
        m = int(lib().mispec_csr_reordering(self.h, C.byref(fb), C.byref(fa)))
        return {"method": {0: "none", 1: "rcm"}[m], "far_fraction_before": fb.value, "far_fraction_after": fa.value}

    def permutation(self):
        """perm[new] = old (identity when the matrix is not reordered)."""
        out = np.empty(self.rows(), dtype=np.int32)
        check(lib().mispec_csr_permutation(self.h, _ip(out)))
        return out

    def to_host_csr(self):
        nl, nnz = self.local_rows(), self.nnz()
        rp = np.empty(nl + 1, dtype=np.int32)
        ci = np.empty(nnz, dtype=np.int32)
        v = np.empty(nnz)
        check(lib().mispec_csr_download(self.h, _ip(rp), _ip(ci), _dp(v)))
        return rp, ci, v

    def __del__(self):
        try:
            lib().mispec_csr_destroy(self.h)
        except Exception:
            pass


def _compressed(mat):
    """(rows, cols, outer, inner, values, row_major) of a scipy.sparse CSR/CSC matrix."""
    fmt = getattr(mat, "format", None)
    if fmt not in ("csr", "csc"):
        raise TypeError("expected a scipy.sparse csr_matrix or csc_matrix (compressed storage)")
    m = mat
    if not mat.has_canonical_format:  # unsorted inner indices or duplicates: canonicalise a copy, never the caller's matrix
        m = mat.copy()
        m.sum_duplicates()
        m.sort_indices()
    # a canonical matrix is handed over as it is (the copy was 0.15 s of single-threaded memcpy per GB at n = 1e7)
    return m.shape[0], m.shape[1], _i32(m.indptr), _i32(m.indices), _f64(m.data), fmt == "csr"


class _reorder_env:
    """reorder=None keeps the library default (MISPEC_REORDER or "auto"); "none" / "rcm" / "auto" override it for one ingest."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.old = os.environ.get("MISPEC_REORDER")
        if self.mode is not None:
            if self.mode not in ("none", "rcm", "auto"):
                raise ValueError("reorder must be None, 'none', 'rcm' or 'auto'")
            os.environ["MISPEC_REORDER"] = self.mode

    def __exit__(self, *exc):
        if self.mode is not None:
            if self.old is None:
                os.environ.pop("MISPEC_REORDER", None)
            else:
                os.environ["MISPEC_REORDER"] = self.old


_TORCH_ACCEPTED = ("a 2-D torch.sparse_csr or torch.sparse_csc tensor on the context's GPU with int32 or int64 indices and float64 "
                   "(or float32, widened) values")


def _torch_compressed(t, ctx):
    """(rows, cols, outer, inner, values, row_major, ctx) of a torch sparse_csr / sparse_csc tensor in device memory: the three
    component tensors (contiguous, values as float64), which the caller keeps alive over the library call.  Anything else is
    refused before a library call is made; torch is imported here only."""
    import torch

    if not isinstance(t, torch.Tensor):
        raise TypeError("expected %s, got %s" % (_TORCH_ACCEPTED, type(t).__name__))
    if t.layout not in (torch.sparse_csr, torch.sparse_csc):
        raise ValueError("expected %s, got layout %s" % (_TORCH_ACCEPTED, t.layout))
    if not t.is_cuda:
        raise ValueError("expected %s, got a tensor on %s (the host constructors take scipy matrices)" % (_TORCH_ACCEPTED, t.device))
    if t.dim() != 2:
        raise ValueError("expected %s, got a batched tensor of %d dimensions" % (_TORCH_ACCEPTED, t.dim()))
    ctx = ctx or default_context()
    if t.device.index != ctx.device:
        raise ValueError("expected %s, got a tensor on %s while the context is on device %d" % (_TORCH_ACCEPTED, t.device, ctx.device))
    row_major = t.layout == torch.sparse_csr
    outer, inner = (t.crow_indices(), t.col_indices()) if row_major else (t.ccol_indices(), t.row_indices())
    val = t.values()
    if val.dtype == torch.float32:
        val = val.to(torch.float64)
    if val.dtype != torch.float64 or outer.dtype not in (torch.int32, torch.int64) or inner.dtype != outer.dtype:
        raise ValueError("expected %s, got values %s and indices %s / %s" % (_TORCH_ACCEPTED, val.dtype, outer.dtype, inner.dtype))
    outer, inner, val = outer.contiguous(), inner.contiguous(), val.contiguous()
    if val.numel() == 0:  # empty tensors have no address; the library wants one (it reads no entry)
        inner = torch.zeros(1, dtype=outer.dtype, device=t.device)
        val = torch.zeros(1, dtype=torch.float64, device=t.device)
    torch.cuda.current_stream(t.device).synchronize()  # the library reads on the context's stream
    return t.shape[0], t.shape[1], outer, inner, val, row_major, ctx


def _from_device(cls, ctx, reorder, call):
    h = C.c_void_p()
    with _reorder_env(reorder):
        check(call(C.byref(h)))
    obj = cls.__new__(cls)
    _DeviceMatrix.__init__(obj, ctx, h)
    return obj


def mirror_triangle_device(t, uplo="L", ctx=None):
    """The full symmetric CSR matrix of the `uplo` triangle of a torch sparse_csr / sparse_csc tensor on the GPU, mirrored by
    the device kernels (mispec_mirror_triangle_device): (rowptr, colind, val) as numpy arrays.  Test hook: equal to
    mirror_triangle_host byte for byte."""
    import torch

    n, nc, outer, inner, val, row_major, ctx = _torch_compressed(t, ctx)
    if n != nc:
        raise ValueError("mirror_triangle_device: matrix must be square")
    cap = 2 * int(t.values().numel()) + 1
    rp = torch.zeros(n + 1, dtype=torch.int32, device=t.device)
    ci = torch.zeros(cap, dtype=torch.int32, device=t.device)
    v = torch.zeros(cap, dtype=torch.float64, device=t.device)
    torch.cuda.current_stream(t.device).synchronize()
    nnz = C.c_int64(0)
    check(lib().mispec_mirror_triangle_device(ctx.h, n, outer.data_ptr(), inner.data_ptr(), outer.element_size(), val.data_ptr(),
                                             uplo.encode()[0:1], int(row_major), rp.data_ptr(), ci.data_ptr(), v.data_ptr(), cap,
                                             C.byref(nnz)))
    return rp.cpu().numpy(), ci[:nnz.value].cpu().numpy(), v[:nnz.value].cpu().numpy()


class SparseSymMatProd(_DeviceMatrix):
    """MatOp/SparseSymMatProd.h: y = selfadjointView<Uplo>(A) * x; only the `uplo` triangle of A is read."""

    def __init__(self, mat, uplo="L", ctx=None, reorder=None):
        ctx = ctx or default_context()
        n, nc, outer, inner, val, row_major = _compressed(mat)
        if n != nc:
            raise ValueError("SparseSymMatProd: matrix must be square")
        h = C.c_void_p()
        with _reorder_env(reorder):
            check(lib().mispec_csr_from_triangle(ctx.h, n, _ip(outer), _ip(inner), _dp(val), uplo.encode()[0:1], int(row_major),
                                                 C.byref(h)))
        super().__init__(ctx, h)

    @classmethod
    def synth_band(cls, n, offsets=BAND_OFFSETS, seed=SYNTH_SEED, ctx=None):
        """The synthetic symmetric benchmark matrix of SURVEY.md §8(d), generated directly in HBM."""
        return _synth(cls, n, offsets, seed, True, ctx)

    @classmethod
    def from_torch(cls, t, uplo="L", ctx=None, reorder=None):
        """The operator of the `uplo` triangle of a torch.sparse_csr / sparse_csc tensor that lives on the context's GPU
        (int32 or int64 indices, float64 or widened float32 values), built on the device: nothing is copied to the host unless
        the pattern needs a host-built structure (reordering, staged image, tiles).  The tensor is copied; it may be freed or
        overwritten afterwards.  Equal to SparseSymMatProd(scipy matrix of the same arrays) bit for bit."""
        n, nc, outer, inner, val, row_major, ctx = _torch_compressed(t, ctx)
        if n != nc:
            raise ValueError("SparseSymMatProd: matrix must be square")
        return cls.from_device_pointers(n, outer.data_ptr(), inner.data_ptr(), outer.element_size(), val.data_ptr(), row_major,
                                        uplo=uplo, ctx=ctx, reorder=reorder)

    @classmethod
    def from_device_pointers(cls, n, outer_ptr, inner_ptr, index_bytes, val_ptr, row_major, uplo="L", ctx=None, reorder=None):
        """from_torch for callers without torch: raw DEVICE addresses of outer (n + 1 indices), inner and the float64 values of
        one triangle, index_bytes = 4 or 8 (mispec_csr_from_triangle_device; the caller has finished writing them)."""
        ctx = ctx or default_context()
        return _from_device(cls, ctx, reorder, lambda out: lib().mispec_csr_from_triangle_device(
            ctx.h, int(n), C.c_void_p(outer_ptr), C.c_void_p(inner_ptr), int(index_bytes), C.c_void_p(val_ptr), uplo.encode()[0:1],
            int(bool(row_major)), out))


class SparseGenMatProd(_DeviceMatrix):
    """MatOp/SparseGenMatProd.h: y = A * x for a general sparse A (CSR or CSC input)."""

    def __init__(self, mat, ctx=None, reorder=None):
        ctx = ctx or default_context()
        nr, nc, outer, inner, val, row_major = _compressed(mat)
        h = C.c_void_p()
        fn = lib().mispec_csr_upload if row_major else lib().mispec_csr_from_csc
        with _reorder_env(reorder):
            check(fn(ctx.h, nr, nc, _ip(outer), _ip(inner), _dp(val), C.byref(h)))
        super().__init__(ctx, h)

    @classmethod
    def synth_band(cls, n, offsets=BAND_OFFSETS, seed=SYNTH_SEED, ctx=None):
        return _synth(cls, n, offsets, seed, False, ctx)

    @classmethod
    def from_torch(cls, t, ctx=None, reorder=None):
        """The operator of a general torch.sparse_csr (taken as it is) or sparse_csc (transposed on the device) tensor on the
        context's GPU; see SparseSymMatProd.from_torch.  Equal to SparseGenMatProd(scipy matrix of the same arrays)."""
        nr, nc, outer, inner, val, row_major, ctx = _torch_compressed(t, ctx)
        return cls.from_device_pointers(nr, nc, outer.data_ptr(), inner.data_ptr(), outer.element_size(), val.data_ptr(), row_major,
                                        ctx=ctx, reorder=reorder)

    @classmethod
    def from_device_pointers(cls, n_rows, n_cols, outer_ptr, inner_ptr, index_bytes, val_ptr, row_major, ctx=None, reorder=None):
        """Raw DEVICE addresses of a compressed general matrix (mispec_csr_from_device): CSR when row_major, else CSC."""
        ctx = ctx or default_context()
        return _from_device(cls, ctx, reorder, lambda out: lib().mispec_csr_from_device(
            ctx.h, int(n_rows), int(n_cols), C.c_void_p(outer_ptr), C.c_void_p(inner_ptr), int(index_bytes), C.c_void_p(val_ptr),
            int(bool(row_major)), out))


def _synth(cls, n, offsets, seed, symmetric, ctx):
    ctx = ctx or default_context()
    offs = np.ascontiguousarray(offsets, dtype=np.int64)
    h = C.c_void_p()
    check(lib().mispec_csr_synth_band(ctx.h, n, seed, offs.ctypes.data_as(C.POINTER(C.c_int64)), len(offs), int(symmetric),
                                      C.byref(h)))
    obj = cls.__new__(cls)
    _DeviceMatrix.__init__(obj, ctx, h)
    return obj


class SparseSymShiftSolve(_ShiftBlock):
    """MatOp/SparseSymShiftSolve.h: y = (A - sigma I)^{-1} x, solved on the GPU after set_shift(sigma).  solver: None (what option
    shift_solver says; its default is direct) | "direct" | "auto" | "iterative" (include/mispec.h mispec_symshift_create_solver)."""

    def __init__(self, mat, uplo="L", ctx=None, solver=None):
        self.ctx = ctx or default_context()
        n, nc, outer, inner, val, row_major = _compressed(mat)
        if n != nc:
            raise ValueError("SparseSymShiftSolve: matrix must be square")
        h = C.c_void_p()
        check(lib().mispec_symshift_create_solver(self.ctx.h, n, _ip(outer), _ip(inner), _dp(val), uplo.encode()[0:1], int(row_major),
                                                  _shift_solver_kind(solver), C.byref(h)))
        self.h = h
        self.n = n

    def rows(self):
        return self.n

    def cols(self):
        return self.n

    def local_rows(self):
        return self.n

    def set_shift(self, sigma):
        check(lib().mispec_symshift_set_shift(self.h, float(sigma)))

    def bandwidth_info(self):
        """{as_given, stored, reordered}: half-bandwidth of the matrix as it came and as it is stored (reverse Cuthill-McKee at
        construction when the band is too wide as given, include/mispec.h mispec_symshift_bandwidth)."""
        a, b, r = C.c_int64(0), C.c_int64(0), C.c_int(0)
        check(lib().mispec_symshift_bandwidth(self.h, C.byref(a), C.byref(b), C.byref(r)))
        return {"as_given": a.value, "stored": b.value, "reordered": bool(r.value)}

    def perform_op(self, x_in):
        x = _f64(x_in)
        if x.shape != (self.n,):
            raise ValueError("perform_op: x_in must have n entries")
        y = np.empty(self.n)
        check(lib().mispec_symshift_solve_host(self.h, _dp(x), _dp(y)))
        return y

    def solve_device(self, x_ptr, y_ptr):
        """y = (A - sigma I)^{-1} x on device pointers, enqueued on the context's stream (mispec_symshift_solve)."""
        check(lib().mispec_symshift_solve(self.h, C.c_void_p(int(x_ptr)), C.c_void_p(int(y_ptr))))

    def __del__(self):
        try:
            lib().mispec_symshift_destroy(self.h)
        except Exception:
            pass


class _DenseMatrix:
    """A dense matrix in HBM (mispec_dense), row-major there."""

    def __init__(self, mat, uplo, ctx):
        self.ctx = ctx or default_context()
        M = np.asarray(mat, dtype=np.float64)
        if M.ndim != 2:
            raise ValueError("dense operator: a 2-d array is expected")
        row_major = M.flags.c_contiguous and not M.flags.f_contiguous
        if not (M.flags.c_contiguous or M.flags.f_contiguous):
            M = np.asfortranarray(M)
        ld = M.shape[1] if row_major else M.shape[0]
        h = C.c_void_p()
        check(lib().mispec_dense_upload(self.ctx.h, M.shape[0], M.shape[1], _dp(M), max(int(ld), 1), int(row_major),
                                        uplo.encode()[0:1] if uplo else b"\0", C.byref(h)))
        self.h = h

    def rows(self):
        return lib().mispec_dense_rows(self.h)

    def cols(self):
        return lib().mispec_dense_cols(self.h)

    def local_rows(self):
        return self.rows()

    def perform_op(self, x_in, y_out=None):
        """y_out = A * x_in with HOST arrays (the reference's perform_op contract)."""
        x = _f64(x_in)
        if x.shape != (self.cols(),):
            raise ValueError("perform_op: x_in must have cols() entries")
        y = np.empty(self.rows()) if y_out is None else y_out
        check(lib().mispec_dense_gemv_host(self.h, _dp(x), _dp(y)))
        return y

    def __matmul__(self, X):
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            return self.perform_op(X)
        Xf = np.asfortranarray(X)
        Y = np.empty((self.rows(), X.shape[1]), order="F")
        check(lib().mispec_dense_gemm_host(self.h, _dp(Xf), Xf.shape[0], X.shape[1], _dp(Y), Y.shape[0]))
        return Y

    def __call__(self, i, j):
        v = C.c_double()
        check(lib().mispec_dense_coeff(self.h, int(i), int(j), C.byref(v)))
        return v.value

    def gemv_device(self, x_ptr, y_ptr):
        check(lib().mispec_dense_gemv(self.h, C.c_void_p(x_ptr), C.c_void_p(y_ptr)))

    def gemv_time(self, x_ptr, y_ptr, reps):
        ms = C.c_float()
        check(lib().mispec_dense_gemv_time(self.h, C.c_void_p(x_ptr), C.c_void_p(y_ptr), reps, C.byref(ms)))
        return ms.value

    def algorithmic_bytes(self):
        return 8.0 * self.rows() * self.cols() + 8.0 * self.cols() + 8.0 * self.rows()

    def __del__(self):
        try:
            lib().mispec_dense_destroy(self.h)
        except Exception:
            pass


class DenseSymMatProd(_DenseMatrix):
    """MatOp/DenseSymMatProd.h: y = A x for a symmetric dense A, reading only the `uplo` triangle of the input."""

    def __init__(self, mat, uplo="L", ctx=None):
        M = np.asarray(mat)
        if M.ndim != 2 or M.shape[0] != M.shape[1]:
            raise ValueError("DenseSymMatProd: matrix must be square")
        if uplo not in ("L", "U"):
            raise ValueError("DenseSymMatProd: uplo must be 'L' or 'U'")
        super().__init__(mat, uplo, ctx)


class DenseGenMatProd(_DenseMatrix):
    """MatOp/DenseGenMatProd.h: y = A x for a general dense A."""

    def __init__(self, mat, ctx=None):
        super().__init__(mat, None, ctx)


class DeviceOp:
    """A user operator on DEVICE pointers: fn(x_ptr, y_ptr, stream) must enqueue y = Op(x) (n doubles each) on the
    given HIP stream.  The perform_op concept of the reference with both vectors in HBM: nothing is staged."""

    def __init__(self, n, fn, ctx=None):
        self.ctx = ctx or default_context()
        self.n = int(n)
        self.fn = fn

        def tramp(user, x_ptr, y_ptr, stream):
            try:
                fn(int(x_ptr or 0), int(y_ptr or 0), int(stream or 0))
                return 0
            except Exception:  # noqa: BLE001 - reported through the return code
                return 1

        self.cb = _capi.device_op_fn(tramp)

    def rows(self):
        return self.n

    def cols(self):
        return self.n

    def local_rows(self):
        return self.n


class _UserOp:
    """Adapter for a Python operator with rows(), cols(), perform_op(x_in) -> y (host numpy arrays)."""

    def __init__(self, op):
        self.op = op
        n = op.rows()

        def tramp(user, x_ptr, y_ptr):
            try:
                x = np.ctypeslib.as_array(x_ptr, shape=(n,))
                y = np.ctypeslib.as_array(y_ptr, shape=(n,))
                y[:] = op.perform_op(x)
                return 0
            except Exception:  # noqa: BLE001 - reported through the return code
                return 1

        self.cb = _capi.op_fn(tramp)


class SparseCholesky:
    """MatOp/SparseCholesky.h: B = G G' (dense factor on the GPU for n <= 4096, the partitioned band factorisation for a
    larger banded B); lower_triangular_solve = G^{-1} x, upper_triangular_solve = G^{-T} x; info() like the reference
    (NumericalIssue when B is not positive definite)."""

    def __init__(self, mat, uplo="L", ctx=None):
        self.ctx = ctx or default_context()
        n, nc, outer, inner, val, row_major = _compressed(mat)
        if n != nc:
            raise ValueError("SparseCholesky: matrix must be square")
        h = C.c_void_p()
        check(lib().mispec_cholesky_create(self.ctx.h, n, _ip(outer), _ip(inner), _dp(val), uplo.encode()[0:1], int(row_major),
                                           C.byref(h)))
        self.h = h
        self.n = n

    def rows(self):
        return self.n

    cols = rows

    def info(self):
        return CompInfo(lib().mispec_cholesky_info(self.h))

    def _solve(self, fn, x_in):
        x = _f64(x_in)
        if x.shape != (self.n,):
            raise ValueError("triangular solve: x_in must have n entries")
        y = np.empty(self.n)
        check(fn(self.h, _dp(x), _dp(y)))
        return y

    def lower_triangular_solve(self, x_in):
        return self._solve(lib().mispec_cholesky_lower_solve_host, x_in)

    def upper_triangular_solve(self, x_in):
        return self._solve(lib().mispec_cholesky_upper_solve_host, x_in)

    def __del__(self):
        try:
            lib().mispec_cholesky_destroy(self.h)
        except Exception:
            pass


class SymShiftInvert(_ShiftBlock):
    """MatOp/SymShiftInvert.h (sparse A, sparse B): y = (A - sigma B)^{-1} x, factored on the GPU at set_shift(sigma).  solver: as for
    SparseSymShiftSolve."""

    def __init__(self, A, B, uplo_a="L", uplo_b="L", ctx=None, solver=None):
        self.ctx = ctx or default_context()
        n, nc, ao, ai, av, arm = _compressed(A)
        nb, ncb, bo, bi, bv, brm = _compressed(B)
        if n != nc or nb != n or ncb != n:
            raise ValueError("SymShiftInvert: A and B must be square matrices of the same size")
        h = C.c_void_p()
        check(lib().mispec_symshift_create_pencil_solver(self.ctx.h, n, _ip(ao), _ip(ai), _dp(av), uplo_a.encode()[0:1], int(arm),
                                                         _ip(bo), _ip(bi), _dp(bv), uplo_b.encode()[0:1], int(brm),
                                                         _shift_solver_kind(solver), C.byref(h)))
        self.h = h
        self.n = n

    def rows(self):
        return self.n

    cols = rows

    def set_shift(self, sigma):
        check(lib().mispec_symshift_set_shift(self.h, float(sigma)))

    def perform_op(self, x_in):
        x = _f64(x_in)
        if x.shape != (self.n,):
            raise ValueError("perform_op: x_in must have n entries")
        y = np.empty(self.n)
        check(lib().mispec_symshift_solve_host(self.h, _dp(x), _dp(y)))
        return y

    def __del__(self):
        try:
            lib().mispec_symshift_destroy(self.h)
        except Exception:
            pass


class SparseRegularInverse:
    """MatOp/SparseRegularInverse.h: the B operator of a generalized problem — perform_op = B x, solve = B^{-1} x by a
    conjugate-gradient iteration on the GPU (the reference's Eigen::ConjugateGradient defaults)."""

    def __init__(self, mat, uplo="L", ctx=None):
        self.ctx = ctx or default_context()
        n, nc, outer, inner, val, row_major = _compressed(mat)
        if n != nc:
            raise ValueError("SparseRegularInverse: matrix must be square")
        h = C.c_void_p()
        check(lib().mispec_reginv_create(self.ctx.h, n, _ip(outer), _ip(inner), _dp(val), uplo.encode()[0:1], int(row_major),
                                         C.byref(h)))
        self.h = h
        self.n = n

    def rows(self):
        return self.n

    cols = rows

    def perform_op(self, x_in):
        x = _f64(x_in)
        if x.shape != (self.n,):
            raise ValueError("perform_op: x_in must have n entries")
        y = np.empty(self.n)
        check(lib().mispec_reginv_perform_op_host(self.h, _dp(x), _dp(y)))
        return y

    def solve(self, x_in):
        x = _f64(x_in)
        if x.shape != (self.n,):
            raise ValueError("solve: x_in must have n entries")
        y = np.empty(self.n)
        check(lib().mispec_reginv_solve_host(self.h, _dp(x), _dp(y)))
        return y

    def last_iterations(self):
        return int(lib().mispec_reginv_last_iterations(self.h))

    def __del__(self):
        try:
            lib().mispec_reginv_destroy(self.h)
        except Exception:
            pass


class SVDMatOp:
    """contrib/PartialSVDSolver.h:16-110: the operator A'A (tall A, SVDTallMatOp) or AA' (wide A, SVDWideMatOp) as two
    device CSR matrices applied one after the other inside the device Lanczos loop."""

    def __init__(self, mat, ctx=None):
        import scipy.sparse as sp

        self.ctx = ctx or default_context()
        mat = sp.csr_matrix(mat)
        self.m, self.n = mat.shape
        self.mat = SparseGenMatProd(mat, ctx=self.ctx)
        self.mat_t = SparseGenMatProd(sp.csr_matrix(mat.T), ctx=self.ctx)
        self.tall = self.m > self.n
        self.first, self.second = (self.mat, self.mat_t) if self.tall else (self.mat_t, self.mat)

    def rows(self):
        return min(self.m, self.n)

    cols = rows

    def local_rows(self):
        return self.rows()

    def perform_op(self, x):
        return self.second.perform_op(self.first.perform_op(x))


class PartialSVDSolver:
    """contrib/PartialSVDSolver.h:112-209: the ncomp largest singular triplets through SymEigsSolver(LargestAlge)."""

    def __init__(self, mat, ncomp, ncv, ctx=None):
        self.op = SVDMatOp(mat, ctx)
        self.eigs = SymEigsSolver(self.op, ncomp, ncv)
        self.nconv = 0
        self._evecs = None

    def compute(self, maxit=1000, tol=1e-10):
        self.eigs.init()
        self.nconv = self.eigs.compute(SortRule.LargestAlge, maxit, tol)
        self._evecs = None
        return self.nconv

    def singular_values(self):
        return np.sqrt(self.eigs.eigenvalues())

    def _vectors(self):
        if self._evecs is None:
            self._evecs = self.eigs.eigenvectors()
        return self._evecs

    def _scaled(self, A, k):
        ev = self.eigs.eigenvalues()
        return A @ np.asfortranarray(self._vectors()[:, :k] / np.sqrt(ev[:k]))

    def matrix_U(self, nu):
        nu = min(int(nu), self.nconv)
        return self._vectors()[:, :nu] if self.op.m <= self.op.n else self._scaled(self.op.mat, nu)

    def matrix_V(self, nv):
        nv = min(int(nv), self.nconv)
        return self._vectors()[:, :nv] if self.op.m > self.op.n else self._scaled(self.op.mat_t, nv)


class _GEigsRegInvOp:
    """MatOp/internal/SymGEigsRegInvOp.h: y = B^{-1} A x."""

    def __init__(self, A, B):
        if not isinstance(A, SparseSymMatProd) or not isinstance(B, SparseRegularInverse):
            raise TypeError("SymGEigsSolver: needs a SparseSymMatProd and a SparseRegularInverse")
        if A.rows() != B.rows():
            raise ValueError("SymGEigsSolver: A and B must have the same size")
        self.A, self.B = A, B

    def rows(self):
        return self.B.rows()

    cols = rows
    local_rows = rows

    def perform_op(self, x):
        return self.B.solve(self.A.perform_op(x))


class SymEigsSolver:
    """SymEigsSolver.h:133-160 / HermEigsBase.h: init(), compute(), info(), eigenvalues(), eigenvectors() ..."""

    def __init__(self, op, nev, ncv, ctx=None):
        self.op = op
        h = C.c_void_p()
        if isinstance(op, _DeviceMatrix):
            self.ctx = op.ctx
            check(lib().mispec_symeigs_create(self.ctx.h, op.h, int(nev), int(ncv), C.byref(h)))
            self._user = None
        elif isinstance(op, _GEigsRegInvOp):  # y = B^{-1}(A x) in the B-inner product
            self.ctx = op.A.ctx
            check(lib().mispec_symeigs_create_geigs_reginv(self.ctx.h, op.A.h, op.B.h, int(nev), int(ncv), C.byref(h)))
            self._user = None
        elif isinstance(op, _GEigsCholeskyOp):  # y = L^{-1} A L^{-T} x
            self.ctx = op.A.ctx
            check(lib().mispec_symeigs_create_geigs_cholesky(self.ctx.h, op.A.h, op.B.h, int(nev), int(ncv), C.byref(h)))
            self._user = None
        elif isinstance(op, _GEigsShiftOp):  # y = (A - sigma B)^{-1} B x (+ Cayley), B-inner product
            self.ctx = op.S.ctx
            check(lib().mispec_symeigs_create_geigs_shift(self.ctx.h, op.S.h, op.B.h, op.mode, int(nev), int(ncv), float(op.sigma),
                                                          C.byref(h)))
            self._user = None
        elif isinstance(op, SVDMatOp):  # y = A2 (A x), both factors in HBM
            self.ctx = op.ctx
            check(lib().mispec_symeigs_create_product(self.ctx.h, op.first.h, op.second.h, int(nev), int(ncv), C.byref(h)))
            self._user = None
        elif isinstance(op, _DenseMatrix):  # dense GEMV on the device
            self.ctx = op.ctx
            check(lib().mispec_symeigs_create_dense(self.ctx.h, op.h, int(nev), int(ncv), C.byref(h)))
            self._user = None
        elif isinstance(op, DeviceOp):  # user operator on device pointers
            self.ctx = op.ctx
            check(lib().mispec_symeigs_create_device_op(self.ctx.h, op.cb, None, op.n, int(nev), int(ncv), C.byref(h)))
            self._user = None
        else:  # any object with rows(), cols(), perform_op(x) -> y: the reference's OpType concept
            self.ctx = ctx or default_context()
            self._user = _UserOp(op)
            check(lib().mispec_symeigs_create_op(self.ctx.h, self._user.cb, None, int(op.rows()), int(nev), int(ncv),
                                                 C.byref(h)))
        self.h = h
        self.nev, self.ncv = int(nev), int(ncv)

    def init(self, init_resid=None):
        v0 = None if init_resid is None else _f64(init_resid)
        if v0 is not None and v0.shape != (self.op.rows(),):
            raise ValueError("init: the initial residual vector must have n entries")
        check(lib().mispec_symeigs_init(self.h, _dp(v0)))

    def compute(self, selection=SortRule.LargestMagn, maxit=1000, tol=1e-10, sorting=SortRule.LargestAlge):
        nconv = C.c_int64()
        check(lib().mispec_symeigs_compute(self.h, int(selection), int(maxit), float(tol), int(sorting), C.byref(nconv)))
        return nconv.value

    def info(self):
        return CompInfo(lib().mispec_symeigs_info(self.h))

    def num_iterations(self):
        return lib().mispec_symeigs_num_iterations(self.h)

    def num_operations(self):
        return lib().mispec_symeigs_num_operations(self.h)

    def eigenvalues(self):
        out = np.empty(self.nev)
        cnt = C.c_int64()
        check(lib().mispec_symeigs_eigenvalues(self.h, _dp(out), C.byref(cnt)))
        return out[:cnt.value].copy()

    def local_rows(self):
        return self.op.local_rows() if isinstance(self.op, (_DeviceMatrix, SVDMatOp, _GEigsRegInvOp, _GEigsShiftOp, _GEigsCholeskyOp,
                                                            _DenseMatrix, DeviceOp)) else self.op.rows()

    def eigenvectors(self, nvec=None, to_host=True, out=None):
        """n x nconv (this shard's rows).  to_host=False leaves the result in HBM and returns the column count.  out: a
        column-major float64 array of at least local_rows x min(nvec, nev) to be filled instead of a fresh one (the reference's
        eigenvectors() returns a new matrix every time; a caller that solves repeatedly saves the first-touch page faults of
        1.6 GB at n = 1e7 by handing the previous result back — SymEigsSolver::eigenvectors_to in the C++ headers)."""
        nvec = self.nev if nvec is None else int(nvec)
        cnt = C.c_int64()
        if not to_host:
            check(lib().mispec_symeigs_eigenvectors(self.h, nvec, None, C.byref(cnt)))
            return cnt.value
        ncol = max(min(nvec, self.nev), 1)
        if out is None:
            out = np.empty((self.local_rows(), ncol), order="F")  # filled by the library's host threads
        elif not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.f_contiguous and out.ndim == 2 and
                  out.shape[0] == self.local_rows() and out.shape[1] >= ncol):
            raise ValueError("eigenvectors(out=...): need a column-major float64 array of local_rows x >= min(nvec, nev)")
        check(lib().mispec_symeigs_eigenvectors(self.h, nvec, _dp(out), C.byref(cnt)))
        return out[:, :cnt.value] if out.shape[1] != cnt.value else out

    def residuals(self):
        """||A x - lambda x|| / ||x|| of the converged pairs, evaluated on the device."""
        out = np.empty(self.nev)
        cnt = C.c_int64()
        check(lib().mispec_symeigs_residuals(self.h, _dp(out), C.byref(cnt)))
        return out[:cnt.value].copy()

    def profile(self, enable):
        check(lib().mispec_symeigs_profile(self.h, int(enable)))  # 0 off, 1 all families, 2 SpMV only

    def get_profile(self):
        p = Profile()
        check(lib().mispec_symeigs_get_profile(self.h, C.byref(p)))
        return p.as_dict()

    def set_orth_mode(self, mode):
        """'onesweep' (default: the correction of a step rides on the next step's pass over V, include/mispec.h
        mispec_fac_set_orth_mode) or 'reference' (Lanczos.h:145-181, two passes over V per step; also MISPEC_ORTH=reference in
        the environment).  'onesweep-wide' (opt-in) extends the one-sweep steps to 128 < ncv <= 512: from step 128 on the pass
        goes in column panels (orth_info()['panel_steps'] counts those steps).  Call before init().  Where the one-sweep steps
        do not apply (ncv > 128 without 'onesweep-wide', ncv > 512, ncv > 128 on a row-sharded context, generalized problems,
        host-pointer user operators) the reference flow runs whatever is set: orth_info()['mode'] says which one is in effect."""
        check(lib().mispec_symeigs_set_orth_mode(self.h, _orth_mode_value(mode)))

    def orth_info(self):
        mode, a, b, c = C.c_int(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        r, k = C.c_double(0.0), C.c_double(0.0)
        check(lib().mispec_symeigs_orth_info(self.h, C.byref(mode), C.byref(a), C.byref(b), C.byref(c), C.byref(r), C.byref(k)))
        fused, again = C.c_int64(0), C.c_int64(0)
        check(lib().mispec_symeigs_restart_info(self.h, C.byref(fused), C.byref(again)))
        ored = C.c_int64(0)
        check(lib().mispec_symeigs_onered_steps(self.h, C.byref(ored)))
        pan = C.c_int64(0)
        check(lib().mispec_symeigs_panel_steps(self.h, C.byref(pan)))
        return {"mode": "onesweep" if (mode.value & 0xFF) else "reference", "eager_last": bool(mode.value & 0x100),
                "wide": bool(mode.value & 0x2000), "panel_steps": pan.value,
                "recorrect_hook": bool(mode.value & 0x200), "one_reduction": bool(mode.value & 0x800), "lagged_steps": a.value, "check_stops": b.value,
                "state_stops": c.value, "max_rel_c": r.value, "max_chk": k.value, "fused_restarts": fused.value,
                "fused_recorrected": again.value, "one_reduction_steps": ored.value}

    def turn_info(self):
        """Host turns of the restarts: count, host seconds between 'sweep state seen' and 'restart enqueued', copy fallbacks."""
        turns, fb, sec = C.c_int64(0), C.c_int64(0), C.c_double(0.0)
        check(lib().mispec_symeigs_turn_info(self.h, C.byref(turns), C.byref(sec), C.byref(fb)))
        return {"turns": turns.value, "host_seconds": sec.value, "fallbacks": fb.value}

    def overlap_info(self):
        """(first interior 256-row block, interior blocks, all blocks): what is multiplied while the exchange is in flight."""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().mispec_symeigs_overlap_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def exchange_info(self):
        """(halo, doubles received per product): how a sharded matrix moves the Krylov vector (mispec_fac_exchange_info)."""
        halo, cnt = C.c_int(0), C.c_int64(0)
        check(lib().mispec_symeigs_exchange_info(self.h, C.byref(halo), C.byref(cnt)))
        return bool(halo.value), int(cnt.value)

    def __del__(self):
        try:
            lib().mispec_symeigs_destroy(self.h)
        except Exception:
            pass


class DavidsonSymEigsSolver:
    """DavidsonSymEigsSolver.h:18-90 / JDSymEigsBase.h:28-187: block Davidson with the diagonal (DPR) correction.
    op: SparseSymMatProd, DenseSymMatProd, or a DeviceOp together with `diagonal` (the solver needs op(i, i))."""

    def __init__(self, op, nev, nvec_init=None, nvec_max=None, diagonal=None):
        nev = int(nev)
        nvec_init = 2 * nev if nvec_init is None else int(nvec_init)
        nvec_max = 10 * nev if nvec_max is None else int(nvec_max)
        self.op = op
        self.ctx = op.ctx
        self.nev = nev
        h = C.c_void_p()
        if isinstance(op, _DeviceMatrix):
            check(lib().mispec_davidson_create(self.ctx.h, op.h, nev, nvec_init, nvec_max, C.byref(h)))
        elif isinstance(op, _DenseMatrix):
            check(lib().mispec_davidson_create_dense(self.ctx.h, op.h, nev, nvec_init, nvec_max, C.byref(h)))
        elif isinstance(op, DeviceOp):
            if diagonal is None:
                raise ValueError("DavidsonSymEigsSolver: a device operator needs its diagonal")
            d = _f64(diagonal)
            if d.shape != (op.n,):
                raise ValueError("DavidsonSymEigsSolver: diagonal must have n entries")
            check(lib().mispec_davidson_create_device_op(self.ctx.h, op.cb, None, op.n, _dp(d), nev, nvec_init, nvec_max, C.byref(h)))
        else:
            raise TypeError("DavidsonSymEigsSolver: the operator must live on the device (SparseSymMatProd, DenseSymMatProd, DeviceOp)")
        self.h = h

    def set_max_search_space_size(self, m):
        check(lib().mispec_davidson_set_sizes(self.h, -1, int(m), -1))

    def set_correction_size(self, m):
        check(lib().mispec_davidson_set_sizes(self.h, -1, -1, int(m)))

    def set_initial_search_space_size(self, m):
        check(lib().mispec_davidson_set_sizes(self.h, int(m), -1, -1))

    def sizes(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        check(lib().mispec_davidson_get_sizes(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def compute(self, selection=SortRule.LargestMagn, maxit=100, tol=1e-10):
        n = C.c_int64()
        check(lib().mispec_davidson_compute(self.h, int(selection), int(maxit), float(tol), None, 0, 0, C.byref(n)))
        return n.value

    def compute_with_guess(self, initial_space, selection=SortRule.LargestMagn, maxit=100, tol=1e-10):
        G = np.asfortranarray(initial_space, dtype=np.float64)
        if G.ndim != 2 or G.shape[0] != self.op.rows():
            raise ValueError("compute_with_guess: the initial space must have n rows")
        n = C.c_int64()
        check(lib().mispec_davidson_compute(self.h, int(selection), int(maxit), float(tol), _dp(G), G.shape[1], G.shape[0], C.byref(n)))
        return n.value

    def info(self):
        return CompInfo(lib().mispec_davidson_info(self.h))

    def num_iterations(self):
        return lib().mispec_davidson_num_iterations(self.h)

    def num_operations(self):
        return lib().mispec_davidson_num_operations(self.h)

    def eigenvalues(self):
        out = np.empty(self.nev)
        check(lib().mispec_davidson_eigenvalues(self.h, _dp(out)))
        return out

    def eigenvectors(self):
        n = self.op.rows()
        out = np.empty((n, self.nev), order="F")
        check(lib().mispec_davidson_eigenvectors(self.h, _dp(out), n))
        return out

    def __del__(self):
        try:
            lib().mispec_davidson_destroy(self.h)
        except Exception:
            pass


class LOBPCGInfo(enum.IntEnum):
    """The info values of contrib/LOBPCGSolver.h (Eigen::ComputationInfo)."""
    Success = 0
    NumericalIssue = 1
    NoConvergence = 2
    InvalidInput = 3


class LOBPCGSolver:
    """contrib/LOBPCGSolver.h on the device: the m smallest (or largest) eigenpairs of A x = lambda B x by LOBPCG.
    op, B: SparseSymMatProd (unsharded); X0: dense n x m start block, or nev columns of SimpleRandom streams (seed j + 1);
    preconditioner: a sparse device operator (SparseSymMatProd, or SparseGenMatProd) applied as R <- T R, a positive definite
    SparseSymShiftSolve / SymShiftInvert whose block solve is applied (a reference is kept), or "jacobi" (1 / diag A); constraints: dense n x c block the
    eigenvectors are kept B-orthogonal to.  1 <= m <= 21, m < n, c <= 21, m + c < n."""

    def __init__(self, op, X0=None, nev=None, B=None, preconditioner=None, constraints=None):
        if not isinstance(op, _DeviceMatrix) or (B is not None and not isinstance(B, _DeviceMatrix)):
            raise TypeError("LOBPCGSolver: the operators must be SparseSymMatProd")
        n = op.rows()
        if X0 is not None:
            X0 = np.asfortranarray(X0, dtype=np.float64)
            if X0.ndim != 2 or X0.shape[0] != n:
                raise ValueError("LOBPCGSolver: the start block must have n rows")
            if nev is not None and int(nev) != X0.shape[1]:
                raise ValueError("LOBPCGSolver: nev differs from the number of start vectors")
            nev = X0.shape[1]
        elif nev is None:
            raise ValueError("LOBPCGSolver: give a start block X0 or the number of eigenpairs nev")
        self.op, self.B, self.T = op, B, None  # keeps the operators alive
        self.ctx = op.ctx
        self.n, self.m = n, int(nev)
        self.h = C.c_void_p()
        check(lib().mispec_lobpcg_create(self.ctx.h, op.h, self.m, C.byref(self.h)))
        if B is not None:
            check(lib().mispec_lobpcg_set_B(self.h, B.h))
        if isinstance(preconditioner, str):
            if preconditioner != "jacobi":
                raise ValueError("LOBPCGSolver: the preconditioner is a SparseSymMatProd or the string 'jacobi'")
            check(lib().mispec_lobpcg_set_jacobi(self.h, 1))
        elif isinstance(preconditioner, _ShiftBlock):
            # a factorisation (SparseSymShiftSolve, SymShiftInvert) applied as R <- (K - sigma M)^{-1} R, one block solve per iteration
            self.T = preconditioner
            check(lib().mispec_lobpcg_set_preconditioner_solver(self.h, preconditioner.h))
        elif preconditioner is not None:
            if not isinstance(preconditioner, _DeviceMatrix):
                raise TypeError("LOBPCGSolver: the preconditioner is a SparseSymMatProd or the string 'jacobi'")
            self.T = preconditioner
            check(lib().mispec_lobpcg_set_preconditioner(self.h, preconditioner.h))
        if constraints is not None:
            Y = np.asfortranarray(constraints, dtype=np.float64)
            if Y.ndim != 2 or Y.shape[0] != n:
                raise ValueError("LOBPCGSolver: the constraints must have n rows")
            check(lib().mispec_lobpcg_set_constraints(self.h, _dp(Y), n, Y.shape[1]))
        if X0 is not None:
            check(lib().mispec_lobpcg_set_initial(self.h, _dp(X0), n))

    def compute(self, selection=SortRule.SmallestAlge, maxit=100, tol=1e-8):
        """tol is absolute: a column is converged when |A x - lambda B x|_2 < tol.  Returns the number of converged columns."""
        nconv = C.c_int64()
        check(lib().mispec_lobpcg_compute(self.h, int(selection), int(maxit), float(tol), C.byref(nconv)))
        return nconv.value

    def info(self):
        return LOBPCGInfo(lib().mispec_lobpcg_info(self.h))

    def num_iterations(self):
        return lib().mispec_lobpcg_num_iterations(self.h)

    def num_operations(self):
        return lib().mispec_lobpcg_num_operations(self.h)

    def num_retries(self):
        """Iterations whose Rayleigh-Ritz step was repeated without the block P."""
        return lib().mispec_lobpcg_num_retries(self.h)

    def eigenvalues(self):
        out = np.empty(self.m)
        check(lib().mispec_lobpcg_eigenvalues(self.h, _dp(out)))
        return out

    def residual_norms(self):
        out = np.empty(self.m)
        check(lib().mispec_lobpcg_residual_norms(self.h, _dp(out)))
        return out

    def eigenvectors(self):
        out = np.empty((self.n, self.m), order="F")
        check(lib().mispec_lobpcg_eigenvectors(self.h, _dp(out), self.n))
        return out

    def residuals(self):
        out = np.empty((self.n, self.m), order="F")
        check(lib().mispec_lobpcg_residuals(self.h, _dp(out), self.n))
        return out

    def __del__(self):
        try:
            lib().mispec_lobpcg_destroy(self.h)
        except Exception:
            pass


def _torch_block(t, name):
    """(device address, leading dimension, columns) of a column-major block held as a float64 CUDA tensor of shape (columns, ld):
    row j of the tensor is column j of the block (slices along the first dimension are blocks of the same buffer)."""
    import torch

    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError("%s: expected a 2-D float64 CUDA tensor of shape (columns, ld) with unit stride along ld" % name)
    return t.data_ptr(), (t.stride(0) if t.shape[0] > 1 else t.shape[1]), t.shape[0]


def _torch_sync():
    import torch

    torch.cuda.current_stream().synchronize()  # the library reads on the context's stream


def lobpcg_gram(U, W, n, symmetric=False, ctx=None):
    """G = U[:, :n]' W[:, :n] by the LOBPCG solver's Gram kernel (mispec_lobpcg_gram): U, W torch blocks (see _torch_block) of p, q <= 64
    columns, possibly overlapping parts of one buffer; returns the p x q numpy array."""
    ctx = ctx or default_context()
    up, ldu, p = _torch_block(U, "lobpcg_gram")
    wp, ldw, q = _torch_block(W, "lobpcg_gram")
    G = np.empty((p, q), order="F")
    _torch_sync()
    check(lib().mispec_lobpcg_gram(ctx.h, C.c_void_p(up), ldu, p, C.c_void_p(wp), ldw, q, int(n), int(bool(symmetric)), _dp(G)))
    return G


def lobpcg_resid(AX, BX, n, lam, idx, R=None, dinv=None, ctx=None):
    """The solver's residual kernel (mispec_lobpcg_resid): R[k] <- (AX - lam BX)[idx k] (times dinv per row when given) for the active
    columns idx, and returns |AX_j - lam_j BX_j|^2 of every column j."""
    ctx = ctx or default_context()
    ap, ld, m = _torch_block(AX, "lobpcg_resid")
    bp, ldb, mb = _torch_block(BX, "lobpcg_resid")
    if ldb != ld or mb != m:
        raise ValueError("lobpcg_resid: AX and BX must have the same shape")
    lam = _f64(lam)
    idx = _i32(idx)
    if lam.shape != (m,):
        raise ValueError("lobpcg_resid: one lambda per column")
    rp, ldr = (None, 0)
    if R is not None:
        rp, ldr, _ = _torch_block(R, "lobpcg_resid")
    out = np.empty(m)
    _torch_sync()
    check(lib().mispec_lobpcg_resid(ctx.h, C.c_void_p(ap), C.c_void_p(bp), ld, m, int(n), _dp(lam), _ip(idx), int(idx.size),
                                    C.c_void_p(dinv.data_ptr()) if dinv is not None else None, C.c_void_p(rp) if rp else None, ldr,
                                    _dp(out)))
    return out


def lobpcg_block_sub(Z, Y, Cmat, n, ctx=None):
    """Z[:, :n] <- Z - Y C in place by the solver's constraint kernel (mispec_lobpcg_block_sub): Z of q, Y of c columns, C c x q."""
    ctx = ctx or default_context()
    zp, ldz, q = _torch_block(Z, "lobpcg_block_sub")
    yp, ldy, c = _torch_block(Y, "lobpcg_block_sub")
    Cm = np.asfortranarray(Cmat, dtype=np.float64)
    if Cm.shape != (c, q):
        raise ValueError("lobpcg_block_sub: C must be c x q")
    _torch_sync()
    check(lib().mispec_lobpcg_block_sub(ctx.h, C.c_void_p(zp), ldz, q, C.c_void_p(yp), ldy, c, _dp(Cm), int(n)))


RECORD_LD = 1032  # doubles of a reduced record (csrc/krylov.hpp kPartialLd): slots 0 ... 1023, sum f^2, max |f|, its root, max |c|
SLOT_BETA2, SLOT_MAXABS, SLOT_BETA, SLOT_ERR = 1024, 1025, 1026, 1027
STEP_OK, STEP_SMALL_BETA, STEP_MORE_CORR, STEP_TINY_F, STEP_LAG_CHECK, STEP_RESTART_CHECK = range(6)  # krylov.hpp kStep*


def lagged_pass(V, i, n, f, src, vout, c_in, alpha, beta, *, pending, onered, diag, subd, status=STEP_OK, lag_last=False,
                lag_chk_max=0.0, lag_rel_c_max=0.0, lag_limit=1e-6, n_op=None, lag_steps=0, onered_steps=0, alpha_parts=None,
                pstride=0, red=None, ctx=None):
    """TEST HOOK (mispec_lagged_pass, include/mispec.h): step i of the one-sweep Lanczos path alone — the ORTH_LAGGED pass over
    V[:, :i] chosen by the library's own dispatch, the reduction of its record and the scalar tail — on the caller's data.
    V: torch block (see _torch_block) of at least i columns; f, src, vout: 1-D float64 CUDA tensors of at least ld entries' worth
    of rows (f is overwritten with the next residual, vout with column i).  Contract for an odd n: row n of V, f and src is 0.
    diag, subd: at least i + 1 entries of H's diagonals; red: the record on entry (RECORD_LD doubles, default zeros).
    Returns a dict: red, diag, subd (numpy) and the scalars the tail leaves."""
    import torch

    ctx = ctx or default_context()
    vp, ldv, ncols = _torch_block(V, "lagged_pass")
    if ncols < i:
        raise ValueError("lagged_pass: V has fewer than i columns")
    for t in (f, src, vout):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError("lagged_pass: f, src and vout must be contiguous 1-D float64 CUDA tensors")
    c_in = _f64(c_in)
    if c_in.shape != (max(i, 0),):
        raise ValueError("lagged_pass: one coefficient per finished column")
    d, s = np.zeros(max(i, 0) + 1), np.zeros(max(i, 0) + 1)
    d[:] = _f64(diag)[: d.size]
    s[:] = _f64(subd)[: s.size]
    rec = np.zeros(RECORD_LD) if red is None else _f64(red).copy()
    if rec.shape != (RECORD_LD,):
        raise ValueError("lagged_pass: a record has RECORD_LD doubles")
    parts = _f64(alpha_parts) if alpha_parts is not None else None
    scal = _f64([alpha, beta, lag_chk_max, lag_rel_c_max, lag_limit, float(n if n_op is None else n_op)])
    flags = _i32([int(pending), int(onered), int(status), int(bool(lag_last)), int(lag_steps), int(onered_steps)])
    so, io = np.zeros(7), np.zeros(9, dtype=np.int64)
    _torch_sync()
    check(lib().mispec_lagged_pass(ctx.h, C.c_void_p(vp), ldv, int(i), int(n), C.c_void_p(f.data_ptr()), C.c_void_p(src.data_ptr()),
                                   C.c_void_p(vout.data_ptr()), _dp(c_in), _dp(parts), 0 if parts is None else int(parts.size),
                                   _dp(scal), _ip(flags), int(pstride), _dp(d), _dp(s), _dp(rec), _dp(so),
                                   io.ctypes.data_as(C.POINTER(C.c_int64))))
    return dict(red=rec, diag=d, subd=s, beta=so[0], alpha=so[1], lag_chk_max=so[2], lag_rel_c_max=so[3], err=so[4], alpha_out=so[6],
                status=int(io[0]), stop_step=int(io[1]), stop_count=int(io[2]), count=int(io[3]), need_corr=int(io[4]),
                lag_pending=int(io[5]), lag_steps=int(io[6]), onered_steps=int(io[7]), nrec=int(io[8]))


def fused_restart_pass(V, m, n, Q, c, ftilde, fnew, q_last, h_sub, kcol, *, status=STEP_OK, force_check=False, pstride=0, red=None,
                       ctx=None):
    """TEST HOOK (mispec_fused_restart_pass, include/mispec.h): the restart's V*Q pass with the pending correction riding on it
    (k_vq_fused, in place: V[:, :p] <- V[:, :m] Q) and the reduction with its tail, as mispec_fac_restart_sym runs them.
    V: torch block of at least m columns; Q: m x p array; c: m coefficients; ftilde, fnew: 1-D float64 CUDA tensors (distinct).
    Contract for an odd n: row n of V and ftilde is 0.  Returns a dict: red (numpy) and the scalars the tail leaves."""
    import torch

    ctx = ctx or default_context()
    vp, ldv, ncols = _torch_block(V, "fused_restart_pass")
    if ncols < m:
        raise ValueError("fused_restart_pass: V has fewer than m columns")
    for t in (ftilde, fnew):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError("fused_restart_pass: ftilde and fnew must be contiguous 1-D float64 CUDA tensors")
    Qm = np.asfortranarray(Q, dtype=np.float64)
    if Qm.ndim != 2 or Qm.shape[0] != m:
        raise ValueError("fused_restart_pass: Q must be m x p")
    c = _f64(c)
    if c.shape != (max(m, 0),):
        raise ValueError("fused_restart_pass: one coefficient per column")
    rec = np.zeros(RECORD_LD) if red is None else _f64(red).copy()
    if rec.shape != (RECORD_LD,):
        raise ValueError("fused_restart_pass: a record has RECORD_LD doubles")
    so, io = np.zeros(3), np.zeros(4, dtype=np.int64)
    _torch_sync()
    check(lib().mispec_fused_restart_pass(ctx.h, C.c_void_p(vp), ldv, int(m), int(n), _dp(Qm), int(Qm.shape[1]), _dp(c),
                                          C.c_void_p(ftilde.data_ptr()), C.c_void_p(fnew.data_ptr()), float(q_last), float(h_sub),
                                          int(kcol), int(status), int(bool(force_check)), int(pstride), _dp(rec), _dp(so),
                                          io.ctypes.data_as(C.POINTER(C.c_int64))))
    return dict(red=rec, beta=so[0], rst_err=so[1], rst_beta_corr=so[2], status=int(io[0]), stop_step=int(io[1]),
                stop_count=int(io[2]), nrec=int(io[3]))


class _GEigsCholeskyOp:
    """MatOp/internal/SymGEigsCholeskyOp.h: y = L^{-1} A L^{-T} x."""

    def __init__(self, A, B):
        if not isinstance(A, SparseSymMatProd) or not isinstance(B, SparseCholesky):
            raise TypeError("SymGEigsSolver (Cholesky mode): needs a SparseSymMatProd and a SparseCholesky")
        if A.rows() != B.rows():
            raise ValueError("SymGEigsSolver: A and B must have the same size")
        self.A, self.B = A, B

    def rows(self):
        return self.B.rows()

    cols = rows
    local_rows = rows

    def perform_op(self, x):
        return self.B.lower_triangular_solve(self.A.perform_op(self.B.upper_triangular_solve(x)))


class _GEigsShiftOp:
    """MatOp/internal/SymGEigs{ShiftInvert,Buckling,Cayley}Op.h."""

    MODES = {"ShiftInvert": 0, "Buckling": 1, "Cayley": 2}

    def __init__(self, S, B, sigma, mode):
        if not isinstance(S, SymShiftInvert) or not isinstance(B, SparseSymMatProd):
            raise TypeError("SymGEigsShiftSolver: needs a SymShiftInvert and a SparseSymMatProd")
        if mode not in self.MODES:
            raise ValueError("SymGEigsShiftSolver: mode must be ShiftInvert, Buckling or Cayley")
        if S.rows() != B.rows():
            raise ValueError("SymGEigsShiftSolver: the operators must have the same size")
        self.S, self.B, self.sigma, self.mode = S, B, float(sigma), self.MODES[mode]

    def rows(self):
        return self.S.rows()

    cols = rows
    local_rows = rows


class SymGEigsShiftSolver(SymEigsSolver):
    """SymGEigsShiftSolver<SymShiftInvert, SparseSymMatProd, mode> (SymGEigsShiftSolver.h:36-207): eigenvalues of the pencil
    near sigma.  op = SymShiftInvert(A, B) (for Buckling: (K, KG)), Bop = SparseSymMatProd of the inner-product matrix
    (B, or K for Buckling).  set_shift(sigma) is called on op by the solver."""

    def __init__(self, op, Bop, nev, ncv, sigma, mode="ShiftInvert"):
        super().__init__(_GEigsShiftOp(op, Bop, sigma, mode), nev, ncv)


class SymGEigsSolver(SymEigsSolver):
    """SymGEigsSolver<OpType, BOpType, mode> (SymGEigsSolver.h:142-238): A x = lambda B x.
    mode "RegularInverse": Bop = SparseRegularInverse(B), B-orthonormal eigenvectors straight from the Lanczos basis;
    mode "Cholesky": Bop = SparseCholesky(B), standard problem L^{-1} A L^{-T}, eigenvectors back-transformed by L^{-T}."""

    def __init__(self, op, Bop, nev, ncv, mode="RegularInverse"):
        if mode == "RegularInverse":
            super().__init__(_GEigsRegInvOp(op, Bop), nev, ncv)
        elif mode == "Cholesky":
            super().__init__(_GEigsCholeskyOp(op, Bop), nev, ncv)
        else:
            raise ValueError("SymGEigsSolver: mode must be RegularInverse or Cholesky (the shift modes are SymGEigsShiftSolver)")


class SymEigsShiftSolver(SymEigsSolver):
    """SymEigsShiftSolver.h:190-195: eigenvalues closest to sigma via (A - sigma I)^{-1}; the constructor calls
    op.set_shift(sigma) and eigenvalues() are mapped back (lambda = 1/nu + sigma)."""

    def __init__(self, op, nev, ncv, sigma, ctx=None):
        if isinstance(op, SparseSymShiftSolve):
            self.op = op
            self.ctx = op.ctx
            self._user = None
            h = C.c_void_p()
            check(lib().mispec_symeigs_create_shift(self.ctx.h, op.h, int(nev), int(ncv), float(sigma), C.byref(h)))
            self.h = h
            self.nev, self.ncv = int(nev), int(ncv)
        else:
            raise TypeError("SymEigsShiftSolver: pass a SparseSymShiftSolve operator")


class SparseGenRealShiftSolve(_ShiftBlock):
    """MatOp/SparseGenRealShiftSolve.h: y = (A - sigma I)^{-1} x for a general sparse A.  solver: None (what option shift_solver
    says; its default is direct) | "direct" (dense device factorisation, n <= 4096) | "auto" (that, and beyond n = 4096 the
    iterative path: Jacobi-preconditioned BiCGStab) | "iterative" (include/mispec.h mispec_symshift_create_general_solver)."""

    def __init__(self, mat, ctx=None, solver=None):
        self.ctx = ctx or default_context()
        n, nc, outer, inner, val, row_major = _compressed(mat)
        if n != nc:
            raise ValueError("SparseGenRealShiftSolve: matrix must be square")
        h = C.c_void_p()
        check(lib().mispec_symshift_create_general_solver(self.ctx.h, n, _ip(outer), _ip(inner), _dp(val), int(row_major),
                                                          _shift_solver_kind(solver), C.byref(h)))
        self.h = h
        self.n = n

    def rows(self):
        return self.n

    cols = rows
    local_rows = rows

    def set_shift(self, sigma):
        check(lib().mispec_symshift_set_shift(self.h, float(sigma)))

    def perform_op(self, x_in):
        x = _f64(x_in)
        if x.shape != (self.n,):
            raise ValueError("perform_op: x_in must have n entries")
        y = np.empty(self.n)
        check(lib().mispec_symshift_solve_host(self.h, _dp(x), _dp(y)))
        return y

    def solve_device(self, x_ptr, y_ptr):
        """y = (A - sigma I)^{-1} x on device pointers, enqueued on the context's stream (mispec_symshift_solve)."""
        check(lib().mispec_symshift_solve(self.h, C.c_void_p(int(x_ptr)), C.c_void_p(int(y_ptr))))

    def __del__(self):
        try:
            lib().mispec_symshift_destroy(self.h)
        except Exception:
            pass


class _GenComplexShiftBinding:
    def __init__(self, S, sigmar, sigmai):
        if not isinstance(S, SparseGenRealShiftSolve):
            raise TypeError("GenEigsComplexShiftSolver: needs a SparseGenComplexShiftSolve / DenseGenComplexShiftSolve operator")
        self.S, self.sigmar, self.sigmai = S, float(sigmar), float(sigmai)

    def rows(self):
        return self.S.rows()

    cols = rows
    local_rows = rows


class _GenShiftBinding:
    def __init__(self, S, sigma):
        if not isinstance(S, SparseGenRealShiftSolve):
            raise TypeError("GenEigsRealShiftSolver: needs a SparseGenRealShiftSolve")
        self.S, self.sigma = S, float(sigma)

    def rows(self):
        return self.S.rows()

    cols = rows
    local_rows = rows


class GenEigsSolver:
    """GenEigsSolver.h:139-186 / GenEigsBase.h: complex eigenvalues / eigenvectors of a general real matrix."""

    def __init__(self, op, nev, ncv, ctx=None):
        self.op = op
        h = C.c_void_p()
        if isinstance(op, _DeviceMatrix):
            self.ctx = op.ctx
            check(lib().mispec_geneigs_create(self.ctx.h, op.h, int(nev), int(ncv), C.byref(h)))
            self._user = None
        elif isinstance(op, _GenComplexShiftBinding):  # Arnoldi on Re((A - sigma I)^{-1} .), complex sigma
            self.ctx = op.S.ctx
            check(lib().mispec_geneigs_create_complex_shift(self.ctx.h, op.S.h, int(nev), int(ncv), float(op.sigmar), float(op.sigmai),
                                                            C.byref(h)))
            self._user = None
        elif isinstance(op, _GenShiftBinding):  # Arnoldi on (A - sigma I)^{-1}
            self.ctx = op.S.ctx
            check(lib().mispec_geneigs_create_shift(self.ctx.h, op.S.h, int(nev), int(ncv), float(op.sigma), C.byref(h)))
            self._user = None
        elif isinstance(op, _DenseMatrix):
            self.ctx = op.ctx
            check(lib().mispec_geneigs_create_dense(self.ctx.h, op.h, int(nev), int(ncv), C.byref(h)))
            self._user = None
        elif isinstance(op, DeviceOp):
            self.ctx = op.ctx
            check(lib().mispec_geneigs_create_device_op(self.ctx.h, op.cb, None, op.n, int(nev), int(ncv), C.byref(h)))
            self._user = None
        else:
            self.ctx = ctx or default_context()
            self._user = _UserOp(op)
            check(lib().mispec_geneigs_create_op(self.ctx.h, self._user.cb, None, int(op.rows()), int(nev), int(ncv),
                                                 C.byref(h)))
        self.h = h
        self.nev, self.ncv = int(nev), int(ncv)

    def init(self, init_resid=None):
        v0 = None if init_resid is None else _f64(init_resid)
        if v0 is not None and v0.shape != (self.op.rows(),):
            raise ValueError("init: the initial residual vector must have n entries")
        check(lib().mispec_geneigs_init(self.h, _dp(v0)))

    def compute(self, selection=SortRule.LargestMagn, maxit=1000, tol=1e-10, sorting=SortRule.LargestMagn):
        nconv = C.c_int64()
        check(lib().mispec_geneigs_compute(self.h, int(selection), int(maxit), float(tol), int(sorting), C.byref(nconv)))
        return nconv.value

    def info(self):
        return CompInfo(lib().mispec_geneigs_info(self.h))

    def num_iterations(self):
        return lib().mispec_geneigs_num_iterations(self.h)

    def num_operations(self):
        return lib().mispec_geneigs_num_operations(self.h)

    def eigenvalues(self):
        out = np.empty(self.nev, dtype=np.complex128)
        cnt = C.c_int64()
        check(lib().mispec_geneigs_eigenvalues(self.h, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(cnt)))
        return out[:cnt.value].copy()

    def eigenvectors(self, nvec=None):
        nvec = self.nev if nvec is None else int(nvec)
        rows = self.op.local_rows() if isinstance(self.op, _DeviceMatrix) else self.op.rows()
        out = np.zeros((rows, max(min(nvec, self.nev), 1)), dtype=np.complex128, order="F")
        cnt = C.c_int64()
        check(lib().mispec_geneigs_eigenvectors(self.h, nvec, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(cnt)))
        return np.asfortranarray(out[:, :cnt.value])

    def residuals(self):
        """||A x - lambda x|| / ||x|| of the converged (complex) pairs, evaluated on the device."""
        out = np.empty(self.nev)
        cnt = C.c_int64()
        check(lib().mispec_geneigs_residuals(self.h, _dp(out), C.byref(cnt)))
        return out[:cnt.value].copy()

    def profile(self, enable):
        check(lib().mispec_geneigs_profile(self.h, int(enable)))

    def get_profile(self):
        p = Profile()
        check(lib().mispec_geneigs_get_profile(self.h, C.byref(p)))
        return p.as_dict()

    def __del__(self):
        try:
            lib().mispec_geneigs_destroy(self.h)
        except Exception:
            pass



class GenEigsRealShiftSolver(GenEigsSolver):
    """GenEigsRealShiftSolver.h:36-82: eigenvalues of a general real A closest to the real shift sigma; op is a
    SparseGenRealShiftSolve (the solver calls set_shift(sigma)); lambda = 1/nu + sigma."""

    def __init__(self, op, nev, ncv, sigma):
        super().__init__(_GenShiftBinding(op, sigma), nev, ncv)

class SparseGenComplexShiftSolve(SparseGenRealShiftSolve):
    """MatOp/SparseGenComplexShiftSolve.h: y = Re((A - sigma I)^{-1} x) for a general sparse A and a complex shift.
    complex_solver: None | "direct" (the dense path, n <= 4096) | "auto" (that, and beyond n = 4096 the iterative path:
    Jacobi-preconditioned BiCGStab in complex arithmetic for a complex shift, the real one for a real shift) | "iterative"
    (include/mispec_extras.h mispec_symshift_create_general_complex).  solver: a kind other than direct is refused — the operator
    that argument selects takes real shifts only; option shift_solver is not read."""

    def __init__(self, mat, ctx=None, solver=None, complex_solver=None):
        if solver not in (None, "direct"):
            raise ValueError("SparseGenComplexShiftSolve: solver %r is not supported: the iterative path takes real shifts only "
                             "(complex shifts need the dense path, solver='direct', n <= 4096, or complex_solver=)" % (solver,))
        if complex_solver in (None, "direct"):
            super().__init__(mat, ctx, "direct")
            return
        kind = _shift_solver_kind(complex_solver)
        self.ctx = ctx or default_context()
        n, nc, outer, inner, val, row_major = _compressed(mat)
        if n != nc:
            raise ValueError("SparseGenComplexShiftSolve: matrix must be square")
        h = C.c_void_p()
        check(lib().mispec_symshift_create_general_complex(self.ctx.h, n, _ip(outer), _ip(inner), _dp(val), int(row_major), kind,
                                                           C.byref(h)))
        self.h = h
        self.n = n

    def set_shift(self, sigmar, sigmai=0.0):
        check(lib().mispec_symshift_set_shift_complex(self.h, float(sigmar), float(sigmai)))


class GenEigsComplexShiftSolver(GenEigsSolver):
    """GenEigsComplexShiftSolver.h:20-150: eigenvalues of a general real A closest to the complex shift sigmar + i sigmai."""

    def __init__(self, op, nev, ncv, sigmar, sigmai):
        super().__init__(_GenComplexShiftBinding(op, sigmar, sigmai), nev, ncv)


def _dense_as_csc(mat, name):
    """The compressed form of a dense host matrix (exact zeros dropped): what the device factorisations ingest."""
    import scipy.sparse as sp

    M = np.asarray(mat, dtype=np.float64)
    if M.ndim != 2 or M.shape[0] != M.shape[1]:
        raise ValueError(f"{name}: matrix must be square")
    return sp.csc_matrix(M)


class DenseSymShiftSolve(SparseSymShiftSolve):
    """MatOp/DenseSymShiftSolve.h: y = (A - sigma I)^{-1} x for a dense symmetric A (the `uplo` triangle is read)."""

    def __init__(self, mat, uplo="L", ctx=None):
        super().__init__(_dense_as_csc(mat, "DenseSymShiftSolve"), uplo, ctx)


class DenseGenRealShiftSolve(SparseGenRealShiftSolve):
    """MatOp/DenseGenRealShiftSolve.h: y = (A - sigma I)^{-1} x for a general dense A and a real shift (n <= 4096)."""

    def __init__(self, mat, ctx=None):
        super().__init__(_dense_as_csc(mat, "DenseGenRealShiftSolve"), ctx, "direct")  # dense: never the iterative path


class DenseGenComplexShiftSolve(SparseGenComplexShiftSolve):
    """MatOp/DenseGenComplexShiftSolve.h: the dense form of SparseGenComplexShiftSolve."""

    def __init__(self, mat, ctx=None):
        super().__init__(_dense_as_csc(mat, "DenseGenComplexShiftSolve"), ctx)


class DenseCholesky(SparseCholesky):
    """MatOp/DenseCholesky.h: B = L L' for a dense positive-definite B (n <= 4096)."""

    def __init__(self, mat, uplo="L", ctx=None):
        super().__init__(_dense_as_csc(mat, "DenseCholesky"), uplo, ctx)


def _c128(a):
    return np.ascontiguousarray(a, dtype=np.complex128)


def _zdp(a):
    """A complex128 array as the interleaved (re, im) double* of include/mispec_extras.h."""
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _uplo_code(uplo):
    if uplo not in ("L", "U"):
        raise ValueError("uplo must be 'L' or 'U'")
    return uplo.encode()


class SparseHermMatProd:
    """MatOp/SparseHermMatProd.h for std::complex<double>: y = A x for a complex Hermitian sparse A of which only the `uplo`
    triangle of `mat` (a scipy sparse matrix, CSR or CSC kept as given, int32 or int64 indices) is read; it is mirrored conjugated
    into full CSR in HBM, the diagonal taken real (mispec_zcsr)."""

    def __init__(self, mat, uplo="L", ctx=None):
        import scipy.sparse as sp

        self.ctx = ctx or default_context()
        if not sp.issparse(mat):
            raise ValueError("SparseHermMatProd: a scipy sparse matrix is expected")
        if mat.format not in ("csr", "csc"):
            mat = mat.tocsc()
        if mat.shape[0] != mat.shape[1]:
            raise ValueError("SparseHermMatProd: matrix must be square")
        itype = np.int64 if mat.indptr.dtype == np.int64 or mat.indices.dtype == np.int64 else np.int32
        outer = np.ascontiguousarray(mat.indptr, dtype=itype)
        inner = np.ascontiguousarray(mat.indices, dtype=itype)
        vals = _c128(mat.data)
        h = C.c_void_p()
        check(lib().mispec_zcsr_upload(self.ctx.h, mat.shape[0], mat.shape[1], outer.ctypes.data, inner.ctypes.data,
                                       outer.dtype.itemsize, _zdp(vals), int(mat.format == "csr"), _uplo_code(uplo), C.byref(h)))
        self.h = h

    def rows(self):
        return lib().mispec_zcsr_rows(self.h)

    def cols(self):
        return lib().mispec_zcsr_cols(self.h)

    def nnz(self):
        """Stored entries of the mirrored (full) matrix."""
        return lib().mispec_zcsr_nnz(self.h)

    def perform_op(self, x_in, y_out=None):
        """y_out = A * x_in with HOST arrays (the reference's perform_op contract), complex128."""
        x = _c128(x_in)
        if x.shape != (self.cols(),):
            raise ValueError("perform_op: x_in must have cols() entries")
        y = np.empty(self.rows(), dtype=np.complex128) if y_out is None else y_out
        check(lib().mispec_zcsr_spmv_host(self.h, _zdp(x), _zdp(y)))
        return y

    def perform_op_lanes(self, lanes_per_row, x_in):
        """perform_op by the kernel with 4, 8 or 16 lanes per row (8 is what perform_op and the solver run)."""
        x = _c128(x_in)
        if x.shape != (self.cols(),):
            raise ValueError("perform_op_lanes: x_in must have cols() entries")
        y = np.empty(self.rows(), dtype=np.complex128)
        check(lib().mispec_zcsr_spmv_host_lanes(self.h, int(lanes_per_row), _zdp(x), _zdp(y)))
        return y

    def __matmul__(self, X):
        X = np.asarray(X, dtype=np.complex128)
        if X.ndim == 1:
            return self.perform_op(X)
        return np.stack([self.perform_op(X[:, j]) for j in range(X.shape[1])], axis=1)

    def __call__(self, i, j):
        v = np.zeros(2)
        check(lib().mispec_zcsr_coeff(self.h, int(i), int(j), _dp(v)))
        return complex(v[0], v[1])

    def spmv_time(self, reps, lanes_per_row=0):
        """Average ms of `reps` back-to-back device products (lanes_per_row 4 / 8 / 16, 0 = the default)."""
        ms = C.c_float()
        check(lib().mispec_zcsr_spmv_time(self.h, int(lanes_per_row), int(reps), C.byref(ms)))
        return ms.value

    def algorithmic_bytes(self):
        """Bytes one product must move: 20 per stored entry (16-byte value, 4-byte column), the row pointers, x and y once."""
        n = self.rows()
        return 20.0 * self.nnz() + 4.0 * (n + 1) + 16.0 * n + 16.0 * n

    def __del__(self):
        try:
            lib().mispec_zcsr_destroy(self.h)
        except Exception:
            pass


class DenseHermMatProd:
    """MatOp/DenseHermMatProd.h for std::complex<double>: y = A x for a complex Hermitian dense A of which only the `uplo`
    triangle is read (mirrored conjugated in HBM, the diagonal taken real; mispec_zdense)."""

    def __init__(self, mat, uplo="L", ctx=None):
        self.ctx = ctx or default_context()
        M = np.asarray(mat, dtype=np.complex128)
        if M.ndim != 2 or M.shape[0] != M.shape[1]:
            raise ValueError("DenseHermMatProd: a square 2-d array is expected")
        row_major = M.flags.c_contiguous and not M.flags.f_contiguous
        if not (M.flags.c_contiguous or M.flags.f_contiguous):
            M = np.asfortranarray(M)
        h = C.c_void_p()
        check(lib().mispec_zdense_upload(self.ctx.h, M.shape[0], M.shape[1], _zdp(M), max(int(M.shape[0]), 1), int(row_major),
                                         _uplo_code(uplo), C.byref(h)))
        self.h = h

    def rows(self):
        return lib().mispec_zdense_rows(self.h)

    def cols(self):
        return lib().mispec_zdense_cols(self.h)

    def perform_op(self, x_in, y_out=None):
        x = _c128(x_in)
        if x.shape != (self.cols(),):
            raise ValueError("perform_op: x_in must have cols() entries")
        y = np.empty(self.rows(), dtype=np.complex128) if y_out is None else y_out
        check(lib().mispec_zdense_gemv_host(self.h, _zdp(x), _zdp(y)))
        return y

    def __call__(self, i, j):
        v = np.zeros(2)
        check(lib().mispec_zdense_coeff(self.h, int(i), int(j), _dp(v)))
        return complex(v[0], v[1])

    def __del__(self):
        try:
            lib().mispec_zdense_destroy(self.h)
        except Exception:
            pass


class HermEigsSolver:
    """HermEigsSolver.h for std::complex<double> over SparseHermMatProd / DenseHermMatProd: the methods of SymEigsSolver;
    eigenvalues() are real (float64), eigenvectors() complex128 (n x nconv)."""

    def __init__(self, op, nev, ncv):
        h = C.c_void_p()
        if isinstance(op, SparseHermMatProd):
            check(lib().mispec_hermeigs_create_csr(op.ctx.h, op.h, int(nev), int(ncv), C.byref(h)))
        elif isinstance(op, DenseHermMatProd):
            check(lib().mispec_hermeigs_create_dense(op.ctx.h, op.h, int(nev), int(ncv), C.byref(h)))
        else:
            raise TypeError("HermEigsSolver: op must be a SparseHermMatProd or a DenseHermMatProd")
        self.op, self.h = op, h
        self.nev, self.ncv = int(nev), int(ncv)

    def init(self, init_resid=None):
        v0 = None if init_resid is None else _c128(init_resid)
        if v0 is not None and v0.shape != (self.op.rows(),):
            raise ValueError("init: the initial residual vector must have n entries")
        check(lib().mispec_hermeigs_init(self.h, _zdp(v0)))

    def compute(self, selection=SortRule.LargestMagn, maxit=1000, tol=1e-10, sorting=SortRule.LargestAlge):
        nconv = C.c_int64()
        check(lib().mispec_hermeigs_compute(self.h, int(selection), int(maxit), float(tol), int(sorting), C.byref(nconv)))
        return nconv.value

    def info(self):
        return CompInfo(lib().mispec_hermeigs_info(self.h))

    def num_iterations(self):
        return lib().mispec_hermeigs_num_iterations(self.h)

    def num_operations(self):
        return lib().mispec_hermeigs_num_operations(self.h)

    def eigenvalues(self):
        out = np.empty(self.nev)
        cnt = C.c_int64()
        check(lib().mispec_hermeigs_eigenvalues(self.h, _dp(out), C.byref(cnt)))
        return out[:cnt.value].copy()

    def eigenvectors(self, nvec=None):
        nvec = self.nev if nvec is None else int(nvec)
        out = np.empty((self.op.rows(), max(min(nvec, self.nev), 1)), dtype=np.complex128, order="F")
        cnt = C.c_int64()
        check(lib().mispec_hermeigs_eigenvectors(self.h, nvec, _zdp(out), C.byref(cnt)))
        return out[:, :cnt.value]

    def __del__(self):
        try:
            lib().mispec_hermeigs_destroy(self.h)
        except Exception:
            pass


def hess_qr(H, shift):
    """UpperHessenbergQR on the host (the general restart's real-shift step): returns (Q, Q'HQ)."""
    H = np.asfortranarray(H, dtype=np.float64)
    n = H.shape[0]
    Q, D = np.empty((n, n), order="F"), np.empty((n, n), order="F")
    check(lib().mispec_hess_qr_host(n, _dp(H), float(shift), _dp(Q), _dp(D)))
    return Q, D


def double_shift_qr(H, s, t):
    """DoubleShiftQR on the host: H^2 - sH + tI = QR; returns (Q, Q'HQ)."""
    H = np.asfortranarray(H, dtype=np.float64)
    n = H.shape[0]
    Q, D = np.empty((n, n), order="F"), np.empty((n, n), order="F")
    check(lib().mispec_double_shift_qr_host(n, _dp(H), float(s), float(t), _dp(Q), _dp(D)))
    return Q, D


def _sweep(fn, H, *args):
    H = np.asfortranarray(H, dtype=np.float64)
    n = H.shape[0]
    Q, D = np.empty((n, n), order="F"), np.empty((n, n), order="F")
    check(fn(*args[:1], n, _dp(H), *args[1:], _dp(Q), _dp(D)) if args and hasattr(args[0], "value") else fn(n, _dp(H), *args, _dp(Q), _dp(D)))
    return Q, D


def hess_qr_device(H, shift, ctx=None):
    """UpperHessenbergQR as a HIP kernel (k_hess_restart, one real shift): returns (Q, Q'HQ).  3 <= n <= 96."""
    ctx = ctx or default_context()
    return _sweep(lib().mispec_hess_qr, H, ctx.h, float(shift))


def double_shift_qr_device(H, s, t, ctx=None):
    """DoubleShiftQR (one Francis step) as a HIP kernel: returns (Q, Q'HQ).  3 <= n <= 96."""
    ctx = ctx or default_context()
    return _sweep(lib().mispec_double_shift_qr, H, ctx.h, float(s), float(t))


def hess_qr_lanes_host(H, shift):
    """The kernel's source (internal/SmallDenseGenLanes.h) run with one lane on the host."""
    return _sweep(lib().mispec_hess_qr_lanes_host, H, float(shift))


def double_shift_qr_lanes_host(H, s, t):
    return _sweep(lib().mispec_double_shift_qr_lanes_host, H, float(s), float(t))


def hess_schur(H):
    """UpperHessenbergSchur on the host: returns (T, U) with H = U T U'."""
    H = np.asfortranarray(H, dtype=np.float64)
    n = H.shape[0]
    T, U = np.empty((n, n), order="F"), np.empty((n, n), order="F")
    check(lib().mispec_hess_schur_host(n, _dp(H), _dp(T), _dp(U)))
    return T, U


def hess_eigen(H):
    """UpperHessenbergEigen on the host: complex (eigenvalues, eigenvectors)."""
    H = np.asfortranarray(H, dtype=np.float64)
    n = H.shape[0]
    ev = np.empty(n, dtype=np.complex128)
    V = np.empty((n, n), dtype=np.complex128, order="F")
    check(lib().mispec_hess_eigen_host(n, _dp(H), ev.ctypes.data_as(C.POINTER(C.c_double)),
                                       V.ctypes.data_as(C.POINTER(C.c_double))))
    return ev, V


class Factorization:
    """LinAlg/Arnoldi.h + LinAlg/Lanczos.h on the device (mispec_fac), for the L2 parity tests."""

    def __init__(self, op, m, symmetric=True, ctx=None):
        self.op = op
        self.m = int(m)
        h = C.c_void_p()
        if isinstance(op, _DeviceMatrix):
            self.ctx = op.ctx
            self.n = op.rows()
            check(lib().mispec_fac_create(self.ctx.h, op.h, _capi.op_fn(), None, self.n, self.m, int(symmetric), C.byref(h)))
            self._user = None
        elif isinstance(op, _DenseMatrix):
            self.ctx = op.ctx
            self.n = op.rows()
            check(lib().mispec_fac_create_dense(self.ctx.h, op.h, self.m, int(symmetric), C.byref(h)))
            self._user = None
        elif isinstance(op, DeviceOp):
            self.ctx = op.ctx
            self.n = op.n
            check(lib().mispec_fac_create_device_op(self.ctx.h, op.cb, None, self.n, self.m, int(symmetric), C.byref(h)))
            self._user = None
        elif isinstance(op, SparseGenRealShiftSolve):  # Arnoldi on (A - sigma I)^{-1}, bound on the device; call set_shift first
            self.ctx = op.ctx
            self.n = op.rows()
            check(lib().mispec_fac_create_shiftsolve(self.ctx.h, op.h, self.m, int(symmetric), C.byref(h)))
            self._user = None
        else:
            self.ctx = ctx or default_context()
            self.n = op.rows()
            self._user = _UserOp(op)
            check(lib().mispec_fac_create(self.ctx.h, None, self._user.cb, None, self.n, self.m, int(symmetric), C.byref(h)))
        self.h = h
        self.nmatop = C.c_int64(0)

    def init(self, v0):
        v0 = _f64(v0)
        check(lib().mispec_fac_init(self.h, _dp(v0), C.byref(self.nmatop)))

    def set_orth_mode(self, mode):
        """'onesweep' (default), 'onesweep-wide' (one-sweep steps up to m = 512) or 'reference' (mispec_fac_set_orth_mode);
        call before factorize_from."""
        check(lib().mispec_fac_set_orth_mode(self.h, _orth_mode_value(mode)))

    def orth_info(self):
        """The mode in effect and the counters of the one-sweep steps (mispec_fac_orth_info, mispec_fac_panel_steps)."""
        mode, a, b, c = C.c_int(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        r, k, pan = C.c_double(0.0), C.c_double(0.0), C.c_int64(0)
        check(lib().mispec_fac_orth_info(self.h, C.byref(mode), C.byref(a), C.byref(b), C.byref(c), C.byref(r), C.byref(k)))
        check(lib().mispec_fac_panel_steps(self.h, C.byref(pan)))
        return {"mode": "onesweep" if (mode.value & 0xFF) else "reference", "wide": bool(mode.value & 0x2000),
                "one_reduction": bool(mode.value & 0x800), "lagged_steps": a.value, "check_stops": b.value, "state_stops": c.value,
                "max_rel_c": r.value, "max_chk": k.value, "panel_steps": pan.value}

    def init_random(self, seed=0):
        check(lib().mispec_fac_init_random(self.h, seed, C.byref(self.nmatop)))

    def factorize_from(self, from_k, to_m):
        check(lib().mispec_fac_factorize(self.h, int(from_k), int(to_m), C.byref(self.nmatop)))

    def subspace_dim(self):
        return lib().mispec_fac_subspace_dim(self.h)

    def num_operations(self):
        return self.nmatop.value

    def f_norm(self):
        b = C.c_double()
        check(lib().mispec_fac_f_norm(self.h, C.byref(b)))
        return b.value

    def local_rows(self):
        return lib().mispec_fac_local_rows(self.h)

    def matrix_H(self):
        H = np.empty((self.m, self.m), order="F")
        check(lib().mispec_fac_get_H(self.h, _dp(H)))
        return H

    def matrix_V(self, ncols=None):
        ncols = self.m if ncols is None else ncols
        V = np.empty((self.local_rows(), ncols), order="F")
        check(lib().mispec_fac_get_V(self.h, ncols, _dp(V)))
        return V

    def vector_f(self):
        f = np.empty(self.local_rows())
        check(lib().mispec_fac_get_f(self.h, _dp(f)))
        return f

    def tridiag_eigen(self):
        ev = np.empty(self.m)
        U = np.empty((self.m, self.m), order="F")
        check(lib().mispec_fac_tridiag_eigen(self.h, _dp(ev), _dp(U)))
        return ev, U

    def restart_sym(self, shifts):
        s = _f64(shifts)
        check(lib().mispec_fac_restart_sym(self.h, _dp(s), len(s)))

    def restart_info(self):
        fused, again = C.c_int64(0), C.c_int64(0)
        check(lib().mispec_fac_restart_info(self.h, C.byref(fused), C.byref(again)))
        return {"fused_restarts": fused.value, "fused_recorrected": again.value}

    def turn_info(self):
        turns, fb, sec = C.c_int64(0), C.c_int64(0), C.c_double(0.0)
        check(lib().mispec_fac_turn_info(self.h, C.byref(turns), C.byref(sec), C.byref(fb)))
        return {"turns": turns.value, "host_seconds": sec.value, "fallbacks": fb.value}

    def compress_V(self, Q, H, new_k):
        Q = np.asfortranarray(Q, dtype=np.float64)
        H = np.asfortranarray(H, dtype=np.float64)
        check(lib().mispec_fac_compress_V(self.h, _dp(Q), _dp(H), int(new_k)))

    def ritz_vectors(self, Y):
        Y = np.asfortranarray(Y, dtype=np.float64)
        X = np.empty((self.local_rows(), Y.shape[1]), order="F")
        check(lib().mispec_fac_ritz_vectors(self.h, _dp(Y), Y.shape[1], _dp(X), None))
        return X

    def residuals(self, lam):
        lam = _f64(lam)
        out = np.empty(len(lam))
        check(lib().mispec_fac_residuals(self.h, _dp(lam), len(lam), _dp(out)))
        return out

    def profile(self, enable):
        check(lib().mispec_fac_profile(self.h, int(enable)))

    def get_profile(self):
        p = Profile()
        check(lib().mispec_fac_get_profile(self.h, C.byref(p)))
        return p.as_dict()

    def exchange_info(self):
        halo, cnt = C.c_int(0), C.c_int64(0)
        check(lib().mispec_fac_exchange_info(self.h, C.byref(halo), C.byref(cnt)))
        return bool(halo.value), int(cnt.value)

    def __del__(self):
        try:
            lib().mispec_fac_destroy(self.h)
        except Exception:
            pass


def tridiag_qr(T, shift, ctx=None):
    """TridiagQR on the device (single-workgroup LDS kernel): returns (Q, Q'TQ), both (n, n)."""
    ctx = ctx or default_context()
    T = np.asfortranarray(T, dtype=np.float64)
    n = T.shape[0]
    Q = np.empty((n, n), order="F")
    D = np.empty((n, n), order="F")
    check(lib().mispec_tridiag_qr(ctx.h, n, _dp(T), float(shift), _dp(Q), _dp(D)))
    return Q, D


RESTART_SWEEP_VARIANTS = {"host-serial": 0, "host-pipelined": 1, "device-pipelined": 2, "device-wavefront": 3}


def restart_sweeps(diag, subd, shifts, variant="host-pipelined", reps=1, ctx=None):
    """All shifted QR sweeps of one restart on the tridiagonal (diag[n], subd[n-1]) — HermEigsBase.h:124-147 — by variant
    (RESTART_SWEEP_VARIANTS; mispec_restart_sweeps).  Returns (diag', subd', Q, microseconds per call); the host variants and
    the pipelined kernel agree bit for bit.  The host variants need no device."""
    v = RESTART_SWEEP_VARIANTS[variant]
    d, e, mu = _f64(diag), _f64(subd), _f64(shifts)
    n = d.size
    h = None
    if v >= 2:
        h = (ctx or default_context()).h
    do, eo, Q = np.empty(n), np.empty(max(n - 1, 0)), np.empty((n, n), order="F")
    us = C.c_double(0.0)
    check(lib().mispec_restart_sweeps(h, n, _dp(d), _dp(e), _dp(mu), mu.size, v, int(reps), _dp(do), _dp(eo), _dp(Q), C.byref(us)))
    return do, eo, Q, us.value


def tridiag_eigen(T, ctx=None):
    """TridiagEigen on the device: returns (eigenvalues, eigenvectors)."""
    ctx = ctx or default_context()
    T = np.asfortranarray(T, dtype=np.float64)
    n = T.shape[0]
    ev = np.empty(n)
    U = np.empty((n, n), order="F")
    check(lib().mispec_tridiag_eigen(ctx.h, n, _dp(T), _dp(ev), _dp(U)))
    return ev, U
