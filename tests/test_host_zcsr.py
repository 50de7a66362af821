"""The host ingest of the complex Hermitian sparse operator (zcsr_mirror, spectra_amd/csrc/zcsr.hpp — the source
mispec_zcsr_upload runs before the device sees anything) behind tests/cpp/zcsr_mirror_host_capi.cpp, against a dense mirror built
here entry by entry.  No GPU.  scipy sums duplicates and sorts indices before the GPU tests hand the library a matrix, so the
conditions below reach the ingest only here: duplicates (summed in input order, so the comparison is exact), unsorted inner indices,
garbage in the triangle that is not read, an imaginary diagonal, empty rows, both index widths, both storage orders, both triangles,
n = 0 and n = 1, and every refusal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISPEC_EINVAL = -1


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("zcsr") / "libzcsr_mirror_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "spectra_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "zcsr_mirror_host_capi.cpp"), "-o", so])
    lib = C.CDLL(so)
    vp, i64 = C.c_void_p, C.c_int64
    lib.zcsr_mirror_host.argtypes = [i64, vp, vp, C.c_int, vp, C.c_int, C.c_char, vp, vp, vp, i64, C.POINTER(i64)]
    lib.zcsr_mirror_host.restype = C.c_int
    return lib


def compress(n, entries, itype):
    """entries: (outer slot, inner index, value) in input order -> outer / inner / values; the order within a slot is kept, so the
    inner indices stay unsorted and duplicates stay where they were."""
    outer = np.zeros(n + 1, dtype=itype)
    inner, vals = [], []
    for o in range(n):
        for (eo, ei, v) in entries:
            if eo == o:
                inner.append(ei)
                vals.append(v)
        outer[o + 1] = len(inner)
    return outer, np.array(inner, dtype=itype), np.array(vals, dtype=np.complex128)


def dense_mirror(n, entries, row_major, uplo):
    """What selfadjointView<uplo> reads, position by position in input order: {(i, j): value} of the full matrix."""
    full = {}

    def add(i, j, v):
        full[(i, j)] = full[(i, j)] + v if (i, j) in full else v

    for o in range(n):
        for (eo, ei, v) in entries:
            if eo != o:
                continue
            i, j = (o, ei) if row_major else (ei, o)
            if not (i >= j if uplo == "L" else i <= j):
                continue
            if i == j:
                add(i, i, complex(v.real, 0.0))
            else:
                add(i, j, v)
                add(j, i, v.conjugate())
    return full


def run(lib, n, outer, inner, vals, row_major, uplo, n_arg=None):
    cap = 2 * len(inner) + 1
    rowptr = np.full(n + 1, -7, dtype=np.int32)
    col = np.full(cap, -7, dtype=np.int32)
    val = np.zeros(cap, dtype=np.complex128)
    nnz = C.c_int64(-1)
    rc = lib.zcsr_mirror_host(n if n_arg is None else n_arg, outer.ctypes.data, inner.ctypes.data, outer.dtype.itemsize,
                              vals.ctypes.data, int(row_major), uplo.encode(), rowptr.ctypes.data, col.ctypes.data, val.ctypes.data,
                              cap, C.byref(nnz))
    return rc, rowptr, col[: max(nnz.value, 0)], val[: max(nnz.value, 0)]


def check(lib, n, entries, row_major, uplo, itype):
    outer, inner, vals = compress(n, entries, itype)
    rc, rowptr, col, val = run(lib, n, outer, inner, vals, row_major, uplo)
    assert rc == 0
    full = dense_mirror(n, entries, row_major, uplo)
    # one stored entry per distinct position (an entry that sums to zero stays), rows in order, columns strictly ascending
    assert rowptr[0] == 0 and rowptr[n] == len(full) == len(col)
    assert np.all(np.diff(rowptr) >= 0)
    got = {}
    for r in range(n):
        c = col[rowptr[r]: rowptr[r + 1]]
        assert np.all(np.diff(c) > 0) and (c.size == 0 or (c[0] >= 0 and c[-1] < n))
        for k in range(rowptr[r], rowptr[r + 1]):
            got[(r, int(col[k]))] = complex(val[k])
    assert got.keys() == full.keys()
    for pos, v in full.items():  # sums in input order: the same additions, so exactly the same bits
        assert got[pos] == v, (pos, got[pos], v)
        if pos[0] == pos[1]:
            assert got[pos].imag == 0.0
        else:
            assert got[(pos[1], pos[0])] == v.conjugate()
    return rowptr, col, val


def random_entries(n, count, seed, empty=()):
    """`count` entries anywhere in the square (so: both triangles, repeated positions, repeated diagonals with imaginary parts),
    in random order, no entry in the outer slots `empty`."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        o, i = int(rng.integers(n)), int(rng.integers(n))
        if o in empty:
            continue
        out.append((o, i, complex(rng.uniform(-1, 1), rng.uniform(-1, 1))))
    return out


@pytest.mark.parametrize("itype", [np.int32, np.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("row_major", [True, False], ids=["csr", "csc"])
def test_mirror_matches_a_dense_mirror(mirror, row_major, uplo, itype):
    # n = 7 with 80 entries: every position of the triangle several times over; n = 40: mostly single entries, empty rows
    for n, count, seed, empty in ((7, 80, 1, ()), (7, 30, 2, (0, 3, 6)), (40, 300, 3, (0, 1, 17, 39)), (2, 9, 4, ())):
        entries = random_entries(n, count, seed, empty)
        dup = len(entries) - len({(o, i) for (o, i, _) in entries})
        assert dup > 0 and any(o == i and v.imag != 0 for (o, i, v) in entries)
        assert any(o < i for (o, i, _) in entries) and any(o > i for (o, i, _) in entries)
        check(mirror, n, entries, row_major, uplo, itype)


@pytest.mark.parametrize("row_major", [True, False], ids=["csr", "csc"])
def test_duplicates_after_an_empty_row_and_on_the_diagonal(mirror, row_major):
    """Slot 1 is empty and slot 2 opens with a position given twice; slot 0 holds its diagonal three times; slot 4's first sorted
    column (after the mirroring) equals the last column of the row stored before it."""
    a, b, c = 0.5 + 0.25j, -0.125 + 2j, 3 - 1j
    entries = [(0, 0, 1 + 2j), (0, 0, 3 - 1j), (0, 0, 0.5 + 7j),
               (2, 1, a), (2, 1, b), (2, 0, c), (2, 2, 9j), (2, 1, a),
               (3, 3, 2.0 + 0j), (4, 3, a), (4, 3, -a), (4, 4, 1 + 1j), (4, 4, 1 - 1j),
               (0, 4, 100 + 100j), (1 + 4, 5, -2 + 0j)]  # (0, 4): the unread triangle of "L" in CSR, the read one in CSC
    for uplo in ("L", "U"):
        rowptr, col, val = check(mirror, 6, entries, row_major, uplo, np.int32)
    # uplo = "L", read by rows (CSR) / uplo = "U", read by columns (CSC), spelt out
    rowptr, col, val = check(mirror, 6, entries, row_major, "L" if row_major else "U", np.int32)
    i, j = (2, 1) if row_major else (1, 2)
    row = slice(rowptr[i], rowptr[i + 1])
    assert val[row][list(col[row]).index(j)] == (a + b) + a
    assert val[rowptr[0]] == complex(1 + 3 + 0.5, 0.0) and col[rowptr[0]] == 0
    k = list(col[rowptr[4]: rowptr[5]]).index(3)
    assert val[rowptr[4] + k] == 0 and rowptr[5] - rowptr[4] == 2  # a - a is kept as a stored zero


def test_sizes_zero_and_one(mirror):
    for itype in (np.int32, np.int64):
        rc, rowptr, col, val = run(mirror, 0, np.zeros(1, dtype=itype), np.zeros(0, dtype=itype), np.zeros(0, dtype=np.complex128),
                                   True, "L")
        assert rc == 0 and list(rowptr) == [0] and col.size == 0
        check(mirror, 1, [], True, "U", itype)
        rowptr, col, val = check(mirror, 1, [(0, 0, 2 + 3j), (0, 0, -0.5 - 3j)], False, "L", itype)
        assert list(rowptr) == [0, 1] and list(col) == [0] and val[0] == 1.5


@pytest.mark.parametrize("itype", [np.int32, np.int64], ids=["int32", "int64"])
def test_refusals_return_the_invalid_argument_code(mirror, itype):
    n = 4
    entries = [(0, 0, 1 + 0j), (1, 0, 2 + 1j), (2, 1, 1j), (3, 3, 4 + 0j)]
    outer, inner, vals = compress(n, entries, itype)
    assert run(mirror, n, outer, inner, vals, True, "L")[0] == 0

    def rc(outer=outer, inner=inner, uplo="L", n_arg=None):
        return run(mirror, n, outer, inner, vals, True, uplo, n_arg)[0]

    assert rc(outer=outer + 1) == MISPEC_EINVAL                                  # outer does not start at 0
    assert rc(outer=np.array([0, 2, 1, 3, 4], dtype=itype)) == MISPEC_EINVAL      # outer decreases inside
    assert rc(outer=np.array([0, 1, 2, 3, -1], dtype=itype)) == MISPEC_EINVAL     # ... and over the whole array
    for bad in (-1, n, n + 5):
        for at in (0, 3):
            broken = inner.copy()
            broken[at] = bad
            assert rc(inner=broken) == MISPEC_EINVAL
    assert rc(uplo="X") == MISPEC_EINVAL
    # n > 2^31 - 1: refused before any array is read
    assert rc(n_arg=2**31) == MISPEC_EINVAL
    assert rc(n_arg=-1) == MISPEC_EINVAL
