"""The parts of the ingest from device memory that need no GPU: the argument checks of the three entry points run before anything
touches a device, from_torch refuses a host tensor before it calls the library, and the package still imports without torch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import spectra_amd as sa
from spectra_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOME = 0x1000  # an address that is not NULL; a refused call never follows it


def _call(name, ctx, outer, inner, val, out=True, extra=SOME):
    lib = sa.lib()
    h, nnz = C.c_void_p(), C.c_int64(0)
    if name == "mispec_csr_from_device":
        return lib.mispec_csr_from_device(ctx, 4, 4, outer, inner, 4, val, 1, C.byref(h) if out else None)
    if name == "mispec_csr_from_triangle_device":
        return lib.mispec_csr_from_triangle_device(ctx, 4, outer, inner, 4, val, b"L", 0, C.byref(h) if out else None)
    return lib.mispec_mirror_triangle_device(ctx, 4, outer, inner, 4, val, b"L", 0, extra, extra, extra, 16, C.byref(nnz) if out else None)


@pytest.mark.parametrize("name", ["mispec_csr_from_device", "mispec_csr_from_triangle_device", "mispec_mirror_triangle_device"])
def test_null_arguments_are_refused_before_a_device_is_touched(name):
    lib = sa.lib()
    cases = [(None, SOME, SOME, SOME, True), (SOME, None, SOME, SOME, True), (SOME, SOME, None, SOME, True),
             (SOME, SOME, SOME, None, True), (SOME, SOME, SOME, SOME, False)]
    for ctx, outer, inner, val, out in cases:
        assert _call(name, ctx, outer, inner, val, out) == _capi.MISPEC_EINVAL, (ctx, outer, inner, val, out)
        msg = lib.mispec_last_error().decode()
        assert name in msg and "NULL argument" in msg, msg
    if name == "mispec_mirror_triangle_device":
        assert _call(name, SOME, SOME, SOME, SOME, True, extra=None) == _capi.MISPEC_EINVAL
        assert "NULL argument" in lib.mispec_last_error().decode()
    with pytest.raises(ValueError, match="NULL argument"):
        _capi.check(_call(name, None, SOME, SOME, SOME))


def _cpu_csr():
    import torch

    return torch.sparse_csr_tensor(torch.tensor([0, 1, 2]), torch.tensor([0, 1]), torch.tensor([1.0, 2.0], dtype=torch.float64), size=(2, 2))


@pytest.mark.filterwarnings("ignore:Sparse CSR tensor support is in beta")
def test_from_torch_refuses_a_host_tensor_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(sa, "lib", no_library)
    monkeypatch.setattr(sa, "default_context", no_library)
    t = _cpu_csr()
    for make in (lambda: sa.SparseSymMatProd.from_torch(t), lambda: sa.SparseGenMatProd.from_torch(t),
                 lambda: sa.mirror_triangle_device(t, "L")):
        with pytest.raises(ValueError, match=r"torch\.sparse_csr or torch\.sparse_csc tensor on the context's GPU.* got a tensor on cpu"):
            make()
    with pytest.raises(ValueError, match="got layout torch.sparse_coo"):
        sa.SparseSymMatProd.from_torch(t.to_sparse_coo())
    with pytest.raises(ValueError, match="got layout torch.strided"):
        sa.SparseGenMatProd.from_torch(t.to_dense())
    with pytest.raises(TypeError, match="got ndarray"):
        sa.SparseGenMatProd.from_torch(np.eye(2))


def test_the_package_imports_without_torch():
    code = ("import sys; sys.path.insert(0, %r); sys.modules['torch'] = None\n"
            "import spectra_amd as sa\n"
            "assert hasattr(sa.SparseSymMatProd, 'from_torch') and hasattr(sa.SparseGenMatProd, 'from_device_pointers')\n"
            "assert 'torch' not in [m for m in sys.modules if sys.modules[m] is not None]\n"
            "try:\n"
            "    sa.SparseSymMatProd.from_torch(object())\n"
            "except ImportError:\n"
            "    print('import spectra_amd: ok; from_torch needs torch')\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and "from_torch needs torch" in r.stdout, r.stderr
