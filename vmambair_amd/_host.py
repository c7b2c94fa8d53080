"""Loader of the compiled torch boundary (``lib/libvmambair_torch.so``, source ``csrc_host/oss_torch_host.cpp``): the C++
``TORCH_LIBRARY`` counterpart of the reference's pybind layer (cus/selective_scan.cpp:157-349) for the scan ops.

``ops()`` loads the library on first use and returns ``torch.ops.vmambair_host`` (``scan_fwd`` / ``scan_bwd``), the only host
path of ``ops/scan.py``.  As in ``_capi.load()``, a missing library or one built against another revision of
include/vmambair_oss.h is a hard error: no fallback path exists."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import _build

_ops = None


def abi_mismatch() -> Optional[str]:
    """None when ``libvmambair_torch.so`` was compiled against the same revision of include/vmambair_oss.h as the loaded
    ``libvmambair_oss.so`` (OSS_ABI_VERSION and the sizeof of the two structs it fills and passes BY POINTER), else the reason.
    A host library left over from a partial rebuild would hand the kernels misread pointers: it is never used."""
    from . import _capi
    lib = _capi.load()   # libvmambair_oss.so first: the host library's DT_NEEDED entry then resolves to the loaded image
    try:
        h = C.CDLL(_build.HOST_LIB)
        h.vmambair_host_abi_version.restype = C.c_int
        h.vmambair_host_struct_bytes.restype = C.c_size_t
        h.vmambair_host_struct_bytes.argtypes = [C.c_int]
    except (OSError, AttributeError) as e:
        return f"{_build.HOST_LIB} cannot be loaded or predates the ABI guard ({e})"
    theirs = (h.vmambair_host_abi_version(), h.vmambair_host_struct_bytes(0), h.vmambair_host_struct_bytes(1))
    core = (lib.oss_abi_version(), lib.oss_abi_struct_bytes(0), lib.oss_abi_struct_bytes(1))
    if theirs != core:
        return (f"{_build.HOST_LIB} was compiled against another revision of include/vmambair_oss.h than {_capi.lib_path()} "
                f"(ABI version, sizeof fwd / bwd params: host {theirs}, core {core}); rebuild with __graft_entry__.build()")
    return None


def ops():
    """``torch.ops.vmambair_host``; raises ``RuntimeError`` when the library is missing or stale"""
    global _ops
    if _ops is None:
        if not os.path.exists(_build.HOST_LIB):
            raise RuntimeError(
                f"{_build.HOST_LIB} is missing: the compiled torch boundary has not been built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'`). There is no fallback path.")
        reason = abi_mismatch()
        if reason is not None:
            raise RuntimeError(reason)
        torch.ops.load_library(_build.HOST_LIB)
        _ops = torch.ops.vmambair_host
    return _ops


def mode() -> str:
    """``"c++"`` once the library has loaded (the build driver asserts it); raises like ``ops()`` otherwise"""
    return ops() and "c++"
