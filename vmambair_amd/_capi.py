"""ctypes binding of include/vmambair_oss.h (the C ABI of the HIP library).

Nothing about the ABI is written down here: the constants, the structures and every entry point's ``restype`` / ``argtypes`` are
read from the header (``_cheader.py``), so a new entry point needs no line in this file.  The library is loaded on first use; a
missing library is a hard error (no fallback path exists).
"""
from __future__ import annotations

import ctypes as C
import os

from . import _build, _cheader

_HDR = _cheader.read(_build.HEADER)
_K = _HDR.constants

OSS_F32, OSS_F16, OSS_BF16 = _K["OSS_F32"], _K["OSS_F16"], _K["OSS_BF16"]
#: per-call selector of the six GEMM-shaped entry points: fp32 tensors, products on split bf16
OSS_F32_BF16X3 = _K["OSS_F32_BF16X3"]
F32_MODE_EXACT, F32_MODE_BF16X3 = 1, 2   # bits of oss_f32_matmul_modes() (the header names none)
METRIC_QUANTISE, METRIC_Y, METRIC_REPLICATE = _K["OSS_METRIC_QUANTISE"], _K["OSS_METRIC_Y"], _K["OSS_METRIC_REPLICATE"]   # flags of oss_image_metrics
NIQE_BLOCK, NIQE_FEATURES, NIQE_GRID = _K["OSS_NIQE_BLOCK"], _K["OSS_NIQE_FEATURES"], _K["OSS_NIQE_GRID"]   # oss_niqe_features
LOSS = {k[len("OSS_LOSS_"):]: v for k, v in _K.items() if k.startswith("OSS_LOSS_")}   # kinds and flags of oss_pixel_loss_fwd / _bwd
FILTER = {k[len("OSS_FILTER"):].lstrip("_"): v for k, v in _K.items() if k.startswith("OSS_FILTER")}   # epilogues and tap limits of oss_filter2d / _sep
JPEG = {k[len("OSS_JPEG_"):]: v for k, v in _K.items() if k.startswith("OSS_JPEG_")}   # flags of oss_jpeg_roundtrip
NOISE = {k[len("OSS_NOISE_"):]: v for k, v in _K.items() if k.startswith("OSS_NOISE_")}   # flags and sampler limits of oss_noise_gaussian / _poisson
PAIRS_HFLIP, PAIRS_ROT = _K["OSS_PAIRS_HFLIP"], _K["OSS_PAIRS_ROT"]   # flags of oss_pairs_draw
FEATURE_FUSED_DT, FEATURE_LANE_STATES = _K["OSS_FEATURE_FUSED_DT"], _K["OSS_FEATURE_LANE_STATES"]   # oss_scan_features()
ADAM_CHUNK = _K["OSS_ADAM_CHUNK"]
#: OSS_ABI_VERSION of the header in the tree; load() refuses a library built from another revision
ABI_VERSION = _K["OSS_ABI_VERSION"]

ERRORS = {_K[name]: f"{name}: {text}" for name, text in {
    "OSS_ERR_NULL": "a required pointer is NULL",
    "OSS_ERR_SHAPE": "invalid batch/dim/seqlen/dstate/n_groups",
    "OSS_ERR_DSTATE": "selective_scan only supports state dimension <= 256",
    "OSS_ERR_WORKSPACE": "workspace missing or too small",
}.items()}

ScanFwdParams = _HDR.structs["oss_scan_fwd_params"]
ScanBwdParams = _HDR.structs["oss_scan_bwd_params"]
ChanParams = _HDR.structs["oss_chan_params"]
AdamChunk = _HDR.structs["oss_adam_chunk"]   # fields in header order: optim.py builds rows positionally
SUM_CHUNK_BYTES = C.sizeof(_HDR.structs["oss_sum_chunk"])

#: every function the header declares
SYMBOLS = list(_HDR.prototypes)

_lib = None


def lib_path() -> str:
    # VMAMBAIR_LIB: a library built from another checkout (its own _build.build()), for A-B timing of two revisions
    return os.environ.get("VMAMBAIR_LIB") or _build.LIB_PATH


def load():
    """dlopen the in-tree library and give every declared entry point its prototype; raise loudly when it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: the HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'`). There is no fallback path.")
    lib = C.CDLL(path)
    if not hasattr(lib, "oss_abi_version"):
        raise RuntimeError(f"{path} predates the ABI guard of include/vmambair_oss.h: rebuild it (__graft_entry__.build())")
    for name, (restype, argtypes) in _HDR.prototypes.items():
        if not hasattr(lib, name):
            raise RuntimeError(f"{path} does not export {name}, which include/vmambair_oss.h declares: rebuild it "
                               "(__graft_entry__.build())")
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    # the structs cross the boundary by pointer: a library built from another revision of the header would misread them
    mine = (ABI_VERSION, C.sizeof(ScanFwdParams), C.sizeof(ScanBwdParams), C.sizeof(ChanParams))
    theirs = (lib.oss_abi_version(), *(lib.oss_abi_struct_bytes(i) for i in range(3)))
    if mine != theirs:
        raise RuntimeError(f"{path} was built from another revision of include/vmambair_oss.h than the one in this tree "
                           f"(version, sizeof fwd / bwd / chan params): library {theirs}, header {mine}; "
                           "rebuild with __graft_entry__.build()")
    _lib = lib
    return lib


def has_feature(bit: int) -> bool:
    """scan forms the loaded library reports (include/vmambair_oss.h: oss_scan_features)"""
    return bool(load().oss_scan_features() & bit)


def require_feature(bit: int, what: str) -> None:
    if not has_feature(bit):
        name = {FEATURE_FUSED_DT: "fused_dt", FEATURE_LANE_STATES: "lane_states"}[bit]
        raise RuntimeError(f"{what}: {lib_path()} does not report the scan form '{name}' "
                           f"(oss_scan_features; every library built from this tree has both)")


def check(rc: int, what: str) -> None:
    if rc == 0:
        return
    if rc < 0:
        raise RuntimeError(f"{what}: {ERRORS.get(rc, rc)}")
    raise RuntimeError(f"{what}: HIP error {rc}")
