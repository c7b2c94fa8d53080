"""vmambair_amd -- MI355X (gfx950) native Omni-Selective-Scan core for VmambaIR.

Only the hot path of the reference is here: the selective-scan forward /
backward as hand-written HIP behind a C ABI (``include/vmambair_oss.h``), the torch-facing
boundary the reference archs import (``selective_scan_cuda_core``), and the host-side mirror of
the OSS block (``SS2D_1`` / ``MamberBlock``) and the UNets that stack it.

There is no CPU implementation of the scan in this package on purpose: every op raises if the
HIP library is missing or the tensors are not on a GPU.
"""
from . import _capi  # noqa: F401  (loads the C-ABI library lazily; import never needs a GPU)
from ._precision import (float32_matmul_precision, get_float32_matmul_precision,  # noqa: F401
                         set_float32_matmul_precision)
from .data import DevicePairPool, ProgressiveSchedule  # noqa: F401
from . import degradations  # noqa: F401  filter2D, USMSharp and the training pair pool of the RealSR degradation pipeline
from . import losses  # noqa: F401  the reference's pixel losses (L1, MSE, PSNR, Charbonnier) on the device
from .ops import selective_scan_fwd, selective_scan_bwd, scan_chunk  # noqa: F401
from .selective_scan import SelectiveScanFn, selective_scan_fn  # noqa: F401

__all__ = ["selective_scan_fwd", "selective_scan_bwd", "scan_chunk", "SelectiveScanFn", "selective_scan_fn",
           "set_float32_matmul_precision", "get_float32_matmul_precision", "float32_matmul_precision", "DevicePairPool", "ProgressiveSchedule", "losses",
           "degradations"]
