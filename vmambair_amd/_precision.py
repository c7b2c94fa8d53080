"""Precision mode of the fp32 GEMM-shaped products (1x1 convolutions, x_proj / dt_proj and their gradients).

``"highest"`` (default): exact fp32 multiplies and adds on ``v_mfma_f32_32x32x2_f32`` (csrc/oss_conv1x1_f32.hip).
``"high"``: the same products on ``v_mfma_f32_32x32x16_bf16`` with every fp32 operand taken as the sum of two bfloat16 numbers
(csrc/oss_conv1x1_f32x3.h; include/vmambair_oss.h: ``OSS_F32_BF16X3``): about 16 mantissa bits per operand,
``|y_high - y| <= (3 * 2**-16 + (K + 2) * 2**-23) * sum_k |w_k||x_k|``.  gfx950 has no TF32 / xf32 matrix instruction; this is the
substitute ``torch.set_float32_matmul_precision("high")`` documents.  The project keeps its own switch and does NOT follow torch's:
no existing run changes behaviour.

The mode is read when an op RUNS and travels with the call into the library (a per-call selector, no process-global state in the
library), so a hipGraph captured under a mode keeps that mode on every replay, whatever the mode is at replay time.
Only float32 tensors are affected; 16-bit tensors and every other op are untouched.
"""
from __future__ import annotations

import contextlib
import os

import torch

from . import _capi

MODES = ("highest", "high")
ENV = "VMAMBAIR_FP32_MATMUL"


def _checked(mode: str, what: str) -> str:
    if mode not in MODES:
        raise ValueError(f"{what}: expected one of {MODES}, got {mode!r}")
    return mode


_mode = _checked(os.environ.get(ENV, "highest"), ENV)


def set_float32_matmul_precision(mode: str) -> None:
    """``"highest"``: exact fp32 matrix-core products (default); ``"high"``: split-bf16 products (see the module docstring).
    Takes effect for ops that run afterwards; a hipGraph captured earlier replays with the mode it was captured under."""
    global _mode
    _mode = _checked(mode, "set_float32_matmul_precision")


def get_float32_matmul_precision() -> str:
    return _mode


@contextlib.contextmanager
def float32_matmul_precision(mode: str):
    """``with float32_matmul_precision("high"): ...`` -- restores the previous mode on exit, on exceptions too."""
    prev = get_float32_matmul_precision()
    set_float32_matmul_precision(mode)
    try:
        yield
    finally:
        set_float32_matmul_precision(prev)


def io_code(dtype: torch.dtype) -> int:
    """the ``oss_dtype`` the six GEMM-shaped entry points get for a tensor type under the current mode"""
    if dtype == torch.float32 and _mode == "high":
        return _capi.OSS_F32_BF16X3
    return {torch.float32: _capi.OSS_F32, torch.float16: _capi.OSS_F16, torch.bfloat16: _capi.OSS_BF16}[dtype]
