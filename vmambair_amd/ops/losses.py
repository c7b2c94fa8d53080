"""Pixel losses on the device: ``torch.ops.vmambair.pixel_loss_fwd`` / ``pixel_loss_bwd`` on ``oss_pixel_loss.hip`` -- the
reference's ``L1Loss``, ``MSELoss``, ``PSNRLoss`` (with ``toY``) and ``CharbonnierLoss`` (Deraining/basicsr/models/losses/losses.py:
26-122, losses/loss_util.py:25-95) with their gradient w.r.t. ``pred``.  ``vmambair_amd.losses`` is the public face (the reference's
modules); kinds and flags as in include/vmambair_oss.h."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import _capi
from ._common import _DT, _LIB, _check, _ptr

L1, MSE, CHARBONNIER, PSNR = (_capi.LOSS[k] for k in ("L1", "MSE", "CHARBONNIER", "PSNR"))
SUM, TOY, WEIGHT, WEIGHT_1CH = (_capi.LOSS[k] for k in ("SUM", "TOY", "WEIGHT", "WEIGHT_1CH"))


def weight_flag(pred: torch.Tensor, weight: Optional[torch.Tensor]) -> int:
    """the flag that names ``weight``'s shape: (N, C, H, W) or (N, 1, H, W) against a (N, C, H, W) ``pred``; 0 without a weight"""
    if weight is None:
        return 0
    return WEIGHT if weight.shape == pred.shape else WEIGHT_1CH


def pixel_loss_ok(pred: torch.Tensor, target: torch.Tensor, kind: int, flags: int) -> bool:
    """whether the kernels take these (N, C, H, W) tensors with this kind and these flags (a host query of the library)"""
    if not (pred.is_cuda and target.is_cuda and pred.dim() == 4 and pred.shape == target.shape and pred.numel()
            and pred.dtype in _DT and target.dtype in _DT):
        return False
    N, C, H, W = pred.shape
    return _capi.load().oss_pixel_loss_partial_doubles(int(kind), int(flags), _DT[pred.dtype], _DT[target.dtype], N, C, H * W) > 0


def _checked(name, pred, target, weight, kind, flags):
    _check(pred.is_cuda and target.is_cuda and (weight is None or weight.is_cuda), f"{name}: pred, target and weight must be CUDA/HIP tensors")
    _check(pred.dim() == 4 and pred.shape == target.shape and pred.device == target.device,
           f"{name}: pred and target must be (N, C, H, W) tensors of one shape and device")
    _check(pred.dtype in _DT and target.dtype in _DT, f"{name}: fp32, fp16 or bf16 tensors")
    _check(pred.is_contiguous() and target.is_contiguous(), f"{name}: pred and target must be contiguous")
    N, C, H, W = pred.shape
    wbits = flags & (WEIGHT | WEIGHT_1CH)
    _check((weight is not None) == (wbits != 0), f"{name}: a weight goes with exactly one of the two weight flags")
    if weight is not None:
        _check(weight.dtype == torch.float32, f"{name}: the weight must be fp32")
        _check(weight.device == pred.device and weight.is_contiguous() and
               tuple(weight.shape) == ((N, C, H, W) if wbits == WEIGHT else (N, 1, H, W)),
               f"{name}: the weight must be a contiguous (N, C, H, W) tensor (WEIGHT) or (N, 1, H, W) tensor (WEIGHT_1CH) on pred's device")
    lib = _capi.load()
    n_part = int(lib.oss_pixel_loss_partial_doubles(int(kind), int(flags), _DT[pred.dtype], _DT[target.dtype], N, C, H * W))
    _check(n_part > 0, f"{name}: kind {kind} with flags {flags} on {tuple(pred.shape)} {pred.dtype} / {target.dtype} is not supported (target: "
           "fp32 or pred's type; weight and sum: L1 and MSE only; toY: PSNR with 3 channels)")
    return lib, n_part, (N, C, H * W)


def pixel_loss_fwd(pred: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor], kind: int, flags: int, loss_weight: float,
                   eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (loss: fp32 scalar, stats: fp64 vector for ``pixel_loss_bwd``), both on the device.  Two launches on the current stream,
    no host synchronisation, bit-reproducible; the scratch comes from the caching allocator, so the call can be captured."""
    lib, n_part, (N, C, P) = _checked("pixel_loss_fwd", pred, target, weight, kind, flags)
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    stats = torch.empty(int(lib.oss_pixel_loss_stat_doubles(int(kind), int(flags), N, C, P)), dtype=torch.float64, device=pred.device)
    part = torch.empty(n_part, dtype=torch.float64, device=pred.device)
    with torch.cuda.device(pred.device):
        _capi.check(lib.oss_pixel_loss_fwd(int(kind), int(flags), _DT[pred.dtype], _DT[target.dtype], pred.data_ptr(), target.data_ptr(),
                                           _ptr(weight), loss.data_ptr(), stats.data_ptr(), part.data_ptr(), N, C, P, float(loss_weight),
                                           float(eps), torch.cuda.current_stream().cuda_stream), "oss_pixel_loss_fwd")
    return loss, stats


def pixel_loss_bwd(pred: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor], stats: torch.Tensor, grad_output: torch.Tensor,
                   kind: int, flags: int, loss_weight: float, eps: float) -> torch.Tensor:
    """-> d loss / d pred * grad_output in pred's dtype: one launch on the current stream; ``grad_output`` is read on the device"""
    lib, _, (N, C, P) = _checked("pixel_loss_bwd", pred, target, weight, kind, flags)
    _check(stats.is_cuda and stats.dtype == torch.float64 and stats.is_contiguous() and
           stats.numel() == int(lib.oss_pixel_loss_stat_doubles(int(kind), int(flags), N, C, P)),
           "pixel_loss_bwd: stats must be the fp64 vector pixel_loss_fwd returned for the same arguments")
    _check(grad_output.is_cuda and grad_output.dtype == torch.float32 and grad_output.numel() == 1,
           "pixel_loss_bwd: grad_output must be one fp32 scalar on the device")
    dpred = torch.empty_like(pred)
    with torch.cuda.device(pred.device):
        _capi.check(lib.oss_pixel_loss_bwd(int(kind), int(flags), _DT[pred.dtype], _DT[target.dtype], pred.data_ptr(), target.data_ptr(),
                                           _ptr(weight), stats.data_ptr(), grad_output.data_ptr(), dpred.data_ptr(), N, C, P,
                                           float(loss_weight), float(eps), torch.cuda.current_stream().cuda_stream), "oss_pixel_loss_bwd")
    return dpred


_LIB.define("pixel_loss_fwd(Tensor pred, Tensor target, Tensor? weight, int kind, int flags, float loss_weight, float eps) -> (Tensor, Tensor)")
_LIB.impl("pixel_loss_fwd", pixel_loss_fwd, "CUDA")
_LIB.define("pixel_loss_bwd(Tensor pred, Tensor target, Tensor? weight, Tensor stats, Tensor grad_output, int kind, int flags, "
            "float loss_weight, float eps) -> Tensor")
_LIB.impl("pixel_loss_bwd", pixel_loss_bwd, "CUDA")
