"""Validation metrics on the device: ``torch.ops.vmambair.image_metrics`` on ``oss_metrics.hip`` -- the mean squared error behind
the reference's ``calculate_psnr`` (Deraining/basicsr/metrics/psnr_ssim.py:9-63) and the mean SSIM of ``_ssim`` (:66-99;
Deraining/Deraining/utils.py:31-78) or ``_ssim_cly`` (:184-222) of a batch of image pairs in one call, with ``tensor2img``'s
quantisation (SRGAN/VmambaIR/utils/img_util.py:68-92) and ``to_y_channel`` (metrics/metric_util.py:34-47) applied on load.
``vmambair_amd.metrics`` is the public face (PSNR in dB, the reference's signatures); flags as in include/vmambair_oss.h.
``torch.ops.vmambair.niqe_features`` on ``oss_niqe.hip``: the per-block features of the reference's no-reference metric ``niqe``
(Deraining/basicsr/metrics/niqe.py:10-140) of a batch of images in one launch, with the same load."""
from __future__ import annotations

import torch

from .. import _capi
from ._common import _DT, _LIB, _check

QUANTISE, Y, REPLICATE = _capi.METRIC_QUANTISE, _capi.METRIC_Y, _capi.METRIC_REPLICATE


def image_metrics_ok(a: torch.Tensor, crop_border: int, flags: int) -> bool:
    """whether ``image_metrics`` takes this (batch, 1 | 3, H, W) tensor with these flags (a host query of the library)"""
    if not (a.is_cuda and a.dim() == 4 and a.dtype in _DT and a.numel()):
        return False
    return bool(_capi.load().oss_image_metrics_ok(_DT[a.dtype], a.shape[1], a.shape[2], a.shape[3], int(crop_border), int(flags)))


def _rows(t: torch.Tensor) -> torch.Tensor:
    return t if t.stride(3) == 1 else t.contiguous()   # any batch / channel / row stride: cropped views are read in place


def image_metrics(a: torch.Tensor, b: torch.Tensor, crop_border: int, flags: int) -> torch.Tensor:
    """a, b (batch, 1 | 3, H, W) RGB, fp32 / fp16 / bf16 -> (batch, 2) float64 on the device: [mean squared error over the cropped
    planes, mean SSIM].  Runs on the current stream, no host synchronisation, bit-reproducible; the scratch comes from the caching
    allocator, so the call can be captured into a graph."""
    _check(a.is_cuda and b.is_cuda, "image_metrics: a and b must be CUDA/HIP tensors")
    _check(a.dim() == 4 and a.shape == b.shape and a.dtype == b.dtype and a.device == b.device,
           "image_metrics: a and b must be (batch, channels, H, W) tensors of one shape, dtype and device")
    _check(a.dtype in _DT, "image_metrics: fp32, fp16 or bf16 tensors")
    B, C, H, W = a.shape
    lib = _capi.load()
    _check(B > 0 and lib.oss_image_metrics_ok(_DT[a.dtype], C, H, W, int(crop_border), int(flags)),
           f"image_metrics: shape {tuple(a.shape)} with crop_border {crop_border} and flags {flags} is not supported (1 or 3 channels, "
           "Y needs 3, crop_border under half a side, valid borders need an 11 x 11 cropped plane)")
    a, b = _rows(a.detach()), _rows(b.detach())
    out = torch.empty((B, 2), dtype=torch.float64, device=a.device)
    part = torch.empty(int(lib.oss_image_metrics_partial_doubles(B, C, H, W, int(crop_border))), dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        _capi.check(lib.oss_image_metrics(_DT[a.dtype], a.data_ptr(), b.data_ptr(), out.data_ptr(), part.data_ptr(), B, C, H, W,
                                          a.stride(0), a.stride(1), a.stride(2), b.stride(0), b.stride(1), b.stride(2),
                                          int(crop_border), int(flags), torch.cuda.current_stream().cuda_stream), "oss_image_metrics")
    return out


def niqe_features_ok(a: torch.Tensor, crop_border: int, flags: int) -> bool:
    """whether ``niqe_features`` takes this (batch, 1 | 3, H, W) tensor with these flags (a host query of the library)"""
    if not (a.is_cuda and a.dim() == 4 and a.dtype in _DT and a.numel()):
        return False
    return bool(_capi.load().oss_niqe_features_ok(a.shape[1], a.shape[2], a.shape[3], int(crop_border), int(flags), _DT[a.dtype]))


def niqe_features(a: torch.Tensor, tables: torch.Tensor, window: torch.Tensor, crop_border: int, flags: int) -> torch.Tensor:
    """a (batch, 1 | 3, H, W) RGB, fp32 / fp16 / bf16 -> (batch, blocks, 36) float64 on the device: the features of the reference's
    ``niqe`` (niqe.py:101-140) for every 96 x 96 block of the cropped plane, blocks in the reference's order.  ``tables``: the
    (4, 9801) float64 tensor of ``metrics.NiqeModel`` on ``a``'s device; ``window``: its 7 x 7 float64 window on the HOST (it
    travels in the kernel's arguments).  One launch on the current stream, no host synchronisation, no scratch, bit-reproducible;
    the call can be captured into a graph."""
    _check(a.is_cuda and tables.is_cuda and tables.device == a.device, "niqe_features: a and tables must be CUDA/HIP tensors on one device")
    _check(a.dim() == 4 and a.dtype in _DT, "niqe_features: a must be a (batch, channels, H, W) fp32, fp16 or bf16 tensor")
    _check(tables.dtype == torch.float64 and tuple(tables.shape) == (4, _capi.NIQE_GRID) and tables.is_contiguous(),
           f"niqe_features: tables must be a contiguous (4, {_capi.NIQE_GRID}) float64 tensor (metrics.NiqeModel.device_tables)")
    _check(not window.is_cuda and window.dtype == torch.float64 and tuple(window.shape) == (7, 7),
           "niqe_features: window must be a 7 x 7 float64 tensor on the host")
    B, C, H, W = a.shape
    lib = _capi.load()
    _check(B > 0 and lib.oss_niqe_features_ok(C, H, W, int(crop_border), int(flags), _DT[a.dtype]),
           f"niqe_features: shape {tuple(a.shape)} with crop_border {crop_border} and flags {flags} is not supported (1 channel, or 3 "
           "with the Y flag; the cropped plane holds a 96 x 96 block)")
    a, window = _rows(a.detach()), window.contiguous()
    blocks = ((H - 2 * int(crop_border)) // _capi.NIQE_BLOCK) * ((W - 2 * int(crop_border)) // _capi.NIQE_BLOCK)
    out = torch.empty((B, blocks, _capi.NIQE_FEATURES), dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        _capi.check(lib.oss_niqe_features(_DT[a.dtype], a.data_ptr(), tables.data_ptr(), window.data_ptr(), out.data_ptr(), B, C, H, W,
                                          a.stride(0), a.stride(1), a.stride(2), int(crop_border), int(flags),
                                          torch.cuda.current_stream().cuda_stream), "oss_niqe_features")
    return out


_LIB.define("image_metrics(Tensor a, Tensor b, int crop_border, int flags) -> Tensor")
_LIB.impl("image_metrics", image_metrics, "CUDA")
_LIB.define("niqe_features(Tensor a, Tensor tables, Tensor window, int crop_border, int flags) -> Tensor")
_LIB.impl("niqe_features", niqe_features, "CUDA")
