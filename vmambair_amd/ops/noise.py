"""The two noise steps of the RealSR degradation on the device: ``torch.ops.vmambair.noise_gaussian`` / ``noise_poisson`` on
``oss_noise.hip`` -- ``random_add_gaussian_noise_pt`` / ``random_add_poisson_noise_pt`` of basicsr.data.degradations and their
siblings as ``MambaRealSR.feed_data`` calls them (RealSR/VmambaIR/models/MambaRealSR_model.py:177-187, :209-219).
``vmambair_amd.degradations`` is the public face; semantics, the counter layout of the random stream and limits as in
include/vmambair_oss.h.  fp32 only, nothing is differentiated, nothing is read back."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import _capi
from ._common import _LIB, _check
from .degrade import _checked_image, _is_f32_image

DRAW_PARAMS, CLIP, ROUNDS, QUANTISE, RAW, ONLY = (_capi.NOISE[k] for k in ("DRAW_PARAMS", "CLIP", "ROUNDS", "QUANTISE", "RAW", "ONLY"))
KNOWN_FLAGS = DRAW_PARAMS | CLIP | ROUNDS | QUANTISE | RAW | ONLY
GAUSSIAN, POISSON = 0, 1


def noise_ok(img: torch.Tensor, kind: int, flags: int = 0) -> bool:
    """whether the kernels of ``kind`` (0 Gaussian, 1 Poisson) take this (B, C, H, W) image (a host query of the library)"""
    return _is_f32_image(img) and _capi.load().oss_noise_workgroups(int(kind), *img.shape, int(flags)) > 0


def _checked_noise(name: str, kind: int, img, state, amount, gray, flags) -> None:
    _checked_image(name, img)
    _check(state.is_cuda and state.device == img.device and state.dtype == torch.int64 and state.dim() == 1 and state.numel() == 2
           and state.is_contiguous(), f"{name}: state must be a contiguous int64 (2,) tensor (seed, call) on img's device")
    for what, t in (("amount", amount), ("gray", gray)):
        if t is not None:
            _check(t.is_cuda and t.device == img.device and t.dtype == torch.float32 and t.dim() == 1 and t.numel() == img.size(0)
                   and t.is_contiguous(), f"{name}: {what} must be a contiguous fp32 (B,) tensor on img's device")
    _check(0 <= int(flags) <= KNOWN_FLAGS and not int(flags) & ~KNOWN_FLAGS, f"{name}: unknown flags {flags}")
    _check(_capi.load().oss_noise_workgroups(kind, *img.shape, int(flags)) > 0,
           f"{name}: a {tuple(img.shape)} image is not supported" + (" (3 channels)" if kind == POISSON else ""))


def noise_gaussian(img: torch.Tensor, state: torch.Tensor, sigma: Optional[torch.Tensor], gray: Optional[torch.Tensor], lo: float,
                   hi: float, gray_scalar: float, flags: int, want_params: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (out, params): ``img + noise`` (``noise`` alone with ONLY) with ``noise = (n_c (1 - g_b) + n_g[y, x] g_b) sigma_b / 255``
    evaluated as the package does, then the epilogue of ``flags``.  ``sigma_b``, ``g_b``: ``sigma[b]`` / ``gray[b]``, or ``lo`` /
    ``gray_scalar`` where the tensor is None, or with DRAW_PARAMS drawn on the device from U[lo, hi) and with probability
    ``gray_scalar``.  ``params`` (2, B) = sigma_b, g_b when ``want_params``.  ``state`` (seed, call) is read on the device and
    its call counter advanced by one.  Two launches on the current stream, no host synchronisation."""
    _checked_noise("noise_gaussian", GAUSSIAN, img, state, sigma, gray, flags)
    B, C, H, W = img.shape
    out = torch.empty_like(img)
    params = img.new_empty(2, B) if want_params else img.new_empty(0)
    with torch.cuda.device(img.device):
        _capi.check(_capi.load().oss_noise_gaussian(
            img.data_ptr(), out.data_ptr(), state.data_ptr(), None if sigma is None else sigma.data_ptr(),
            None if gray is None else gray.data_ptr(), float(lo), float(hi), float(gray_scalar),
            params.data_ptr() if want_params else None, B, C, H, W, int(flags), torch.cuda.current_stream().cuda_stream),
            "oss_noise_gaussian")
    return out, params


def noise_poisson(img: torch.Tensor, state: torch.Tensor, scale: Optional[torch.Tensor], gray: Optional[torch.Tensor], lo: float,
                  hi: float, gray_scalar: float, flags: int, want_params: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (out, params): ``img + noise`` (``noise`` alone with ONLY) with the package's Poisson noise of ``img`` (B, 3, H, W): the
    level census of every sample, the counts and the grey mix all on the device.  Arguments as ``noise_gaussian``; ``params``
    (4, B) = scale_b, g_b, vals of the colour levels, vals of the grey levels.  With RAW ``img`` holds lambda and ``out`` receives
    the counts.  A memset and three launches on the current stream (RAW: two launches), no host synchronisation."""
    _checked_noise("noise_poisson", POISSON, img, state, scale, gray, flags)
    B, C, H, W = img.shape
    lib = _capi.load()
    out = torch.empty_like(img)
    raw = bool(int(flags) & RAW)
    params = img.new_empty(4, B) if want_params and not raw else img.new_empty(0)
    scratch = None if raw else torch.empty(int(lib.oss_noise_scratch_words(B)), dtype=torch.int32, device=img.device)
    with torch.cuda.device(img.device):
        _capi.check(lib.oss_noise_poisson(
            img.data_ptr(), out.data_ptr(), state.data_ptr(), None if scale is None else scale.data_ptr(),
            None if gray is None else gray.data_ptr(), float(lo), float(hi), float(gray_scalar),
            params.data_ptr() if params.numel() else None, None if raw else scratch.data_ptr(), B, C, H, W, int(flags),
            torch.cuda.current_stream().cuda_stream), "oss_noise_poisson")
    return out, params


_LIB.define("noise_gaussian(Tensor img, Tensor(a!) state, Tensor? sigma, Tensor? gray, float lo, float hi, float gray_scalar, "
            "int flags, bool want_params) -> (Tensor, Tensor)")
_LIB.impl("noise_gaussian", noise_gaussian, "CUDA")
_LIB.define("noise_poisson(Tensor img, Tensor(a!) state, Tensor? scale, Tensor? gray, float lo, float hi, float gray_scalar, "
            "int flags, bool want_params) -> (Tensor, Tensor)")
_LIB.impl("noise_poisson", noise_poisson, "CUDA")
