"""The degradation filters on the device: ``torch.ops.vmambair.filter2d`` / ``filter_sep`` / ``usm_sharp`` on ``oss_degrade.hip`` --
``filter2D`` and ``USMSharp`` as ``MambaRealSR.feed_data`` calls them (RealSR/VmambaIR/models/MambaRealSR_model.py:146-263) -- and
``torch.ops.vmambair.jpeg_roundtrip`` on ``oss_jpeg.hip``, the ``DiffJPEG`` of the same method in one launch.
``vmambair_amd.degradations`` is the public face; semantics and limits as in include/vmambair_oss.h.  fp32 only, nothing is
differentiated."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import _capi
from ._common import _LIB, _check

NONE, CLAMP, QUANTISE = (_capi.FILTER[k] for k in ("NONE", "CLAMP", "QUANTISE"))
FILTER2D_MAX_K, FILTER_SEP_MAX_K = _capi.FILTER["2D_MAX_K"], _capi.FILTER["SEP_MAX_K"]
JPEG_CLAMP_INPUT, JPEG_QUANTISE, JPEG_DIFF_ROUND = (_capi.JPEG[k] for k in ("CLAMP_INPUT", "QUANTISE", "DIFF_ROUND"))


def _is_f32_image(img: torch.Tensor) -> bool:
    return img.is_cuda and img.dim() == 4 and img.dtype == torch.float32 and img.numel() > 0


def filter2d_ok(img: torch.Tensor, kernel: torch.Tensor) -> bool:
    """whether the kernel takes this (B, C, H, W) image with this (1 or B, k, k) kernel (a host query of the library)"""
    if not (_is_f32_image(img) and kernel.is_cuda and kernel.dim() == 3 and kernel.dtype == torch.float32
            and kernel.size(1) == kernel.size(2)):
        return False
    return _capi.load().oss_filter2d_workgroups(*img.shape, kernel.size(-1), kernel.size(0)) > 0


def filter_sep_ok(img: torch.Tensor, k: int) -> bool:
    """whether the separable kernels take this (B, C, H, W) image with a vector of ``k`` taps (a host query of the library)"""
    return _is_f32_image(img) and _capi.load().oss_filter_sep_scratch_floats(*img.shape, int(k)) > 0


def _checked_image(name: str, img: torch.Tensor) -> None:
    _check(img.is_cuda, f"{name}: img must be a CUDA/HIP tensor")
    _check(img.dim() == 4 and img.numel() > 0, f"{name}: img must be a non-empty (B, C, H, W) tensor")
    _check(img.dtype == torch.float32, f"{name}: fp32 tensors")
    _check(img.is_contiguous(), f"{name}: img must be contiguous")


def _checked_vector(name: str, img: torch.Tensor, g: torch.Tensor) -> int:
    _check(g.is_cuda and g.device == img.device and g.dtype == torch.float32 and g.dim() == 1 and g.is_contiguous(),
           f"{name}: g must be a contiguous fp32 vector on img's device")
    return g.numel()


def filter2d(img: torch.Tensor, kernel: torch.Tensor, epilogue: int) -> torch.Tensor:
    """-> the k x k correlation of ``img`` (reflect padded by k // 2) with ``kernel`` (1, k, k) or (B, k, k), then the epilogue
    (0 none, 1 clamp to [0, 1], 2 clamp(round(x * 255), 0, 255) / 255).  One launch on the current stream, no host synchronisation."""
    _checked_image("filter2d", img)
    _check(kernel.is_cuda and kernel.device == img.device and kernel.dtype == torch.float32 and kernel.is_contiguous(),
           "filter2d: kernel must be a contiguous fp32 tensor on img's device")
    _check(kernel.dim() == 3 and kernel.size(1) == kernel.size(2), "filter2d: kernel must be (1, k, k) or (B, k, k)")
    B, C, H, W = img.shape
    k, nk = kernel.size(-1), kernel.size(0)
    lib = _capi.load()
    _check(lib.oss_filter2d_workgroups(B, C, H, W, k, nk) > 0,
           f"filter2d: a {tuple(kernel.shape)} kernel on a {tuple(img.shape)} image is not supported (k odd and <= {FILTER2D_MAX_K}, "
           "H and W > k // 2, 1 or B kernels)")
    _check(int(epilogue) in (NONE, CLAMP, QUANTISE), f"filter2d: unknown epilogue {epilogue}")
    out = torch.empty_like(img)
    with torch.cuda.device(img.device):
        _capi.check(lib.oss_filter2d(img.data_ptr(), kernel.data_ptr(), out.data_ptr(), B, C, H, W, k, nk, int(epilogue),
                                     torch.cuda.current_stream().cuda_stream), "oss_filter2d")
    return out


def filter_sep(img: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """-> the correlation of ``img`` (reflect padded) with the rank-1 kernel ``outer(g, g)``: a row and a column pass on the current
    stream, the intermediate from the caching allocator, no host synchronisation."""
    _checked_image("filter_sep", img)
    k = _checked_vector("filter_sep", img, g)
    B, C, H, W = img.shape
    lib = _capi.load()
    n = int(lib.oss_filter_sep_scratch_floats(B, C, H, W, k))
    _check(n > 0, f"filter_sep: {k} taps on a {tuple(img.shape)} image are not supported (k odd and <= {FILTER_SEP_MAX_K}, "
           "H and W > k // 2)")
    out, scratch = torch.empty_like(img), torch.empty(n, dtype=torch.float32, device=img.device)
    with torch.cuda.device(img.device):
        _capi.check(lib.oss_filter_sep(img.data_ptr(), g.data_ptr(), out.data_ptr(), scratch.data_ptr(), B, C, H, W, k,
                                       torch.cuda.current_stream().cuda_stream), "oss_filter_sep")
    return out


def usm_sharp(img: torch.Tensor, g: torch.Tensor, weight: float, threshold: float, want_mask: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (sharpened image, mask): unsharp masking with the Gaussian ``outer(g, g)`` in four separable passes on the current stream.
    ``mask`` is the 0 / 1 map ``|img - blur| * 255 > threshold`` when ``want_mask``, an empty tensor otherwise."""
    _checked_image("usm_sharp", img)
    k = _checked_vector("usm_sharp", img, g)
    B, C, H, W = img.shape
    lib = _capi.load()
    n = int(lib.oss_usm_scratch_floats(B, C, H, W, k))
    _check(n > 0, f"usm_sharp: {k} taps on a {tuple(img.shape)} image are not supported (k odd and <= {FILTER_SEP_MAX_K}, "
           "H and W > k // 2)")
    out, scratch = torch.empty_like(img), torch.empty(n, dtype=torch.float32, device=img.device)
    mask = torch.empty_like(img) if want_mask else img.new_empty(0)
    with torch.cuda.device(img.device):
        _capi.check(lib.oss_usm_sharp(img.data_ptr(), g.data_ptr(), out.data_ptr(), mask.data_ptr() if want_mask else None,
                                      scratch.data_ptr(), B, C, H, W, k, float(weight), float(threshold),
                                      torch.cuda.current_stream().cuda_stream), "oss_usm_sharp")
    return out, mask


def jpeg_ok(img: torch.Tensor) -> bool:
    """whether the JPEG kernel takes this (B, 3, h, w) image (a host query of the library)"""
    return _is_f32_image(img) and img.size(1) == 3 and _capi.load().oss_jpeg_workgroups(img.size(0), img.size(2), img.size(3)) > 0


def jpeg_roundtrip(img: torch.Tensor, quality: Optional[torch.Tensor], quality_scalar: float, flags: int,
                   want_coefficients: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (out, y, cb, cr): JPEG compression and decompression of ``img`` (B, 3, h, w) in [0, 1] as basicsr's ``DiffJPEG`` defines
    them, with the quality of sample b read from ``quality`` (B,) on the device, or ``quality_scalar`` for all when ``quality`` is
    None.  ``flags``: JPEG_CLAMP_INPUT | JPEG_QUANTISE | JPEG_DIFF_ROUND.  ``y`` (B, H W / 64, 8, 8), ``cb``, ``cr`` (B, H W / 256, 8, 8)
    are the quantised coefficients of the image padded to H, W = multiples of 16 when ``want_coefficients``, empty tensors
    otherwise.  One launch on the current stream, no host synchronisation."""
    _checked_image("jpeg_roundtrip", img)
    B, C, h, w = img.shape
    _check(C == 3, "jpeg_roundtrip: img must have 3 channels")
    if quality is not None:
        _check(quality.is_cuda and quality.device == img.device and quality.dtype == torch.float32 and quality.dim() == 1
               and quality.numel() == B and quality.is_contiguous(),
               "jpeg_roundtrip: quality must be a contiguous fp32 (B,) tensor on img's device")
    lib = _capi.load()
    _check(lib.oss_jpeg_workgroups(B, h, w) > 0, f"jpeg_roundtrip: a {tuple(img.shape)} image is not supported")
    _check(0 <= int(flags) <= JPEG_CLAMP_INPUT | JPEG_QUANTISE | JPEG_DIFF_ROUND, f"jpeg_roundtrip: unknown flags {flags}")
    out = torch.empty_like(img)
    if want_coefficients:
        blocks = ((h + 15) // 16) * ((w + 15) // 16)
        y, cb, cr = img.new_empty(B, 4 * blocks, 8, 8), img.new_empty(B, blocks, 8, 8), img.new_empty(B, blocks, 8, 8)
    else:
        y, cb, cr = img.new_empty(0), img.new_empty(0), img.new_empty(0)
    with torch.cuda.device(img.device):
        _capi.check(lib.oss_jpeg_roundtrip(img.data_ptr(), None if quality is None else quality.data_ptr(), float(quality_scalar),
                                           out.data_ptr(), *((t.data_ptr() if want_coefficients else None) for t in (y, cb, cr)),
                                           B, h, w, int(flags), torch.cuda.current_stream().cuda_stream), "oss_jpeg_roundtrip")
    return out, y, cb, cr


_LIB.define("filter2d(Tensor img, Tensor kernel, int epilogue) -> Tensor")
_LIB.impl("filter2d", filter2d, "CUDA")
_LIB.define("filter_sep(Tensor img, Tensor g) -> Tensor")
_LIB.impl("filter_sep", filter_sep, "CUDA")
_LIB.define("usm_sharp(Tensor img, Tensor g, float weight, float threshold, bool want_mask) -> (Tensor, Tensor)")
_LIB.impl("usm_sharp", usm_sharp, "CUDA")
_LIB.define("jpeg_roundtrip(Tensor img, Tensor? quality, float quality_scalar, int flags, bool want_coefficients) -> "
            "(Tensor, Tensor, Tensor, Tensor)")
_LIB.impl("jpeg_roundtrip", jpeg_roundtrip, "CUDA")
