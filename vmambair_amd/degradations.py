"""The custom operators of the RealSR degradation pipeline, which ``MambaRealSR.feed_data`` runs on the GPU under ``no_grad`` before
every training step (RealSR/VmambaIR/models/MambaRealSR_model.py:146-263):

  ``filter2D(img, kernel)``         a different 21 x 21 blur or sinc kernel per sample after reflect padding (:165, :196, :232/245)
  ``USMSharp(radius=50, sigma=0)``  unsharp masking of the ground truth with a 51 x 51 Gaussian (:154-155, :262)
  ``gaussian_kernel1d(k, sigma)``   the Gaussian vector ``USMSharp`` is built from
  ``DiffJPEG(differentiable)``      JPEG compression and decompression with a quality per sample (:86, :189-191, :234-241)
  ``random_add_gaussian_noise_pt``, ``random_add_poisson_noise_pt`` and their six siblings: the two noise branches (:177-187, :209-219)
  ``TrainingPairPool(queue_size)``  the training pair pool ``_dequeue_and_enqueue`` (:109-144)

The reference imports ``filter2D``, ``USMSharp`` and ``DiffJPEG`` from the pip ``basicsr`` package (``basicsr.utils``,
``basicsr.utils.img_process_util``, ``basicsr.utils.diffjpeg``), which is not part of the reference tree.  Their definitions are
restated here from that package's published source, and every test is anchored to an independent float64 evaluation of these formulas
(``scipy.ndimage.correlate(..., mode='mirror')``, tests/golden/make_golden_degrade.py; ``scipy.fft.dctn`` per 8 x 8 block,
tests/golden/make_golden_jpeg.py), not to reference code.  The pair pool is in the
reference tree; its fixture is a trace of the reference's own method.

fp32 device tensors go to the HIP kernels of ``csrc/oss_degrade.hip`` (``torch.ops.vmambair.filter2d`` / ``usm_sharp``):
``filter2D`` for odd k <= 21, reflect addressing inside the load, with the ``clamp`` to [0, 1] (:190, :235, :240) or the final
quantisation ``clamp((x * 255).round(), 0, 255) / 255`` (:248) as the kernel's last stage; ``USMSharp`` as four separable passes with
the 51-vector it built itself (4 k taps per pixel where the dense form has 2 k^2).  Nothing in ``feed_data`` is differentiated, so no
backward exists: the device paths run under ``torch.no_grad`` and return tensors without a graph.  A plain-torch restatement serves
CPU tensors, non-fp32 input, k above the kernels' limits and, in ``filter2D``, a large (1, k, k) kernel, which need not be rank 1 -- as
``losses.py`` and ``metrics.py`` do for CPU inputs.  ``DiffJPEG`` on a contiguous fp32 device tensor is one launch of
``csrc/oss_jpeg.hip`` (``torch.ops.vmambair.jpeg_roundtrip``) per call, with the quality of every sample read on the device; its
restatement ``restate_diffjpeg`` follows the package operation by operation.  The two noise steps (:177-187, :209-219) -- the eight
``*_gaussian_noise_pt`` / ``*_poisson_noise_pt`` functions of ``basicsr.data.degradations``, here with the package's names,
positional signatures and defaults -- run on ``csrc/oss_noise.hip`` (``torch.ops.vmambair.noise_gaussian`` / ``noise_poisson``): one
sampling launch for the Gaussian noise, a level census and a sampling launch for the Poisson noise, both drawing from a
``NoiseStream`` -- a Philox4x32-10 key and a call counter in device memory -- without a host read, so that a whole degradation
stage (``filter2D`` -> ``F.interpolate`` -> noise -> ``DiffJPEG``) can be captured into a graph and draws a new field at every replay;
their restatements ``restate_*_noise_pt`` follow the package operation by operation, host reads and ``unique`` loop included.  What
is left of ``feed_data`` is ``F.interpolate``, a vendor operator that is one launch without a host read.
"""
from __future__ import annotations

import functools
import math
from typing import Optional, Tuple

import torch
from torch import nn
from torch.nn import functional as F

from . import ops as _ops

# OpenCV's getGaussianKernel uses these fixed vectors for sigma <= 0 and k <= 7
_SMALL_GAUSSIAN = {1: (1.0,), 3: (0.25, 0.5, 0.25), 5: (0.0625, 0.25, 0.375, 0.25, 0.0625),
                   7: (0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125)}


# ---------------------------------------------------------------------------------------------
# the restatement (dtype-preserving: on float64 inputs it is the formula in float64)
# ---------------------------------------------------------------------------------------------
def restate_filter2d(img: torch.Tensor, kernel: torch.Tensor) -> torch.Tensor:
    """basicsr.utils.img_process_util.filter2D: reflect pad, then a grouped cross-correlation (no kernel flip)"""
    k = kernel.size(-1)
    b, c, h, w = img.size()
    if k % 2 == 1:
        img = F.pad(img, (k // 2, k // 2, k // 2, k // 2), mode='reflect')
    else:
        raise ValueError('Wrong kernel size')
    ph, pw = img.size()[-2:]
    if kernel.size(0) == 1:
        # one kernel for all samples
        img = img.view(b * c, 1, ph, pw)
        kernel = kernel.view(1, 1, k, k)
        return F.conv2d(img, kernel, padding=0).view(b, c, h, w)
    img = img.view(1, b * c, ph, pw)
    kernel = kernel.view(b, 1, k, k).repeat(1, c, 1, 1).view(b * c, 1, k, k)
    return F.conv2d(img, kernel, groups=b * c).view(b, c, h, w)


def restate_quantise(x: torch.Tensor) -> torch.Tensor:
    """MambaRealSR_model.py:248"""
    return torch.clamp((x * 255.0).round(), 0, 255) / 255.


def restate_usm(img: torch.Tensor, kernel: torch.Tensor, weight: float = 0.5, threshold: float = 10) -> torch.Tensor:
    """basicsr.utils.img_process_util.USMSharp.forward"""
    blur = restate_filter2d(img, kernel)
    residual = img - blur
    mask = (torch.abs(residual) * 255 > threshold).to(img.dtype)
    soft_mask = restate_filter2d(mask, kernel)
    sharp = torch.clip(img + weight * residual, 0, 1)
    return soft_mask * sharp + (1 - soft_mask) * img


# basicsr.utils.diffjpeg: the luminance table is the standard one TRANSPOSED (the package transposes it when it builds the parameter),
# the chrominance table is 99 outside its symmetric top-left 4 x 4 block; all matrices are float32 constants in the package
_JPEG_Y_TABLE = ((16, 11, 10, 16, 24, 40, 51, 61), (12, 12, 14, 19, 26, 58, 60, 55), (14, 13, 16, 24, 40, 57, 69, 56),
                 (14, 17, 22, 29, 51, 87, 80, 62), (18, 22, 37, 56, 68, 109, 103, 77), (24, 35, 55, 64, 81, 104, 113, 92),
                 (49, 64, 78, 87, 103, 121, 120, 101), (72, 92, 95, 98, 112, 100, 103, 99))
_JPEG_C_BLOCK = ((17, 18, 24, 47), (18, 21, 26, 66), (24, 26, 56, 99), (47, 66, 99, 99))
_JPEG_RGB2YCC = ((0.299, 0.587, 0.114), (-0.168736, -0.331264, 0.5), (0.5, -0.418688, -0.081312))
_JPEG_YCC2RGB = ((1., 0., 1.402), (1., -0.344136, -0.714136), (1., 1.772, 0.))


@functools.lru_cache(maxsize=None)
def _jpeg_constants(dtype: torch.dtype, device: torch.device):
    f32 = functools.partial(torch.tensor, dtype=torch.float32)
    y_table = f32(_JPEG_Y_TABLE).t().contiguous()
    c_table = torch.full((8, 8), 99., dtype=torch.float32)
    c_table[:4, :4] = f32(_JPEG_C_BLOCK).t()
    n = torch.arange(8, dtype=torch.float64)
    cos = torch.cos((2 * n[:, None] + 1) * n[None, :] * math.pi / 16)            # [x][u]
    dct = cos[:, None, :, None] * cos[None, :, None, :]                           # [x][y][u][v]
    alpha = torch.tensor([1. / math.sqrt(2)] + [1.] * 7, dtype=torch.float64)
    alpha = torch.outer(alpha, alpha)
    out = dict(y_table=y_table, c_table=c_table, rgb2ycc=f32(_JPEG_RGB2YCC).t(), ycc2rgb=f32(_JPEG_YCC2RGB).t(),
               shift=f32([0., 128., 128.]), unshift=f32([0., -128., -128.]), dct=dct, idct=dct.permute(2, 3, 0, 1).contiguous(),
               scale=alpha * 0.25, alpha=alpha)
    return {k: v.to(device=device, dtype=dtype) for k, v in out.items()}


def quality_to_factor(quality):
    """basicsr.utils.diffjpeg.quality_to_factor, on a Python number or a 0-dim tensor (then ``if`` reads the value on the host)"""
    if quality < 50:
        quality = 5000. / quality
    else:
        quality = 200. - quality * 2
    return quality / 100.


def _jpeg_blocks(plane: torch.Tensor) -> torch.Tensor:
    """(B, H, W) -> (B, H W / 64, 8, 8), blocks row-major"""
    b = plane.size(0)
    return plane.view(b, plane.size(1) // 8, 8, -1, 8).permute(0, 1, 3, 2, 4).contiguous().view(b, -1, 8, 8)


def _jpeg_merge(blocks: torch.Tensor, height: int, width: int) -> torch.Tensor:
    b = blocks.size(0)
    return blocks.view(b, height // 8, width // 8, 8, 8).permute(0, 1, 3, 2, 4).contiguous().view(b, height, width)


def _jpeg_round(v: torch.Tensor, differentiable: bool) -> torch.Tensor:
    r = torch.round(v)
    return r + (v - r) ** 3 if differentiable else r


def _restate_jpeg_from_factor(x: torch.Tensor, factor, differentiable: bool):
    """``factor``: a Python number or a (B,) tensor of x's dtype -> (out, (y, cb, cr)), operation by operation as the package"""
    if x.dim() != 4 or x.size(1) != 3:
        raise ValueError(f"DiffJPEG: x must be (B, 3, h, w), not {tuple(x.shape)}")
    k = _jpeg_constants(x.dtype, x.device)
    b, _, h, w = x.size()
    x = F.pad(x, (0, -w % 16, 0, -h % 16), mode='constant', value=0)
    height, width = x.size()[-2:]
    if torch.is_tensor(factor):
        factor = factor.view(b, 1, 1, 1)
    # CompressJpeg: rgb2ycbcr_jpeg, chroma_subsampling, block_splitting, dct_8x8, y_quantize / c_quantize
    ycc = torch.tensordot((x * 255).permute(0, 2, 3, 1), k['rgb2ycc'], dims=1) + k['shift']
    planes = ycc.permute(0, 3, 1, 2).clone()
    cb = F.avg_pool2d(planes[:, 1:2], kernel_size=2, stride=(2, 2), count_include_pad=False).squeeze(1)
    cr = F.avg_pool2d(planes[:, 2:3], kernel_size=2, stride=(2, 2), count_include_pad=False).squeeze(1)
    coef, tables = [], []
    for plane, table in ((ycc[..., 0], k['y_table']), (cb, k['c_table']), (cr, k['c_table'])):
        freq = k['scale'] * torch.tensordot(_jpeg_blocks(plane) - 128, k['dct'], dims=2)
        tables.append(table.expand(b, 1, 8, 8) * factor)
        coef.append(_jpeg_round(freq / tables[-1], differentiable))
    # DeCompressJpeg: dequantize, idct_8x8, block_merging, chroma_upsampling, ycbcr2rgb_jpeg
    rec = []
    for c, table, (hh, ww) in zip(coef, tables, ((height, width), (height // 2, width // 2), (height // 2, width // 2))):
        rec.append(_jpeg_merge(0.25 * torch.tensordot(c * table * k['alpha'], k['idct'], dims=2) + 128, hh, ww))
    up = [p.unsqueeze(-1).repeat(1, 1, 2, 2).view(-1, height, width) for p in rec[1:]]
    image = torch.stack([rec[0], up[0], up[1]], dim=3)
    image = torch.tensordot(image + k['unshift'], k['ycc2rgb'], dims=1).permute(0, 3, 1, 2)
    image = torch.min(255 * torch.ones_like(image), torch.max(torch.zeros_like(image), image))
    return (image / 255)[:, :, 0:h, 0:w], tuple(coef)


def _restate_jpeg(x: torch.Tensor, quality, differentiable: bool):
    if torch.is_tensor(quality):
        if quality.dim() != 1 or quality.numel() != x.size(0):
            raise ValueError(f"DiffJPEG: quality must be a number or a (B,) tensor, not {tuple(quality.shape)}")
        q = quality.to(device=x.device, dtype=x.dtype)
        factor = torch.where(q < 50, 5000. / q, 200. - q * 2) / 100.   # the package loops over the samples on the host
    else:
        factor = quality_to_factor(quality)
    return _restate_jpeg_from_factor(x, factor, differentiable)


def restate_diffjpeg(x: torch.Tensor, quality, differentiable: bool = False) -> torch.Tensor:
    """basicsr.utils.diffjpeg.DiffJPEG.forward for ``x`` (B, 3, h, w) in [0, 1] and ``quality`` a Python number or a (B,) tensor,
    which is left as it is"""
    return _restate_jpeg(x, quality, differentiable)[0]


# ---------------------------------------------------------------------------------------------
# the public face
# ---------------------------------------------------------------------------------------------
def filter2D(img: torch.Tensor, kernel: torch.Tensor, *, clamp: bool = False, quantise: bool = False) -> torch.Tensor:
    """``img`` (B, C, H, W) correlated with ``kernel`` (1, k, k), (B, k, k) or (k, k) after reflect padding by k // 2:
    ``out[b,c,y,x] = sum_ij kernel[b or 0, i, j] * pad[b,c,y+i,x+j]``.  k must be odd (``ValueError('Wrong kernel size')``) and H, W
    > k // 2 (torch's reflect pad raises otherwise).  ``clamp`` then clamps to [0, 1], ``quantise`` applies
    ``clamp((x * 255).round(), 0, 255) / 255``; on the device both are the kernel's last stage, bit-equal to torch's expressions
    there (torch divides a device tensor by 255 as a multiplication by fp32(1 / 255), the CPU path divides: one unit in the last place
    apart at some levels, as the reference itself is between the two).  No gradient flows through the device path."""
    if kernel.dim() == 2:
        kernel = kernel.unsqueeze(0)
    if kernel.dim() != 3 or kernel.size(-1) != kernel.size(-2) or img.dim() != 4 or kernel.size(0) not in (1, img.size(0)):
        raise ValueError(f"filter2D: img must be (B, C, H, W) and kernel (k, k), (1, k, k) or (B, k, k): {tuple(img.shape)}, "
                         f"{tuple(kernel.shape)}")
    if kernel.size(-1) % 2 == 0:
        raise ValueError('Wrong kernel size')
    if img.is_cuda and kernel.device == img.device and img.dtype == kernel.dtype and _ops.filter2d_ok(img, kernel):
        with torch.no_grad():
            return _ops.filter2d(img.contiguous(), kernel.contiguous(),
                                 _ops.degrade.QUANTISE if quantise else _ops.degrade.CLAMP if clamp else _ops.degrade.NONE)
    out = restate_filter2d(img, kernel)
    if clamp:
        out = torch.clamp(out, 0, 1)
    return restate_quantise(out) if quantise else out


def gaussian_kernel1d(k: int, sigma: float = 0) -> torch.Tensor:
    """cv2.getGaussianKernel(k, sigma) as a float64 vector: ``g_i ~ exp(-(i - (k - 1) / 2)^2 / (2 sigma^2))`` normalised to sum 1;
    ``sigma <= 0`` stands for ``0.3 * ((k - 1) * 0.5 - 1) + 0.8`` (OpenCV's fixed vectors for k <= 7 in that case)."""
    k = int(k)
    if k < 1:
        raise ValueError(f"gaussian_kernel1d: k must be positive, not {k}")
    if sigma <= 0 and k % 2 == 1 and k in _SMALL_GAUSSIAN:
        return torch.tensor(_SMALL_GAUSSIAN[k], dtype=torch.float64)
    s = float(sigma) if sigma > 0 else 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    x = torch.arange(k, dtype=torch.float64) - (k - 1) * 0.5
    g = torch.exp(x * x * (-0.5 / (s * s)))
    return g * (1.0 / g.sum())


class USMSharp(nn.Module):
    """basicsr.utils.img_process_util.USMSharp: the buffer ``kernel`` is float32(g g^T), shape (1, k, k), k = ``radius`` made odd
    (51), so a reference ``state_dict`` loads.  ``forward(img, weight=0.5, threshold=10)``::

        blur = filter2D(img, kernel); residual = img - blur; mask = (|residual| * 255 > threshold)
        soft = filter2D(mask, kernel); sharp = clip(img + weight * residual, 0, 1)
        return soft * sharp + (1 - soft) * img

    fp32 device tensors run as four separable passes with ``g`` (``torch.ops.vmambair.usm_sharp``, no gradient); everything else, and
    a module whose ``kernel`` was loaded with other values than g g^T, uses the restatement with ``self.kernel``."""

    def __init__(self, radius: int = 50, sigma: float = 0):
        super().__init__()
        if radius % 2 == 0:
            radius += 1
        self.radius = radius
        g = gaussian_kernel1d(radius, sigma)
        self.register_buffer('kernel', torch.outer(g, g).float().unsqueeze_(0))
        self.register_buffer('_g', g.float(), persistent=False)
        self._separable = True

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        # a kernel made elsewhere (cv2 in the reference) differs from ours in the last bits only; anything else is another kernel
        g = self._g.double().to(self.kernel.device)
        self._separable = bool(torch.allclose(self.kernel.double(), torch.outer(g, g).unsqueeze(0), rtol=1e-5, atol=1e-10))

    def forward(self, img: torch.Tensor, weight: float = 0.5, threshold: float = 10) -> torch.Tensor:
        on_device = img.is_cuda and self._g.device == img.device and self._g.dtype == torch.float32
        if self._separable and on_device and _ops.filter_sep_ok(img, self.radius):
            with torch.no_grad():
                return _ops.usm_sharp(img.contiguous(), self._g, float(weight), float(threshold), False)[0]
        return restate_usm(img, self.kernel, weight, threshold)


class DiffJPEG(nn.Module):
    """basicsr.utils.diffjpeg.DiffJPEG: ``forward(x, quality)`` compresses ``x`` (B, 3, h, w) in [0, 1] to quantised DCT coefficients
    and decompresses them again; ``quality`` is a Python number or a (B,) tensor, one quality per sample.  The reference's
    ``DiffJPEG(differentiable=False).cuda()(out, quality=jpeg_p)`` (MambaRealSR_model.py:86, :189-191, :234-241) works unchanged::

        factor = (5000 / q if q < 50 else 200 - 2 q) / 100              pad bottom and right with zeros to multiples of 16
        Y, Cb, Cr = M (255 x) + (0, 128, 128)                            Cb, Cr averaged over 2 x 2
        per 8 x 8 block:  F = DCT-II(block - 128), orthonormal;  c = round(F / (T factor));  block' = IDCT(c T factor) + 128
        Cb', Cr' replicated 2 x 2;  out = clamp(M' (Y', Cb' - 128, Cr' - 128), 0, 255) / 255, cropped to h x w

    with ``T`` the luminance table transposed (as the package holds it) or the chrominance table, and round-half-even.
    ``differentiable=True`` (the package's default) replaces ``round(v)`` by ``round(v) + (v - round(v))^3``.

    A contiguous fp32 device tensor is one launch of ``csrc/oss_jpeg.hip`` (``torch.ops.vmambair.jpeg_roundtrip``) without a graph.
    Keyword-only extras, stages of that launch: ``clamp_input`` clamps ``x`` to [0, 1] first (:190, :235, :240), ``quantise``
    applies ``clamp((out * 255).round(), 0, 255) / 255`` (:248) last, ``return_coefficients`` returns ``(out, (y, cb, cr))`` with
    the quantised coefficients in the layout of the package's ``CompressJpeg``: ``y`` (B, H W / 64, 8, 8), ``cb`` and ``cr``
    (B, H W / 256, 8, 8) for the padded H x W.  ``restate_diffjpeg``, plain torch, serves CPU tensors, other dtypes, non-contiguous
    views, shapes the kernel refuses, and every call that can carry a gradient: ``differentiable=True`` with gradients enabled, or
    an ``x`` that requires one.  ``C != 3`` raises ``ValueError``.

    Deviations from the package: the caller's ``quality`` tensor is left unchanged (the package overwrites it in place with the
    factors); nothing is read back to the host (the package's loop ``for i in range(B): factor[i] = quality_to_factor(factor[i])``
    reads B device scalars), so a call can be captured into a graph and replayed with other qualities.  ``quality = 100`` gives
    factor 0 and NaN, as in the package."""

    def __init__(self, differentiable: bool = True):
        super().__init__()
        self.differentiable = bool(differentiable)

    def forward(self, x: torch.Tensor, quality, *, clamp_input: bool = False, quantise: bool = False,
                return_coefficients: bool = False):
        if x.dim() != 4 or x.size(1) != 3:
            raise ValueError(f"DiffJPEG: x must be (B, 3, h, w), not {tuple(x.shape)}")
        per_sample = torch.is_tensor(quality)
        if per_sample and (quality.dim() != 1 or quality.numel() != x.size(0)):
            raise ValueError(f"DiffJPEG: quality must be a number or a (B,) tensor, not {tuple(quality.shape)}")
        carries_grad = torch.is_grad_enabled() and (self.differentiable or x.requires_grad)
        if not carries_grad and x.is_contiguous() and _ops.jpeg_ok(x):
            flags = ((_ops.degrade.JPEG_CLAMP_INPUT if clamp_input else 0) | (_ops.degrade.JPEG_QUANTISE if quantise else 0)
                     | (_ops.degrade.JPEG_DIFF_ROUND if self.differentiable else 0))
            q = quality.detach().to(device=x.device, dtype=torch.float32).contiguous() if per_sample else None
            with torch.no_grad():
                out, y, cb, cr = _ops.jpeg_roundtrip(x, q, 0.0 if per_sample else float(quality), flags, return_coefficients)
            return (out, (y, cb, cr)) if return_coefficients else out
        out, coef = _restate_jpeg(torch.clamp(x, 0, 1) if clamp_input else x, quality, self.differentiable)
        if quantise:
            out = restate_quantise(out)
        return (out, coef) if return_coefficients else out


# ---------------------------------------------------------------------------------------------
# the two noise steps (basicsr.data.degradations, the *_pt functions)
# ---------------------------------------------------------------------------------------------
def _is_number(v) -> bool:
    return isinstance(v, (float, int))


def _rgb_to_grayscale(img: torch.Tensor) -> torch.Tensor:
    """torchvision.transforms.functional.rgb_to_grayscale(img, num_output_channels=1), which the package calls"""
    if img.shape[-3] not in (1, 3):
        raise TypeError(f"Input image tensor permitted channel values are [1, 3], but found {img.shape[-3]}")
    if img.shape[-3] == 1:
        return img.clone()
    r, g, b = img.unbind(dim=-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).to(img.dtype).unsqueeze(dim=-3)


def _poisson_vals(levels: torch.Tensor) -> list:
    """the package's ``vals`` of a quantised (B, C, h, w) image: per sample 2 ** ceil(log2(number of distinct values)) -- a sort and a
    read-back per sample"""
    return [2 ** math.ceil(math.log2(len(torch.unique(levels[i, :, :, :])))) for i in range(levels.size(0))]


def _restate_finish(out: torch.Tensor, clip: bool, rounds: bool) -> torch.Tensor:
    if clip and rounds:
        return torch.clamp((out * 255.0).round(), 0, 255) / 255.
    if clip:
        return torch.clamp(out, 0, 1)
    if rounds:
        return (out * 255.0).round() / 255.
    return out


def restate_generate_gaussian_noise_pt(img: torch.Tensor, sigma=10, gray_noise=0) -> torch.Tensor:
    """basicsr.data.degradations.generate_gaussian_noise_pt, operation by operation, from torch's default generator of img's
    device: the host read ``torch.sum(gray_noise) > 0`` and the ONE (h, w) grey field shared by the batch included (with a number
    ``sigma`` that field cannot be viewed as (b, 1, h, w) for b > 1 and the call raises, as the package's does)"""
    b, _, h, w = img.size()
    if not _is_number(sigma):
        sigma = sigma.view(img.size(0), 1, 1, 1)
    if _is_number(gray_noise):
        cal_gray_noise = gray_noise > 0
    else:
        gray_noise = gray_noise.view(b, 1, 1, 1)
        cal_gray_noise = torch.sum(gray_noise) > 0
    if cal_gray_noise:
        noise_gray = torch.randn(*img.size()[2:4], dtype=img.dtype, device=img.device) * sigma / 255.
        noise_gray = noise_gray.view(b, 1, h, w)
    noise = torch.randn(*img.size(), dtype=img.dtype, device=img.device) * sigma / 255.
    if cal_gray_noise:
        noise = noise * (1 - gray_noise) + noise_gray * gray_noise
    return noise


def restate_generate_poisson_noise_pt(img: torch.Tensor, scale=1.0, gray_noise=0) -> torch.Tensor:
    """basicsr.data.degradations.generate_poisson_noise_pt, operation by operation: ``torch.poisson`` from the default generator,
    the ``unique`` loop over the samples (twice) and the host read of ``gray_noise`` included.  Grey noise needs 1 or 3 channels
    (``rgb_to_grayscale`` raises ``TypeError`` otherwise) and is expanded to 3."""
    b, _, h, w = img.size()
    if _is_number(gray_noise):
        cal_gray_noise = gray_noise > 0
    else:
        gray_noise = gray_noise.view(b, 1, 1, 1)
        cal_gray_noise = torch.sum(gray_noise) > 0
    if cal_gray_noise:
        img_gray = _rgb_to_grayscale(img)
        img_gray = torch.clamp((img_gray * 255.0).round(), 0, 255) / 255.
        vals = img_gray.new_tensor(_poisson_vals(img_gray)).view(b, 1, 1, 1)
        out = torch.poisson(img_gray * vals) / vals
        noise_gray = out - img_gray
        noise_gray = noise_gray.expand(b, 3, h, w)
    img = torch.clamp((img * 255.0).round(), 0, 255) / 255.
    vals = img.new_tensor(_poisson_vals(img)).view(b, 1, 1, 1)
    out = torch.poisson(img * vals) / vals
    noise = out - img
    if cal_gray_noise:
        noise = noise * (1 - gray_noise) + noise_gray * gray_noise
    if not _is_number(scale):
        scale = scale.view(b, 1, 1, 1)
    return noise * scale


def _restate_random_params(img: torch.Tensor, value_range, gray_prob):
    """the draws of random_generate_*_noise_pt, in the package's order"""
    amount = torch.rand(img.size(0), dtype=img.dtype, device=img.device) * (value_range[1] - value_range[0]) + value_range[0]
    gray_noise = torch.rand(img.size(0), dtype=img.dtype, device=img.device)
    return amount, (gray_noise < gray_prob).float()


def restate_random_generate_gaussian_noise_pt(img: torch.Tensor, sigma_range=(0, 10), gray_prob=0) -> torch.Tensor:
    """basicsr.data.degradations.random_generate_gaussian_noise_pt"""
    sigma, gray_noise = _restate_random_params(img, sigma_range, gray_prob)
    return restate_generate_gaussian_noise_pt(img, sigma, gray_noise)


def restate_random_generate_poisson_noise_pt(img: torch.Tensor, scale_range=(0, 1.0), gray_prob=0) -> torch.Tensor:
    """basicsr.data.degradations.random_generate_poisson_noise_pt"""
    scale, gray_noise = _restate_random_params(img, scale_range, gray_prob)
    return restate_generate_poisson_noise_pt(img, scale, gray_noise)


def restate_add_gaussian_noise_pt(img, sigma=10, gray_noise=0, clip=True, rounds=False):
    """basicsr.data.degradations.add_gaussian_noise_pt"""
    return _restate_finish(img + restate_generate_gaussian_noise_pt(img, sigma, gray_noise), clip, rounds)


def restate_add_poisson_noise_pt(img, scale=1.0, clip=True, rounds=False, gray_noise=0):
    """basicsr.data.degradations.add_poisson_noise_pt (``clip`` and ``rounds`` come before ``gray_noise`` in this one)"""
    return _restate_finish(img + restate_generate_poisson_noise_pt(img, scale, gray_noise), clip, rounds)


def restate_random_add_gaussian_noise_pt(img, sigma_range=(0, 10), gray_prob=0, clip=True, rounds=False):
    """basicsr.data.degradations.random_add_gaussian_noise_pt"""
    return _restate_finish(img + restate_random_generate_gaussian_noise_pt(img, sigma_range, gray_prob), clip, rounds)


def restate_random_add_poisson_noise_pt(img, scale_range=(0, 1.0), gray_prob=0, clip=True, rounds=False):
    """basicsr.data.degradations.random_add_poisson_noise_pt"""
    return _restate_finish(img + restate_random_generate_poisson_noise_pt(img, scale_range, gray_prob), clip, rounds)


def _indexed_device(device) -> torch.device:
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        return torch.device("cuda", torch.cuda.current_device())
    return device


class NoiseStream:
    """The random stream of the device noise functions: a (2,) int64 tensor in device memory, ``seed`` (the Philox key) and ``call``
    (the number of noise calls made so far).  The kernels read both on the device and a one-thread launch after the sampling
    launch stores ``call + 1``: nothing is read back, and a call captured into a graph draws a new field at every replay -- the
    fields N eager calls from the same state draw.  The tensor is created at the first use on a device (or at construction with
    ``device=``), which must happen outside a capture, and a stream serves one device.  ``state_dict()`` reads the two numbers back
    (the only read-back here), ``load_state_dict()`` writes them into the same tensor, so a captured graph follows a resumed run."""

    def __init__(self, seed: int, device=None):
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.seed = seed - (1 << 64) if seed >= (1 << 63) else seed     # as the int64 the device holds
        self._state: Optional[torch.Tensor] = None
        if device is not None:
            self.state(torch.device(device))

    def state(self, device) -> torch.Tensor:
        device = _indexed_device(device)
        if self._state is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("NoiseStream: the first use on a device creates the state tensor, which cannot happen inside a "
                                   "graph capture; construct the stream with device=, or call a noise function once before capturing")
            self._state = torch.tensor([self.seed, 0], dtype=torch.int64, device=device)
        if self._state.device != device:
            raise RuntimeError(f"NoiseStream: the stream lives on {self._state.device}, the image on {device}")
        return self._state

    def clone(self) -> "NoiseStream":
        """a stream that continues from this one's present state, independently"""
        other = NoiseStream(self.seed)
        if self._state is not None:
            other._state = self._state.clone()
        return other

    def state_dict(self) -> dict:
        seed, calls = (self.seed, 0) if self._state is None else self._state.tolist()
        return {"seed": seed, "calls": calls}

    def load_state_dict(self, state: dict) -> None:
        self.seed = int(state["seed"])
        if self._state is None:
            if int(state["calls"]):
                raise RuntimeError("NoiseStream: bind the stream to a device (device=) before loading a state that has made calls")
            return
        self._state.copy_(torch.tensor([self.seed, int(state["calls"])], dtype=torch.int64))


_DEFAULT_NOISE_STREAMS: dict = {}


def default_noise_stream(device) -> NoiseStream:
    """the module's stream of ``device``, seeded from ``torch.initial_seed()`` at its first use"""
    device = _indexed_device(device)
    if device not in _DEFAULT_NOISE_STREAMS:
        _DEFAULT_NOISE_STREAMS[device] = NoiseStream(torch.initial_seed(), device)
    return _DEFAULT_NOISE_STREAMS[device]


def _noise_on_device(kind: int, img: torch.Tensor, amount, gray_noise) -> bool:
    """a contiguous fp32 device image the kernels take, with ``amount`` / ``gray_noise`` numbers or (B,) tensors"""
    if not (torch.is_tensor(img) and img.is_cuda and img.is_contiguous() and _ops.noise_ok(img, kind)):
        return False
    return all(_is_number(v) or (torch.is_tensor(v) and v.numel() == img.size(0)) for v in (amount, gray_noise))


def _noise_device(kind: int, img, stream, amount, gray_noise, flags: int, want_params: bool):
    n = _ops.noise
    state = (stream if stream is not None else default_noise_stream(img.device)).state(img.device)
    if flags & n.DRAW_PARAMS:
        (lo, hi), gray_scalar, amount_t, gray_t = amount, gray_noise, None, None
    else:
        as_vector = lambda v: None if _is_number(v) else v.detach().reshape(-1).to(device=img.device, dtype=torch.float32).contiguous()
        amount_t, gray_t = as_vector(amount), as_vector(gray_noise)
        lo = hi = float(amount) if amount_t is None else 0.0
        gray_scalar = float(gray_noise) if gray_t is None else 0.0
    with torch.no_grad():
        op = _ops.noise_gaussian if kind == n.GAUSSIAN else _ops.noise_poisson
        return op(img, state, amount_t, gray_t, float(lo), float(hi), float(gray_scalar), flags, want_params)


def _noise_flags(clip: bool, rounds: bool, quantise: bool) -> int:
    n = _ops.noise
    return (n.CLIP if clip else 0) | (n.ROUNDS if rounds else 0) | (n.QUANTISE if quantise else 0)


_NOISE_DOC = """

    A contiguous fp32 device tensor runs on ``csrc/oss_noise.hip`` (``torch.ops.vmambair.noise_{kind}``) under ``no_grad``, drawing
    from ``stream`` (a ``NoiseStream``; default: the module's stream of the device, seeded from ``torch.initial_seed()`` at its
    first use).  CPU tensors, other dtypes, non-contiguous views{extra} and shapes the kernels refuse take ``restate_{name}``, the
    package's operations in plain torch from torch's generator.  Deviations of the device path from the package: nothing is read
    back to the host -- the grey term is always evaluated and mixed with weight 0 or 1, which is algebraically the package's
    result, and the level census of the Poisson noise stays on the device; the Gaussian grey field is ONE (h, w) field shared by
    all samples, as the package has it, and a number ``sigma`` with grey noise works for any batch (the package can only view it
    for b = 1); the random numbers are Philox4x32-10 words (counter layout: include/vmambair_oss.h), not torch's, so a seed
    reproduces the distribution of the package's samples, not the samples."""


def _noise_doc(kind: str, name: str, extra: str = ""):
    def wrap(f):
        f.__doc__ += _NOISE_DOC.format(kind=kind, name=name, extra=extra)
        return f
    return wrap


@_noise_doc("gaussian", "generate_gaussian_noise_pt")
def generate_gaussian_noise_pt(img, sigma=10, gray_noise=0, *, stream: Optional[NoiseStream] = None):
    """basicsr.data.degradations.generate_gaussian_noise_pt: the noise ``randn * sigma / 255`` for ``img`` (B, C, h, w), colour noise
    mixed with grey noise by the weights ``gray_noise``; ``sigma`` and ``gray_noise`` are numbers or (B,) tensors."""
    if _noise_on_device(0, img, sigma, gray_noise):
        return _noise_device(0, img, stream, sigma, gray_noise, _ops.noise.ONLY, False)[0]
    return restate_generate_gaussian_noise_pt(img, sigma, gray_noise)


@_noise_doc("gaussian", "add_gaussian_noise_pt")
def add_gaussian_noise_pt(img, sigma=10, gray_noise=0, clip=True, rounds=False, *, stream: Optional[NoiseStream] = None,
                          quantise: bool = False):
    """basicsr.data.degradations.add_gaussian_noise_pt: ``img + generate_gaussian_noise_pt(img, sigma, gray_noise)``, then ``clip``
    to [0, 1] and / or ``rounds`` to multiples of 1 / 255.  ``quantise`` applies ``clamp((x * 255).round(), 0, 255) / 255`` last
    (MambaRealSR_model.py:248), on the device as a stage of the same launch."""
    if _noise_on_device(0, img, sigma, gray_noise):
        return _noise_device(0, img, stream, sigma, gray_noise, _noise_flags(clip, rounds, quantise), False)[0]
    out = restate_add_gaussian_noise_pt(img, sigma, gray_noise, clip, rounds)
    return restate_quantise(out) if quantise else out


@_noise_doc("gaussian", "random_generate_gaussian_noise_pt")
def random_generate_gaussian_noise_pt(img, sigma_range=(0, 10), gray_prob=0, *, stream: Optional[NoiseStream] = None,
                                      return_params: bool = False):
    """basicsr.data.degradations.random_generate_gaussian_noise_pt: ``sigma`` ~ U[sigma_range) and ``gray_noise`` = 1 with
    probability ``gray_prob`` per sample, then ``generate_gaussian_noise_pt``.  ``return_params``: -> (noise, sigma, gray_noise)
    with the (B,) values drawn (on the device: by the kernel)."""
    if _noise_on_device(0, img, 0, 0):
        n = _ops.noise
        out, params = _noise_device(0, img, stream, sigma_range, gray_prob, n.ONLY | n.DRAW_PARAMS, return_params)
        return (out, params[0], params[1]) if return_params else out
    sigma, gray_noise = _restate_random_params(img, sigma_range, gray_prob)
    out = restate_generate_gaussian_noise_pt(img, sigma, gray_noise)
    return (out, sigma, gray_noise) if return_params else out


@_noise_doc("gaussian", "random_add_gaussian_noise_pt")
def random_add_gaussian_noise_pt(img, sigma_range=(0, 10), gray_prob=0, clip=True, rounds=False, *,
                                 stream: Optional[NoiseStream] = None, return_params: bool = False, quantise: bool = False):
    """basicsr.data.degradations.random_add_gaussian_noise_pt, the first noise branch of ``feed_data`` (MambaRealSR_model.py:177-180,
    :209-212): ``img + random_generate_gaussian_noise_pt(img, sigma_range, gray_prob)``, then ``clip`` / ``rounds``.
    ``return_params``: -> (out, sigma, gray_noise); ``quantise``: ``clamp((x * 255).round(), 0, 255) / 255`` last."""
    if _noise_on_device(0, img, 0, 0):
        flags = _noise_flags(clip, rounds, quantise) | _ops.noise.DRAW_PARAMS
        out, params = _noise_device(0, img, stream, sigma_range, gray_prob, flags, return_params)
        return (out, params[0], params[1]) if return_params else out
    sigma, gray_noise = _restate_random_params(img, sigma_range, gray_prob)
    out = _restate_finish(img + restate_generate_gaussian_noise_pt(img, sigma, gray_noise), clip, rounds)
    out = restate_quantise(out) if quantise else out
    return (out, sigma, gray_noise) if return_params else out


@_noise_doc("poisson", "generate_poisson_noise_pt", ", images without exactly 3 channels")
def generate_poisson_noise_pt(img, scale=1.0, gray_noise=0, *, stream: Optional[NoiseStream] = None):
    """basicsr.data.degradations.generate_poisson_noise_pt: with ``q = clamp((img * 255).round(), 0, 255) / 255`` and ``vals`` = the
    next power of two >= the number of distinct values of ``q`` in a sample, ``(poisson(q * vals) / vals - q) * scale``; the grey
    noise likewise from the sample's grey image, one count per pixel for the three channels, mixed in by ``gray_noise``."""
    if _noise_on_device(1, img, scale, gray_noise):
        return _noise_device(1, img, stream, scale, gray_noise, _ops.noise.ONLY, False)[0]
    return restate_generate_poisson_noise_pt(img, scale, gray_noise)


@_noise_doc("poisson", "add_poisson_noise_pt", ", images without exactly 3 channels")
def add_poisson_noise_pt(img, scale=1.0, clip=True, rounds=False, gray_noise=0, *, stream: Optional[NoiseStream] = None,
                         quantise: bool = False):
    """basicsr.data.degradations.add_poisson_noise_pt (the package puts ``clip`` and ``rounds`` before ``gray_noise`` here):
    ``img + generate_poisson_noise_pt(img, scale, gray_noise)``, then ``clip`` / ``rounds``; ``quantise`` as in
    ``add_gaussian_noise_pt``."""
    if _noise_on_device(1, img, scale, gray_noise):
        return _noise_device(1, img, stream, scale, gray_noise, _noise_flags(clip, rounds, quantise), False)[0]
    out = restate_add_poisson_noise_pt(img, scale, clip, rounds, gray_noise)
    return restate_quantise(out) if quantise else out


@_noise_doc("poisson", "random_generate_poisson_noise_pt", ", images without exactly 3 channels")
def random_generate_poisson_noise_pt(img, scale_range=(0, 1.0), gray_prob=0, *, stream: Optional[NoiseStream] = None,
                                     return_params: bool = False):
    """basicsr.data.degradations.random_generate_poisson_noise_pt: ``scale`` ~ U[scale_range) and ``gray_noise`` = 1 with
    probability ``gray_prob`` per sample, then ``generate_poisson_noise_pt``.  ``return_params``: -> (noise, scale, gray_noise)."""
    if _noise_on_device(1, img, 0, 0):
        n = _ops.noise
        out, params = _noise_device(1, img, stream, scale_range, gray_prob, n.ONLY | n.DRAW_PARAMS, return_params)
        return (out, params[0], params[1]) if return_params else out
    scale, gray_noise = _restate_random_params(img, scale_range, gray_prob)
    out = restate_generate_poisson_noise_pt(img, scale, gray_noise)
    return (out, scale, gray_noise) if return_params else out


@_noise_doc("poisson", "random_add_poisson_noise_pt", ", images without exactly 3 channels")
def random_add_poisson_noise_pt(img, scale_range=(0, 1.0), gray_prob=0, clip=True, rounds=False, *,
                                stream: Optional[NoiseStream] = None, return_params: bool = False, quantise: bool = False):
    """basicsr.data.degradations.random_add_poisson_noise_pt, the second noise branch of ``feed_data`` (MambaRealSR_model.py:181-187,
    :213-219): ``img + random_generate_poisson_noise_pt(img, scale_range, gray_prob)``, then ``clip`` / ``rounds``.
    ``return_params``: -> (out, scale, gray_noise); ``quantise``: ``clamp((x * 255).round(), 0, 255) / 255`` last."""
    if _noise_on_device(1, img, 0, 0):
        flags = _noise_flags(clip, rounds, quantise) | _ops.noise.DRAW_PARAMS
        out, params = _noise_device(1, img, stream, scale_range, gray_prob, flags, return_params)
        return (out, params[0], params[1]) if return_params else out
    scale, gray_noise = _restate_random_params(img, scale_range, gray_prob)
    out = _restate_finish(img + restate_generate_poisson_noise_pt(img, scale, gray_noise), clip, rounds)
    out = restate_quantise(out) if quantise else out
    return (out, scale, gray_noise) if return_params else out


class TrainingPairPool:
    """``MambaRealSR._dequeue_and_enqueue`` (MambaRealSR_model.py:109-144): a pool of ``queue_size`` (lq, gt) pairs that mixes the
    degradations of several batches into one.  ``push_pop(lq, gt)`` while the pool fills only stores the batch and returns it
    unchanged; once full it draws ``idx = torch.randperm(queue_size)`` (the CPU default generator, exactly where the reference draws
    it, so the same seed gives the same stream), reorders the pool by ``idx``, hands out its first b pairs and puts the new batch in
    their place.  ``queue_size % b == 0`` is asserted at the first call.

    The reference copies the whole pool (``queue[idx]``, about 2 x 150 MB per step at queue 180) to reorder it; here the order is a
    slot permutation on the host and only the b pairs that leave and the b that enter move.  ``queue()`` gives the pool in the
    reference's order."""

    def __init__(self, queue_size: int):
        self.queue_size = int(queue_size)
        self.queue_lr: Optional[torch.Tensor] = None
        self.queue_gt: Optional[torch.Tensor] = None
        self.queue_ptr = 0
        self.slots = torch.arange(self.queue_size)   # position in the reference's queue -> row of queue_lr / queue_gt

    @torch.no_grad()
    def push_pop(self, lq: torch.Tensor, gt: torch.Tensor, perm: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        b, c, h, w = lq.size()
        if self.queue_lr is None:
            assert self.queue_size % b == 0, f'queue size {self.queue_size} should be divisible by batch size {b}'
            self.queue_lr = torch.zeros(self.queue_size, c, h, w, dtype=lq.dtype, device=lq.device)
            _, c, h, w = gt.size()
            self.queue_gt = torch.zeros(self.queue_size, c, h, w, dtype=gt.dtype, device=gt.device)
            self.queue_ptr = 0
        if self.queue_ptr == self.queue_size:   # the pool is full: shuffle, dequeue the first b, enqueue the batch there
            idx = torch.randperm(self.queue_size) if perm is None else torch.as_tensor(perm, dtype=torch.long, device='cpu')
            self.slots = self.slots[idx]
            rows = self.slots[:b].to(lq.device)
            lq_out, gt_out = self.queue_lr.index_select(0, rows), self.queue_gt.index_select(0, rows)
            self.queue_lr.index_copy_(0, rows, lq)
            self.queue_gt.index_copy_(0, rows, gt)
            return lq_out, gt_out
        self.queue_lr[self.queue_ptr:self.queue_ptr + b] = lq   # only enqueue
        self.queue_gt[self.queue_ptr:self.queue_ptr + b] = gt
        self.queue_ptr += b
        return lq, gt

    def queue(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """the pool in the reference's order (``queue_lr``, ``queue_gt`` of the reference after the same calls)"""
        rows = self.slots.to(self.queue_lr.device)
        return self.queue_lr.index_select(0, rows), self.queue_gt.index_select(0, rows)
