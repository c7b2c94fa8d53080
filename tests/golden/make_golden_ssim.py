#!/usr/bin/env python3
"""Generate tests/golden/g10_ssim.npz by RUNNING THE REFERENCE's SSIM / PSNR functions in the build container.

Needs /root/reference (read-only) and scipy; never runs on the GPU box.  Nothing of the reference is copied: its functions are
compiled out of the files where they lie (``make_golden._extract``) and only the input images and the numbers they return are
stored.  Re-run with:  python tests/golden/make_golden_ssim.py

What is run
  * ``_ssim``, ``_ssim_cly``, ``calculate_ssim`` (Deraining/basicsr/metrics/psnr_ssim.py:66-99, :184-222, :225-303) with
    ``reorder_image`` / ``to_y_channel`` (metrics/metric_util.py) and ``calculate_psnr`` (:9-63)
  * ``calculate_ssim`` / ``ssim`` of Deraining/Deraining/utils.py:31-78 -- the per-channel "valid" form
  * ``tensor2img`` (SRGAN/VmambaIR/utils/img_util.py:36-95)
cv2 is not installed here, so the functions get a stand-in namespace with the two calls they make:
  ``getGaussianKernel(k, s)``   exp(-(i - (k - 1) / 2)^2 / (2 s^2)), normalised, (k, 1) float64
  ``filter2D(img, -1, w, borderType=...)``   scipy.ndimage.correlate in float64, mode "nearest" for BORDER_REPLICATE, else
                                "mirror" (cv2's default BORDER_REFLECT_101; ``_ssim`` slices [5:-5, 5:-5], so it never shows)

Stored per case ``<name>`` and crop c in {0, 4} (uint8 BGR HWC images a = ``<name>.a`` and b = a + ``<name>.d``):
  ``ssim_valid_rgb_c``      utils.calculate_ssim(a, b, border=c): mean of the per-channel ``ssim``
  ``ssim_valid_y_c``        crop, to_y_channel, ``_ssim`` (the calculate_ssim of the released basicsr package)
  ``ssim_replicate_y_c``    psnr_ssim.calculate_ssim(a, b, c, test_y_channel=True) -> ``_ssim_cly``
  ``psnr_c_y0`` / ``_y1``   psnr_ssim.calculate_psnr(a, b, c, test_y_channel=False / True)
"""
import math
import os
import sys
import types

import numpy as np
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, _extract, load_by_path  # noqa: E402


def _gaussian_kernel(ksize, sigma):
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) / 2.0
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return (g / g.sum()).reshape(ksize, 1)


BORDER_REPLICATE = 1


def _filter2d(img, ddepth, window, borderType=None):
    assert ddepth == -1 and img.dtype == np.float64 and img.ndim == 2
    return ndimage.correlate(img, window, mode="nearest" if borderType == BORDER_REPLICATE else "mirror")


def load_ref_ssim():
    cv2 = types.SimpleNamespace(getGaussianKernel=_gaussian_kernel, filter2D=_filter2d, BORDER_REPLICATE=BORDER_REPLICATE,
                                COLOR_RGB2BGR=4, cvtColor=lambda img, code: np.ascontiguousarray(img[..., ::-1]))
    mf = load_by_path("ref_matlab_functions", f"{REF}/Deraining/basicsr/utils/matlab_functions.py")
    ns = {"np": np, "torch": torch, "cv2": cv2, "bgr2ycbcr": mf.bgr2ycbcr}
    _extract(f"{REF}/Deraining/basicsr/metrics/metric_util.py", ["reorder_image", "to_y_channel"], ns)
    _extract(f"{REF}/Deraining/basicsr/metrics/psnr_ssim.py", ["calculate_psnr", "_ssim", "_ssim_cly", "calculate_ssim"], ns)
    ns_u = {"np": np, "cv2": cv2, "math": math}
    _extract(f"{REF}/Deraining/Deraining/utils.py", ["calculate_ssim", "ssim"], ns_u)
    ns_t = {"np": np, "torch": torch, "math": math, "cv2": cv2, "make_grid": None}
    _extract(f"{REF}/SRGAN/VmambaIR/utils/img_util.py", ["tensor2img"], ns_t)
    return ns, ns_u, ns_t["tensor2img"]


def main():
    ns, ns_u, tensor2img = load_ref_ssim()
    rng = np.random.RandomState(0)
    images = {}

    def noisy(a, n):
        return np.clip(a.astype(np.int32) + rng.randint(-n, n + 1, a.shape), 0, 255).astype(np.uint8)

    for name, (h, w), n in (("u8_40x52", (40, 52), 12), ("u8_33x47", (33, 47), 3), ("u8_128x160", (128, 160), 1)):
        a = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        images[name] = (a, noisy(a, n))
    i, j = np.meshgrid(np.arange(96), np.arange(96), indexing="ij")
    ramp = np.repeat(((i + j) % 256).astype(np.uint8)[..., None], 3, axis=2)     # smooth: E[x^2] - mu^2 cancels (fp32 fails here)
    images["ramp_96x96"] = (ramp, noisy(ramp, 1))
    a = rng.randint(0, 256, (19, 19, 3)).astype(np.uint8)                       # one window at crop 4
    images["u8_19x19"] = (a, noisy(a, 6))
    a = rng.randint(0, 256, (30, 34, 3)).astype(np.uint8)
    images["same_30x34"] = (a, a.copy())                                         # SSIM 1, PSNR inf
    a = rng.randint(0, 256, (25, 31)).astype(np.uint8)
    images["grey_25x31"] = (a, noisy(a, 8))
    # float tensors reaching outside [0, 1], through the reference's tensor2img (clones: it clamps CPU tensors in place)
    ta = torch.from_numpy((rng.rand(1, 3, 24, 28) * 1.4 - 0.2).astype(np.float32))
    tb = ta + 0.04 * torch.from_numpy(rng.randn(1, 3, 24, 28).astype(np.float32))
    images["t2i_24x28"] = (tensor2img([ta.clone()]), tensor2img([tb.clone()]))

    out = {"t2i_24x28.ta": ta.numpy(), "t2i_24x28.tb": tb.numpy()}
    for name, (a, b) in images.items():
        out[f"{name}.a"], out[f"{name}.d"] = a, b.astype(np.int16) - a      # b = a + d: small differences compress, random bytes do not
        for crop in (0, 4):
            ac = a[crop:a.shape[0] - crop, crop:a.shape[1] - crop].astype(np.float64)
            bc = b[crop:b.shape[0] - crop, crop:b.shape[1] - crop].astype(np.float64)
            ya, yb = ns["to_y_channel"](ac), ns["to_y_channel"](bc)
            if ya.ndim == 3:
                ya, yb = ya[..., 0], yb[..., 0]
            out[f"{name}.ssim_valid_rgb_{crop}"] = np.float64(ns_u["calculate_ssim"](a, b, border=crop))
            out[f"{name}.ssim_valid_y_{crop}"] = np.float64(ns["_ssim"](ya, yb))
            out[f"{name}.ssim_replicate_y_{crop}"] = np.float64(ns["calculate_ssim"](a, b, crop, "HWC", True))
            for yc in (False, True):
                out[f"{name}.psnr_{crop}_y{int(yc)}"] = np.float64(ns["calculate_psnr"](a, b, crop, "HWC", yc))
    path = os.path.join(OUT, "g10_ssim.npz")
    np.savez_compressed(path, **out)
    print(f"wrote g10_ssim.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
