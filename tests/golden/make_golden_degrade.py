#!/usr/bin/env python3
"""Generate tests/golden/g15_degrade.npz: inputs, kernels and float64 results for ``vmambair_amd.degradations``.

``filter2D`` and ``USMSharp`` live in the pip ``basicsr`` package, which is neither in the reference tree nor installed, so this
script does not run reference code for them.  It holds an INDEPENDENT float64 evaluation of the published formulas --
``scipy.ndimage.correlate(plane, kernel, mode='mirror')`` per plane: cross-correlation, no flip, mirror without repeating the edge
pixel = torch's 'reflect' -- and the test kernels.  The pair-pool trace does come from the reference: ``_dequeue_and_enqueue`` is
compiled out of RealSR/VmambaIR/models/MambaRealSR_model.py where it lies (``make_golden._extract``), with ``.cuda()`` a no-op and
``torch.randperm`` recorded.  Needs /root/reference (read-only) and scipy; never runs on the GPU box.
Re-run with:  python tests/golden/make_golden_degrade.py

Stored (float32 inputs, float64 results; the exact integer results as int32):
  ex.<s>.img, ex.<s>.<kern>, ex.<s>.<kern>.out   exactly summable: img holds integers 0...255, the per-sample kernels integers in
        {-2...2} (non-zero at the four corners), so every partial sum is an integer below 2^24 and fp32 must reproduce float64 bit
        for bit in any order.  s = a (3, 2, 11, 13: every window reflects on both sides), b (2, 3, 45, 70: ragged tiles);
        kern = k21, k3, k7 and k7pad (a 7-tap kernel zero-padded to 21: the support-trimming path)
  ro.img, ro.kernels, ro.out    round-off: img in [0, 1] (3, 1, 45, 70), per-sample 21 x 21 kernels: isotropic Gaussian, rotated
        anisotropic Gaussian, circular low-pass (sinc, negative lobes)
  sep.g, sep.<s>.img, sep.<s>.out    the rank-1 kernel g g^T of the 51-vector (sigma 8) at s = a (2, 1, 26, 26: the smallest legal
        size, pad 25), b (1, 3, 27, 33)
  usm.kernel, usm.<s>.img / .mask / .blur / .out (the last two not for c)    USMSharp (weight 0.5, threshold 10) with the
        (1, 51, 51) float32 buffer float32(g g^T); inputs: smoothed noise stretched to [0, 1] plus a step edge, so that the mask
        holds 0.69-0.81 of the pixels and the clip is active; s = a (1, 3, 27, 33), b (2, 1, 26, 26), c (2, 3, 64, 80)
  pool.lq, pool.gt (7 calls of b = 2), pool.perm (the recorded permutation per call, -1 while the pool of 6 fills), pool.lq_out,
        pool.gt_out, pool.queue_lr, pool.queue_gt (the reference's queue after the 7 calls)
"""
import os
import sys

import numpy as np
import torch
from scipy import ndimage, special

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, _extract  # noqa: E402


# ---- the float64 evaluation -------------------------------------------------------------------------------------------------------
def filter2d_f64(img, kernel):
    """img (B, C, H, W), kernel (1 or B, k, k) -> float64 (B, C, H, W)"""
    img, kernel = np.asarray(img, np.float64), np.asarray(kernel, np.float64)
    return np.stack([np.stack([ndimage.correlate(img[b, c], kernel[b if kernel.shape[0] > 1 else 0], mode='mirror')
                               for c in range(img.shape[1])]) for b in range(img.shape[0])])


def gaussian_vector(k, sigma=0):
    s = sigma if sigma > 0 else 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    x = np.arange(k) - (k - 1) / 2
    g = np.exp(-x * x / (2 * s * s))
    return g / g.sum()


def usm_f64(img, kernel, weight=0.5, threshold=10, mask=None):
    img = np.asarray(img, np.float64)
    blur = filter2d_f64(img, kernel)
    residual = img - blur
    if mask is None:
        mask = (np.abs(residual) * 255 > threshold).astype(np.float64)
    soft = filter2d_f64(mask, kernel)
    sharp = np.clip(img + weight * residual, 0, 1)
    return blur, mask, soft * sharp + (1 - soft) * img


# ---- the test kernels -------------------------------------------------------------------------------------------------------------
def integer_kernel(rng, b, k):
    w = rng.randint(-2, 3, size=(b, k, k)).astype(np.float32)
    for i, j in ((0, 0), (0, k - 1), (k - 1, 0), (k - 1, k - 1)):
        w[:, i, j] = rng.choice([-2.0, -1.0, 1.0, 2.0], size=b)
    return w


def bivariate_gaussian(k, sig_x, sig_y, theta):
    """exp(-0.5 v^T S^-1 v) on the k x k grid, S = R diag(sig_x^2, sig_y^2) R^T, normalised to sum 1"""
    ax = np.arange(k) - (k - 1) / 2
    xx, yy = np.meshgrid(ax, ax)
    r = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
    inv = np.linalg.inv(r @ np.diag([sig_x ** 2, sig_y ** 2]) @ r.T)
    v = np.stack([xx, yy], -1)
    w = np.exp(-0.5 * np.einsum('...i,ij,...j->...', v, inv, v))
    return w / w.sum()


def circular_lowpass(k, cutoff):
    """the 2-D sinc: cutoff * J1(cutoff r) / (2 pi r), cutoff^2 / (4 pi) at r = 0, normalised to sum 1"""
    ax = np.arange(k) - (k - 1) / 2
    xx, yy = np.meshgrid(ax, ax)
    r = np.sqrt(xx * xx + yy * yy)
    with np.errstate(invalid='ignore', divide='ignore'):
        w = cutoff * special.j1(cutoff * r) / (2 * np.pi * r)
    w[(k - 1) // 2, (k - 1) // 2] = cutoff ** 2 / (4 * np.pi)
    return w / w.sum()


def usm_image(seed, shape):
    """smoothed noise stretched to [0, 1] plus a step edge"""
    r = np.random.RandomState(seed)
    n, c, h, w = shape
    a = r.rand(n, c, h, w)
    a = ndimage.gaussian_filter(a, (0, 0, 1.5, 1.5), mode='mirror')
    a = (a - a.min()) / (a.max() - a.min())
    a[..., h // 3:, w // 2:] = np.clip(a[..., h // 3:, w // 2:] * 0.5 + 0.5, 0, 1)
    return a.astype(np.float32)


# ---- the reference's pair pool ----------------------------------------------------------------------------------------------------
def pool_trace(rng, queue_size=6, b=2, calls=7):
    perms = []

    class Recorder:
        """torch with a recording randperm"""
        def __getattr__(self, name):
            return getattr(torch, name)

        @staticmethod
        def randperm(n):
            perms.append(torch.randperm(n))
            return perms[-1]

    ns = _extract(f"{REF}/RealSR/VmambaIR/models/MambaRealSR_model.py", ["_dequeue_and_enqueue"], {"torch": Recorder()},
                  cls="MambaRealSR")

    class Model:
        pass

    m = Model()
    m.queue_size = queue_size
    cuda, torch.Tensor.cuda = torch.Tensor.cuda, lambda self, *a, **k: self
    try:
        torch.manual_seed(15)
        lq = torch.from_numpy(rng.rand(calls, b, 1, 2, 3).astype(np.float32))
        gt = torch.from_numpy(rng.rand(calls, b, 1, 4, 6).astype(np.float32))
        lq_out, gt_out, perm = [], [], []
        for i in range(calls):
            m.lq, m.gt, n = lq[i].clone(), gt[i].clone(), len(perms)
            ns["_dequeue_and_enqueue"](m)
            lq_out.append(m.lq.clone()), gt_out.append(m.gt.clone())
            perm.append(perms[-1].numpy() if len(perms) > n else np.full(queue_size, -1))
    finally:
        torch.Tensor.cuda = cuda
    assert len(perms) == calls - queue_size // b
    return {"pool.lq": lq.numpy(), "pool.gt": gt.numpy(), "pool.perm": np.stack(perm).astype(np.int64),
            "pool.lq_out": torch.stack(lq_out).numpy(), "pool.gt_out": torch.stack(gt_out).numpy(),
            "pool.queue_lr": m.queue_lr.numpy(), "pool.queue_gt": m.queue_gt.numpy()}


def main():
    rng = np.random.RandomState(15)
    out = {}
    for s, shape in (("a", (3, 2, 11, 13)), ("b", (2, 3, 45, 70))):
        img = rng.randint(0, 256, size=shape).astype(np.float32)
        out[f"ex.{s}.img"] = img
        k7pad = np.zeros((shape[0], 21, 21), np.float32)
        k7pad[:, 7:14, 7:14] = integer_kernel(rng, shape[0], 7)
        for name, kern in (("k21", integer_kernel(rng, shape[0], 21)), ("k3", integer_kernel(rng, shape[0], 3)),
                           ("k7", integer_kernel(rng, shape[0], 7)), ("k7pad", k7pad)):
            if kern.shape[-1] // 2 >= min(shape[2:]):
                continue
            out[f"ex.{s}.{name}"] = kern
            want = filter2d_f64(img, kern)
            assert np.array_equal(want, np.rint(want)) and 441 * 2 * 255 < 2 ** 24
            out[f"ex.{s}.{name}.out"] = want.astype(np.int32)   # integers: stored as such

    img = rng.rand(3, 1, 45, 70).astype(np.float32)
    kernels = np.stack([bivariate_gaussian(21, 2.5, 2.5, 0.0), bivariate_gaussian(21, 3.0, 1.0, 0.7),
                        circular_lowpass(21, np.pi / 3)]).astype(np.float32)
    assert kernels[2].min() < 0
    out.update({"ro.img": img, "ro.kernels": kernels, "ro.out": filter2d_f64(img, kernels)})

    g = gaussian_vector(51)
    g32 = g.astype(np.float32)
    out["sep.g"] = g32
    for s, shape in (("a", (2, 1, 26, 26)), ("b", (1, 3, 27, 33))):
        img = rng.rand(*shape).astype(np.float32)
        out[f"sep.{s}.img"] = img
        out[f"sep.{s}.out"] = filter2d_f64(img, np.outer(g32.astype(np.float64), g32.astype(np.float64))[None])

    kernel = np.outer(g, g).astype(np.float32)[None]
    out["usm.kernel"] = kernel
    for seed, (s, shape) in enumerate((("a", (1, 3, 27, 33)), ("b", (2, 1, 26, 26)), ("c", (2, 3, 64, 80)))):
        img = usm_image(seed, shape)
        blur, mask, sharp = usm_f64(img, kernel)
        out.update({f"usm.{s}.img": img, f"usm.{s}.mask": mask.astype(np.uint8)})
        if s != "c":   # the largest case keeps the fixture small: its float64 values are recomputed by the float64 restatement,
            out.update({f"usm.{s}.blur": blur, f"usm.{s}.out": sharp})   # which tests/test_degrade_host.py pins to these two
        clip = np.mean((img + 0.5 * (img - blur) > 1) | (img + 0.5 * (img - blur) < 0))
        print(f"usm.{s}: mask share {mask.mean():.3f}, clip active on {clip:.4f}")

    out.update(pool_trace(rng))
    path = os.path.join(OUT, "g15_degrade.npz")
    np.savez_compressed(path, **out)
    print(f"wrote g15_degrade.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
