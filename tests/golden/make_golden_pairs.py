#!/usr/bin/env python3
"""Generate tests/golden/g11_pairs.npz by RUNNING THE REFERENCE's crop / augmentation / tensor conversion in the build container.

Needs /root/reference (read-only); never runs on the GPU box.  Nothing of the reference is copied: its functions are compiled
out of the files where they lie (``make_golden._extract``) and only the input images and the arrays they return are stored.
Re-run with:  python tests/golden/make_golden_pairs.py

What is run
  * ``paired_random_crop``, ``augment``, ``data_augmentation`` (Deraining/basicsr/data/transforms.py:24-83, :136-200, :223-268)
  * ``img2tensor(bgr2rgb=True, float32=True)`` (Deraining/basicsr/utils/img_util.py:9-33) on ``img.astype(np.float32) / 255.``
cv2 is not installed here, so the functions get a NumPy stand-in namespace with the two calls they make:
  ``flip(src, code, dst)``      code 1: columns reversed, code 0: rows reversed, written into ``dst`` (``augment`` flips in place)
  ``cvtColor(img, COLOR_BGR2RGB)``   the channel axis reversed
``paired_random_crop`` draws with the real ``random`` module (seeded); its (top, left) are re-derived by replaying the same two
``randint`` calls from the same seed.  ``augment`` draws its three coins from a scripted stand-in, one run per (hflip, vflip,
transpose) triple.

Stored per case ``<name>`` (uint8 BGR HWC images ``<name>.gt`` / ``<name>.lq``, ``<name>.meta`` = scale, LQ patch, top, left):
  ``<name>.mode<m>.lq`` / ``.gt``      m = 0..7: crop, ``data_augmentation(., m)``, ``img2tensor``  -> float32 (3, p, p) / (3, sp, sp)
  ``<name>.aug<h><v><t>.lq`` / ``.gt`` h, v, t in {0, 1}: crop, ``augment`` with those three outcomes, ``img2tensor``
"""
import os
import random
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, _extract  # noqa: E402


def _flip(src, code, dst=None):
    out = src[:, ::-1].copy() if code == 1 else src[::-1].copy()
    if dst is None:
        return out
    dst[...] = out
    return dst


class _Coins:
    """``random.random()`` for ``augment``: below 0.5 where the scripted outcome is True"""

    def __init__(self, outcomes):
        self.values = [0.25 if o else 0.75 for o in outcomes]

    def random(self):
        return self.values.pop(0)


def load_ref():
    cv2 = types.SimpleNamespace(flip=_flip, COLOR_BGR2RGB=4, cvtColor=lambda img, code: np.ascontiguousarray(img[..., ::-1]))
    ns = {"np": np, "cv2": cv2, "random": random}
    _extract(f"{REF}/Deraining/basicsr/data/transforms.py", ["paired_random_crop", "augment", "data_augmentation"], ns)
    ns_t = {"np": np, "torch": torch, "cv2": cv2}
    _extract(f"{REF}/Deraining/basicsr/utils/img_util.py", ["img2tensor"], ns_t)
    return ns, ns_t["img2tensor"]


def main():
    ns, img2tensor = load_ref()
    rng = np.random.RandomState(11)
    out = {}
    for name, scale, (h, w), patch, seed in (("s1_12x20", 1, (12, 20), 4, 5), ("s4_6x10", 4, (6, 10), 3, 9)):
        lq8 = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        gt8 = rng.randint(0, 256, (h * scale, w * scale, 3)).astype(np.uint8)
        lq, gt = lq8.astype(np.float32) / 255., gt8.astype(np.float32) / 255.
        random.seed(seed)
        gt_c, lq_c = ns["paired_random_crop"](gt, lq, patch, scale, "golden")
        random.seed(seed)
        top, left = random.randint(0, h - patch), random.randint(0, w - patch)
        assert np.array_equal(lq_c, lq[top:top + patch, left:left + patch]) and gt_c.shape == (patch * scale, patch * scale, 3)
        out[f"{name}.gt"], out[f"{name}.lq"] = gt8, lq8
        out[f"{name}.meta"] = np.array([scale, patch, top, left], dtype=np.int64)
        for m in range(8):
            g, l = (ns["data_augmentation"](x, m).copy() for x in (gt_c, lq_c))   # random_augmentation: one flag for both, .copy()
            g, l = img2tensor([g, l], bgr2rgb=True, float32=True)
            out[f"{name}.mode{m}.gt"], out[f"{name}.mode{m}.lq"] = g.numpy(), l.numpy()
        for hf in (0, 1):
            for vf in (0, 1):
                for tr in (0, 1):
                    ns["random"] = _Coins((hf, vf, tr))
                    g, l = ns["augment"]([gt_c.copy(), lq_c.copy()], True, True)
                    ns["random"] = random
                    g, l = img2tensor([np.ascontiguousarray(g), np.ascontiguousarray(l)], bgr2rgb=True, float32=True)
                    out[f"{name}.aug{hf}{vf}{tr}.gt"], out[f"{name}.aug{hf}{vf}{tr}.lq"] = g.numpy(), l.numpy()
    path = os.path.join(OUT, "g11_pairs.npz")
    np.savez_compressed(path, **out)
    print(f"wrote g11_pairs.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
