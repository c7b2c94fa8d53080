#!/usr/bin/env python3
"""Generate tests/golden/g13_pairs_pad.npz by RUNNING THE REFERENCE's Deraining data path: pad, crop, augment, convert, window.

Needs /root/reference (read-only); never runs on the GPU box.  Nothing of the reference is copied: its functions are compiled
out of the files where they lie (``make_golden._extract``) and only the input images and the arrays they return are stored.
Re-run with:  python tests/golden/make_golden_pairs_pad.py

What is run, in the order of ``Dataset_PairedImage.__getitem__`` (Deraining/basicsr/data/paired_image_dataset.py:101-118)
  * ``padding(img_gt, img_lq, gt_size)`` (Deraining/basicsr/utils/img_util.py:148-164)
  * ``paired_random_crop(., ., gt_size, 1, .)`` and ``data_augmentation(., mode)`` for the 8 modes (basicsr/data/transforms.py:24-83,
    :223-268; ``random_augmentation`` draws one mode for both images)
  * ``img2tensor(bgr2rgb=True, float32=True)`` (utils/img_util.py:9-33) on ``img.astype(np.float32) / 255.``
and then the window of the training loop, Deraining/basicsr/train.py:269-270 at scale 1: ``t[:, x0:x0 + m, y0:y0 + m]`` -- ``x0``
indexes ROWS, ``y0`` columns -- on the tensors ``img2tensor`` returned (one sample: no batch axis).
cv2 is not installed here, so the functions get a NumPy stand-in namespace with the calls they make:
  ``copyMakeBorder(img, 0, hp, 0, wp, BORDER_REFLECT)``   ``np.pad(img, ((0, hp), (0, wp), (0, 0)), mode="symmetric")``.  Both are
        the map fedcba|abcdefgh|hgfedcb: index i >= n reads r = i mod 2n, r < n ? r : 2n - 1 - r (OpenCV's ``borderInterpolate``
        loops ``p = n - 1 - (p - n)`` / ``p = -p - 1`` until 0 <= p < n, which is that map); any number of periods
  ``cvtColor(img, COLOR_BGR2RGB)``   the channel axis reversed (``img2tensor`` calls it for 3 channels only)
``paired_random_crop`` draws with the real ``random`` module (seeded); its (top, left) are re-derived by replaying the same two
``randint`` calls from the same seed.  The window offsets are fixed per case, inside the support {0 .. G - m - 1} of
``int((G - m) * random.random())`` ({0} when m == G).

The small images are independent random bytes.  The 33 x 70 images are ``img[y, x, c] = base[(3 y + x + 83 c) mod 251]`` with 251
random bytes per image: 16 float32 arrays of up to 3 x 96 x 96 would not fit a small fixture if every pixel were independent, while
here a row is its neighbour shifted by 3 pixels and the file compresses.  A displacement (dy, dx) goes unseen there only where
3 dy + dx = 0 mod 251, which no off-by-one in a row, a column, a reflection or a tile is; the tests with independent random pixels
at such sizes are those against the NumPy twin, which this file pins to the reference.

Stored per case ``<name>`` (uint8 HWC images ``<name>.gt`` / ``<name>.lq``; ``<name>.meta`` = G, m, top, left, x0, y0):
  ``<name>.modes.lq`` / ``.gt``       float32 (8, C, m, m): ``data_augmentation``'s modes 0..7
and ``options.<file>.iters`` / ``.mini_batch_sizes`` / ``.gt_sizes`` / ``.gt_size`` / ``.batch_size_per_gpu`` of the four
Deraining option files (settings only).  The members are LZMA-compressed (``zipfile.ZIP_LZMA``), which ``np.load`` reads as it does
deflate: the shifted rows repeat at distances and lengths deflate cannot use.
"""
import glob
import io
import os
import random
import re
import sys
import types
import zipfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, _extract  # noqa: E402

BORDER_REFLECT = 2

# name, (h, w), channels, G, m, (x0, y0), seed
CASES = (("p5x7_g16_m16", (5, 7), 3, 16, 16, (0, 0), 1),
         ("p5x7_g16_m4", (5, 7), 3, 16, 4, (11, 2), 2),
         ("p15x16_g16", (15, 16), 3, 16, 16, (0, 0), 3),
         ("p12x20_g16_m8", (12, 20), 3, 16, 8, (7, 3), 4),
         ("p33x70_g96_m96", (33, 70), 3, 96, 96, (0, 0), 5),
         ("p33x70_g96_m40", (33, 70), 3, 96, 40, (55, 17), 6),
         ("p31x31_c1_g32", (31, 31), 1, 32, 32, (0, 0), 7))


def _copy_make_border(img, top, bottom, left, right, kind):
    assert kind == BORDER_REFLECT and top == 0 and left == 0
    return np.pad(img, ((0, bottom), (0, right)) + ((0, 0),) * (img.ndim - 2), mode="symmetric")


def load_ref():
    cv2 = types.SimpleNamespace(copyMakeBorder=_copy_make_border, BORDER_REFLECT=BORDER_REFLECT, COLOR_BGR2RGB=4, cvtColor=lambda img, code: np.ascontiguousarray(img[..., ::-1]))
    ns = {"np": np, "cv2": cv2, "random": random}
    _extract(f"{REF}/Deraining/basicsr/data/transforms.py", ["paired_random_crop", "data_augmentation"], ns)
    ns_u = {"np": np, "torch": torch, "cv2": cv2}
    _extract(f"{REF}/Deraining/basicsr/utils/img_util.py", ["img2tensor", "padding"], ns_u)
    return ns, ns_u["padding"], ns_u["img2tensor"]


def option_lists():
    """the progressive-learning settings of Deraining/Deraining/Options/*.yml, read as text (PyYAML is not needed for five keys)"""
    out = {}
    for path in sorted(glob.glob(f"{REF}/Deraining/Deraining/Options/Deraining_mamber*.yml")):
        name, text = os.path.basename(path)[:-4], open(path).read()
        for key in ("iters", "mini_batch_sizes", "gt_sizes"):
            m = re.search(rf"^\s*{key}:\s*\[([0-9,\s]+)\]", text, re.M)
            out[f"options.{name}.{key}"] = np.array([int(v) for v in m.group(1).split(",")], dtype=np.int64)
        for key in ("gt_size", "batch_size_per_gpu"):
            out[f"options.{name}.{key}"] = np.array(int(re.search(rf"^\s*{key}:\s*(\d+)", text, re.M).group(1)), dtype=np.int64)
    assert len(out) == 20, sorted(out)
    return out


def main():
    ns, padding, img2tensor = load_ref()
    rng = np.random.RandomState(13)
    out = option_lists()
    for name, (h, w), ch, G, m, (x0, y0), seed in CASES:
        if h * w <= 1024:
            lq8, gt8 = (rng.randint(0, 256, (h, w, ch)).astype(np.uint8) for _ in range(2))
        else:
            at = (3 * np.arange(h)[:, None, None] + np.arange(w)[None, :, None] + 83 * np.arange(ch)[None, None, :]) % 251
            lq8, gt8 = (rng.randint(0, 256, 251).astype(np.uint8)[at] for _ in range(2))
        lq, gt = lq8.astype(np.float32) / 255., gt8.astype(np.float32) / 255.
        gt_p, lq_p = padding(gt, lq, G)
        hp, wp = max(h, G), max(w, G)
        assert gt_p.shape == lq_p.shape == (hp, wp, ch)
        random.seed(seed)
        gt_c, lq_c = ns["paired_random_crop"](gt_p, lq_p, G, 1, "golden")
        random.seed(seed)
        top, left = random.randint(0, hp - G), random.randint(0, wp - G)
        assert np.array_equal(lq_c, lq_p[top:top + G, left:left + G]) and gt_c.shape == (G, G, ch)
        assert 0 <= x0 <= max(G - m - 1, 0) and 0 <= y0 <= max(G - m - 1, 0)
        out[f"{name}.gt"], out[f"{name}.lq"] = gt8, lq8
        out[f"{name}.meta"] = np.array([G, m, top, left, x0, y0], dtype=np.int64)
        modes_gt, modes_lq = [], []
        for mode in range(8):
            g, l = (ns["data_augmentation"](x, mode).copy() for x in (gt_c, lq_c))
            g, l = img2tensor([g, l], bgr2rgb=True, float32=True)
            assert g.shape == l.shape == (ch, G, G)
            x1, y1 = x0 + m, y0 + m
            modes_gt.append(g[:, x0:x1, y0:y1].numpy())
            modes_lq.append(l[:, x0:x1, y0:y1].numpy())
        out[f"{name}.modes.gt"], out[f"{name}.modes.lq"] = np.stack(modes_gt), np.stack(modes_lq)
    path = os.path.join(OUT, "g13_pairs_pad.npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_LZMA) as f:     # an .npz is a zip of .npy members; np.load reads any method
        for key, value in out.items():                                       # zipfile knows, and deflate's 258-byte matches leave 121 KiB
            member = io.BytesIO()
            np.lib.format.write_array(member, np.asarray(value), allow_pickle=False)
            f.writestr(key + ".npy", member.getvalue())
    print(f"wrote g13_pairs_pad.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
