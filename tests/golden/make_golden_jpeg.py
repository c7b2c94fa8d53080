#!/usr/bin/env python3
"""Generate tests/golden/g16_jpeg.npz: inputs, qualities and float64 results for ``vmambair_amd.degradations.DiffJPEG``.

``DiffJPEG`` lives in the pip ``basicsr`` package (``basicsr.utils.diffjpeg``), which is neither in the reference tree nor
installed, so this script runs no reference code.  It holds an INDEPENDENT float64 evaluation of the published definition with
numpy and ``scipy.fft.dctn`` / ``idctn`` (``norm='ortho'``, per 8 x 8 block) and shares no code with the restatement in
``vmambair_amd/degradations.py``.  Needs scipy; never runs on the GPU box.
Re-run with:  python tests/golden/make_golden_jpeg.py

The definition (x (B, 3, h, w) in [0, 1], quality q per sample):
  factor = (5000 / q if q < 50 else 200 - 2 q) / 100;  zero padding at the bottom and right to multiples of 16;  p = 255 x
  Y = 0.299 R + 0.587 G + 0.114 B;  Cb = -0.168736 R - 0.331264 G + 0.5 B + 128;  Cr = 0.5 R - 0.418688 G - 0.081312 B + 128
  (the package's matrices are float32 constants: the float32 values of these decimals, here promoted to float64)
  Cb, Cr averaged over 2 x 2;  per 8 x 8 block F = DCT-II(block - 128), orthonormal;  v = F / (T factor);  c = round-half-even(v)
  T: the standard luminance table TRANSPOSED for Y, the chrominance table for Cb and Cr
  block' = IDCT(c T factor) + 128;  Cb', Cr' replicated 2 x 2
  R = Y' + 1.402 (Cr' - 128);  G = Y' - 0.344136 (Cb' - 128) - 0.714136 (Cr' - 128);  B = Y' + 1.772 (Cb' - 128)
  out = clip(., 0, 255) / 255, cropped to h x w

Stored per case <n> (float32 inputs, float64 results):
  <n>.x    the input            <n>.q    the qualities, float32 (B,); ``<n>.scalar`` = 1 where the test passes q[0] as a Python number
  <n>.out  the float64 output   <n>.vy, <n>.vcb, <n>.vcr   the UNROUNDED scaled coefficients v = F / (T factor), (B, blocks, 8, 8)
Cases (the smallest at which the kernel can still go wrong):
  mb1    (1, 3, 16, 16)   one exact macroblock, scalar 50          pad    (2, 3, 1, 1)   everything but one pixel is padding
  low    (1, 3, 8, 24)    less than a macroblock high, scalar 30   edges  (3, 3, 17, 33) partial macroblocks on both edges,
  rect   (2, 3, 48, 40)   non-square, 50 and 72.3                         30, 95, 49.5: both branches of the factor
  odd    (1, 3, 80, 144)  45 macroblocks, an odd count: any grouping of macroblocks per workgroup has a tail; scalar 88
Inputs alternate between a smooth field plus noise and plain uniform noise, rounded to float32.
"""
import os

import numpy as np
from scipy import fft

OUT = os.path.dirname(os.path.abspath(__file__))
TAU = 0.01   # tests/test_jpeg_gpu.py: the band around the half-integers inside which the device may round the other way

Y_STANDARD = np.array([[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56],
                       [14, 17, 22, 29, 51, 87, 80, 62], [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92],
                       [49, 64, 78, 87, 103, 121, 120, 101], [72, 92, 95, 98, 112, 100, 103, 99]], np.float64)
T_Y = Y_STANDARD.T
T_C = np.full((8, 8), 99.0)
T_C[:4, :4] = [[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]]
assert list(T_Y[0]) == [16, 12, 14, 14, 18, 24, 49, 72] and np.array_equal(T_C, T_C.T)
FWD = np.array([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]], np.float32).astype(np.float64)
INV = np.array([[1.0, 0.0, 1.402], [1.0, -0.344136, -0.714136], [1.0, 1.772, 0.0]], np.float32).astype(np.float64)


def factor_f64(q):
    q = np.asarray(q, np.float64)
    return np.where(q < 50, 5000.0 / q, 200.0 - 2.0 * q) / 100.0


def to_blocks(plane):
    """(B, H, W) -> (B, H W / 64, 8, 8), blocks row-major"""
    b, hh, ww = plane.shape
    return plane.reshape(b, hh // 8, 8, ww // 8, 8).transpose(0, 1, 3, 2, 4).reshape(b, -1, 8, 8)


def from_blocks(blocks, hh, ww):
    b = blocks.shape[0]
    return blocks.reshape(b, hh // 8, ww // 8, 8, 8).transpose(0, 1, 3, 2, 4).reshape(b, hh, ww)


def compress_f64(x, q):
    """-> the unrounded scaled coefficients (vy, vcb, vcr) of the padded image"""
    x = np.asarray(x, np.float64)
    b, _, h, w = x.shape
    p = np.pad(x, ((0, 0), (0, 0), (0, -h % 16), (0, -w % 16))) * 255.0
    ycc = np.einsum('kc,bchw->bkhw', FWD, p) + np.array([0.0, 128.0, 128.0])[None, :, None, None]
    hh, ww = p.shape[2:]
    sub = ycc[:, 1:].reshape(b, 2, hh // 2, 2, ww // 2, 2).mean(axis=(3, 5))
    f = factor_f64(q)[:, None, None, None]
    out = []
    for plane, table in ((ycc[:, 0], T_Y), (sub[:, 0], T_C), (sub[:, 1], T_C)):
        out.append(fft.dctn(to_blocks(plane) - 128.0, type=2, axes=(-2, -1), norm='ortho') / (table * f))
    return out


def decompress_f64(cy, ccb, ccr, q, h, w):
    """quantised coefficients of the padded image -> the float64 output (B, 3, h, w)"""
    hh, ww = h + -h % 16, w + -w % 16
    f = factor_f64(q)[:, None, None, None]
    planes = []
    for c, table, (ph, pw) in ((cy, T_Y, (hh, ww)), (ccb, T_C, (hh // 2, ww // 2)), (ccr, T_C, (hh // 2, ww // 2))):
        planes.append(from_blocks(fft.idctn(np.asarray(c, np.float64) * (table * f), type=2, axes=(-2, -1), norm='ortho') + 128.0, ph, pw))
    y, cb, cr = planes[0], *(np.repeat(np.repeat(pl, 2, axis=1), 2, axis=2) - 128.0 for pl in planes[1:])
    rgb = np.einsum('ck,bkhw->bchw', INV, np.stack([y, cb, cr], axis=1))
    return (np.clip(rgb, 0.0, 255.0) / 255.0)[:, :, :h, :w]


def image(rng, shape, kind):
    b, c, h, w = shape
    if kind:   # plain uniform noise
        return rng.rand(*shape).astype(np.float32)
    yy, xx = np.meshgrid(np.arange(h) / max(h - 1, 1), np.arange(w) / max(w - 1, 1), indexing='ij')
    phase = rng.rand(b, c, 1, 1) * 2 * np.pi
    field = 0.5 + 0.3 * np.sin(2.2 * np.pi * xx + phase) * np.cos(1.7 * np.pi * yy + 0.5 * phase) + 0.1 * (xx - yy)
    return np.clip(field + 0.08 * (rng.rand(*shape) - 0.5), 0.0, 1.0).astype(np.float32)


CASES = (("mb1", (1, 3, 16, 16), (50.0,), True), ("pad", (2, 3, 1, 1), (61.0, 38.0), False), ("low", (1, 3, 8, 24), (30.0,), True),
         ("edges", (3, 3, 17, 33), (30.0, 95.0, 49.5), False), ("rect", (2, 3, 48, 40), (50.0, 72.3), False),
         ("odd", (1, 3, 80, 144), (88.0,), True))


def main():
    rng = np.random.RandomState(16)
    out = {}
    for n, (name, shape, quality, scalar) in enumerate(CASES):
        x = np.concatenate([image(rng, (1,) + shape[1:], (n + b) % 2) for b in range(shape[0])])
        q = np.asarray(quality, np.float32)
        v = compress_f64(x, q)
        flat = np.concatenate([a.ravel() for a in v])
        dist = np.abs(np.abs(flat - np.floor(flat)) - 0.5)   # distance to the nearest half-integer
        share = float(np.mean(dist < TAU))
        print(f"{name:6s}{str(shape):18s} {flat.size:6d} coefficients, max |v| {np.abs(flat).max():7.1f}, within {TAU} of a "
              f"half-integer: {100 * share:.2f} %, nearest {dist.min():.2e}")
        assert share <= 0.03 and dist.min() > 1e-6, name   # test (b); and no value that float64 round-off could flip
        res = decompress_f64(*(np.rint(a) for a in v), q, *shape[2:])
        out.update({f"{name}.x": x, f"{name}.q": q, f"{name}.scalar": np.int64(scalar), f"{name}.out": res,
                    f"{name}.vy": v[0], f"{name}.vcb": v[1], f"{name}.vcr": v[2]})
    path = os.path.join(OUT, "g16_jpeg.npz")
    np.savez_compressed(path, **out)
    print(f"wrote g16_jpeg.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
