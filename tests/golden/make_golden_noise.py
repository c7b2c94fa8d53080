#!/usr/bin/env python3
"""Generate tests/golden/g17_noise.npz: inputs, random fields and float64 results for the Gaussian noise functions of
``vmambair_amd.degradations``, and inputs with the expected level counts for the Poisson ones.

``generate_gaussian_noise_pt`` / ``generate_poisson_noise_pt`` and their siblings live in the pip ``basicsr`` package
(``basicsr.data.degradations``), which is neither in the reference tree nor installed, so this script runs no reference and no
package code.  It holds an INDEPENDENT float64 evaluation of the published definitions with numpy and shares no code with the
restatement in ``vmambair_amd/degradations.py``.  The random fields come from torch's CPU generator, drawn in float64 in the order
the package draws them (``rand(b)`` twice for the random_* forms, ``randn(h, w)`` when grey noise is drawn, ``randn(b, c, h, w)``), so
that a restatement that follows the package reproduces them from the same seed.  Needs torch and numpy; never runs on the GPU box.
Re-run with:  python tests/golden/make_golden_noise.py

The definitions (img (b, c, h, w); sigma, gray numbers or (b,) vectors seen as (b, 1, 1, 1)):
  Gaussian  noise = randn(b, c, h, w) sigma / 255;  with grey noise (gray > 0, or sum(gray) > 0 for a vector):
            noise = noise (1 - gray) + (randn(h, w) sigma / 255) gray -- ONE (h, w) field for all samples and channels
  Poisson   q = clip(round(255 img), 0, 255) / 255;  vals_b = 2 ** ceil(log2(number of distinct q in sample b, all channels));
            g = clip(round(255 (0.2989 R + 0.587 G + 0.114 B)), 0, 255) / 255, vals likewise from g
  add_*     out = img + noise;  clip and rounds: clip(round(255 out), 0, 255) / 255;  clip: clip(out, 0, 1);  rounds: round(255 out) / 255
  random_*  sigma = rand(b) (hi - lo) + lo;  gray = (rand(b) < gray_prob)

Stored per Gaussian case <n>: <n>.x the input (float64), <n>.seed, <n>.sigma and <n>.gray ((b,) float64; ``<n>.numbers`` = 1 where the
test passes sigma[0] and gray[0] as Python numbers), <n>.range = (lo, hi, gray_prob) for the random forms (then sigma and gray are
what the generator drew), <n>.noise the float64 noise and <n>.out_c, <n>.out_r, <n>.out_cr the three clip / rounds combinations.
Cases:
  num     (1, 3, 5, 7)  numbers 10, 0: no grey draw          grey1   (1, 3, 5, 7)  numbers 25, 1: all grey (the package can view the
  vec     (3, 3, 6, 5)  sigma 1, 15, 30; gray 0, 1, 1                               grey field of a NUMBER sigma only for b = 1)
  vec0    (2, 3, 4, 4)  a gray vector of zeros: no grey draw  c1      (2, 1, 4, 4)  one channel, gray 1, 0
  c4      (2, 4, 3, 3)  four channels, gray 0, 1              rand    (4, 3, 5, 5)  random forms, range (1, 30), gray_prob 0.4
Poisson: p.x (7, 3, 12, 12) float32 images with exactly 1, 2, 3, 128, 129, 256 distinct levels over all channels and one with 100
levels confined to channel 1; p.vals_c, p.vals_g the expected vals, p.q, p.g the quantised images.  Every grey value 255 (0.2989 R +
...) keeps at least 1e-3 from a half-integer, so fp32 and float64 agree on its level.
"""
import math
import os

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))


def finish(v, clip, rounds):
    if clip and rounds:
        return np.clip(np.rint(v * 255.0), 0, 255) / 255.0
    if clip:
        return np.clip(v, 0, 1)
    if rounds:
        return np.rint(v * 255.0) / 255.0
    return v


def gaussian_case(name, shape, seed, sigma=None, gray=None, numbers=False, rng=None):
    b, c, h, w = shape
    torch.manual_seed(1000 + seed)
    x = (torch.rand(shape, dtype=torch.float64) * 1.2 - 0.1).numpy()          # beyond [0, 1] on both sides: the clip matters
    torch.manual_seed(seed)
    if rng is not None:
        lo, hi, prob = rng
        sigma = torch.rand(b, dtype=torch.float64).numpy() * (hi - lo) + lo
        gray = (torch.rand(b, dtype=torch.float64).numpy() < prob).astype(np.float64)
    sigma, gray = np.asarray(sigma, np.float64), np.asarray(gray, np.float64)
    s, g = sigma.reshape(b, 1, 1, 1), gray.reshape(b, 1, 1, 1)
    grey_drawn = gray.sum() > 0
    if grey_drawn:
        field = torch.randn(h, w, dtype=torch.float64).numpy()
    noise = torch.randn(shape, dtype=torch.float64).numpy() * s / 255.0
    if grey_drawn:
        noise = noise * (1 - g) + (field * s / 255.0).reshape(b, 1, h, w) * g
    out = {f"{name}.x": x, f"{name}.seed": np.int64(seed), f"{name}.sigma": sigma, f"{name}.gray": gray,
           f"{name}.numbers": np.int64(numbers), f"{name}.noise": noise}
    if rng is not None:
        out[f"{name}.range"] = np.asarray(rng, np.float64)
    for tag, (clip, rounds) in (("c", (True, False)), ("r", (False, True)), ("cr", (True, True))):
        out[f"{name}.out_{tag}"] = finish(x + noise, clip, rounds)
    return out


def levels_image(rng, n_levels, channel=None):
    """(3, 12, 12) float32 with exactly ``n_levels`` distinct levels k / 255 (over all channels, or in ``channel`` with the others
    0, which then counts as one of them)"""
    levels = np.sort(rng.choice(np.arange(1, 256), n_levels - 1, replace=False)) if channel is not None else \
        np.sort(rng.choice(256, n_levels, replace=False))
    img = np.zeros((3, 144), np.int64)
    if channel is None:
        flat = np.concatenate([levels, rng.choice(levels, 3 * 144 - n_levels)])
        img = rng.permutation(flat).reshape(3, 144)
    else:
        img[channel] = rng.permutation(np.concatenate([levels, rng.choice(levels, 144 - len(levels))]))
    return (img.astype(np.float32) / np.float32(255)).reshape(3, 12, 12)


def poisson_part():
    rng = np.random.default_rng(17)
    counts = (1, 2, 3, 128, 129, 256)
    for _ in range(200):                                    # redraw until every grey value is clear of a level boundary
        x = np.stack([levels_image(rng, n) for n in counts] + [levels_image(rng, 100, channel=1)])
        x64 = x.astype(np.float64)
        t = 255.0 * (0.2989 * x64[:, 0] + 0.587 * x64[:, 1] + 0.114 * x64[:, 2])
        if np.abs(t - np.floor(t) - 0.5).min() > 1e-3:
            break
    else:
        raise SystemExit("no image set clear of the level boundaries")
    q = np.clip(np.rint(255.0 * x64), 0, 255) / 255.0
    g = (np.clip(np.rint(t), 0, 255) / 255.0)[:, None]
    vals = lambda lv: np.array([2.0 ** math.ceil(math.log2(len(np.unique(s)))) for s in lv])
    vc, vg = vals(q), vals(g)
    assert list(vc) == [1, 2, 4, 128, 256, 256, 128], vc
    return {"p.x": x, "p.q": q, "p.g": g, "p.vals_c": vc, "p.vals_g": vg}


def main():
    out = {}
    out.update(gaussian_case("num", (1, 3, 5, 7), 1, [10.0], [0.0], numbers=True))
    out.update(gaussian_case("grey1", (1, 3, 5, 7), 2, [25.0], [1.0], numbers=True))
    out.update(gaussian_case("vec", (3, 3, 6, 5), 3, [1.0, 15.0, 30.0], [0.0, 1.0, 1.0]))
    out.update(gaussian_case("vec0", (2, 3, 4, 4), 4, [5.0, 20.0], [0.0, 0.0]))
    out.update(gaussian_case("c1", (2, 1, 4, 4), 5, [12.0, 3.0], [1.0, 0.0]))
    out.update(gaussian_case("c4", (2, 4, 3, 3), 6, [7.0, 28.0], [0.0, 1.0]))
    out.update(gaussian_case("rand", (4, 3, 5, 5), 7, rng=(1.0, 30.0, 0.4)))
    assert 0 < out["rand.gray"].sum() < 4, "the random case should mix grey and colour samples"
    out.update(poisson_part())
    path = os.path.join(OUT, "g17_noise.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
