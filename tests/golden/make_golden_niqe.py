#!/usr/bin/env python3
"""Generate tests/golden/g14_niqe.npz and g14_niqe_pris_params.npz by RUNNING THE REFERENCE's NIQE in the build container.

Needs /root/reference (read-only) and scipy; never runs on the GPU box.  Nothing of the reference is copied: its functions are
compiled out of the files where they lie (``make_golden._extract``) and only the input images and the numbers they return are
stored.  ``g14_niqe_pris_params.npz`` is the reference's data file ``niqe_pris_params.npz`` (the pristine-image model), byte for
byte.  Re-run with:  python tests/golden/make_golden_niqe.py

What is run
  * ``estimate_aggd_param``, ``compute_feature``, ``niqe`` (Deraining/basicsr/metrics/niqe.py:10-155) with ``reorder_image`` /
    ``to_y_channel`` (metrics/metric_util.py), ``bgr2ycbcr`` (utils/matlab_functions.py) and, for the float tensor, ``tensor2img``
    (SRGAN/VmambaIR/utils/img_util.py:36-95).  ``calculate_niqe`` itself (:158-205) opens the parameter file by a relative path,
    so its ten lines of loading -- ``astype(float32)``, ``reorder_image``, ``to_y_channel``, ``squeeze``, the crop -- are done
    here in its order.  ``compute_feature`` is wrapped by a recorder, which is how the (blocks, 36) features leave ``niqe``.
  * cv2 is not installed here, so ``niqe`` gets a stand-in for the one call it makes, ``cv2.resize(img / 255., (w // 2, h // 2),
    interpolation=cv2.INTER_LINEAR)``.  The plane's sides are multiples of 96, the target is EXACTLY half (asserted), and
    INTER_LINEAR is then the mean of every 2 x 2 cell: ``(a * .5 + b * .5) * .5 + (c * .5 + d * .5) * .5`` in float32 with a, b the
    upper and c, d the lower pixels.  THIS STAND-IN, NOT OPENCV, DEFINES THE LAST-ULP ORDER OF THAT MEAN in the stored values
    (also said in the fixture's ``meta``).

Stored per case ``<name>`` and crop c in {0, 4} (the crops at which the cropped plane holds a 96 x 96 block):
  ``<name>.img``          the input: uint8 (H, W, 3) BGR or (H, W); ``<name>.order`` its input_order
  ``<name>.feat_c``       the reference's (blocks, 36) features, blocks in its order (idx_w outer, idx_h inner)
  ``<name>.niqe_c``       the value ``niqe`` returns
  ``const_200x301``       has no ``img``: it is ``bgr_200x301`` with ``.region`` (r0, r1, c0, c1) set to ``.colour`` (B, G, R) -- one block
                          plus a 6-pixel margin at both crops, the all-zero MSCN block whose alphas are 0.2 and whose other
                          features are NaN (``.nan_block``: its row)
  ``t2i_110x210.tensor``  float16-valued (1, 3, 110, 210) RGB tensor reaching outside [0, 1]; ``.img`` is the reference's tensor2img of it
  ``r_gam_every_100``     ``r_gam`` of estimate_aggd_param (scipy.special.gamma) at every 100th grid point

Condition on the inputs: the CPU restatement ``vmambair_amd.metrics.niqe_features`` is evaluated too and a case is REFUSED unless
every alpha equals the reference's -- alpha lives on a 0.001 grid, the reference carries ``rhatnorm`` in float32, and a fixture
must not sit on a midpoint.  The measured differences of the restatement are printed (they are quoted in tests/test_niqe_host.py).
"""
import math
import os
import shutil
import sys
import types
import warnings

import numpy as np
import torch
from scipy import ndimage, special

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, _extract, load_by_path  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from vmambair_amd import metrics  # noqa: E402

PARAMS = f"{REF}/Deraining/basicsr/metrics/niqe_pris_params.npz"
ALPHA_COLS = [c + 18 * s for s in (0, 1) for c in (0, 2, 6, 10, 14)]
INTER_LINEAR = 1


def _resize_half(img, dsize, interpolation=None):
    h, w = img.shape
    assert interpolation == INTER_LINEAR and img.dtype == np.float32 and dsize == (w // 2, h // 2) and h % 2 == 0 and w % 2 == 0, \
        "the stand-in is INTER_LINEAR at exactly half the size only"
    half = np.float32(0.5)
    top = img[0::2, 0::2] * half + img[0::2, 1::2] * half
    bottom = img[1::2, 0::2] * half + img[1::2, 1::2] * half
    return top * half + bottom * half


def load_ref_niqe():
    cv2 = types.SimpleNamespace(resize=_resize_half, INTER_LINEAR=INTER_LINEAR, COLOR_RGB2BGR=4,
                                cvtColor=lambda img, code: np.ascontiguousarray(img[..., ::-1]))
    mf = load_by_path("ref_matlab_functions", f"{REF}/Deraining/basicsr/utils/matlab_functions.py")
    ns = {"np": np, "math": math, "cv2": cv2, "convolve": ndimage.convolve, "gamma": special.gamma, "bgr2ycbcr": mf.bgr2ycbcr}
    _extract(f"{REF}/Deraining/basicsr/metrics/metric_util.py", ["reorder_image", "to_y_channel"], ns)
    _extract(f"{REF}/Deraining/basicsr/metrics/niqe.py", ["estimate_aggd_param", "compute_feature", "niqe"], ns)
    ns_t = {"np": np, "torch": torch, "math": math, "cv2": cv2, "make_grid": None}
    _extract(f"{REF}/SRGAN/VmambaIR/utils/img_util.py", ["tensor2img"], ns_t)
    return ns, ns_t["tensor2img"]


def ref_plane(ns, img, order, crop):
    """niqe.py:191-201"""
    img = img.astype(np.float32)
    if order != "HW":
        img = ns["reorder_image"](img, input_order=order)
        img = np.squeeze(ns["to_y_channel"](img))
    if crop != 0:
        img = img[crop:-crop, crop:-crop]
    return img


def ref_niqe(ns, params, plane):
    """``niqe`` of the reference -> (its (blocks, 36) features, its value)"""
    rows, inner = [], ns["compute_feature"]
    ns["compute_feature"] = lambda block: rows.append(inner(block)) or rows[-1]
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")     # the all-zero block: means of empty slices
            value = ns["niqe"](plane, params["mu_pris_param"], params["cov_pris_param"], params["gaussian_window"])
    finally:
        ns["compute_feature"] = inner
    rows = np.array(rows, dtype=np.float64)
    n = rows.shape[0] // 2
    return np.concatenate([rows[:n], rows[n:]], axis=1), float(np.asarray(value).reshape(()))


def feature_scale(want, tables):
    """what a feature's difference is relative to (the same rule as tests/test_niqe_host.py): its own magnitude, except for the
    four ``mean`` features per scale (niqe.py:62), ``(beta_r - beta_l) * ratio(alpha)``: a difference of two betas that each carry
    the reference's float32 rounding, so its error scales with ``ratio(alpha) * (beta_l + beta_r) / 2``, not with what is left
    after the cancellation"""
    gam, _, _, ratio = tables
    scale = np.abs(want).copy()
    for s in (0, 18):
        for c in (2, 6, 10, 14):
            idx = np.rint((want[:, s + c] - gam[0]) / 0.001).astype(int)
            assert np.array_equal(gam[idx], want[:, s + c])
            scale[:, s + c + 1] = np.maximum(scale[:, s + c + 1], ratio[idx] * (want[:, s + c + 2] + want[:, s + c + 3]) / 2)
    return scale


def rel_diff(got, want, tables):
    """max |got - want| / feature_scale over the entries that are no NaN; NaN positions must coincide"""
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    return float(np.max(np.abs(got[ok] - want[ok]) / feature_scale(want, tables)[ok])) if ok.any() else 0.0


def textured(rng, h, w, channels, cell=8, noise=10.0):
    """a random mosaic of cell x cell patches under Gaussian noise: edges, flat areas and grain, like a photograph's"""
    shape = (h, w, channels) if channels else (h, w)
    coarse = rng.randint(20, 236, ((h + cell - 1) // cell, (w + cell - 1) // cell) + shape[2:]).astype(np.float64)
    img = np.repeat(np.repeat(coarse, cell, axis=0), cell, axis=1)[:h, :w]
    return np.clip(np.rint(img + noise * rng.randn(*shape)), 0, 255).astype(np.uint8)


def build_inputs(tensor2img, seeds):
    cases = {}
    cases["u8_96x192"] = (textured(np.random.RandomState(seeds["u8_96x192"]), 96, 192, 3), "HWC")
    base = textured(np.random.RandomState(seeds["bgr_200x301"]), 200, 301, 3)
    cases["bgr_200x301"] = (base, "HWC")
    const = base.copy()
    region, colour = (90, 200, 90, 206), (37, 141, 202)
    const[region[0]:region[1], region[2]:region[3]] = colour
    cases["const_200x301"] = (const, "HWC")
    rng = np.random.RandomState(seeds["smooth_192x288"])
    i, j = np.meshgrid(np.arange(192), np.arange(288), indexing="ij")
    smooth = 128.0 + 6.0 * np.sin(i / 23.0 + j / 31.0) + 0.6 * rng.randn(192, 288)
    cases["smooth_192x288"] = (np.repeat(np.clip(np.rint(smooth), 0, 255).astype(np.uint8)[..., None], 3, axis=2), "HWC")
    cases["grey_120x200"] = (textured(np.random.RandomState(seeds["grey_120x200"]), 120, 200, 0), "HW")
    rng = np.random.RandomState(seeds["t2i_110x210"])
    t = textured(rng, 110, 210, 3).astype(np.float64).transpose(2, 0, 1)[::-1] / 255.0 * 1.4 - 0.2 + 0.002 * rng.randn(3, 110, 210)
    tensor = torch.from_numpy(np.ascontiguousarray(t)).to(torch.float16).to(torch.float32)[None]
    cases["t2i_110x210"] = (tensor2img([tensor.clone()]), "HWC")
    extra = {"const_200x301.region": np.array(region), "const_200x301.colour": np.array(colour, dtype=np.uint8),
             "const_200x301.nan_block": np.array(3), "t2i_110x210.tensor": tensor.numpy().astype(np.float16)}
    return cases, extra


SEEDS = {"u8_96x192": 0, "bgr_200x301": 1, "smooth_192x288": 2, "grey_120x200": 3, "t2i_110x210": 5}


def evaluate(ns, params, model, name, img, order):
    """the stored values of one case and the restatement's differences; raises when an alpha differs"""
    out, worst = {}, (0.0, 0.0)
    for crop in (0, 4):
        if min(img.shape[:2]) - 2 * crop < 96:
            continue
        plane = ref_plane(ns, img, order, crop)
        feat, value = ref_niqe(ns, params, plane)
        mine = metrics.niqe_features(plane, model)
        if not np.array_equal(mine[:, ALPHA_COLS], feat[:, ALPHA_COLS]):
            raise ValueError(f"{name} crop {crop}: {int((mine[:, ALPHA_COLS] != feat[:, ALPHA_COLS]).sum())} alphas of the restatement "
                             "differ from the reference's: an input on a midpoint of the alpha grid, choose another seed")
        got = metrics.calculate_niqe(img, crop, order, "y", model)
        d_feat = rel_diff(mine, feat, model.tables)
        d_val = abs(got - value) / abs(value) if value == value else 0.0
        assert (got == got) == (value == value)
        print(f"{name} crop {crop}: plane {plane.shape} blocks {feat.shape[0]} niqe {value!r} restatement: features {d_feat:.2e} "
              f"value {d_val:.2e} relative")
        worst = (max(worst[0], d_feat), max(worst[1], d_val))
        out[f"{name}.feat_{crop}"], out[f"{name}.niqe_{crop}"] = feat, np.float64(value)
    return out, worst


def main():
    ns, tensor2img = load_ref_niqe()
    params = np.load(PARAMS)
    model = metrics.NiqeModel.load(PARAMS)
    cases, out = build_inputs(tensor2img, SEEDS)
    worst = (0.0, 0.0)
    for name, (img, order) in cases.items():
        vals, w = evaluate(ns, params, model, name, img, order)
        worst = (max(worst[0], w[0]), max(worst[1], w[1]))
        out.update(vals)
        out[f"{name}.order"] = np.array(order)
        if name != "const_200x301":
            out[f"{name}.img"] = img
    row = out["const_200x301.feat_4"][3]
    assert np.array_equal(out["const_200x301.feat_0"][3], row, equal_nan=True) or np.isnan(out["const_200x301.feat_0"][3]).sum() == 26
    assert (row[ALPHA_COLS] == 0.2).all() and np.isnan(np.delete(row, ALPHA_COLS)).all(), "the all-zero block's quirk"
    gam = np.arange(0.2, 10.001, 0.001)
    r = np.reciprocal(gam)
    out["r_gam_every_100"] = (np.square(special.gamma(r * 2)) / (special.gamma(r) * special.gamma(r * 3)))[::100]
    out["meta"] = np.array("reference: Deraining/basicsr/metrics/niqe.py (estimate_aggd_param, compute_feature, niqe) with scipy "
                           f"{ndimage.__name__.split('.')[0]} convolve / special.gamma; cv2.resize is a stand-in of the generator "
                           "(exact halving, (a*.5+b*.5)*.5+(c*.5+d*.5)*.5 in float32): it, not OpenCV, defines the last-ulp order "
                           "of the 2 x 2 mean")
    print(f"restatement against the reference, worst case: features {worst[0]:.2e}, value {worst[1]:.2e} relative")
    assert max(worst) < 2.5e-7, "a step of the restatement does not follow the reference"
    path = os.path.join(OUT, "g14_niqe.npz")
    np.savez_compressed(path, **out)
    shutil.copyfile(PARAMS, os.path.join(OUT, "g14_niqe_pris_params.npz"))
    print(f"wrote g14_niqe.npz: {os.path.getsize(path) / 1024:.1f} KiB, g14_niqe_pris_params.npz: {os.path.getsize(PARAMS) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
