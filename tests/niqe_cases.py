"""What tests/test_niqe_host.py and tests/test_niqe_gpu.py share: the G14 cases (tests/golden/g14_niqe.npz, made by
tests/golden/make_golden_niqe.py by RUNNING the reference's ``niqe``), the pristine model (g14_niqe_pris_params.npz, the
reference's data file) and the comparison rule for (blocks, 36) feature arrays."""
import functools
import os

import numpy as np

from conftest import GOLDEN
from vmambair_amd import metrics

ALPHA_COLS = [c + 18 * s for s in (0, 1) for c in (0, 2, 6, 10, 14)]
REF_TOL = 1e-6        # against the reference: the bound the feature was specified with (see test_niqe_host.py)
DEVICE_TOL = 1e-10    # device against the CPU restatement: the same fp32 values summed in float64 in another order


@functools.lru_cache(maxsize=None)
def model() -> metrics.NiqeModel:
    return metrics.NiqeModel.load(os.path.join(GOLDEN, "g14_niqe_pris_params.npz"))


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(os.path.join(GOLDEN, "g14_niqe.npz"))
    return {k: z[k] for k in z.files}


def cases():
    """name -> (uint8 image, input_order, {crop: (reference features, reference value)})"""
    z = golden()
    out = {}
    for name in sorted({k.split(".")[0] for k in z if "." in k}):
        if name == "const_200x301":
            img = z["bgr_200x301.img"].copy()
            r0, r1, c0, c1 = (int(v) for v in z[f"{name}.region"])
            img[r0:r1, c0:c1] = z[f"{name}.colour"]
        else:
            img = z[f"{name}.img"]
        per_crop = {crop: (z[f"{name}.feat_{crop}"], float(z[f"{name}.niqe_{crop}"])) for crop in (0, 4) if f"{name}.feat_{crop}" in z}
        out[name] = (img, str(z[f"{name}.order"]), per_crop)
    return out


def feature_scale(want: np.ndarray) -> np.ndarray:
    """What a feature's difference is taken relative to: its own magnitude -- except for the four ``mean`` features per scale,
    ``(beta_r - beta_l) * ratio(alpha)`` (niqe.py:62).  That one is a difference of two betas which each carry a rounding error
    proportional to themselves (the reference's float32 sums; the summation order on the device), so its error scales with
    ``ratio(alpha) * (beta_l + beta_r) / 2`` and not with what the cancellation leaves: measured against its own magnitude the
    restatement is 1.2e-5 from the reference on a block whose two betas differ by 1 %, at 6e-8 per beta."""
    gam, _, _, ratio = model().tables
    scale = np.abs(want).copy()
    for s in (0, 18):
        for c in (2, 6, 10, 14):
            idx = np.rint((want[:, s + c] - gam[0]) / 0.001).astype(int)
            assert np.array_equal(gam[idx], want[:, s + c]), "an alpha off the grid"
            scale[:, s + c + 1] = np.maximum(scale[:, s + c + 1], ratio[idx] * (want[:, s + c + 2] + want[:, s + c + 3]) / 2)
    return scale


def check_features(got: np.ndarray, want: np.ndarray, tol: float, what) -> float:
    """alphas EQUAL, NaN positions identical, every other feature within ``tol`` of ``want`` relative to ``feature_scale``;
    prints and returns the measured figure"""
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape, got.dtype)
    assert np.array_equal(got[:, ALPHA_COLS], want[:, ALPHA_COLS]), (what, "alphas differ", got[:, ALPHA_COLS], want[:, ALPHA_COLS])
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN positions differ")
    ok = ~np.isnan(want)
    worst = float(np.max(np.abs(got[ok] - want[ok]) / feature_scale(want)[ok]))
    print(f"{what}: features {worst:.2e} relative (bound {tol:.0e})")
    assert worst <= tol, (what, worst, tol)
    return worst


def check_value(got: float, want: float, tol: float, what) -> float:
    if want != want:
        assert got != got, (what, got)
        return 0.0
    d = abs(got - want) / abs(want)
    print(f"{what}: niqe {got!r} want {want!r}: {d:.2e} relative (bound {tol:.0e})")
    assert d <= tol, (what, got, want, d)
    return d


def planes(img: np.ndarray, order: str) -> np.ndarray:
    """uint8 (H, W[, 3]) BGR -> (1, C, H, W) float32 RGB planes in [0, 255] for the op (integers: exact in fp16 and bf16 too)"""
    if order == "HW":
        return img[None, None].astype(np.float32)
    return np.ascontiguousarray(img.transpose(2, 0, 1)[::-1])[None].astype(np.float32)
