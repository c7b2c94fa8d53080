"""SSIM next to PSNR (the second column of the reference's tables): the float64 restatement in ``vmambair_amd.metrics`` against the
values the reference's own functions return, and the host side of the C ABI of ``oss_metrics.hip``.  No GPU here.

Fixture tests/golden/g10_ssim.npz (tests/golden/make_golden_ssim.py, produced by RUNNING the reference): uint8 BGR image pairs
(b = a + d) and, per pair and crop in {0, 4}, ``_ssim`` per channel and on the Y plane, ``_ssim_cly`` on the Y plane, and
``calculate_psnr`` with and without the Y channel.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from vmambair_amd import _capi, metrics

MODES = (("ssim_valid_rgb", False, "valid"), ("ssim_valid_y", True, "valid"), ("ssim_replicate_y", True, "replicate"))
Q, Y, R = _capi.METRIC_QUANTISE, _capi.METRIC_Y, _capi.METRIC_REPLICATE


def golden_cases():
    z = np.load(os.path.join(GOLDEN, "g10_ssim.npz"))
    for name in sorted({k.split(".")[0] for k in z.files}):
        a = z[f"{name}.a"]
        yield name, z, a, (a.astype(np.int16) + z[f"{name}.d"]).astype(np.uint8)


def test_ssim_matches_reference_values():
    """|ours - reference| <= 1e-12: float64 round-off (11 taps along rows then columns against the reference's 121-tap window
    measured <= 2e-14 on these cases), two orders of margin"""
    n = 0
    for name, z, a, b in golden_cases():
        for crop in (0, 4):
            for key, yc, border in MODES:
                want = float(z[f"{name}.{key}_{crop}"])
                got = metrics.calculate_ssim(a, b, crop, "HWC", yc, border)
                print(f"{name} crop {crop} {key}: {got!r} reference {want!r} diff {abs(got - want):.2e}")
                assert abs(got - want) <= 1e-12, (name, crop, key, got, want)
                n += 1
    assert n == 8 * 2 * 3
    name, z, a, b = next(c for c in golden_cases() if c[0].startswith("same"))
    assert metrics.calculate_ssim(a, b, 4, "HWC", True) == 1.0 and metrics.calculate_psnr(a, b, 4, "HWC", True) == float("inf")


def test_psnr_of_the_ssim_cases_matches_reference_values():
    """the same tolerances, for the same reasons, as test_checkpoint_psnr.py::test_psnr_matches_reference_values"""
    for name, z, a, b in golden_cases():
        for crop in (0, 4):
            for yc in (0, 1):
                want, got = float(z[f"{name}.psnr_{crop}_y{yc}"]), metrics.calculate_psnr(a, b, crop, "HWC", bool(yc))
                assert got == want or abs(got - want) < (2e-5 if yc else 1e-9), (name, crop, yc, got, want)
                mse = metrics.calculate_mse(a, b, crop, "HWC", bool(yc))
                assert (mse == 0 and got == float("inf")) or abs(10 * np.log10(255.0 ** 2 / mse) - got) < 1e-9


def test_input_orders_and_tensors_give_the_same_value():
    cases = {c[0]: c for c in golden_cases()}
    _, z, a, b = cases["u8_40x52"]
    for yc, border in ((False, "valid"), (True, "valid"), (True, "replicate")):
        want = metrics.calculate_ssim(a, b, 4, "HWC", yc, border)
        assert metrics.calculate_ssim(a.transpose(2, 0, 1), b.transpose(2, 0, 1), 4, "CHW", yc, border) == want
        ta, tb = torch.from_numpy(a.transpose(2, 0, 1).copy()), torch.from_numpy(b.transpose(2, 0, 1).copy())
        assert metrics.calculate_ssim(ta, tb, 4, "HWC", yc, border) == want
        assert metrics.calculate_ssim(ta[None].float(), tb[None].float(), 4, "CHW", yc, border) == want
    _, z, g, h = cases["grey_25x31"]
    want = float(z["grey_25x31.ssim_valid_rgb_0"])
    for form in (lambda v: v, lambda v: v[..., None], lambda v: torch.from_numpy(v)[None]):
        assert abs(metrics.calculate_ssim(form(g), form(h), 0) - want) <= 1e-12
    assert abs(metrics.calculate_ssim(g[None], h[None], 0, "CHW") - want) <= 1e-12


def test_validation_ssim_and_mean_metrics_on_cpu_tensors():
    _, z, a, b = next(c for c in golden_cases() if c[0].startswith("t2i"))
    ta, tb = torch.from_numpy(z["t2i_24x28.ta"]), torch.from_numpy(z["t2i_24x28.tb"])
    assert np.array_equal(metrics.tensor2img(ta).numpy(), a) and np.array_equal(metrics.tensor2img(tb).numpy(), b)
    for border, key in (("valid", "ssim_valid_y"), ("replicate", "ssim_replicate_y")):
        assert abs(metrics.validation_ssim(ta, tb, 4, True, border) - float(z[f"t2i_24x28.{key}_4"])) <= 1e-12
    m = metrics.mean_metrics([(ta, tb), (tb, ta)])
    assert abs(m["ssim"] - float(z["t2i_24x28.ssim_valid_y_4"])) <= 1e-12
    assert abs(m["psnr"] - metrics.mean_psnr([(ta, tb)])) < 1e-12


def test_unsupported_forms_raise():
    _, z, a, b = next(golden_cases())
    _, _, c3, d3 = next(c for c in golden_cases() if c[0] == "u8_33x47")
    with pytest.raises(ValueError, match="_ssim_3d"):
        metrics.calculate_ssim(c3, d3, 4, "HWC", False, "replicate")
    with pytest.raises(ValueError, match="input_order"):
        metrics.calculate_ssim(c3, d3, 4, "WHC")
    with pytest.raises(ValueError, match="border"):
        metrics.calculate_ssim(c3, d3, 4, "HWC", True, "reflect")
    with pytest.raises(ValueError, match="11 x 11"):
        metrics.calculate_ssim(c3[:18, :18], d3[:18, :18], 4, "HWC", True)
    with pytest.raises(AssertionError):
        metrics.calculate_ssim(c3, d3[:-1], 0)
    with pytest.raises(ValueError, match="_ssim_3d"):
        metrics.image_metrics(torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 32), 4, False, "replicate")


def test_shape_queries_are_pure_host_calls():
    lib = _capi.load()
    ok = lib.oss_image_metrics_ok
    for io in (_capi.OSS_F32, _capi.OSS_F16, _capi.OSS_BF16):
        assert ok(io, 3, 2048, 2048, 4, Q | Y) == 1 and ok(io, 1, 19, 19, 4, 0) == 1 and ok(io, 3, 64, 48, 0, Q | R | Y) == 1
    assert ok(3, 3, 64, 64, 4, 0) == 0                                         # no such dtype
    assert ok(0, 2, 64, 64, 4, 0) == 0 and ok(0, 4, 64, 64, 4, 0) == 0         # channels not in {1, 3}
    assert ok(0, 1, 64, 64, 4, Y) == 0                                         # Y needs three channels
    assert ok(0, 3, 64, 64, 32, R) == 0 and ok(0, 3, 64, 20, 10, R) == 0       # crop_border >= half a side
    assert ok(0, 3, 64, 64, -1, 0) == 0 and ok(0, 3, 0, 64, 0, 0) == 0
    assert ok(0, 3, 18, 64, 4, 0) == 0 and ok(0, 3, 64, 18, 4, 0) == 0         # valid mode: cropped plane under 11
    assert ok(0, 3, 18, 18, 4, R) == 1 and ok(0, 3, 9, 9, 4, R) == 1           # replicate: any non-empty cropped plane
    assert ok(0, 3, 64, 64, 4, 8) == 0                                         # unknown flag
    assert ok(0, 1, 16 * 65535 + 8, 32, 4, R) == 1 and ok(0, 1, 16 * 65535 + 9, 32, 4, R) == 0   # grid.y
    n = lib.oss_image_metrics_partial_doubles
    # one (squared error, SSIM sum) pair per 16 x 32 tile of the cropped plane and per channel (room for either border mode)
    assert n(1, 3, 2048, 2048, 4) == 2 * 3 * ((2040 + 15) // 16) * ((2040 + 31) // 32)
    assert n(8, 1, 19, 19, 4) == 2 * 8 and n(2, 3, 64, 48, 0) == 2 * 2 * 3 * 4 * 2
    assert n(0, 3, 64, 64, 4) == 0 and n(1, 2, 64, 64, 4) == 0 and n(1, 3, 64, 64, 32) == 0


def test_bad_arguments_are_answered_before_any_launch():
    """OSS_ERR_NULL / OSS_ERR_SHAPE come back from the host checks: no GPU is touched (this test runs without one)"""
    lib = _capi.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def call(a=p, b=p, out=p, part=p, batch=1, c=3, h=64, w=64, crop=4, flags=0):
        return lib.oss_image_metrics(_capi.OSS_F32, a, b, out, part, batch, c, h, w, c * h * w, h * w, w, c * h * w, h * w, w, crop, flags, None)

    for kw in (dict(a=None), dict(b=None), dict(out=None), dict(part=None)):
        assert call(**kw) == -1, kw
    for kw in (dict(c=2), dict(c=1, flags=Y), dict(crop=32), dict(h=18), dict(w=18, flags=Q | Y), dict(batch=0),
               dict(batch=65536, c=1), dict(batch=21846, c=3), dict(flags=16), dict(c=1, h=16 * 65535 + 9, w=32, flags=R)):
        assert call(**kw) == -2, kw
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        from vmambair_amd import ops
        ops.image_metrics(torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 32), 4, 0)
