"""``vmambair_amd.degradations.DiffJPEG`` without a GPU: the plain-torch restatement against the independent float64 evaluation of
tests/golden/g16_jpeg.npz (numpy + ``scipy.fft.dctn`` per 8 x 8 block, tests/golden/make_golden_jpeg.py -- basicsr, where the reference
takes the operator from, is not available, so no reference code stands behind it), its argument handling, and the library's host
query and error codes.

Tolerance: the restatement in float64 against scipy's float64 evaluation of the same coefficients.  Both round the same values --
the generator refuses a fixture with a coefficient closer than 1e-6 to a half-integer, six orders above float64 round-off of values
below 2048 -- so the two differ by float64 round-off of sums of at most 64 terms below 2048 each: below 1e-12 of 255; 1e-9 is the
issue's figure."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from vmambair_amd import _build, _capi, degradations as D

CASES = {"mb1": (1, 3, 16, 16), "pad": (2, 3, 1, 1), "low": (1, 3, 8, 24), "edges": (3, 3, 17, 33), "rect": (2, 3, 48, 40),
         "odd": (1, 3, 80, 144)}
TAU = 0.01


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("g16_jpeg.npz")


def case(name):
    """-> (x fp32, quality as the test passes it: a Python number or a fp32 (B,) tensor, the (B,) tensor)"""
    z = golden()
    x, q = z[f"{name}.x"], z[f"{name}.q"]
    assert tuple(x.shape) == CASES[name] and x.dtype == torch.float32 and q.dtype == torch.float32
    return x, (float(q[0]) if int(z[f"{name}.scalar"]) else q.clone()), q


def unrounded(name):
    z = golden()
    return [z[f"{name}.{k}"] for k in ("vy", "vcb", "vcr")]


def band(v):
    """which float64 coefficients lie within TAU of a half-integer"""
    return ((v - torch.floor(v)) - 0.5).abs() < TAU


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_float64(name):
    x, quality, q = case(name)
    z = golden()
    got = D.restate_diffjpeg(x.double(), quality, False)
    assert got.dtype == torch.float64 and got.shape == x.shape
    err = float((got - z[f"{name}.out"]).abs().max())
    print(f"[jpeg] {name} {tuple(x.shape)}: float64 restatement vs scipy, max err {err:.2e}")
    assert err <= 1e-9
    # the coefficients it rounds are the fixture's, in the package's layout
    _, coef = D.DiffJPEG(differentiable=False)(x.double(), quality, return_coefficients=True)
    blocks = ((x.size(2) + 15) // 16) * ((x.size(3) + 15) // 16)
    assert [tuple(c.shape) for c in coef] == [(x.size(0), 4 * blocks, 8, 8), (x.size(0), blocks, 8, 8), (x.size(0), blocks, 8, 8)]
    for c, v in zip(coef, unrounded(name)):
        assert torch.equal(c, torch.round(v))
    # fp32 on the CPU is the restatement too, dtype-preserving
    got32 = D.DiffJPEG(differentiable=False)(x, quality)
    assert got32.dtype == torch.float32 and torch.equal(got32, D.restate_diffjpeg(x, quality, False))


@pytest.mark.parametrize("name", CASES)
def test_band_share_of_the_fixture(name):
    """(b) of tests/test_jpeg_gpu.py, on the float64 fixture alone: at most 3 % of the coefficients of every case lie within TAU of
    a half-integer, where an fp32 evaluation may round the other way"""
    flat = torch.cat([v.flatten() for v in unrounded(name)])
    share = float(band(flat).double().mean())
    print(f"[jpeg] {name}: {flat.numel()} coefficients, {100 * share:.2f} % within {TAU} of a half-integer")
    assert share <= 0.03


def test_quality_tensor_is_not_modified_and_both_branches_of_the_factor():
    x, quality, q = case("edges")
    before = quality.clone()
    D.DiffJPEG(differentiable=False)(x, quality)
    D.restate_diffjpeg(x, quality, False)
    assert torch.equal(quality, before)
    assert float(q.min()) < 50 <= float(q.max())
    # a scalar is B copies of it; the factor as the package defines it
    one = D.restate_diffjpeg(x.double(), 49.5, False)
    assert torch.equal(one, D.restate_diffjpeg(x.double(), torch.full((3,), 49.5), False))
    assert D.quality_to_factor(49.5) == 5000. / 49.5 / 100. and D.quality_to_factor(50) == 1.0 and D.quality_to_factor(95) == 0.1


def test_differentiable_rounding_gives_a_gradient():
    x, quality, _ = case("rect")
    x = x.double().requires_grad_(True)
    out = D.DiffJPEG()(x, quality)                     # the package's default: differentiable=True
    assert out.requires_grad
    out.square().sum().backward()
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    # the forward value: round(v) + (v - round(v))^3 moves a coefficient by at most 1/8
    hard = D.restate_diffjpeg(x.detach(), quality, False)
    assert 0 < float((out.detach() - hard).abs().max()) < 0.5
    # hard rounding passes no gradient
    x.grad = None
    D.DiffJPEG(differentiable=False)(x, quality).sum().backward()
    assert float(x.grad.abs().max()) == 0


def test_argument_errors_and_stages():
    jpeg = D.DiffJPEG(differentiable=False)
    assert D.DiffJPEG().differentiable is True and list(jpeg.state_dict()) == []
    for shape in ((2, 1, 16, 16), (2, 4, 16, 16), (3, 16, 16)):
        with pytest.raises(ValueError):
            jpeg(torch.rand(shape), 50)
    with pytest.raises(ValueError):
        D.restate_diffjpeg(torch.rand(2, 1, 16, 16), 50)
    with pytest.raises(ValueError):
        jpeg(torch.rand(2, 3, 16, 16), torch.tensor([50., 60., 70.]))
    x, quality, _ = case("edges")
    wide = x * 1.5 - 0.2
    assert float(wide.min()) < 0 and float(wide.max()) > 1
    assert torch.equal(jpeg(wide, quality, clamp_input=True), jpeg(torch.clamp(wide, 0, 1), quality))
    plain = jpeg(x, quality)
    assert torch.equal(jpeg(x, quality, quantise=True), torch.clamp((plain * 255.0).round(), 0, 255) / 255.)


def test_workgroup_query_is_pure_and_entry_point_refuses_without_a_launch():
    lib = _capi.load()
    raw = ctypes.CDLL(_build.LIB_PATH)
    for name in ("oss_jpeg_workgroups", "oss_jpeg_roundtrip"):
        assert hasattr(raw, name) and name in _capi.SYMBOLS, name
    assert _capi.JPEG == {"CLAMP_INPUT": 1, "QUANTISE": 2, "DIFF_ROUND": 4} and _capi.ABI_VERSION >= 12
    # four 16 x 16 macroblocks per workgroup
    assert lib.oss_jpeg_workgroups(1, 16, 16) == 1 and lib.oss_jpeg_workgroups(2, 1, 1) == 1
    assert lib.oss_jpeg_workgroups(3, 17, 33) == 5            # 3 * 2 * 3 = 18 macroblocks
    assert lib.oss_jpeg_workgroups(1, 80, 144) == 12          # 45
    assert lib.oss_jpeg_workgroups(9, 400, 400) == (9 * 25 * 25 + 3) // 4
    for b, h, w in ((0, 16, 16), (1, 0, 16), (1, 16, 0), (-1, 16, 16), (1, -16, 16), (1, 16, -1), ((1 << 24) + 1, 16, 16),
                    (1, (1 << 24) + 1, 16), (1 << 20, 1 << 20, 1 << 20)):
        assert lib.oss_jpeg_workgroups(b, h, w) == 0, (b, h, w)
    # the entry point refuses the same, and a missing pointer, with an error code and no launch (no device is touched here)
    err_null, err_shape = _capi._K["OSS_ERR_NULL"], _capi._K["OSS_ERR_SHAPE"]
    buf = (ctypes.c_float * 4)()
    p = ctypes.addressof(buf)
    assert lib.oss_jpeg_roundtrip(None, None, 50.0, None, None, None, None, 1, 16, 16, 0, None) == err_null
    assert lib.oss_jpeg_roundtrip(p, None, 50.0, None, None, None, None, 1, 16, 16, 0, None) == err_null
    assert lib.oss_jpeg_roundtrip(None, p, 50.0, p, p, p, p, 1, 16, 16, 0, None) == err_null
    assert lib.oss_jpeg_roundtrip(p, None, 50.0, p, None, None, None, 0, 16, 16, 0, None) == err_shape
    assert lib.oss_jpeg_roundtrip(p, None, 50.0, p, None, None, None, 1, 16, -3, 0, None) == err_shape
    assert lib.oss_jpeg_roundtrip(p, p, 50.0, p, None, None, None, 1, 16, 16, 8, None) == err_shape      # an unknown flag
    assert lib.oss_jpeg_roundtrip(p, p, 50.0, p, None, None, None, 1, 16, 16, -1, None) == err_shape
