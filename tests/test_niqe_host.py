"""NIQE, the no-reference quality metric (Deraining/basicsr/metrics/niqe.py): the dtype-following CPU restatement in
``vmambair_amd.metrics`` against the values the reference's own functions return, ``NiqeModel``, and the host side of the C ABI of
``oss_niqe.hip``.  No GPU here.

Fixture tests/golden/g14_niqe.npz (tests/golden/make_golden_niqe.py, produced by RUNNING the reference's ``niqe``; its
``cv2.resize`` is the generator's exact-halving stand-in, which defines the last-ulp order of the 2 x 2 mean): per case the uint8
input and, per crop in {0, 4}, the reference's (blocks, 36) features and its NIQE value.

Tolerance against the reference: alphas EQUAL (the generator refuses inputs on a midpoint of the 0.001 grid), NaN positions
identical, every other feature and the value within 1e-6 relative (a feature relative to ``niqe_cases.feature_scale``).  The bound
is not tuned on the code under test: an evaluation that follows the reference's dtypes differs from it only by the reference's own
float32 moment sums, an evaluation that does not (plain float64) misses by 2.2e-4 on a smooth image and 2.5e-2 on one with a
constant region; 1e-6 sits between the two.  Measured when G14 was generated (restatement against reference, features / value):
    u8_96x192      crop 0  1.15e-07 / 4.44e-08
    bgr_200x301    crop 0  1.08e-07 / 1.68e-07     crop 4  1.39e-07 / 1.13e-09
    const_200x301  crop 0  1.24e-07 / 1.86e-08     crop 4  1.09e-07 / 3.91e-08
    smooth_192x288 crop 0  1.13e-07 / 3.26e-09     crop 4  9.74e-08 / 1.24e-08
    grey_120x200   crop 0  1.01e-07 / 4.29e-08     crop 4  7.04e-08 / 4.99e-08
    t2i_110x210    crop 0  7.73e-08 / 2.09e-07     crop 4  1.01e-07 / 1.66e-07
worst 2.09e-07, under the 2.5e-7 the bound was specified for.  The MSCN maps of the restatement equal scipy's bit for bit.
"""
import math

import numpy as np
import pytest
import torch

import niqe_cases as nc
from vmambair_amd import _capi, metrics

Q, Y, R = _capi.METRIC_QUANTISE, _capi.METRIC_Y, _capi.METRIC_REPLICATE


def y_plane(img, order, crop):
    """niqe.py:191-201 with this package's to_y_channel"""
    t = torch.from_numpy(img).to(torch.float32)
    plane = (metrics.to_y_channel(t)[..., 0] if order != "HW" else t).numpy()
    return plane[crop:plane.shape[0] - crop, crop:plane.shape[1] - crop]


def test_restatement_matches_reference_golden():
    n = 0
    for name, (img, order, per_crop) in nc.cases().items():
        assert (name == "u8_96x192") == (sorted(per_crop) == [0]), "96 x 192 holds no block at crop 4; every other case has both"
        for crop, (feat, value) in per_crop.items():
            got = metrics.niqe_features(y_plane(img, order, crop), nc.model())
            nc.check_features(got, feat, nc.REF_TOL, (name, crop))
            nc.check_value(metrics.calculate_niqe(img, crop, order, "y", nc.model()), value, nc.REF_TOL, (name, crop))
            n += 1
    assert n == 11


def test_all_zero_block_has_alpha_0_2_and_nan_elsewhere():
    img, order, per_crop = nc.cases()["const_200x301"]
    row = int(nc.golden()["const_200x301.nan_block"])
    others = np.delete(np.arange(36), nc.ALPHA_COLS)
    for crop, (feat, value) in per_crop.items():
        got = metrics.niqe_features(y_plane(img, order, crop), nc.model())
        for f in (feat, got):
            assert (f[row, nc.ALPHA_COLS] == 0.2).all() and np.isnan(f[row, others]).all()
            assert not np.isnan(np.delete(f, row, axis=0)).any()
        # nanmean counts the 0.2 in the alpha columns and skips the row elsewhere; the covariance drops the row
        mu = np.nanmean(got, axis=0)
        assert np.allclose(mu[nc.ALPHA_COLS], got[:, nc.ALPHA_COLS].mean(axis=0), rtol=1e-15)
        assert np.allclose(mu[others], np.delete(got, row, axis=0)[:, others].mean(axis=0), rtol=1e-15)
        kept = np.delete(got, row, axis=0)
        inv = np.linalg.pinv((nc.model().cov + np.cov(kept, rowvar=False)) / 2)
        d = nc.model().mu - mu
        assert metrics.niqe_from_features(got, nc.model()) == float(np.sqrt(d @ inv @ d.T).reshape(()))
        assert math.isfinite(value)


def test_input_orders_and_tensors_give_the_same_value():
    img, order, per_crop = nc.cases()["bgr_200x301"]
    want = metrics.calculate_niqe(img, 4, "HWC", "y", nc.model())
    assert metrics.calculate_niqe(np.ascontiguousarray(img.transpose(2, 0, 1)), 4, "CHW", "y", nc.model()) == want
    assert metrics.calculate_niqe(torch.from_numpy(img), 4, "HWC", model=nc.model()) == want
    assert metrics.calculate_niqe(torch.from_numpy(img).permute(2, 0, 1)[None].float(), 4, "CHW", model=nc.model()) == want
    grey, _, _ = nc.cases()["grey_120x200"]
    # a single channel in HWC order goes through to_y_channel's x / 255 * 255 round trip: the identity on integers
    assert metrics.calculate_niqe(grey[..., None], 0, "HWC", model=nc.model()) == metrics.calculate_niqe(grey, 0, "HW", model=nc.model())


def test_image_niqe_on_the_host_quantises_like_tensor2img():
    z = nc.golden()
    t = torch.from_numpy(z["t2i_110x210.tensor"].astype(np.float32))
    img = metrics.tensor2img(t).numpy()
    assert np.array_equal(img, z["t2i_110x210.img"]), "tensor2img of the stored tensor is the reference's"
    for crop in (0, 4):
        got = metrics.image_niqe(t, nc.model(), crop)
        assert got.shape == (1,) and got.dtype == torch.float64
        nc.check_value(float(got[0]), float(z[f"t2i_110x210.niqe_{crop}"]), nc.REF_TOL, ("t2i", crop))
    pair = [(t, t)]
    plain = metrics.mean_metrics(pair, 4)
    assert sorted(plain) == ["psnr", "ssim"], "the default changes nothing"
    with_niqe = metrics.mean_metrics(pair, 4, niqe_model=nc.model())
    assert with_niqe["niqe"] == float(metrics.image_niqe(t, nc.model(), 4)[0]) and with_niqe["ssim"] == plain["ssim"]
    assert metrics.mean_metrics([], niqe_model=nc.model()) == {"psnr": 0.0, "ssim": 0.0, "niqe": 0.0}


def test_errors():
    img = np.zeros((120, 130, 3), dtype=np.uint8)
    m = nc.model()
    with pytest.raises(ValueError, match="gray"):
        metrics.calculate_niqe(img, 0, "HWC", "gray", m)
    with pytest.raises(ValueError, match="96 x 96"):
        metrics.calculate_niqe(img, 13, "HWC", "y", m)          # 94 x 104
    with pytest.raises(ValueError, match="96 x 96"):
        metrics.calculate_niqe(img[:, :95], 0, "HWC", "y", m)
    with pytest.raises(ValueError, match="96 x 96"):
        metrics.niqe_features(np.zeros((95, 200), dtype=np.float32), m)
    with pytest.raises(ValueError, match="input_order"):
        metrics.calculate_niqe(img, 0, "WHC", "y", m)
    with pytest.raises(ValueError, match="input_order"):
        metrics.calculate_niqe(img, 0, "HW", "y", m)            # three dimensions are no HW image
    with pytest.raises(ValueError, match="NiqeModel.load"):
        metrics.calculate_niqe(img, 0)
    with pytest.raises(ValueError, match="96 x 96"):
        metrics.image_niqe(torch.zeros(1, 3, 100, 95), m)
    with pytest.raises(ValueError, match="7 x 7"):
        metrics.NiqeModel(m.mu, m.cov, np.ones((5, 5)))


def test_fewer_than_two_usable_blocks_give_nan():
    m = nc.model()
    img, order, _ = nc.cases()["grey_120x200"]
    one = metrics.calculate_niqe(img[:, :100], 0, "HW", "y", m)                   # one block: np.cov has nothing to estimate
    assert math.isnan(one)
    flat = img.copy()
    flat[:, :104] = 77                                                            # two blocks, the first all zero
    feat = metrics.niqe_features(flat.astype(np.float32), m)
    assert feat.shape == (2, 36) and np.isnan(feat[0]).sum() == 26 and not np.isnan(feat[1]).any()
    assert math.isnan(metrics.niqe_from_features(feat, m))
    assert math.isnan(metrics.calculate_niqe(np.full((96, 192), 9, dtype=np.uint8), 0, "HW", "y", m))   # no usable block at all


def test_model_window_and_tables():
    m = nc.model()
    # fspecial('gaussian', 7, 7 / 6)
    x = np.arange(7, dtype=np.float64) - 3.0
    g = np.exp(-(x[:, None] ** 2 + x[None, :] ** 2) / (2.0 * (7.0 / 6.0) ** 2))
    g /= g.sum()
    print("window - fspecial:", np.abs(m.window - g).max())
    assert np.abs(m.window - g).max() < 1e-16
    assert m.mu.shape == (1, 36) and m.cov.shape == (36, 36) and np.array_equal(m.cov, m.cov.T)
    gam, r_gam, scale, ratio = m.tables
    assert m.tables.shape == (4, _capi.NIQE_GRID) == (4, 9801) and m.tables.dtype == np.float64
    assert np.array_equal(gam, np.arange(0.2, 10.001, 0.001)) and gam[0] == 0.2
    # the search needs r_gam strictly increasing; the other two are looked up by index (sqrt(G(1/a) / G(3/a)) is not monotone)
    assert (np.diff(r_gam) > 0).all() and (scale > 0).all() and (ratio > 0).all() and np.isfinite(m.tables).all()
    # the reference's expression (scipy.special.gamma, stored by the generator) at every 100th grid point: two gamma
    # implementations, a few units of float64 round-off
    want = nc.golden()["r_gam_every_100"]
    assert want.shape == (99,) and np.abs(r_gam[::100] / want - 1.0).max() < 1e-13
    for i in (0, 800, 1800, 9800):     # alpha 0.2, 1 (Laplace), 2 (Gauss), 10
        a = gam[i]
        assert scale[i] == math.sqrt(math.gamma(1 / a) / math.gamma(3 / a)) and ratio[i] == math.gamma(2 / a) / math.gamma(1 / a)
    assert abs(r_gam[800] - 0.5) < 1e-12 and abs(r_gam[1800] - 2.0 / math.pi) < 1e-12
    assert m.device_tables("cpu") is m.device_tables(torch.device("cpu")) and torch.equal(m.device_tables("cpu"), torch.from_numpy(m.tables))


def test_alpha_search_is_argmin():
    """the neighbour search the restatement (and, in the same form, the kernel) uses against ``np.argmin((r_gam - r) ** 2)``"""
    r_gam = nc.model().tables[1]
    rng = np.random.RandomState(0)
    mid = (r_gam[:-1] + r_gam[1:]) / 2
    r = np.concatenate([rng.uniform(r_gam[0] - 0.01, r_gam[-1] + 0.01, 300), r_gam[::977], mid[::1013], np.nextafter(mid[::1013], 1.0),
                        [0.0, -1.0, 5.0, np.inf, np.nan]])
    got = metrics._niqe_alpha_index(r_gam, r)
    with np.errstate(invalid="ignore"):
        want = np.array([np.argmin((r_gam - v) ** 2) for v in r[:-2]] + [len(r_gam) - 2, 0])   # inf: see below; NaN: index 0
    # r = inf never arises (the moments are finite); the search answers the last interval, argmin of an all-inf array 0
    assert np.array_equal(got, want), np.nonzero(got != want)


def test_shape_rules_are_a_pure_host_query():
    ok = _capi.load().oss_niqe_features_ok
    F32, F16, BF16 = _capi.OSS_F32, _capi.OSS_F16, _capi.OSS_BF16
    for io in (F32, F16, BF16):
        assert ok(3, 200, 301, 4, Q | Y, io) == 1 and ok(1, 96, 96, 0, 0, io) == 1 and ok(1, 104, 200, 4, Q, io) == 1
    for io in (3, 7, -1):              # OSS_F32_BF16X3 and out-of-range values are no element type
        assert ok(3, 200, 301, 4, Q | Y, io) == 0 and ok(1, 96, 96, 0, 0, io) == 0
    assert ok(2, 200, 301, 0, 0, F32) == 0 and ok(4, 200, 301, 0, Y, F32) == 0          # channels
    assert ok(1, 200, 301, 0, Y, F32) == 0                                               # Y needs three channels ...
    assert ok(3, 200, 301, 0, 0, F32) == 0 and ok(3, 200, 301, 0, Q, F32) == 0            # ... and three channels need Y: one plane
    assert ok(3, 200, 301, 0, Y | R, F32) == 0 and ok(1, 200, 301, 0, 8, F32) == 0        # flags of another entry point
    assert ok(1, 95, 301, 0, 0, F32) == 0 and ok(1, 200, 95, 0, 0, F32) == 0             # under one block
    assert ok(1, 103, 200, 4, 0, F32) == 0 and ok(1, 104, 103, 4, 0, F32) == 0 and ok(1, 104, 104, 4, 0, F32) == 1
    assert ok(1, 200, 200, -1, 0, F32) == 0 and ok(1, 0, 200, 0, 0, F32) == 0 and ok(1, 200, -5, 0, 0, F32) == 0
    assert ok(1, 2 ** 31 - 1, 2 ** 31 - 1, 0, 0, F32) == 0 and ok(1, 96 * 40000, 96 * 40000, 0, 0, F32) == 1   # blocks beyond grid.x
    # the launcher answers before anything reaches a device: NULL pointers, bad shapes, no element type
    lib = _capi.load()
    assert lib.oss_niqe_features(F32, None, None, None, None, 1, 1, 96, 96, 0, 0, 96, 0, 0, None) == _capi._K["OSS_ERR_NULL"]
    from vmambair_amd import ops
    assert not ops.niqe_features_ok(torch.zeros(1, 1, 96, 96), 0, 0)      # a CPU tensor
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        ops.niqe_features(torch.zeros(1, 1, 96, 96), torch.zeros(4, 9801, dtype=torch.float64), torch.zeros(7, 7, dtype=torch.float64), 0, 0)
