"""``vmambair_amd.degradations`` without a GPU: the plain-torch restatement of ``filter2D`` / ``USMSharp`` against the independent
float64 evaluation of tests/golden/g15_degrade.npz (scipy, tests/golden/make_golden_degrade.py -- basicsr, where the reference takes
the two from, is not available, so no reference code stands behind these), the argument errors, the ``USMSharp`` buffer, the
training pair pool against the trace of the reference's own ``_dequeue_and_enqueue``, and the library's size queries.

Tolerances: the restatement evaluated in float64 against scipy's float64 sums of the same <= 2601 terms below 1: 1e-12 (a float64
sum of n terms is off by at most n 2^-53 sum|w||x| = 3e-13).  Integer data must agree exactly.  The fp32 restatement is held to the
bound of an fp32 dot product of k^2 terms in any order, (k^2 + 2) 2^-24 sum|w| max|x|."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from vmambair_amd import _build, _capi, degradations as D

U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("g15_degrade.npz")


def exact_cases():
    return [(s, kern) for s in ("a", "b") for kern in ("k21", "k3", "k7", "k7pad")]


def dot_bound(kernel, img):
    """(k^2 + 2) 2^-24 sum|w| max|x| per sample, shaped to broadcast over (B, C, H, W)"""
    k = kernel.shape[-1]
    return ((k * k + 2) * U * kernel.double().abs().sum(dim=(1, 2)) * float(img.abs().max())).view(-1, 1, 1, 1)


@pytest.mark.parametrize("s, kern", exact_cases())
def test_restatement_is_exact_on_integer_data(s, kern):
    z = golden()
    img, kernel, want = z[f"ex.{s}.img"], z[f"ex.{s}.{kern}"], torch.from_numpy(z[f"ex.{s}.{kern}.out"])
    for dtype in (torch.float64, torch.float32):
        got = D.restate_filter2d(img.to(dtype), kernel.to(dtype))
        assert got.dtype == dtype and torch.equal(got.double(), want.double()), (s, kern, dtype)
    assert torch.equal(D.filter2D(img, kernel).double(), want.double())


def test_restatement_matches_float64_on_the_blur_kernels():
    z = golden()
    img, kernels, want = z["ro.img"], z["ro.kernels"], z["ro.out"]
    got64 = D.restate_filter2d(img.double(), kernels.double())
    assert float((got64 - want).abs().max()) <= 1e-12
    err = (D.restate_filter2d(img, kernels).double() - want).abs()
    worst = float((err / dot_bound(kernels, img)).max())
    print(f"fp32 restatement on the CPU: max err {float(err.max()):.3e}, {worst:.4f} of the bound")
    assert worst <= 1.0
    # a shared (1, k, k) kernel and a bare (k, k) one are B copies of it
    for i in range(3):
        one = D.filter2D(img.double(), kernels[i].double())
        assert torch.equal(one, D.filter2D(img.double(), kernels[i:i + 1].double()))
        assert float((one[i] - want[i]).abs().max()) <= 1e-12


@pytest.mark.parametrize("s", ("a", "b"))
def test_restatement_matches_float64_on_the_rank_one_kernel(s):
    z = golden()
    g = z["sep.g"].double()
    assert float((D.gaussian_kernel1d(51, 0) - g).abs().max()) <= 2.0 ** -25 * float(g.max())   # the fixture holds float32(g)
    got = D.restate_filter2d(z[f"sep.{s}.img"].double(), torch.outer(g, g)[None])
    assert float((got - z[f"sep.{s}.out"]).abs().max()) <= 1e-12


@pytest.mark.parametrize("s", ("a", "b"))
def test_usm_restatement_matches_float64(s):
    z = golden()
    img, kernel = z[f"usm.{s}.img"].double(), z["usm.kernel"].double()
    blur = D.restate_filter2d(img, kernel)
    assert float((blur - z[f"usm.{s}.blur"]).abs().max()) <= 1e-12
    mask = (blur.sub(img).abs() * 255 > 10)
    assert np.array_equal(mask.numpy(), z[f"usm.{s}.mask"].astype(bool)) and 0.6 < float(mask.double().mean()) < 0.9
    assert float((D.restate_usm(img, kernel) - z[f"usm.{s}.out"]).abs().max()) <= 1e-12
    # the module on CPU tensors is the restatement with its own buffer, in fp32
    got = D.USMSharp()(z[f"usm.{s}.img"])
    assert got.dtype == torch.float32 and torch.equal(got, D.restate_usm(z[f"usm.{s}.img"], D.USMSharp().kernel))


def test_filter2d_stages_and_errors():
    z = golden()
    img, kernels = z["ro.img"] + torch.linspace(-1.2, 1.2, z["ro.img"].size(-1)), z["ro.kernels"]   # a ramp: both clamps act
    plain = D.filter2D(img, kernels)
    assert float(plain.min()) < 0 and float(plain.max()) > 1
    assert torch.equal(D.filter2D(img, kernels, clamp=True), torch.clamp(plain, 0, 1))
    assert torch.equal(D.filter2D(img, kernels, quantise=True), torch.clamp((plain * 255.0).round(), 0, 255) / 255.)
    with pytest.raises(ValueError, match="Wrong kernel size"):
        D.filter2D(img, torch.ones(1, 4, 4))
    with pytest.raises(ValueError, match="Wrong kernel size"):
        D.restate_filter2d(img, torch.ones(3, 20, 20))
    with pytest.raises(RuntimeError):   # H <= k // 2: whatever torch's reflect pad raises
        D.filter2D(torch.rand(1, 1, 10, 30), torch.ones(1, 21, 21))
    with pytest.raises(ValueError):
        D.filter2D(img, kernels[:2])    # neither 1 nor B kernels


def test_usm_sharp_buffer():
    usm = D.USMSharp()
    assert usm.radius == 51 and tuple(usm.kernel.shape) == (1, 51, 51) and usm.kernel.dtype == torch.float32
    assert abs(float(usm.kernel.double().sum()) - 1.0) <= 1e-6
    assert list(usm.state_dict().keys()) == ['kernel']
    assert D.USMSharp(radius=51).radius == 51 and D.USMSharp(radius=4).radius == 5
    want = golden()["usm.kernel"]
    assert float((usm.kernel - want).abs().max()) <= 2.0 ** -23 * float(want.max())
    # sigma = 8.0 at k = 51, and the vector is what the formula says
    g = D.gaussian_kernel1d(51, 0)
    x = torch.arange(51, dtype=torch.float64) - 25
    ref = torch.exp(-x * x / (2 * 8.0 ** 2))
    assert g.dtype == torch.float64 and float((g - ref / ref.sum()).abs().max()) <= 1e-15
    assert float((D.gaussian_kernel1d(9, 1.7).sum() - 1).abs()) <= 1e-15
    # a reference state_dict loads and keeps the separable path; another kernel of the same shape turns it off
    usm.load_state_dict({'kernel': want.clone()})
    assert usm._separable
    usm.load_state_dict({'kernel': torch.full((1, 51, 51), 1 / 2601.)})
    assert not usm._separable


def replay(pool, z, with_perm):
    for i in range(z["pool.lq"].shape[0]):
        perm = z["pool.perm"][i]
        filling = perm[0] < 0
        lq, gt = z["pool.lq"][i].clone(), z["pool.gt"][i].clone()
        lq_out, gt_out = pool.push_pop(lq, gt, perm=None if filling or not with_perm else torch.from_numpy(perm))
        assert torch.equal(lq_out, z["pool.lq_out"][i]) and torch.equal(gt_out, z["pool.gt_out"][i]), i
        if filling:   # the incoming batch comes back unchanged
            assert lq_out is lq and gt_out is gt
    q_lr, q_gt = pool.queue()
    assert torch.equal(q_lr, z["pool.queue_lr"]) and torch.equal(q_gt, z["pool.queue_gt"])


def test_training_pair_pool_reproduces_the_reference_trace():
    z = golden()
    assert (z["pool.perm"][:3] < 0).all() and (z["pool.perm"][3:] >= 0).all()   # queue 6, b 2: three calls fill it
    replay(D.TrainingPairPool(6), z, with_perm=True)
    torch.manual_seed(15)   # the generator's seed: randperm is drawn where the reference draws it
    replay(D.TrainingPairPool(6), z, with_perm=False)
    with pytest.raises(AssertionError, match="queue size 6 should be divisible by batch size 4"):
        D.TrainingPairPool(6).push_pop(torch.zeros(4, 1, 2, 3), torch.zeros(4, 1, 4, 6))


def test_size_queries_are_pure_host_calls():
    lib = _capi.load()
    raw = ctypes.CDLL(_build.LIB_PATH)
    for name in ("oss_filter2d_workgroups", "oss_filter2d", "oss_filter_sep_scratch_floats", "oss_filter_sep", "oss_usm_scratch_floats",
                 "oss_usm_sharp"):
        assert hasattr(raw, name) and name in _capi.SYMBOLS, name
    # 32 x 64 output tiles per plane
    assert lib.oss_filter2d_workgroups(9, 3, 600, 600, 21, 9) == 27 * 19 * 10
    assert lib.oss_filter2d_workgroups(3, 2, 11, 13, 21, 1) == 6 and lib.oss_filter2d_workgroups(1, 1, 2, 2, 3, 1) == 1
    assert lib.oss_filter_sep_scratch_floats(2, 1, 26, 26, 51) == 2 * 26 * 26
    assert lib.oss_usm_scratch_floats(2, 3, 64, 80, 51) == 2 * 2 * 3 * 64 * 80
    for k in (0, 2, 20, 23, -3):                                    # even, above the limit, not positive
        assert lib.oss_filter2d_workgroups(2, 3, 64, 64, k, 2) == 0, k
    for k in (0, 50, 65, -1):
        assert lib.oss_filter_sep_scratch_floats(2, 3, 64, 64, k) == 0 and lib.oss_usm_scratch_floats(2, 3, 64, 64, k) == 0, k
    assert lib.oss_filter_sep_scratch_floats(2, 3, 64, 64, 63) > 0
    for h, w in ((10, 30), (30, 10), (0, 30), (30, -1), ((1 << 24) + 1, 30)):   # one reflection must be enough: H, W > k // 2
        assert lib.oss_filter2d_workgroups(1, 1, h, w, 21, 1) == 0, (h, w)
    assert lib.oss_filter2d_workgroups(1, 1, 11, 11, 21, 1) == 1
    assert lib.oss_filter_sep_scratch_floats(1, 1, 25, 40, 51) == 0 and lib.oss_usm_scratch_floats(1, 1, 40, 25, 51) == 0
    for kernels in (0, 2, 4):                                       # a batch that does not match the kernel count
        assert lib.oss_filter2d_workgroups(3, 2, 32, 32, 21, kernels) == 0
    assert lib.oss_filter2d_workgroups(0, 2, 32, 32, 21, 1) == 0 and lib.oss_filter2d_workgroups(1 << 20, 1 << 20, 32, 32, 3, 1) == 0
    # the entry points refuse the same, and a missing pointer, with an error code and no launch (no device is touched here)
    err_null, err_shape = _capi._K["OSS_ERR_NULL"], _capi._K["OSS_ERR_SHAPE"]
    assert lib.oss_filter2d(None, None, None, 1, 1, 32, 32, 21, 1, 0, None) == err_null
    assert lib.oss_filter_sep(None, None, None, None, 1, 1, 32, 32, 21, None) == err_null
    assert lib.oss_usm_sharp(None, None, None, None, None, 1, 1, 32, 32, 21, 0.5, 10.0, None) == err_null
    buf = (ctypes.c_float * 4)()
    p = ctypes.addressof(buf)
    assert lib.oss_filter2d(p, p, p, 1, 1, 32, 32, 20, 1, 0, None) == err_shape
    assert lib.oss_filter2d(p, p, p, 1, 1, 10, 32, 21, 1, 0, None) == err_shape
    assert lib.oss_filter2d(p, p, p, 2, 1, 32, 32, 21, 3, 0, None) == err_shape
    assert lib.oss_filter2d(p, p, p, 1, 1, 32, 32, 21, 1, 3, None) == err_shape
    assert lib.oss_filter_sep(p, p, p, p, 1, 1, 25, 32, 51, None) == err_shape
    assert lib.oss_usm_sharp(p, p, p, None, p, 1, 1, 32, 25, 51, 0.5, 10.0, None) == err_shape
