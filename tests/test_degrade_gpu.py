"""``oss_degrade.hip`` on the device (``torch.ops.vmambair.filter2d`` / ``filter_sep`` / ``usm_sharp`` and their public face
``vmambair_amd.degradations``) against the independent float64 evaluation of tests/golden/g15_degrade.npz (scipy; the float64
restatement, which tests/test_degrade_host.py pins to that evaluation at 1e-12, where a reference depends on the device's own mask).

Bounds (derived, not tuned; u = 2^-24):
  exact data   integers with every partial sum below 2^24: fp32 equals float64 bit for bit in any summation order
  filter2d     |out - f64| <= (k^2 + 2) u sum|w| max|x|: an fp32 dot product of k^2 terms in any order
  filter_sep   |out - f64| <= (2 k + 6) u max|x|: two dot products of k terms with sum|g| = 1, the second on the rounded first
  usm_sharp    the threshold is discontinuous, so in stages: (a) the device mask equals the float64 mask wherever
               ||residual| 255 - threshold| >= 0.01 in float64 (>= 5 x the blur bound x 255); (b) that band holds at most 0.5 % of
               the pixels (asserted on the float64 reference alone); (c) |out - f64 formula with the DEVICE's mask| <= (2 k + 10) u on
               every pixel
Measured on an MI355X (profiles/degrade_error.txt): see the figures there; every test prints its own.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_degrade_host import dot_bound, exact_cases, golden
from vmambair_amd import degradations as D
from vmambair_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
USM_SHAPES = {"a": (1, 3, 27, 33), "b": (2, 1, 26, 26), "c": (2, 3, 64, 80)}


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(bits(a), bits(b))


def reflected_shift(img, k, i, j):
    """what a single 1.0 at (i, j) of a k x k kernel gives: pure data movement"""
    p = k // 2
    return F.pad(img, (p, p, p, p), mode='reflect')[:, :, i:i + img.size(2), j:j + img.size(3)].contiguous()


# ---- 1. exact summation, every tap -------------------------------------------------------------------------------------------
@pytest.mark.tier(0)
@pytest.mark.parametrize("s, kern", exact_cases())
def test_filter2d_bit_exact_on_integer_data(s, kern):
    z = golden()
    img, kernel, want = z[f"ex.{s}.img"], z[f"ex.{s}.{kern}"], torch.from_numpy(z[f"ex.{s}.{kern}.out"]).float()
    got = ops.filter2d(img.to(DEV), kernel.to(DEV), 0)
    wrong = int((got.cpu() != want).sum())
    print(f"[degrade] exact {s} {kern} {tuple(img.shape)}: {wrong} of {want.numel()} differ")
    assert same_bits(got, want)
    assert same_bits(D.filter2D(img.to(DEV), kernel.to(DEV)), want)


@pytest.mark.tier(0)
@pytest.mark.parametrize("box", ((13, 9, 2, 5), (9, 13, 8, 0), (16, 16, 5, 5), (17, 8, 0, 13), (1, 21, 20, 0), (21, 1, 0, 20)))
def test_filter2d_bit_exact_for_every_support_width(box):
    """the three window widths of the kernel (support up to 8, 16 and 24 columns) with the support anywhere in the 21 x 21 kernel"""
    rows, cols, i0, j0 = box
    z = golden()
    img = z["ex.b.img"]
    rng = np.random.RandomState(rows * 100 + cols)
    kernel = torch.zeros(img.size(0), 21, 21)
    block = torch.from_numpy(rng.randint(-2, 3, size=(img.size(0), rows, cols)).astype(np.float32))
    block[:, 0, 0], block[:, -1, -1] = 1.0, -2.0   # the box is exactly rows x cols
    kernel[:, i0:i0 + rows, j0:j0 + cols] = block
    want = D.restate_filter2d(img.double(), kernel.double()).float()   # integers: exact in float64
    assert same_bits(ops.filter2d(img.to(DEV), kernel.to(DEV), 0), want)
    # a kernel of zeros gives zeros
    assert same_bits(ops.filter2d(img.to(DEV), torch.zeros(1, 21, 21, device=DEV), 0), torch.zeros_like(img))


# ---- 2. single-tap kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", ("a", "b"))
def test_single_tap_kernels_shift_the_reflected_image(s):
    z = golden()
    img = (z[f"ex.{s}.img"] / 255.0 + 0.001).to(DEV)   # no longer integers
    for i in (0, 10, 20):
        for j in (0, 10, 20):
            shared = torch.zeros(1, 21, 21, device=DEV)
            shared[0, i, j] = 1.0
            want = reflected_shift(img, 21, i, j)
            got = ops.filter2d(img, shared, 0)
            assert same_bits(got, want), (i, j)
            assert same_bits(ops.filter2d(img, shared.expand(img.size(0), 21, 21).contiguous(), 0), got), (i, j)
    # per sample: every sample its own tap
    taps = [(0, 20), (20, 0), (10, 3)][:img.size(0)]
    kernel = torch.zeros(img.size(0), 21, 21, device=DEV)
    for b, (i, j) in enumerate(taps):
        kernel[b, i, j] = 1.0
    got = ops.filter2d(img, kernel, 0)
    for b, (i, j) in enumerate(taps):
        assert same_bits(got[b:b + 1], reflected_shift(img[b:b + 1], 21, i, j)), b


# ---- 3. round-off ------------------------------------------------------------------------------------------------------------
@pytest.mark.tier(0)
def test_filter2d_round_off_against_float64():
    z = golden()
    img, kernels, want = z["ro.img"], z["ro.kernels"], z["ro.out"]
    got = ops.filter2d(img.to(DEV), kernels.to(DEV), 0).cpu().double()
    err, bound = (got - want).abs(), dot_bound(kernels, img)
    for b, name in enumerate(("isotropic Gaussian", "rotated anisotropic Gaussian", "circular low-pass")):
        ratio = float((err[b] / bound[b]).max())
        print(f"[degrade] filter2d 21 x 21 {name}: max|out - f64| {float(err[b].max()):.3e}, bound {float(bound[b]):.3e}, "
              f"ratio {ratio:.4f}")
        assert ratio <= 1.0, name
    # a shared kernel is B copies of it
    one = ops.filter2d(img.to(DEV), kernels[2:3].to(DEV), 0)
    assert same_bits(one[2:3], ops.filter2d(img[2:3].to(DEV), kernels[2:3].to(DEV), 0))
    assert float(((one.cpu().double()[2] - want[2]).abs() / bound[2]).max()) <= 1.0


# ---- 4. epilogues ------------------------------------------------------------------------------------------------------------
def half_way_values():
    """fp32 values v with fp32(v * 255) == n + 0.5 exactly, n = -3 ... 257"""
    out = []
    for n in range(-3, 258):
        v = np.float32((n + 0.5) / 255.0)
        for cand in (v, np.nextafter(v, np.float32(-9)), np.nextafter(v, np.float32(9))):
            if np.float32(cand * np.float32(255.0)) == np.float32(n + 0.5):
                out.append(cand)
                break
    return np.asarray(out, np.float32)


def test_epilogues_equal_torch_on_the_unquantised_output():
    z = golden()
    img = (z["ro.img"] + torch.linspace(-1.2, 1.2, z["ro.img"].size(-1))).to(DEV)   # a ramp: both clamps act
    kernels = z["ro.kernels"].to(DEV)
    base = ops.filter2d(img, kernels, 0)
    assert float(base.min()) < 0 and float(base.max()) > 1
    assert int(((base * 255.0).round() == 0).logical_and(base < 0).sum()) > 0   # rounds to -0: torch's clamp makes it +0
    assert same_bits(ops.filter2d(img, kernels, 1), torch.clamp(base, 0, 1))
    assert same_bits(ops.filter2d(img, kernels, 2), torch.clamp((base * 255.0).round(), 0, 255) / 255.)
    assert same_bits(D.filter2D(img, kernels, clamp=True), torch.clamp(base, 0, 1))
    assert same_bits(D.filter2D(img, kernels, quantise=True), torch.clamp((base * 255.0).round(), 0, 255) / 255.)
    # x * 255 exactly on .5: round half to even, through the identity kernel
    v = half_way_values()
    assert v.size >= 200
    img = torch.zeros(1, 1, 17, 17)
    img.view(-1)[:v.size] = torch.from_numpy(v)
    img = img.to(DEV)
    ident = torch.zeros(1, 3, 3, device=DEV)
    ident[0, 1, 1] = 1.0
    base = ops.filter2d(img, ident, 0)
    assert same_bits(base, img)
    x = base * 255.0
    assert int(((x - x.floor()) == 0.5).sum()) == v.size
    got = ops.filter2d(img, ident, 2)
    assert same_bits(got, torch.clamp(x.round(), 0, 255) / 255.)
    assert same_bits(ops.filter2d(img, ident, 1), torch.clamp(base, 0, 1))
    # half to even, spelled out: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 254.5 -> 254
    for half, even in ((0.5, 0.0), (1.5, 2.0), (2.5, 2.0), (254.5, 254.0)):
        at = (x.view(-1) == half).nonzero().view(-1)
        assert at.numel() == 1 and float((got.view(-1)[at] * 255.0).round()) == even, half


# ---- 5. the separable kernel -------------------------------------------------------------------------------------------------
@pytest.mark.tier(0)
@pytest.mark.parametrize("s", ("a", "b"))
def test_filter_sep_against_float64(s):
    z = golden()
    img, g, want = z[f"sep.{s}.img"], z["sep.g"], z[f"sep.{s}.out"]
    got = ops.filter_sep(img.to(DEV), g.to(DEV)).cpu().double()
    err, bound = float((got - want).abs().max()), (2 * 51 + 6) * U * float(img.abs().max())
    print(f"[degrade] filter_sep k 51 {tuple(img.shape)}: max|out - f64| {err:.3e}, bound {bound:.3e}, ratio {err / bound:.4f}")
    assert err <= bound


def test_filter_sep_other_lengths_and_ragged_tiles():
    """3, 9 and 63 taps (one, two and eight chunks of 8) on a plane that is no multiple of the 64 x 64 tile, exact integer data"""
    rng = np.random.RandomState(5)
    img = torch.from_numpy(rng.randint(0, 256, size=(2, 2, 70, 133)).astype(np.float32))
    for k in (3, 9, 63):
        g = torch.from_numpy(rng.randint(-2, 3, size=k).astype(np.float32))
        g[0], g[-1] = 1.0, -1.0
        want = D.restate_filter2d(img.double(), torch.outer(g, g).double()[None]).float()   # |sums| <= 255 * 4 * 63^2 < 2^24
        assert same_bits(ops.filter_sep(img.to(DEV), g.to(DEV)), want), k


# ---- 6. USM ------------------------------------------------------------------------------------------------------------------
@pytest.mark.tier(0)
@pytest.mark.parametrize("s", ("a", "b", "c"))
def test_usm_sharp_against_float64_in_stages(s):
    z = golden()
    img32, kernel = z[f"usm.{s}.img"], z["usm.kernel"].double()
    assert tuple(img32.shape) == USM_SHAPES[s]
    img = img32.double()
    weight, threshold, k = 0.5, 10.0, 51
    blur = z[f"usm.{s}.blur"] if f"usm.{s}.blur" in z else D.restate_filter2d(img, kernel)
    residual = img - blur
    t = residual.abs() * 255
    mask64 = t > threshold
    assert np.array_equal(mask64.numpy(), z[f"usm.{s}.mask"].astype(bool))
    g = D.USMSharp()._g.to(DEV)
    out, mask = ops.usm_sharp(img32.to(DEV), g, weight, threshold, True)
    out, mask = out.cpu().double(), mask.cpu()
    assert set(mask.unique().tolist()) <= {0.0, 1.0}
    # (a) the mask, outside the band around the threshold
    band = (t - threshold).abs() < 0.01
    flips = (mask.bool() != mask64)
    share = float(mask64.double().mean())
    print(f"[degrade] usm {tuple(img.shape)}: mask share {share:.3f}, band {int(band.sum())} px ({float(band.double().mean()):.5f}), "
          f"flips {int(flips.sum())}, flips outside the band {int((flips & ~band).sum())}")
    assert not bool((flips & ~band).any())
    # (b) the band is small, on the float64 reference alone
    assert float(band.double().mean()) <= 0.005
    # (c) the output against the float64 formula with the DEVICE's mask, every pixel
    soft = D.restate_filter2d(mask.double(), kernel)
    sharp = torch.clip(img + weight * residual, 0, 1)
    want = soft * sharp + (1 - soft) * img
    clipped = float(((img + weight * residual > 1) | (img + weight * residual < 0)).double().mean())
    err, bound = float((out - want).abs().max()), (2 * k + 10) * U
    print(f"[degrade] usm {tuple(img.shape)}: clip active on {clipped:.4f}, max|out - f64| {err:.3e}, bound {bound:.3e}, "
          f"ratio {err / bound:.4f}")
    assert 0.5 < share < 0.9 and clipped > 0
    assert err <= bound
    # without the mask output the result is the same
    assert same_bits(ops.usm_sharp(img32.to(DEV), g, weight, threshold, False)[0], out.float())


@pytest.mark.parametrize("s", ("a", "b", "c"))
def test_usm_sharp_returns_the_input_where_nothing_is_sharpened(s):
    img = golden()[f"usm.{s}.img"].to(DEV)
    g = D.USMSharp()._g.to(DEV)
    assert same_bits(ops.usm_sharp(img, g, 0.0, 10.0, False)[0], img)      # weight 0: sharp == img
    out, mask = ops.usm_sharp(img, g, 0.5, 255.0, True)                    # threshold 255: an empty mask
    assert float(mask.abs().max()) == 0.0 and same_bits(out, img)


# ---- 7. the public face ------------------------------------------------------------------------------------------------------
def test_modules_route_device_tensors_to_the_kernels(monkeypatch):
    z = golden()
    calls = []
    for name in ("filter2d", "usm_sharp"):
        real = getattr(D._ops, name)
        monkeypatch.setattr(D._ops, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    img, kernels = z["usm.c.img"].to(DEV), z["ro.kernels"][:2].to(DEV)
    usm = D.USMSharp().to(DEV)
    assert list(usm.state_dict().keys()) == ['kernel'] and usm._g.is_cuda
    x = img.clone().requires_grad_(True)
    blurred = D.filter2D(x, kernels)
    sharp = usm(blurred)
    assert calls == ["filter2d", "usm_sharp"]
    assert not blurred.requires_grad and not sharp.requires_grad       # nothing of feed_data is differentiated
    assert same_bits(blurred, ops.filter2d(img, kernels, 0))
    assert same_bits(sharp, ops.usm_sharp(blurred, usm._g, 0.5, 10.0, False)[0])
    assert same_bits(D.filter2D(img, kernels[0]), ops.filter2d(img, kernels[:1], 0))   # a bare (k, k) kernel
    assert same_bits(torch.ops.vmambair.filter2d(img, kernels, 0), blurred)
    assert same_bits(torch.ops.vmambair.usm_sharp(blurred, usm._g, 0.5, 10.0, False)[0], sharp)
    assert same_bits(torch.ops.vmambair.filter_sep(img, usm._g), ops.filter_sep(img, usm._g))
    # what the kernels do not take goes to the restatement: 51 x 51 dense, float64
    calls.clear()
    big = D.filter2D(img, usm.kernel)
    assert calls == [] and float((big - ops.filter_sep(img, usm._g)).abs().max()) <= (51 * 51 + 2 + 2 * 51 + 6) * U   # both bounds
    assert D.filter2D(img.double(), kernels.double()).dtype == torch.float64 and calls == []
    with pytest.raises(ValueError, match="Wrong kernel size"):
        D.filter2D(img, torch.ones(1, 4, 4, device=DEV))
    with pytest.raises(RuntimeError):
        ops.filter2d(img[:, :, :10].contiguous(), kernels, 0)   # H <= k // 2: refused before any launch
    with pytest.raises(RuntimeError):
        ops.filter2d(img.cpu(), kernels.cpu(), 0)


def test_filter2d_then_usm_inside_a_captured_graph():
    z = golden()
    a, b = z["usm.c.img"].to(DEV), z["usm.c.img"].flip(-1).contiguous().to(DEV)
    kernels = z["ro.kernels"][:2].to(DEV)
    usm = D.USMSharp().to(DEV)

    def step(x):
        return usm(D.filter2D(x, kernels, clamp=True), weight=0.7, threshold=4)

    static = a.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(static)   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(static)
    for x in (a, b, a):
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out, step(x))
    assert not same_bits(step(a), step(b))


def test_training_pair_pool_on_device_tensors():
    z = golden()
    pool = D.TrainingPairPool(6)
    for i in range(z["pool.lq"].shape[0]):
        perm = z["pool.perm"][i]
        lq, gt = pool.push_pop(z["pool.lq"][i].to(DEV), z["pool.gt"][i].to(DEV), perm=None if perm[0] < 0 else torch.from_numpy(perm))
        assert lq.is_cuda and torch.equal(lq.cpu(), z["pool.lq_out"][i]) and torch.equal(gt.cpu(), z["pool.gt_out"][i]), i
    q_lr, q_gt = pool.queue()
    assert torch.equal(q_lr.cpu(), z["pool.queue_lr"]) and torch.equal(q_gt.cpu(), z["pool.queue_gt"])
