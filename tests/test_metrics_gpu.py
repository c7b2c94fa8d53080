"""``torch.ops.vmambair.image_metrics`` (oss_metrics.hip): PSNR + SSIM of a batch of image pairs on the device, against the values
the reference's functions return (tests/golden/g10_ssim.npz) and against the float64 CPU restatement at the sizes users run.

Tolerances (derived, not tuned):
  SSIM   |diff| <= 1e-10.  A float64 evaluation in another summation order measured 2e-14 against the reference, a float32
         evaluation 7e-9 ... 8.7e-7 (the cancellation in E[x^2] - mu^2): the bound sits between the two with margin on both sides.
  mse    without the Y channel EQUAL to the CPU value: sums of integer squares below 2^53 are exact in any order, one division.
         With it (differences and squares in fp32, float64 sum) relative |diff| <= 1e-12: reordering of a float64 sum.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from vmambair_amd import _capi, metrics, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q, Y, R = _capi.METRIC_QUANTISE, _capi.METRIC_Y, _capi.METRIC_REPLICATE
MODES = (("ssim_valid_rgb", False, "valid"), ("ssim_valid_y", True, "valid"), ("ssim_replicate_y", True, "replicate"))
SSIM_TOL, MSE_RTOL = 1e-10, 1e-12


def golden_cases():
    z = np.load(os.path.join(GOLDEN, "g10_ssim.npz"))
    for name in sorted({k.split(".")[0] for k in z.files}):
        a = z[f"{name}.a"]
        yield name, z, a, (a.astype(np.int16) + z[f"{name}.d"]).astype(np.uint8)


def chw(img: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(img[None] if img.ndim == 2 else np.ascontiguousarray(img.transpose(2, 0, 1)))


def rgb_planes(img: np.ndarray, dtype=torch.float32) -> torch.Tensor:
    """uint8 (H, W[, 3]) BGR -> (1, C, H, W) RGB float planes in [0, 255] on the device (exact in all three dtypes)"""
    return chw(img).flip(0)[None].to(DEV).to(dtype)


def flags_of(yc: bool, border: str, channels: int) -> int:
    return (Y if yc and channels == 3 else 0) | (R if border == "replicate" else 0)


def check_mse(got: float, want: float, yc: bool, what):
    print(f"{what}: mse {got!r} cpu {want!r}")
    if yc:
        assert abs(got - want) <= MSE_RTOL * abs(want), (what, got, want)
    else:
        assert got == want, (what, got, want)


def test_image_metrics_match_reference_golden():
    n = 0
    for name, z, a, b in golden_cases():
        ch = 1 if a.ndim == 2 else 3
        for crop in (0, 4):
            for key, yc, border in MODES:
                want = float(z[f"{name}.{key}_{crop}"])
                got = metrics.calculate_ssim(chw(a).to(DEV), chw(b).to(DEV), crop, "HWC", yc, border)
                dtype = (torch.float32, torch.float16, torch.bfloat16)[n % 3]
                out = torch.ops.vmambair.image_metrics(rgb_planes(a, dtype), rgb_planes(b, dtype), crop, flags_of(yc, border, ch)).cpu()
                print(f"{name} crop {crop} {key}: reference {want!r} calculate_ssim {got - want:+.2e} op({dtype}) {float(out[0, 1]) - want:+.2e}")
                assert abs(got - want) <= SSIM_TOL and abs(float(out[0, 1]) - want) <= SSIM_TOL, (name, crop, key, got, float(out[0, 1]), want)
                check_mse(float(out[0, 0]), metrics.calculate_mse(a, b, crop, "HWC", yc), yc, (name, crop, key))
                ref_db = float(z[f"{name}.psnr_{crop}_y{int(yc)}"])
                db = float(10.0 * torch.log10(255.0 ** 2 / out[0, 0]))
                # Y: the reference's own mean runs in fp32 (test_checkpoint_psnr.py::test_psnr_matches_reference_values)
                assert db == ref_db or abs(db - ref_db) < (2e-5 if yc else 1e-9), (name, crop, yc, db, ref_db)
                n += 1
    assert n == 8 * 2 * 3
    # the float pair that reaches outside [0, 1]: quantised on load, as the reference's tensor2img did for the stored values
    z = np.load(os.path.join(GOLDEN, "g10_ssim.npz"))
    ta, tb = torch.from_numpy(z["t2i_24x28.ta"]).to(DEV), torch.from_numpy(z["t2i_24x28.tb"]).to(DEV)
    for crop in (0, 4):
        for key, yc, border in MODES:
            out = metrics.image_metrics(ta, tb, crop, yc, border).cpu()
            assert abs(float(out[0, 1]) - float(z[f"t2i_24x28.{key}_{crop}"])) <= SSIM_TOL
            assert abs(float(out[0, 0]) - float(z[f"t2i_24x28.psnr_{crop}_y{int(yc)}"])) < (2e-5 if yc else 1e-9)
    same = torch.rand(2, 3, 40, 40, device=DEV)
    out = metrics.image_metrics(same, same.clone()).cpu()
    assert torch.isinf(out[:, 0]).all() and (out[:, 1] == 1.0).all()


@pytest.mark.parametrize("height,width,dtype,batch", [(321, 481, torch.float32, 1), (508, 764, torch.float32, 1),
                                                      (1356, 2040, torch.float32, 1), (2048, 2048, torch.float16, 1),
                                                      (256, 256, torch.bfloat16, 3)])
def test_image_metrics_match_the_cpu_restatement_at_user_sizes(height, width, dtype, batch):
    g = torch.Generator().manual_seed(height * 10007 + width)
    gt = torch.rand(batch, 3, height, width, generator=g) * 1.1 - 0.05
    # a smooth image under noise: large windows of nearly constant brightness, where E[x^2] - mu^2 cancels
    yy, xx = torch.meshgrid(torch.arange(height) / height, torch.arange(width) / width, indexing="ij")
    gt[:, :, : height // 2] = (0.5 + 0.45 * torch.sin(3.0 * yy + 2.0 * xx))[: height // 2]
    sr = gt + 0.01 * torch.randn(gt.shape, generator=g)
    sr, gt = sr.to(dtype), gt.to(dtype)
    sr_d, gt_d = sr.to(DEV), gt.to(DEV)
    for crop in (0, 4):
        for yc, border in ((True, "valid"), (False, "valid"), (True, "replicate")):
            out = torch.ops.vmambair.image_metrics(sr_d, gt_d, crop, Q | flags_of(yc, border, 3)).cpu()
            pub = metrics.image_metrics(sr_d, gt_d, crop, yc, border).cpu()
            for i in range(batch):
                a, b = metrics.tensor2img(sr[i]).numpy(), metrics.tensor2img(gt[i]).numpy()
                want = metrics.calculate_ssim(a, b, crop, "HWC", yc, border)
                what = (height, width, str(dtype), i, crop, yc, border)
                print(f"{what}: ssim {float(out[i, 1])!r} cpu {want!r} diff {float(out[i, 1]) - want:+.2e}")
                assert abs(float(out[i, 1]) - want) <= SSIM_TOL, what
                check_mse(float(out[i, 0]), metrics.calculate_mse(a, b, crop, "HWC", yc), yc, what)
                assert float(pub[i, 1]) == float(out[i, 1])
                assert abs(float(pub[i, 0]) - metrics.calculate_psnr(a, b, crop, "HWC", yc)) < 1e-9
            if batch == 1:
                assert metrics.validation_ssim(sr_d, gt_d, crop, yc, border) == float(out[0, 1])


def test_quantise_flag_is_bit_identical_to_tensor2img():
    g = torch.Generator().manual_seed(3)
    sr = torch.rand(2, 3, 45, 70, generator=g) * 1.6 - 0.3           # reaches outside [0, 1]
    gt = torch.rand(2, 3, 45, 70, generator=g)
    ties = (torch.arange(0, 70 * 3, dtype=torch.float32) + 0.5) / 255.0    # k + 0.5 after * 255 where fp32 keeps it: half to even
    sr[0, :, 7] = ties.view(3, 70)
    gt[1, :, 9] = ties.flip(0).view(3, 70)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        s, t = sr.to(dtype).to(DEV), gt.to(dtype).to(DEV)
        # tensor2img's arithmetic, batched: (H, W, 3) BGR uint8 per image -> float RGB planes in [0, 255]
        planes = [torch.stack([metrics.tensor2img(v[i]).permute(2, 0, 1).flip(0).float() for i in range(2)]) for v in (s, t)]
        for single in (False, True):
            if single:
                s, t, planes = s[:, 1:2], t[:, 1:2], [p[:, 1:2] for p in planes]
            for yc, border in ((True, "valid"), (False, "valid"), (True, "replicate")):
                fl = flags_of(yc, border, s.shape[1])
                got = torch.ops.vmambair.image_metrics(s, t, 4, fl | Q)
                want = torch.ops.vmambair.image_metrics(planes[0], planes[1], 4, fl)
                assert torch.equal(got, want), (dtype, single, yc, border, got, want)
                pub = metrics.image_metrics(s, t, 4, yc, border)
                assert torch.equal(pub[:, 1], got[:, 1]) and torch.equal(pub[:, 0], 10.0 * torch.log10(255.0 * 255.0 / got[:, 0]))


def test_strided_views_need_no_copy():
    g = torch.Generator().manual_seed(5)
    for dtype in (torch.float32, torch.float16):
        big_a = torch.rand(2, 3, 90, 131, generator=g).to(dtype).to(DEV)
        big_b = (big_a.float() + 0.02 * torch.randn(big_a.shape, generator=g).to(DEV)).to(dtype)
        va, vb = big_a[:, :, 3:81, 7:120], big_b[:, :, 3:81, 7:120]       # RealSREnhancer.post_process style crops
        assert not va.is_contiguous() and va.stride(3) == 1
        for fl in (Q | Y, Q, Q | Y | R):
            got = torch.ops.vmambair.image_metrics(va, vb, 4, fl)
            assert torch.equal(got, torch.ops.vmambair.image_metrics(va.contiguous(), vb.contiguous(), 4, fl))
            mixed = torch.ops.vmambair.image_metrics(va, vb.contiguous(), 4, fl)    # the two images carry their own strides
            assert torch.equal(got, mixed)
        one = torch.ops.vmambair.image_metrics(big_a[1:, 1:2, 3:81, 7:120], big_b[1:, 1:2, 3:81, 7:120], 0, Q)
        assert torch.equal(one, torch.ops.vmambair.image_metrics(va[1:, 1:2].contiguous(), vb[1:, 1:2].contiguous(), 0, Q))


def test_image_metrics_reruns_are_bit_identical():
    g = torch.Generator().manual_seed(7)
    a = torch.rand(3, 3, 300, 420, generator=g).to(DEV)
    b = (a + 0.03 * torch.randn(a.shape, generator=g).to(DEV)).half()
    a = a.half()
    for fl in (Q | Y, Q, Q | Y | R):
        first = torch.ops.vmambair.image_metrics(a, b, 4, fl)
        for _ in range(4):
            assert torch.equal(torch.ops.vmambair.image_metrics(a, b, 4, fl), first)
        # an image's result does not depend on its place in the batch
        assert torch.equal(torch.ops.vmambair.image_metrics(a[2:], b[2:], 4, fl), first[2:])


def test_image_metrics_inside_a_captured_graph():
    g = torch.Generator().manual_seed(11)
    inputs = []
    for _ in range(2):
        x = torch.rand(2, 3, 128, 192, generator=g)
        inputs.append((x.to(DEV), (x + 0.05 * torch.randn(x.shape, generator=g)).to(DEV)))
    sa, sb = torch.zeros_like(inputs[0][0]), torch.zeros_like(inputs[0][1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):   # warm-up outside the capture
            metrics.image_metrics(sa, sb)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = metrics.image_metrics(sa, sb)
    for a, b in inputs:
        sa.copy_(a)
        sb.copy_(b)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, metrics.image_metrics(a, b))
    assert not torch.equal(metrics.image_metrics(*inputs[0]), metrics.image_metrics(*inputs[1]))


def test_cpu_tensors_and_bad_shapes_are_rejected():
    cpu, dev = torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 32, device=DEV)
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        ops.image_metrics(cpu, cpu, 4, 0)
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        ops.image_metrics(dev, cpu, 4, 0)
    with pytest.raises(RuntimeError):
        torch.ops.vmambair.image_metrics(cpu, cpu, 4, 0)
    for a, b, crop, fl in ((dev[:, :2], dev[:, :2], 4, 0), (dev[:, :1], dev[:, :1], 4, Y), (dev, dev, 16, R), (dev[..., :18], dev[..., :18], 4, 0),
                           (dev, dev[:, :, :31], 4, 0), (dev, dev.half(), 4, 0), (dev.double(), dev.double(), 4, 0), (dev[0], dev[0], 4, 0),
                           (dev, dev, 4, 8)):
        with pytest.raises(RuntimeError):
            torch.ops.vmambair.image_metrics(a, b, crop, fl)
        assert not ops.image_metrics_ok(a, crop, fl) or a.shape != b.shape or a.dtype != b.dtype
    assert ops.image_metrics_ok(dev, 4, Q | Y) and ops.image_metrics_ok(dev[..., :18], 4, R) and not ops.image_metrics_ok(cpu, 4, 0)
    with pytest.raises(ValueError, match="_ssim_3d"):
        metrics.image_metrics(dev, dev, 4, False, "replicate")
