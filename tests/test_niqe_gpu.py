"""``torch.ops.vmambair.niqe_features`` (oss_niqe.hip) and the device paths of ``vmambair_amd.metrics.calculate_niqe`` /
``image_niqe``: the NIQE features of a batch of images in one launch, against the values the reference's functions return
(tests/golden/g14_niqe.npz) and against the CPU restatement at a size users run.

Tolerances (derived, not tuned; ``niqe_cases``):
  against the reference    alphas EQUAL, NaN positions identical, the other features and the value within 1e-6 relative -- the
                           bound of tests/test_niqe_host.py, for its reasons
  against the restatement  alphas EQUAL, NaN positions identical, the other features within 1e-10 relative: both follow the
                           same dtypes to the same fp32 MSCN values and products and differ in the ORDER of the float64 moment
                           sums (9216 terms: a few 1e-16 each way) -- the reasoning of SSIM_TOL in tests/test_metrics_gpu.py.  An
                           fp32 step taken differently would show at 1e-8 and more.
"""
import numpy as np
import pytest
import torch

import niqe_cases as nc
from vmambair_amd import _capi, metrics, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q, Y = _capi.METRIC_QUANTISE, _capi.METRIC_Y
DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def window():
    return torch.from_numpy(nc.model().window)


def features(planes: torch.Tensor, crop: int, flags: int) -> torch.Tensor:
    return torch.ops.vmambair.niqe_features(planes, nc.model().device_tables(DEV), window(), crop, flags)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """bit for bit, NaNs included (a block with a constant stretch has NaN features)"""
    return a.shape == b.shape and torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_niqe_features_match_reference_golden():
    n = 0
    for name, (img, order, per_crop) in nc.cases().items():
        planes = torch.from_numpy(nc.planes(img, order)).to(DEV)
        for crop, (feat, value) in per_crop.items():
            dtype = DTYPES[n % 3]        # uint8 values are exact in all three
            got = features(planes.to(dtype), crop, Y if order != "HW" else 0)
            assert got.shape == (1,) + feat.shape and got.dtype == torch.float64 and got.device.type == "cuda"
            got = got[0].cpu().numpy()
            nc.check_features(got, feat, nc.REF_TOL, (name, crop, str(dtype), "reference"))
            nc.check_value(metrics.niqe_from_features(got, nc.model()), value, nc.REF_TOL, (name, crop, "reference"))
            arg = torch.from_numpy(img).to(DEV)
            nc.check_value(metrics.calculate_niqe(arg, crop, order, "y", nc.model()), value, nc.REF_TOL, (name, crop, "calculate_niqe"))
            plane = torch.from_numpy(img).to(torch.float32)
            plane = (metrics.to_y_channel(plane)[..., 0] if order != "HW" else plane).numpy()
            cpu = metrics.niqe_features(plane[crop:plane.shape[0] - crop, crop:plane.shape[1] - crop], nc.model())
            nc.check_features(got, cpu, nc.DEVICE_TOL, (name, crop, str(dtype), "restatement"))
            n += 1
    assert n == 11


def test_image_niqe_quantises_on_load():
    z = nc.golden()
    t = torch.from_numpy(z["t2i_110x210.tensor"].astype(np.float32))
    for crop in (0, 4):
        want = float(z[f"t2i_110x210.niqe_{crop}"])
        for dtype in (torch.float32, torch.float16):       # the stored tensor is float16-valued
            got = metrics.image_niqe(t.to(dtype).to(DEV), nc.model(), crop)
            assert got.shape == (1,) and got.dtype == torch.float64 and not got.is_cuda
            nc.check_value(float(got[0]), want, nc.REF_TOL, ("t2i", crop, str(dtype)))
        # the quantise flag is tensor2img's arithmetic: the same bits as the op on the uint8 image
        img = torch.from_numpy(nc.planes(z["t2i_110x210.img"], "HWC")).to(DEV)
        assert torch.equal(features(t.to(DEV), crop, Q | Y), features(img, crop, Y))
    grey = t[:, 1:2].to(DEV)
    assert torch.equal(features(grey, 4, Q), features((grey.clamp(0, 1) * 255.0).round(), 4, 0))
    pairs = [(t.to(DEV), t.to(DEV))]
    m = metrics.mean_metrics(pairs, 4, niqe_model=nc.model())
    assert sorted(m) == ["niqe", "psnr", "ssim"] and m["niqe"] == float(metrics.image_niqe(t.to(DEV), nc.model(), 4)[0])
    assert sorted(metrics.mean_metrics(pairs, 4)) == ["psnr", "ssim"]


def test_batch_through_a_cropped_view_equals_single_images_bit_for_bit():
    g = torch.Generator().manual_seed(5)
    for dtype in (torch.float32, torch.float16):
        big = torch.rand(3, 3, 215, 330, generator=g)
        big[1] = 0.5 + 0.02 * torch.randn(3, 215, 330, generator=g)          # three different images
        big[2, :, 100:] = 0.25
        big = big.to(dtype).to(DEV)
        view = big[:, :, 3:211, 7:318]                                           # 208 x 311: crop 4 -> 200 x 303, 2 x 3 blocks
        assert not view.is_contiguous() and view.stride(3) == 1
        got = features(view, 4, Q | Y)
        assert got.shape == (3, 6, 36)
        assert same_bits(got, features(view.contiguous(), 4, Q | Y))
        for i in range(3):
            assert same_bits(got[i:i + 1], features(view[i:i + 1].contiguous(), 4, Q | Y)), (dtype, i)
        assert not same_bits(got[0], got[1])
        one = features(big[1:, 1:2, 3:211, 7:318], 0, Q)                         # a channel slice of a batch slice
        assert same_bits(one, features(view[1:, 1:2].contiguous(), 0, Q))


def test_niqe_features_reruns_are_bit_identical():
    g = torch.Generator().manual_seed(7)
    a = (torch.rand(2, 3, 200, 300, generator=g) * 1.2 - 0.1).half().to(DEV)
    first = features(a, 0, Q | Y)
    for _ in range(4):
        assert same_bits(features(a, 0, Q | Y), first)
    assert same_bits(metrics.image_niqe(a, nc.model()), metrics.image_niqe(a, nc.model()))


def test_user_size_matches_the_cpu_restatement():
    """508 x 764 (a x4 RealSR tile row), fp16 in [0, 1]: 5 x 7 blocks with a remainder on both sides, half smooth"""
    height, width = 508, 764
    g = torch.Generator().manual_seed(height * 10007 + width)
    sr = torch.rand(1, 3, height, width, generator=g) * 1.1 - 0.05
    yy, xx = torch.meshgrid(torch.arange(height) / height, torch.arange(width) / width, indexing="ij")
    sr[:, :, : height // 2] = (0.5 + 0.45 * torch.sin(3.0 * yy + 2.0 * xx) + 0.01 * torch.randn(height, width, generator=g))[: height // 2]
    sr = sr.half()
    got = features(sr.to(DEV), 4, Q | Y)[0].cpu().numpy()
    img = metrics.tensor2img(sr).numpy()
    plane = metrics.to_y_channel(torch.from_numpy(img).to(torch.float32))[4:-4, 4:-4, 0].numpy()
    want = metrics.niqe_features(plane, nc.model())
    assert got.shape == want.shape == (35, 36)
    nc.check_features(got, want, nc.DEVICE_TOL, (height, width, "fp16", "restatement"))
    value = float(metrics.image_niqe(sr.to(DEV), nc.model(), 4)[0])
    print(f"niqe {value!r}, of the restatement's features {metrics.niqe_from_features(want, nc.model())!r}")
    assert value == metrics.niqe_from_features(got, nc.model())     # the same host arithmetic on the same features


def test_niqe_features_inside_a_captured_graph():
    g = torch.Generator().manual_seed(11)
    inputs = [torch.rand(2, 3, 128, 200, generator=g).to(DEV) for _ in range(2)]
    tables, win = nc.model().device_tables(DEV), window()
    static = torch.zeros_like(inputs[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):   # warm-up outside the capture
            torch.ops.vmambair.niqe_features(static, tables, win, 4, Q | Y)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = torch.ops.vmambair.niqe_features(static, tables, win, 4, Q | Y)
    for x in inputs:
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out, features(x, 4, Q | Y))
    assert not same_bits(features(inputs[0], 4, Q | Y), features(inputs[1], 4, Q | Y))


def test_bad_arguments_are_rejected():
    dev = torch.zeros(1, 3, 120, 130, device=DEV)
    tables, win = nc.model().device_tables(DEV), window()
    for a, crop, fl in ((dev[:, :2], 0, 0), (dev[:, :1], 0, Y), (dev, 0, 0), (dev, 13, Y), (dev[..., :95], 0, Y), (dev.double(), 0, Y),
                        (dev[0], 0, Y), (dev, 0, Y | 4)):
        with pytest.raises(RuntimeError):
            torch.ops.vmambair.niqe_features(a, tables, win, crop, fl)
        assert not ops.niqe_features_ok(a, crop, fl)
    assert ops.niqe_features_ok(dev, 12, Q | Y) and ops.niqe_features_ok(dev[:, :1], 0, Q)
    with pytest.raises(RuntimeError, match="tables"):
        torch.ops.vmambair.niqe_features(dev, tables[:3], win, 0, Y)
    with pytest.raises(RuntimeError, match="window"):
        torch.ops.vmambair.niqe_features(dev, tables, win.to(DEV), 0, Y)
    with pytest.raises(ValueError, match="gray"):
        metrics.calculate_niqe(dev[0], 0, "CHW", "gray", nc.model())
    with pytest.raises(ValueError, match="96 x 96"):
        metrics.image_niqe(dev[..., :95], nc.model())
