#!/usr/bin/env python3
"""Timing of DiffJPEG on the device (torch.ops.vmambair.jpeg_roundtrip, oss_jpeg.hip) against its plain-torch restatement, on the
same card.

  python tools/jpeg_bench.py > profiles/jpeg_kernel_timing.txt        (MI355X; profiler off)

Cases: (9, 3, 400, 400) -- the first JPEG step of MambaRealSR.feed_data at scale 1 and batch_size_per_gpu 9 -- and (9, 3, 100, 100),
the final one, with one quality per sample in [30, 95] in a device tensor.  The baseline is what the reference pays with the pip
package: the package's loop ``for i in range(B): factor[i] = quality_to_factor(factor[i])`` over the device tensor (B host reads)
followed by vmambair_amd.degradations' restatement of the package's tensor operations on the same device tensors -- never the new
code.  Per case both sides are warmed up, then timed alternately, every call between its own pair of device events; the median, the
fastest and the slowest are printed.  Acceptance: the slowest new run is faster than the fastest baseline run at both shapes.
A third line gives the new call captured into a graph and replayed, the device's time alone (not part of the acceptance).
Launches per call are counted with torch.profiler in a call of their own, outside the timed ones.  Algorithmic bytes: the image
read once and written once, 2 * 4 * B * 3 * h * w; the fraction is of the 8 TB/s HBM peak of the MI355X.
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vmambair_amd import degradations as D  # noqa: E402

SHAPES = ((9, 3, 400, 400), (9, 3, 100, 100))
WARMUP, REPS = 3, 15
HBM_PEAK = 8.0e12


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, out


def compare(new, base):
    for _ in range(WARMUP):
        new(), base()
    torch.cuda.synchronize()
    tn, tb = [], []
    for _ in range(REPS):
        t, a = timed(new)
        tn.append(t)
        t, b = timed(base)
        tb.append(t)
    return tn, tb, a, b


def replayed(fn):
    """the same call captured into a graph and replayed: the device's time without the host's share of a launch"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    for _ in range(WARMUP):
        graph.replay()
    torch.cuda.synchronize()
    return [timed(graph.replay)[0] for _ in range(REPS)]


def launches(fn):
    """device kernels and copies of one call"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def package_call(x, quality):
    """the package's forward: the per-sample loop that reads every quality on the host, then its tensor operations"""
    factor = quality.clone()   # the package overwrites the caller's tensor; the clone keeps the next call's input intact
    for i in range(factor.size(0)):
        factor[i] = D.quality_to_factor(factor[i])
    return D._restate_jpeg_from_factor(x, factor, False)[0]


def main():
    assert torch.cuda.is_available(), "jpeg_bench.py measures on the GPU"
    print("# DiffJPEG (differentiable=False, one quality per sample in [30, 95]) on one MI355X, fp32; every call between its own pair of")
    print(f"# device events, {REPS} calls of each side, alternating, after {WARMUP} warm-up calls each, profiler off: median "
          "(fastest - slowest);")
    print("# baseline: the package's per-sample quality loop (B host reads) + the plain-torch restatement of its tensor operations on the")
    print("# same device tensors; launches: device kernels and copies of one call (torch.profiler, a call of its own)")
    print("# max|new - baseline|: two fp32 evaluations of a discontinuous operator; a coefficient that the two round to different")
    print("# sides moves a block (tests/test_jpeg_gpu.py compares with float64 in stages for that reason)")
    jpeg = D.DiffJPEG(differentiable=False).cuda()
    all_ok = True
    for shape in SHAPES:
        b, c, h, w = shape
        g = torch.Generator().manual_seed(h * 10007 + w)
        img = torch.rand(shape, generator=g).cuda()
        quality = (30 + 65 * torch.rand(b, generator=g)).cuda()
        with torch.no_grad():
            tn, tb, a, ref = compare(lambda: jpeg(img, quality), lambda: package_call(img, quality))
            n_new, n_base = launches(lambda: jpeg(img, quality)), launches(lambda: package_call(img, quality))
            tg = replayed(lambda: jpeg(img, quality))
        nbytes = 2 * 4 * b * c * h * w
        mn, mb = statistics.median(tn), statistics.median(tb)
        diff = (a - ref).abs()
        print(f"\n## {shape}")
        print(f"{'DiffJPEG, HIP kernel':<34}{mn:10.1f} us  ({min(tn):.1f} - {max(tn):.1f})  {n_new:3d} launches; "
              f"{nbytes / 1e6:.1f} MB -> {nbytes / (mn * 1e-6) / 1e12:.2f} TB/s = {100 * nbytes / (mn * 1e-6) / HBM_PEAK:.1f} % of HBM peak")
        mg = statistics.median(tg)
        print(f"{'  the same launch, graph replay':<34}{mg:10.1f} us  ({min(tg):.1f} - {max(tg):.1f})  "
              f"{nbytes / (mg * 1e-6) / 1e12:.2f} TB/s = {100 * nbytes / (mg * 1e-6) / HBM_PEAK:.1f} % of HBM peak "
              "(the package's form cannot be captured: it reads the qualities on the host)")
        print(f"{'DiffJPEG, package loop + torch':<34}{mb:10.1f} us  ({min(tb):.1f} - {max(tb):.1f})  {n_base:3d} launches; "
              f"{nbytes / (mb * 1e-6) / 1e12:.3f} TB/s = {100 * nbytes / (mb * 1e-6) / HBM_PEAK:.2f} % of HBM peak")
        ok = max(tn) < min(tb)
        all_ok &= ok
        print(f"    medians {mb / mn:.1f} x; slowest new {max(tn):.1f} us vs fastest baseline {min(tb):.1f} us: "
              f"{'faster in every run' if ok else 'NOT faster in every run'}; max|new - baseline| {float(diff.max()):.2e}, "
              f"{float((diff > 1e-5).float().mean()) * 100:.3f} % of the pixels above 1e-5")
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
