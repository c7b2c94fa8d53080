#!/usr/bin/env python3
"""Timing of the degradation filters (torch.ops.vmambair.filter2d / usm_sharp, oss_degrade.hip) against their plain-torch restatement
through the vendor library, on the same card.

  python tools/degrade_bench.py > profiles/degrade_kernel_timing.txt        (MI355X; profiler off)

Cases: per-sample filter2D with 21 x 21 kernels and USMSharp at radius 50 (a 51 x 51 Gaussian), each at (9, 3, 600, 600) -- the
dataset's crop at batch_size_per_gpu 9 -- and (9, 3, 400, 400).  The baseline is vmambair_amd.degradations.restate_filter2d /
restate_usm on the same device tensors: F.pad(reflect) + a grouped conv2d, never the new code.  Per case both sides are warmed up,
then timed alternately, every call between its own pair of device events; the median, the fastest and the slowest are printed.
Acceptance: the slowest new run is faster than the fastest baseline run.  Work counted from the shapes: one multiply-add per tap
and output pixel; bytes = the tensors each launch has to read and write once.
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vmambair_amd import degradations as D  # noqa: E402

SHAPES = ((9, 3, 600, 600), (9, 3, 400, 400))
WARMUP, REPS = 3, 15


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
    return tn, tb, float((a - b).abs().max())


def report(name, tn, tb, diff, fma_new, fma_base, nbytes):
    mn, mb = statistics.median(tn), statistics.median(tb)
    print(f"{name + ', HIP kernels':<44}{mn:10.1f} us  ({min(tn):.1f} - {max(tn):.1f})  {fma_new / 1e9:7.2f} G multiply-adds -> "
          f"{2 * fma_new / (mn * 1e-6) / 1e12:6.2f} TFLOP/s; {nbytes / 1e6:.0f} MB -> {nbytes / (mn * 1e-6) / 1e12:.2f} TB/s")
    print(f"{name + ', torch restatement':<44}{mb:10.1f} us  ({min(tb):.1f} - {max(tb):.1f})  {fma_base / 1e9:7.2f} G multiply-adds -> "
          f"{2 * fma_base / (mb * 1e-6) / 1e12:6.2f} TFLOP/s")
    ok = max(tn) < min(tb)
    print(f"    medians {mb / mn:.1f} x; slowest new {max(tn):.1f} us vs fastest baseline {min(tb):.1f} us: "
          f"{'faster in every run' if ok else 'NOT faster in every run'}; max|new - baseline| {diff:.2e}")


def main():
    assert torch.cuda.is_available(), "degrade_bench.py measures on the GPU"
    print("# filter2D (per-sample 21 x 21 kernels) and USMSharp (radius 50) on one MI355X, fp32; every call between its own pair of")
    print(f"# device events, {REPS} calls of each side, alternating, after {WARMUP} warm-up calls each, profiler off: median "
          "(fastest - slowest);")
    print("# baseline: the plain-torch restatement (F.pad reflect + grouped conv2d through the vendor library) on the same tensors")
    print("# max|new - baseline|: two fp32 evaluations; for USM it is set by the pixels of this random image whose residual the two put")
    print("# on different sides of the threshold (tests/test_degrade_gpu.py compares with float64 in stages for that reason)")
    usm = D.USMSharp().cuda()
    for shape in SHAPES:
        b, c, h, w = shape
        g = torch.Generator().manual_seed(h * 10007 + w)
        img = torch.rand(shape, generator=g).cuda()
        kernels = torch.rand(b, 21, 21, generator=g)
        kernels = (kernels / kernels.sum(dim=(1, 2), keepdim=True)).cuda()
        n = b * c * h * w
        print(f"\n## {shape}")
        tn, tb, diff = compare(lambda: D.filter2D(img, kernels), lambda: D.restate_filter2d(img, kernels))
        report("filter2D k 21, one kernel per sample", tn, tb, diff, n * 441, n * 441, 2 * n * 4)
        tn, tb, diff = compare(lambda: usm(img), lambda: D.restate_usm(img, usm.kernel))
        # four passes: each reads one or three planes and writes one or two (row: 1 + 1, mask: 2 + 2, row: 1 + 1, blend: 3 + 1)
        report("USMSharp radius 50", tn, tb, diff, n * 4 * 51, n * 2 * 2601, 12 * n * 4)


if __name__ == "__main__":
    main()
