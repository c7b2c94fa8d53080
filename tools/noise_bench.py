#!/usr/bin/env python3
"""Timing of the two noise steps of the RealSR degradation on the device (torch.ops.vmambair.noise_gaussian / noise_poisson,
oss_noise.hip) against their plain-torch restatement, on the same card.

  python tools/noise_bench.py > profiles/noise_kernel_timing.txt        (MI355X; profiler off)

Cases: random_add_gaussian_noise_pt (sigma_range [1, 30]) and random_add_poisson_noise_pt (scale_range [0.05, 3]), gray_prob 0.4,
clip=True, rounds=False -- the calls of MambaRealSR.feed_data with the values of the options files -- at (9, 3, 400, 400) and
(9, 3, 100, 100), the sizes of the first and second noise step at batch_size_per_gpu 9.  The baseline is what the reference pays with
the pip package: vmambair_amd.degradations' restatement of the package's operations on the same device tensors with torch's
generator, host reads and ``unique`` loop included -- never the new code.  Per case both sides are warmed up, then timed
alternately, every call between its own pair of device events; the median, the fastest and the slowest are printed, and the ratio
of the medians as measured (no speed-up is fixed in advance).  A third line gives the new call captured into a graph and replayed,
the device's time alone; the restatement cannot be captured (it reads on the host).  Launches per call (device kernels, memsets and
copies) are counted with torch.profiler in a call of their own; host synchronisations per call are counted by running the call
under torch.cuda.set_sync_debug_mode("warn") and counting the warnings.
"""
import os
import statistics
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vmambair_amd import degradations as D  # noqa: E402

SHAPES = ((9, 3, 400, 400), (9, 3, 100, 100))
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
        tn.append(timed(new)[0])
        tb.append(timed(base)[0])
    return tn, tb


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
    """device kernels, memsets and copies of one call"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def host_syncs(fn):
    """synchronising calls of one call, as torch's sync debug mode reports them"""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return sum(1 for w in caught if "synchroniz" in str(w.message).lower())


def main():
    assert torch.cuda.is_available(), "noise_bench.py measures on the GPU"
    print("# random_add_gaussian_noise_pt (sigma_range [1, 30]) and random_add_poisson_noise_pt (scale_range [0.05, 3]), gray_prob 0.4,")
    print("# clip=True, rounds=False on one MI355X, fp32; every call between its own pair of device events,")
    print(f"# {REPS} calls of each side, alternating, after {WARMUP} warm-up calls each, profiler off: median (fastest - slowest);")
    print("# baseline: the plain-torch restatement of the package's operations on the same device tensors (torch's generator, the host")
    print("# reads and the per-sample unique loop included); launches: device kernels, memsets and copies of one call (torch.profiler,")
    print("# a call of its own); host syncs: synchronising calls torch's sync debug mode reports for one call")
    stream = D.NoiseStream(1234, "cuda")
    cases = (("random_add_gaussian_noise_pt", lambda x: D.random_add_gaussian_noise_pt(x, (1, 30), 0.4, stream=stream),
              lambda x: D.restate_random_add_gaussian_noise_pt(x, (1, 30), 0.4)),
             ("random_add_poisson_noise_pt", lambda x: D.random_add_poisson_noise_pt(x, (0.05, 3), 0.4, stream=stream),
              lambda x: D.restate_random_add_poisson_noise_pt(x, (0.05, 3), 0.4)))
    for shape in SHAPES:
        g = torch.Generator().manual_seed(shape[2] * 10007 + shape[3])
        img = torch.rand(shape, generator=g).cuda()
        for name, new, base in cases:
            torch.manual_seed(0)
            tn, tb = compare(lambda: new(img), lambda: base(img))
            n_new, n_base = launches(lambda: new(img)), launches(lambda: base(img))
            s_new, s_base = host_syncs(lambda: new(img)), host_syncs(lambda: base(img))
            tg = replayed(lambda: new(img))
            mn, mb, mg = statistics.median(tn), statistics.median(tb), statistics.median(tg)
            print(f"\n## {name} {shape}")
            print(f"{'HIP kernels':<32}{mn:10.1f} us  ({min(tn):.1f} - {max(tn):.1f})  {n_new:3d} launches, {s_new} host syncs")
            print(f"{'  the same call, graph replay':<32}{mg:10.1f} us  ({min(tg):.1f} - {max(tg):.1f})")
            print(f"{'restatement, plain torch':<32}{mb:10.1f} us  ({min(tb):.1f} - {max(tb):.1f})  {n_base:3d} launches, {s_base} host syncs")
            print(f"    medians: restatement / HIP = {mb / mn:.1f} x, restatement / replay = {mb / mg:.1f} x; slowest HIP {max(tn):.1f} us vs "
                  f"fastest restatement {min(tb):.1f} us")
    return 0


if __name__ == "__main__":
    sys.exit(main())
