#!/usr/bin/env python3
"""Timing of the NIQE features launch (torch.ops.vmambair.niqe_features, oss_niqe.hip) against the CPU restatement.

  python tools/niqe_bench.py > profiles/niqe_kernel_timing.txt        (MI355X; profiler off)

Cases: fp16 network outputs in [0, 1] (quantise + Y channel on load, crop 0) of 508 x 764, 1356 x 2040 and 2048 x 2048 pixels,
batch 1 and batch 8.  Per case WARMUP launches, then REPS launches each between its own pair of device events; the median, the
fastest and the slowest are printed.  The launch is the whole device side of image_niqe: one kernel, no scratch, no finishing
launch.  The CPU column is the wall time of vmambair_amd.metrics.niqe_features (numpy, 16 threads) on one plane of the same
size, once; the host part both share (one copy of the features, the 36 x 36 covariance and pseudo-inverse) is timed separately.
Work counted from the shapes: per pixel of both scales 2 x 49 fp64 products and 2 x 49 fp64 additions of the window sums.
"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vmambair_amd import _capi, metrics  # noqa: E402

SIZES = ((508, 764), (1356, 2040), (2048, 2048))
BATCHES = (1, 8)
WARMUP, REPS = 5, 25
Q, Y = _capi.METRIC_QUANTISE, _capi.METRIC_Y


def main():
    if len(sys.argv) != 2:
        sys.exit("usage: niqe_bench.py <niqe_pris_params.npz of the reference>")
    assert torch.cuda.is_available(), "niqe_bench.py measures on the GPU"
    torch.set_num_threads(16)
    model = metrics.NiqeModel.load(sys.argv[1])
    tables, window = model.device_tables("cuda"), torch.from_numpy(model.window)
    print("# niqe_features (quantise + Y on load, crop 0, fp16 input) on one MI355X; every launch between its own pair of")
    print(f"# device events, {REPS} launches after {WARMUP} warm-up launches, profiler off: median (fastest - slowest);")
    print("# CPU: vmambair_amd.metrics.niqe_features (numpy, 16 threads) on one plane of the size, wall time, once")
    for height, width in SIZES:
        g = torch.Generator().manual_seed(height * 10007 + width)
        blocks = (height // 96) * (width // 96)
        pixels = blocks * 96 * 96 * 1.25
        cpu_ms = host_ms = None
        for batch in BATCHES:
            sr = torch.rand(batch, 3, height, width, generator=g).half().cuda()
            for _ in range(WARMUP):
                out = torch.ops.vmambair.niqe_features(sr, tables, window, 0, Q | Y)
            torch.cuda.synchronize()
            times = []
            for _ in range(REPS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = torch.ops.vmambair.niqe_features(sr, tables, window, 0, Q | Y)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1) * 1e3)
            med = statistics.median(times)
            flop = batch * pixels * 4 * 49
            print(f"\n## {height} x {width}, batch {batch}: {blocks} blocks per image, grid {blocks} x 2 x {batch} workgroups")
            print(f"launch (device events)                  {med:10.1f} us  ({min(times):.1f} - {max(times):.1f})  = {med / batch:.1f} us per image")
            print(f"fp64 operations of the window sums      {flop / 1e6:10.1f} M   -> {flop / (med * 1e-6) / 1e12:.2f} TFLOP/s of the 78.6 TFLOP/s fp64 vector peak "
                  f"(data sheet) = {100 * flop / (med * 1e-6) / 78.6e12:.1f} %")
            nbytes = batch * 3 * height * width * 2
            print(f"bytes (the image read once)             {nbytes / 1e6:10.1f} MB  -> {nbytes / (med * 1e-6) / 1e12:.3f} TB/s: far below the memory roof")
            if batch == 1:
                t0 = time.perf_counter()
                feat = out.cpu().numpy()
                value = metrics.niqe_from_features(feat[0], model)
                host_ms = (time.perf_counter() - t0) * 1e3
                img = metrics.tensor2img(sr[0].cpu()).numpy()
                plane = metrics.to_y_channel(torch.from_numpy(img).to(torch.float32))[..., 0].numpy()
                t0 = time.perf_counter()
                want = metrics.niqe_features(plane, model)
                cpu_ms = (time.perf_counter() - t0) * 1e3
                ok = ~np.isnan(want)
                same = np.array_equal(np.isnan(feat[0]), np.isnan(want))
                diff = float(np.max(np.abs(feat[0][ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-300)))
                print(f"host part of image_niqe (copy + covariance + pinv) {host_ms:7.2f} ms, NIQE {value:.6f}")
                print(f"CPU restatement of the features         {cpu_ms:10.1f} ms = {cpu_ms * 1e3 / med:.0f} x the launch; largest relative difference "
                      f"device - CPU over the features {diff:.2e}, NaN positions {'equal' if same else 'DIFFER'}")


if __name__ == "__main__":
    main()
