#!/usr/bin/env python3
"""Timing of the on-device validation metrics (vmambair_amd.metrics.image_metrics, oss_metrics.hip) against the CPU restatement.

Three runs, in this order (MI355X; the profiler gets a run of its own, end-to-end numbers are taken with it off):
  python tools/metrics_bench.py --events OUT.json        device events around CALLS calls per case after warm-up, and the same
                                                          metrics on the CPU (16 threads) including the device-to-host copy
  rocprofv3 --kernel-trace --stats -d DIR -o metrics -- python tools/metrics_bench.py --profile
                                                          each case between the library's marker kernels
  python tools/metrics_bench.py --report DIR OUT.json    kernel time per case from the trace + the events -> the text of
                                                          profiles/metrics_kernel_timing.txt on stdout
Cases: one 2048 x 2048 fp16 pair (the RealSR x4 output of a 512 x 512 input), Y channel and RGB, valid borders, crop 4; a batch of
eight 256 x 256 pairs.  Bytes = both images read once; peaks from the data sheet (8.0 TB/s) and the measured copy rate (6.29 TB/s).
"""
import glob
import json
import os
import sqlite3
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vmambair_amd import _capi, metrics  # noqa: E402

CASES = (("2048x2048 fp16, Y, valid", (1, 3, 2048, 2048), torch.float16, True),
         ("2048x2048 fp16, RGB, valid", (1, 3, 2048, 2048), torch.float16, False),
         ("8 x 256x256 fp16, Y, valid", (8, 3, 256, 256), torch.float16, True))
WARMUP, CALLS, CPU_REPS = 20, 200, 3
FORWARD_MS = 33.8   # untiled RealSR 512^2 -> 2048^2 forward (profiles/r06_rocprof_realsr_untiled_steady_state.txt)


def make(shape, dtype):
    g = torch.Generator().manual_seed(0)
    gt = torch.rand(shape, generator=g)
    sr = (gt + 0.02 * torch.randn(shape, generator=g)).to(dtype)
    return sr.cuda(), gt.to(dtype).cuda()


def events():
    torch.set_num_threads(16)
    rows = []
    for name, shape, dtype, yc in CASES:
        sr, gt = make(shape, dtype)
        for _ in range(WARMUP):
            out = metrics.image_metrics(sr, gt, 4, yc)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            out = metrics.image_metrics(sr, gt, 4, yc)
        e1.record()
        torch.cuda.synchronize()
        call_us = e0.elapsed_time(e1) * 1e3 / CALLS
        cpu = []
        for _ in range(CPU_REPS):
            t0 = time.perf_counter()
            vals = []
            for i in range(shape[0]):
                a, b = metrics.tensor2img(sr[i].cpu()).numpy(), metrics.tensor2img(gt[i].cpu()).numpy()
                vals.append((metrics.calculate_psnr(a, b, 4, "HWC", yc), metrics.calculate_ssim(a, b, 4, "HWC", yc)))
            cpu.append((time.perf_counter() - t0) * 1e3)
        dev = out.cpu()
        worst = max(abs(float(dev[i, 1]) - vals[i][1]) for i in range(shape[0]))
        rows.append({"case": name, "call_us": call_us, "cpu_ms": min(cpu), "cpu_ms_all": cpu, "ssim_diff": worst,
                     "bytes": 2 * sr.numel() * sr.element_size(),
                     # 11 taps x 5 moments along rows for 26 halo rows per 16 centre rows, then along columns (oss_metrics.hip)
                     "fma": (1 if yc else 3) * shape[0] * (shape[2] - 18) * (shape[3] - 18) * 55 * (1 + 26 / 16)})
        print(rows[-1], flush=True)
    return rows


def profile():
    lib = _capi.load()
    stream = torch.cuda.current_stream().cuda_stream
    for name, shape, dtype, yc in CASES:
        sr, gt = make(shape, dtype)
        for _ in range(WARMUP):
            metrics.image_metrics(sr, gt, 4, yc)
        lib.oss_prof_marker(1, stream)
        for _ in range(50):
            metrics.image_metrics(sr, gt, 4, yc)
        lib.oss_prof_marker(2, stream)
        torch.cuda.synchronize()


def report(trace_dir, events_json):
    rows = json.load(open(events_json))
    db = sorted(glob.glob(os.path.join(trace_dir, "**", "*results.db"), recursive=True))[0]
    cur = sqlite3.connect(db).cursor()
    begins = [r[0] for r in cur.execute("select end from kernels where name like '%oss_prof_marker_begin%' order by start")]
    ends = [r[0] for r in cur.execute("select start from kernels where name like '%oss_prof_marker_end%' order by start")]
    print("# image_metrics (PSNR + SSIM, crop 4) on one MI355X; device events around %d calls after %d warm-up calls, profiler off;" % (CALLS, WARMUP))
    print("# kernel time from a separate rocprofv3 --kernel-trace run (50 calls per case between marker kernels);")
    print("# CPU: tensor2img + calculate_psnr + calculate_ssim of vmambair_amd.metrics, 16 threads, device-to-host copy included, best of %d" % CPU_REPS)
    for row, t0, t1 in zip(rows, begins, ends):
        ks = list(cur.execute("select name, count(*), avg(end-start)/1e3, min(end-start)/1e3, max(end-start)/1e3 from kernels "
                              "where start>=? and end<=? group by name order by 3 desc", (t0, t1)))
        main = [k for k in ks if "oss_image_metrics_kernel" in k[0]][0]
        fin = [k for k in ks if "oss_image_metrics_finish" in k[0]][0]
        total = sum(k[1] * k[2] for k in ks) / main[1]
        print(f"\n## {row['case']}")
        print(f"call (device events, per call)          {row['call_us']:9.1f} us")
        print(f"kernels per call (trace)                {total:9.1f} us  = oss_image_metrics_kernel {main[2]:.1f} (min {main[3]:.1f}, max {main[4]:.1f}) "
              f"+ finish {fin[2]:.1f} + {len(ks) - 2} small torch kernels (stack / log10 / division of the PSNR)")
        tb = row["bytes"] / (main[2] * 1e-6) / 1e12
        print(f"bytes (both images read once)           {row['bytes'] / 1e6:9.1f} MB -> {tb:.2f} TB/s over the main kernel = {100 * tb / 8.0:.1f} % of the 8.0 TB/s "
              f"HBM peak ({100 * tb / 6.29:.1f} % of the measured 6.29 TB/s copy rate): far below the memory roof, the kernel's time is fp64 arithmetic")
        tf = 2 * row["fma"] / (main[2] * 1e-6) / 1e12
        print(f"fp64 FMAs of the two filter passes      {row['fma'] / 1e6:9.1f} M  -> {tf:.1f} TFLOP/s = {100 * tf / 78.6:.0f} % of the 78.6 TFLOP/s fp64 vector peak "
              "(data sheet); the rest of the kernel's time: the conversion on load (per luma pixel three fp32 and one fp64 correctly rounded "
              "division, 2.1 halo pixels per centre), the fp64 division of the SSIM quotient, LDS traffic and two barriers per tile at 3 waves per SIMD")
        print(f"CPU restatement incl. device-to-host copy {row['cpu_ms']:9.1f} ms  (all repeats: {', '.join('%.1f' % v for v in row['cpu_ms_all'])})")
        print(f"largest |SSIM device - SSIM CPU|         {row['ssim_diff']:.2e}")
        if row["case"].startswith("2048"):
            print(f"share of the {FORWARD_MS} ms untiled RealSR forward that produces such an image: {100 * row['call_us'] / 1e3 / FORWARD_MS:.2f} % "
                  f"(call), {100 * main[2] / 1e3 / FORWARD_MS:.2f} % (main kernel)")
        for k in ks:
            print(f"    {k[1]:5d} x {k[2]:9.1f} us  {k[0][:140]}")


if __name__ == "__main__":
    if sys.argv[1] == "--events":
        json.dump(events(), open(sys.argv[2], "w"), indent=1)
    elif sys.argv[1] == "--profile":
        profile()
    elif sys.argv[1] == "--report":
        report(sys.argv[2], sys.argv[3])
