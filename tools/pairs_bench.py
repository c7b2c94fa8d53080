#!/usr/bin/env python3
"""Timing of the device-resident pair sampler (vmambair_amd.data.DevicePairPool, oss_pairs.hip): draw + gather per batch.

Three runs, in this order (MI355X; the profiler gets a run of its own, end-to-end numbers are taken with it off):
  python tools/pairs_bench.py --events OUT.json          device events around CALLS batches per case after warm-up: eager calls,
                                                          replays of a captured graph, and the same batch assembled from torch ops
  rocprofv3 --kernel-trace --stats -d DIR -o pairs -- python tools/pairs_bench.py --profile
                                                          each case between the library's marker kernels
  python tools/pairs_bench.py --report DIR OUT.json STEP_MS [DERAIN_128_MS DERAIN_384_MS]
                                                          kernel time per case from the trace + the events -> the text of
                                                          profiles/pairs_kernel_timing.txt on stdout; STEP_MS = the training step
                                                          (bench.py line of the same visit) the batches feed; the two Deraining
                                                          steps (bench.py --config deraining --patch 128 --batch-per-gpu 8 / --patch
                                                          384 --batch-per-gpu 1) are what the padded cases feed
Cases: the headline batch (8 pairs, LQ 64 x 64, x4 -> GT 256 x 256) from a pool of 512 sub-image pairs of 120 x 120 / 480 x 480
(376 MB: more than the 256 MiB Infinity Cache) and the Deraining batch (8 pairs of 128 x 128, x1) from 512 pairs of 384 x 384
(453 MB); and Deraining's own rule (``dataset_gt_size`` 384: reflect padding, crop at 384, augmentation, the common window;
oss_pairs_draw_window + oss_pairs_gather_padded) on 512 pairs of 321 x 481 (474 MB): the first stage, 8 windows of 128 x 128, and the
last, 1 patch of 384 x 384.  Bytes = every source byte read once, every float written once; copy rate 6.29 TB/s (profiles/, the
measured rate).
"""
import glob
import json
import os
import sqlite3
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vmambair_amd import DevicePairPool, _capi  # noqa: E402

# name, batch, LQ patch, scale, LQ image (h, w), pairs, dataset_gt_size, the step of --report the case feeds
CASES = (("headline: batch 8, LQ 64x64, x4", 8, 64, 4, (120, 120), 512, None, 0),
         ("Deraining: batch 8, 128x128, x1", 8, 128, 1, (384, 384), 512, None, 0),
         ("Deraining rule: batch 8, 128x128 windows of 384 crops, 321x481 images padded to 384", 8, 128, 1, (321, 481), 512, 384, 1),
         ("Deraining rule: batch 1, 384x384, 321x481 images padded to 384", 1, 384, 1, (321, 481), 512, 384, 2))
WARMUP, CALLS = 20, 500
COPY_TBS = 6.29


def make_pool(size, scale, n):
    h, w = size
    g, l = h * w * scale * scale * 3, h * w * 3
    gen = torch.Generator(device="cuda").manual_seed(0)
    data = torch.randint(0, 256, (n * (g + l),), dtype=torch.uint8, device="cuda", generator=gen)
    table = torch.tensor([[i * (g + l), i * (g + l) + g, h, w] for i in range(n)], dtype=torch.int64)
    return DevicePairPool(data, table, scale, 3, seed=1)


def reflected(start, count, n):
    """indices start .. start + count - 1 of an axis of n elements extended by cv2.BORDER_REFLECT"""
    r = torch.arange(start, start + count, device="cuda") % (2 * n)
    return torch.where(r < n, r, 2 * n - 1 - r)


def torch_batch(pool, samples, p, padded=False):
    """the same batch from torch ops on the device (views of the pool; one stack per output)"""
    s, lqs, gts = pool.scale, [], []
    for pair, top, left, code in samples:
        go, lo, h, w = pool.table_host[pair].tolist()
        for off, k, out in ((lo, 1, lqs), (go, s, gts)):
            img = pool.data[off:off + h * w * k * k * 3].view(h * k, w * k, 3)
            if padded:
                img = img[reflected(top, p, h)][:, reflected(left, p, w)]
            else:
                img = img[top * k:(top + p) * k, left * k:(left + p) * k]
            if code & 1:
                img = img.flip(1)
            if code & 2:
                img = img.flip(0)
            if code & 4:
                img = img.transpose(0, 1)
            out.append(img.flip(2).permute(2, 0, 1).float() / 255.0)
    return torch.stack(lqs), torch.stack(gts)


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def events():
    rows = []
    for name, batch, p, scale, size, n, G, _ in CASES:
        pool = make_pool(size, scale, n)
        lq = torch.empty(batch, 3, p, p, device="cuda")
        gt = torch.empty(batch, 3, p * scale, p * scale, device="cuda")
        for _ in range(WARMUP):
            pool.next_into(lq, gt, dataset_gt_size=G)
        eager = [timed(lambda: pool.next_into(lq, gt, dataset_gt_size=G), CALLS) for _ in range(3)]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            pool.next_into(lq, gt, dataset_gt_size=G)
        for _ in range(WARMUP):
            graph.replay()
        replay = [timed(graph.replay, CALLS) for _ in range(3)]
        samples = pool._samples[batch].cpu().tolist()
        a, b = torch_batch(pool, samples, p, G is not None)
        same = bool(torch.equal(a, lq) and torch.equal(b, gt))
        for _ in range(5):
            torch_batch(pool, samples, p, G is not None)
        torch_us = [timed(lambda: torch_batch(pool, samples, p, G is not None), 50) for _ in range(3)]
        rows.append({"case": name, "eager_us": eager, "graph_us": replay, "torch_us": torch_us, "torch_equal": same,
                     "clamped": int(pool.clamped.item()), "bytes": 5 * batch * 3 * p * p * (1 + scale * scale)})
        print(rows[-1], flush=True)
    return rows


def profile():
    lib = _capi.load()
    stream = torch.cuda.current_stream().cuda_stream
    for name, batch, p, scale, size, n, G, _ in CASES:
        pool = make_pool(size, scale, n)
        lq = torch.empty(batch, 3, p, p, device="cuda")
        gt = torch.empty(batch, 3, p * scale, p * scale, device="cuda")
        for _ in range(WARMUP):
            pool.next_into(lq, gt, dataset_gt_size=G)
        lib.oss_prof_marker(1, stream)
        for _ in range(50):
            pool.next_into(lq, gt, dataset_gt_size=G)
        lib.oss_prof_marker(2, stream)
        torch.cuda.synchronize()


def report(trace_dir, events_json, steps_ms):
    rows = json.load(open(events_json))
    db = sorted(glob.glob(os.path.join(trace_dir, "**", "*results.db"), recursive=True))[0]
    cur = sqlite3.connect(db).cursor()
    begins = [r[0] for r in cur.execute("select end from kernels where name like '%oss_prof_marker_begin%' order by start")]
    ends = [r[0] for r in cur.execute("select start from kernels where name like '%oss_prof_marker_end%' order by start")]
    print(f"# DevicePairPool.next_into (oss_pairs_draw + oss_pairs_gather) on one MI355X; device events around {CALLS} batches after {WARMUP} warm-up")
    print("# batches, three repeats, profiler off; kernel time from a separate rocprofv3 --kernel-trace run (50 batches per case between")
    print("# marker kernels); (a) the same batch from torch ops on the device, 50 batches, three repeats (\"equal\": bit-equality with the")
    print("# kernels' output, which tests/test_pairs_gpu.py pins to the reference's arrays); the (c) step is the headline x4 SR step, and for the")
    print("# \"Deraining rule\" cases (dataset_gt_size 384: oss_pairs_draw_window + oss_pairs_gather_padded) the Deraining step of their own shape")
    for row, case, t0, t1 in zip(rows, CASES, begins, ends):
        step_ms = steps_ms[case[7]] if case[7] < len(steps_ms) else steps_ms[0]
        ks = list(cur.execute("select name, count(*), avg(end-start)/1e3, min(end-start)/1e3, max(end-start)/1e3 from kernels "
                              "where start>=? and end<=? group by name order by 3 desc", (t0, t1)))
        gather = [k for k in ks if "oss_pairs_gather" in k[0]][0]
        draw = [k for k in ks if "oss_pairs_draw" in k[0]][0]
        fmt = lambda v: ", ".join("%.1f" % x for x in v)   # noqa: E731
        floor_us = row["bytes"] / (COPY_TBS * 1e12) * 1e6
        print(f"\n## {row['case']}")
        print(f"draw + gather, eager calls (device events, per batch)   {min(row['eager_us']):8.1f} us  (all repeats: {fmt(row['eager_us'])}; host-bound: two launches from Python)")
        print(f"draw + gather, captured graph replay (per batch)        {min(row['graph_us']):8.1f} us  (all repeats: {fmt(row['graph_us'])})")
        print(f"kernels per batch (trace)                                {draw[2] + gather[2]:8.1f} us  = oss_pairs_draw {draw[2]:.1f} (min {draw[3]:.1f}, max {draw[4]:.1f}) "
              f"+ oss_pairs_gather {gather[2]:.1f} (min {gather[3]:.1f}, max {gather[4]:.1f})")
        print(f"(a) same batch from torch ops on the device              {min(row['torch_us']):8.1f} us  (all repeats: {fmt(row['torch_us'])}; equal to the kernels' output: {row['torch_equal']})")
        tb = row["bytes"] / (gather[2] * 1e-6) / 1e12
        print(f"(b) algorithmic bytes {row['bytes'] / 1e6:.2f} MB / {COPY_TBS} TB/s copy rate          {floor_us:8.2f} us  -> the gather kernel moves {tb:.2f} TB/s = "
              f"{100 * tb / COPY_TBS:.0f} % of the copy rate")
        print(f"(c) training step of the same visit                      {step_ms * 1e3:8.1f} us  -> draw + gather = {100 * (draw[2] + gather[2]) / (step_ms * 1e3):.3f} % (kernels), "
              f"{100 * min(row['graph_us']) / (step_ms * 1e3):.3f} % (graph replay), {100 * min(row['eager_us']) / (step_ms * 1e3):.3f} % (eager calls); target <= 1 %")
        print(f"device-side clamp flag after the run: {row['clamped']}")
        for k in ks:
            print(f"    {k[1]:5d} x {k[2]:9.1f} us  {k[0][:140]}")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    if sys.argv[1] == "--events":
        json.dump(events(), open(sys.argv[2], "w"), indent=1)
    elif sys.argv[1] == "--profile":
        profile()
    elif sys.argv[1] == "--report":
        report(sys.argv[2], sys.argv[3], [float(v) for v in sys.argv[4:]])
