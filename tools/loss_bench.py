#!/usr/bin/env python3
"""Timing of the device pixel loss (vmambair_amd.losses.L1Loss, oss_pixel_loss.hip) against the torch expression the training step
uses by default, forward + backward of the loss alone at the headline step's shape.

Three runs, in this order (MI355X; the profiler gets a run of its own, end-to-end numbers are taken with it off):
  python tools/loss_bench.py --events OUT.json           device events around CALLS replays of a captured graph per form (what the
                                                          captured training step pays) and around CALLS eager calls, three repeats
                                                          each, the two forms alternating
  rocprofv3 --kernel-trace --stats -d DIR -o loss -- python tools/loss_bench.py --profile
                                                          each form of each case between the library's marker kernels: launch counts
  python tools/loss_bench.py --report DIR OUT.json       -> the text of profiles/pixel_loss_timing.txt on stdout
Cases: pred (8, 3, 256, 256) bf16 with an fp32 target (the bf16 step), then fp32 / fp32.  The two forms:
  device   loss = losses.L1Loss()(pred, gt); d loss / d pred by autograd (two launches forward, one backward)
  torch    loss = F.l1_loss(pred.float(), gt); d loss / d pred by autograd (GraphedTrainStep's default loss_fn)
Bytes = pred and target read by the forward and by the backward, dpred written once.
"""
import glob
import json
import os
import sqlite3
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vmambair_amd import _capi, losses  # noqa: E402

SHAPE = (8, 3, 256, 256)
CASES = (("pred bf16, target fp32", torch.bfloat16), ("pred fp32, target fp32", torch.float32))
WARMUP, CALLS, REPEATS, TRACED = 20, 500, 3, 50
COPY_TBS = 6.29


def make(dtype):
    g = torch.Generator().manual_seed(0)
    gt = torch.rand(SHAPE, generator=g)
    pred = (gt + 0.05 * torch.randn(SHAPE, generator=g)).to(dtype)
    return pred.cuda().requires_grad_(True), gt.cuda()


def forms():
    l1 = losses.L1Loss()
    return (("device", lambda p, t: l1(p, t)), ("torch", lambda p, t: F.l1_loss(p.float(), t)))


def fwd_bwd(fn, pred, gt):
    loss = fn(pred, gt)
    grad, = torch.autograd.grad(loss, pred)
    return loss, grad


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
    for name, dtype in CASES:
        pred, gt = make(dtype)
        row = {"case": name, "bytes": pred.numel() * (3 * pred.element_size() + 2 * 4)}
        graphs, outs = {}, {}
        for form, fn in forms():
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(WARMUP):
                    fwd_bwd(fn, pred, gt)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graphs[form] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[form]):
                outs[form] = fwd_bwd(fn, pred, gt)
            for _ in range(WARMUP):
                graphs[form].replay()
            row[form + "_graph_us"], row[form + "_eager_us"] = [], []
        for _ in range(REPEATS):   # alternating: the two forms see the same machine
            for form, fn in forms():
                row[form + "_graph_us"].append(timed(graphs[form].replay, CALLS))
        for _ in range(REPEATS):
            for form, fn in forms():
                row[form + "_eager_us"].append(timed(lambda: fwd_bwd(fn, pred, gt), CALLS))
        torch.cuda.synchronize()
        (ld, gd), (lt, gt_) = outs["device"], outs["torch"]
        row["loss_device"], row["loss_torch"] = float(ld), float(lt)
        row["grad_equal"] = bool(torch.equal(gd, gt_))
        row["grad_max_diff"] = float((gd.float() - gt_.float()).abs().max())
        rows.append(row)
        print(row, flush=True)
    return rows


def profile():
    lib = _capi.load()
    stream = torch.cuda.current_stream().cuda_stream
    for name, dtype in CASES:
        pred, gt = make(dtype)
        for form, fn in forms():
            for _ in range(WARMUP):
                fwd_bwd(fn, pred, gt)
            lib.oss_prof_marker(1, stream)
            for _ in range(TRACED):
                fwd_bwd(fn, pred, gt)
            lib.oss_prof_marker(2, stream)
            torch.cuda.synchronize()


def report(trace_dir, events_json):
    rows = json.load(open(events_json))
    db = sorted(glob.glob(os.path.join(trace_dir, "**", "*results.db"), recursive=True))[0]
    cur = sqlite3.connect(db).cursor()
    begins = [r[0] for r in cur.execute("select end from kernels where name like '%oss_prof_marker_begin%' order by start")]
    ends = [r[0] for r in cur.execute("select start from kernels where name like '%oss_prof_marker_end%' order by start")]
    fmt = lambda v: ", ".join("%.1f" % x for x in v)   # noqa: E731
    print(f"# L1 loss forward + backward alone at pred {SHAPE} on one MI355X: vmambair_amd.losses.L1Loss (oss_pixel_loss.hip) against")
    print(f"# F.l1_loss(pred.float(), gt) with autograd, the training step's default.  Device events around {CALLS} replays of a captured")
    print(f"# graph / {CALLS} eager calls after {WARMUP} warm-up calls, {REPEATS} repeats, the two forms alternating, profiler off; launch counts and")
    print(f"# kernel times from a separate rocprofv3 --kernel-trace --stats run ({TRACED} eager calls per form between marker kernels)")
    windows = iter(zip(begins, ends))
    for row in rows:
        print(f"\n## {row['case']}")
        floor_us = row["bytes"] / (COPY_TBS * 1e12) * 1e6
        print(f"algorithmic bytes {row['bytes'] / 1e6:.2f} MB / {COPY_TBS} TB/s measured copy rate = {floor_us:.2f} us")
        traced = {}
        for form in ("device", "torch"):
            t0, t1 = next(windows)
            ks = list(cur.execute("select name, count(*), avg(end-start)/1e3, min(end-start)/1e3, max(end-start)/1e3 from kernels "
                                  "where start>=? and end<=? group by name order by 3 desc", (t0, t1)))
            traced[form] = (sum(k[1] for k in ks) / TRACED, sum(k[1] * k[2] for k in ks) / TRACED, ks)
        for form in ("device", "torch"):
            launches, kernel_us, ks = traced[form]
            print(f"{form:6s}  launches per forward + backward {launches:5.1f}   kernels {kernel_us:7.1f} us   graph replay {min(row[form + '_graph_us']):7.1f} us "
                  f"(all repeats: {fmt(row[form + '_graph_us'])})   eager call {min(row[form + '_eager_us']):7.1f} us (all repeats: {fmt(row[form + '_eager_us'])})")
            for k in ks:
                print(f"    {k[1]:5d} x {k[2]:9.1f} us (min {k[3]:.1f}, max {k[4]:.1f})  {k[0][:150]}")
        d, t = min(row["device_graph_us"]), min(row["torch_graph_us"])
        print(f"graph replay: device {d:.1f} us against torch {t:.1f} us = {t / d:.2f} x; kernels: {traced['torch'][1] / traced['device'][1]:.2f} x")
        print(f"loss device {row['loss_device']:.9g}, torch {row['loss_torch']:.9g}; gradients bit-equal: {row['grad_equal']} "
              f"(largest difference {row['grad_max_diff']:.3e})")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    if sys.argv[1] == "--events":
        json.dump(events(), open(sys.argv[2], "w"), indent=1)
    elif sys.argv[1] == "--profile":
        profile()
    elif sys.argv[1] == "--report":
        report(sys.argv[2], sys.argv[3])
