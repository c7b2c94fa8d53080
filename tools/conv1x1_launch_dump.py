#!/usr/bin/env python
"""What the 1x1-convolution launchers decide and compute, as text: run it in two checkouts (each with its own built library) and
diff the outputs.  The workgroup-level and the wave-level kernels are bit-identical by design, so result hashes alone cannot show a
changed dispatch; the launches themselves come from a kernel trace of the same run:

    rocprofv3 --kernel-trace --output-format csv -d trace -- python tools/conv1x1_launch_dump.py > dump.txt
    python tools/conv1x1_launch_dump.py --reduce trace > profiles/conv1x1_launch_trace_<revision>.txt
    python tools/conv1x1_launch_dump.py --check dump.txt profiles/conv1x1_launch_trace_<revision>.txt

The run goes through a fixed list of calls (tests/conv1x1_plan_cases.py: one smallest call per instantiation; then the headline's
8 x 96 x 64 x 64 and 8 x 48 x 64 x 64 projections, the EFFN widths 127 / 254 / 255 / 510 and a Deraining level-0 call at batch 4,
forward and input gradient, with and without PackedConv1x1Weights) through the public Python ops and prints per call a sha256 of
the result and, where the library has it, ``oss_conv1x1_describe`` of the call.  ``--reduce`` turns the trace into one line per
forward / input-gradient dispatch: kernel name with template arguments, grid in workgroups, workgroup size, LDS bytes.  ``--check``
compares the describe lines of a dump with those dispatches, in order: kernel, grid and workgroup size.  (The trace's LDS column is
the kernel's static allocation -- 0 for the workgroup-level and the fp32 split-K kernels, whose LDS is dynamic -- so the planned
dynamic bytes have no traced counterpart; they stay in the describe lines.)"""
import csv
import glob
import hashlib
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNEL = re.compile(r"oss::(oss_conv1x1_(?:wg_|pair_|pairw_|pairk_|reuse_|f32_)?kernel)<([^<>]*)>")


def calls():
    from conv1x1_plan_cases import FAMILY_NAMES, SMALLEST
    for t in sorted(SMALLEST):
        yield FAMILY_NAMES[t[0]] + "-" + "-".join(map(str, t[1:])), SMALLEST[t]
    extra = [(8, 96, c, 4096, r) for c, r in ((192, 0), (96, 1), (510, 0))] + [(8, 255, 96, 4096, 1)]          # 8 x 96 x 64 x 64
    extra += [(8, 48, c, 4096, r) for c, r in ((96, 0), (48, 1), (254, 0))] + [(8, 127, 48, 4096, 1)]          # 8 x 48 x 64 x 64
    extra += [(4, 48, 96, 16384, 0), (4, 48, 254, 16384, 0), (4, 127, 48, 16384, 1)]                            # Deraining level 0, batch 4
    for B, cin, cout, P, res in extra:
        for io in ("bf16", "f32"):
            for img in ((0, 1) if io == "bf16" else (0,)):
                yield f"{io}_fwd_{B}x{cin}to{cout}x{P}_res{res}_img{img}", (io, 0, B, cout, cin, P, res, img, 0, 0, 0, (1, 0))
                yield f"{io}_dgrad_{B}x{cin}to{cout}x{P}_img{img}", (io, 1, B, cin, cout, P, 0, img, 0, 0, 0, (1, 0))


def kernel_name(o, io):
    T = {"bf16": "oss::bf16_t", "f16": "oss::f16_t"}.get(io)
    b = lambda v: "true" if v else "false"
    return ("oss_conv1x1_wg_kernel<%s, %d, %s, %d, false, %s, false, %s>" % (T, o.ks, b(o.wt), o.pt, b(o.pf), b(o.wimg)),
            "oss_conv1x1_pair_kernel<%s, %d, %s, %s, %s, %s, %s>" % (T, o.ks, b(o.wt), b(o.wvec), b(o.res), b(o.pf), b(o.wimg)),
            "oss_conv1x1_pairw_kernel<%s>" % T,
            "oss_conv1x1_pairk_kernel<%s, 8, %d, %s, %s, %s>" % (T, o.mt, b(o.wt), b(o.wvec), b(o.wimg)),
            "oss_conv1x1_reuse_kernel<%s, %d, %s>" % (T, o.ks, b(o.wt)),
            "oss_conv1x1_kernel<%s>" % T,
            "oss_conv1x1_f32_kernel<2, false, %s>" % b(o.x3), "oss_conv1x1_f32_kernel<1, false, %s>" % b(o.x3),
            "oss_conv1x1_f32_kernel<1, true, %s>" % b(o.x3))[o.family]


def run():
    import torch

    from conv1x1_plan_cases import run_case
    from vmambair_amd import _capi
    has_describe = hasattr(_capi.load(), "oss_conv1x1_describe")
    for name, case in calls():
        r = run_case(case, seed=7, describe=has_describe)
        torch.cuda.synchronize()
        digest = hashlib.sha256(r["got"].detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]
        print(name, "sha256", digest, flush=True)
        if has_describe:
            o = r["describe"]
            print(name, "describe", kernel_name(o, case[0]), f"grid=({o.grid_x},{o.grid_y},{o.grid_z}) block={o.block} lds={o.lds_bytes}",
                  flush=True)


def reduce(trace_dir):
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    assert len(files) == 1, files
    rows = list(csv.DictReader(open(files[0])))
    col = {k.lower(): k for k in rows[0]}
    rows.sort(key=lambda r: int(r[col["start_timestamp"]]))
    for r in rows:
        m = KERNEL.search(r[col["kernel_name"]].replace("(int)", "").replace("(bool)", ""))
        if not m:
            continue
        wg = [int(r[col["workgroup_size_" + a]]) for a in "xyz"]
        grid = [int(r[col["grid_size_" + a]]) // w for a, w in zip("xyz", wg)]       # the trace counts work-items
        print("%s<%s>" % m.groups(), "grid=(%d,%d,%d)" % tuple(grid), "block=%d" % (wg[0] * wg[1] * wg[2]), "static_lds=%s" % r[col["lds_block_size"]])


def check(dump, reduction):
    want = [l.split(" describe ", 1)[1].split() for l in open(dump) if " describe " in l]
    got = [l.split() for l in open(reduction) if l.strip()]
    assert len(want) == len(got) and len(want) > 0, (len(want), len(got))
    for i, (w, g) in enumerate(zip(want, got)):
        assert w[:-1] == g[:-1], (i, w, g)   # kernel with template arguments, grid, workgroup size
    print(len(want), "described calls equal their traced dispatches")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--reduce":
        reduce(sys.argv[2])
    elif len(sys.argv) > 1 and sys.argv[1] == "--check":
        check(sys.argv[2], sys.argv[3])
    else:
        run()
