#!/usr/bin/env python
"""What the scan launchers decide and compute, as text: run it in two checkouts (each with its own built library) and diff the
outputs.  Per seeded case one line with oss_scan_last_variant / _segments / _lane_states of the forward and the backward call and
a sha256 of out, x and each gradient.  The kernels are atomic-free and bit-reproducible, so a differing line is a changed launch
decision (or changed arithmetic).  Uses only the Python API and the oss_scan_last_* / oss_scan_set_* entry points.

    python tools/scan_launch_dump.py > profiles/scan_launch_dump_<revision>.txt
"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vmambair_amd                      # noqa: E402
from vmambair_amd import _capi           # noqa: E402

DEV = "cuda:0"


def sha(t):
    if t is None:
        return "-"
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def inputs(batch, dim, N, G, L, itype, seed):
    g = torch.Generator().manual_seed(seed)
    A = -0.5 * torch.rand(dim, N, generator=g)
    B = torch.randn(batch, G, N, L, generator=g).to(itype)
    C = torch.randn(batch, G, N, L, generator=g).to(itype)
    D = torch.randn(dim, generator=g)
    bias = 0.5 * torch.rand(dim, generator=g)
    u = torch.randn(batch, dim, L, generator=g).to(itype)
    delta = (0.5 * torch.rand(batch, dim, L, generator=g)).to(itype)
    dout = torch.randn(batch, dim, L, generator=g).to(itype)
    return [t.to(DEV) for t in (u, delta, A, B, C, D, bias, dout)]


def report(lib, name, out, x, grads):
    torch.cuda.synchronize()
    print(name, "hashes", sha(out), sha(x), *[sha(g) for g in grads], flush=True)


def plain(lib, name, shape, itype, seed, tune_b=None, hs=False):
    u, delta, A, B, C, D, bias, dout = inputs(*shape, itype, seed)
    res = vmambair_amd.selective_scan_fwd(u, delta, A, B, C, D, bias, True, 1, want_hs=hs)
    shape_f = (lib.oss_scan_last_variant(0), lib.oss_scan_last_segments(0))
    grads = vmambair_amd.selective_scan_bwd(u, delta, A, B, C, D, bias, dout, res[1], True, 1, hs=res[2] if hs else None, tune=tune_b)
    print(name, "fwd", *shape_f, "bwd", lib.oss_scan_last_variant(1), lib.oss_scan_last_segments(1), lib.oss_scan_last_lane_states())
    report(lib, name, res[0], res[1], grads)


def fused(lib, name):
    K, N, Bsz, rows, R, L = 4, 16, 2, 24, 5, 700
    g = torch.Generator().manual_seed(5)
    x2 = torch.randn(Bsz, 2 * rows, L, generator=g).to(DEV)
    xdbl = torch.randn(Bsz, K, R + 2 * N, L, generator=g).to(DEV)
    W = (torch.randn(K * rows, R, generator=g) * 0.5).to(DEV)
    A_log = torch.log(0.5 + torch.rand(K * rows, N, generator=g)).to(DEV)
    dout = torch.randn(Bsz, 2 * rows, L, generator=g).to(DEV)
    kw = dict(rev_group_start=2, u_row_mod=2 * rows, a_log_form=True, dt_weight=W)
    out, x = vmambair_amd.selective_scan_fwd(x2, xdbl, A_log, xdbl[:, :, R:R + N], xdbl[:, :, R + N:], None, None, True, 1, **kw)
    shape_f = (lib.oss_scan_last_variant(0), lib.oss_scan_last_segments(0))
    into = torch.zeros_like(xdbl)
    grads = vmambair_amd.selective_scan_bwd(x2, xdbl, A_log, xdbl[:, :, R:R + N], xdbl[:, :, R + N:], None, None, dout, x, True, 1,
                                            dout_row_mod=2 * rows, dbc_into=into, tune=(13, None, None), **kw)
    print(name, "fwd", *shape_f, "bwd", lib.oss_scan_last_variant(1), lib.oss_scan_last_segments(1), lib.oss_scan_last_lane_states())
    report(lib, name, out, x, list(grads) + [into])


def main():
    lib = _capi.load()
    try:
        for segs in (3, 4):
            for bv in (1, 10, 11, 12, 13):
                lib.oss_scan_set_segments(segs, segs)
                lib.oss_scan_set_variant(-1, bv)
                plain(lib, f"f32_2x26x3000_seg{segs}_bv{bv}", (2, 26, 16, 2, 3000), torch.float32, 1)
        lib.oss_scan_set_segments(-1, -1)
        lib.oss_scan_set_variant(-1, -1)
        plain(lib, "f32_1x8x1500_dstate72", (1, 8, 72, 2, 1500), torch.float32, 2, tune_b=(11, 2, None))
        plain(lib, "bf16_2x24x2085_lane_states", (2, 24, 16, 2, 2085), torch.bfloat16, 3, hs=True)
        plain(lib, "bf16_2x24x2085_bf16_partials", (2, 24, 16, 2, 2085), torch.bfloat16, 3, tune_b=(10, 1, None, "bf16"))
        lib.oss_scan_set_segments(2, 2)
        fused(lib, "f32_fused_delta_700_r5_bv13")
        lib.oss_scan_set_segments(-1, -1)
        for shape in ((8, 384, 16, 4, 4096), (4, 192, 16, 4, 16384), (1, 384, 16, 4, 16384)):
            plain(lib, "bf16_heuristic_%dx%dx%d" % (shape[0], shape[1], shape[4]), shape, torch.bfloat16, 4)
            plain(lib, "bf16_heuristic_hs_%dx%dx%d" % (shape[0], shape[1], shape[4]), shape, torch.bfloat16, 4, hs=True)
    finally:
        lib.oss_scan_set_segments(-1, -1)
        lib.oss_scan_set_variant(-1, -1)


if __name__ == "__main__":
    main()
