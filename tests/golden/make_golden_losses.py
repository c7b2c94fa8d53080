#!/usr/bin/env python3
"""Generate tests/golden/g12_losses.npz by RUNNING THE REFERENCE's pixel-loss classes in the build container.

Needs /root/reference (read-only); never runs on the GPU box.  Nothing of the reference is copied: its two files are compiled where
they lie (``make_golden.load_by_path``; losses.py imports ``models.losses.loss_util``, which is loaded from its own file first) and
only the input tensors and the numbers the classes return are stored.  Re-run with:  python tests/golden/make_golden_losses.py

What is run, on float64 copies of the stored fp32 inputs, each with the autograd gradient w.r.t. ``pred``
  * ``L1Loss`` / ``MSELoss`` (Deraining/basicsr/models/losses/losses.py:26-82, losses/loss_util.py:25-95) x ``mean`` / ``sum`` x
    no weight / (N, C, H, W) weight / (N, 1, H, W) weight
  * ``CharbonnierLoss`` (:111-122), default eps and eps = 1e-2
  * ``PSNRLoss`` (:84-109), ``toY`` off and -- on the 3-channel sets -- on
  * one ``loss_weight`` != 1 case per class
Stored per input set ``<s>``: ``<s>.pred``, ``<s>.target`` (fp32; a fifth of pred's elements equal target's exactly), ``<s>.w4``,
``<s>.w1`` (the two weight shapes) and per cell ``<s>.<cell>.loss`` (float64 scalar), ``<s>.<cell>.grad`` (float64, pred's shape);
cell = ``l1|mse _ mean|sum _ none|w4|w1 [_lw<loss_weight>]``, ``charb[_eps<eps>][_lw<loss_weight>]``, ``psnr[_y][_lw<loss_weight>]``.
"""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, load_by_path  # noqa: E402

SETS = (("a", (2, 3, 5, 7)), ("b", (3, 1, 4, 8)), ("c", (1, 3, 3, 5)))


def load_ref_losses():
    for name in ("models", "models.losses"):
        sys.modules.setdefault(name, types.ModuleType(name))
    load_by_path("models.losses.loss_util", f"{REF}/Deraining/basicsr/models/losses/loss_util.py")
    return load_by_path("ref_losses", f"{REF}/Deraining/basicsr/models/losses/losses.py")


def run(module, pred, target, *weight):
    p = pred.double().requires_grad_(True)
    loss = module(p, target.double(), *[w.double() for w in weight])
    grad, = torch.autograd.grad(loss, p)
    return loss.detach(), grad


def main():
    ref = load_ref_losses()
    rng = np.random.RandomState(12)
    out = {}
    for s, shape in SETS:
        n, c, h, w = shape
        target = torch.from_numpy(rng.rand(*shape).astype(np.float32))
        pred = target + torch.from_numpy((0.1 * rng.randn(*shape)).astype(np.float32))
        tie = torch.from_numpy(rng.rand(*shape) < 0.2)
        pred = torch.where(tie, target, pred)                 # sign(0) = 0 must show
        w4 = torch.from_numpy(rng.rand(*shape).astype(np.float32))
        w1 = torch.from_numpy(rng.rand(n, 1, h, w).astype(np.float32))
        out.update({f"{s}.pred": pred, f"{s}.target": target, f"{s}.w4": w4, f"{s}.w1": w1})
        cells = {}
        for name, cls in (("l1", ref.L1Loss), ("mse", ref.MSELoss)):
            for red in ("mean", "sum"):
                for wname, wt in (("none", ()), ("w4", (w4,)), ("w1", (w1,))):
                    cells[f"{name}_{red}_{wname}"] = run(cls(reduction=red), pred, target, *wt)
        cells["l1_mean_w1_lw0.5"] = run(ref.L1Loss(loss_weight=0.5), pred, target, w1)
        cells["mse_sum_none_lw2.5"] = run(ref.MSELoss(loss_weight=2.5, reduction="sum"), pred, target)
        cells["charb"] = run(ref.CharbonnierLoss(), pred, target)
        cells["charb_eps0.01"] = run(ref.CharbonnierLoss(eps=1e-2), pred, target)
        cells["charb_lw3.0"] = run(ref.CharbonnierLoss(loss_weight=3.0), pred, target)   # accepted and unused by the reference
        cells["psnr"] = run(ref.PSNRLoss(), pred, target)
        cells["psnr_lw0.5"] = run(ref.PSNRLoss(loss_weight=0.5), pred, target)
        if c == 3:
            cells["psnr_y"] = run(ref.PSNRLoss(toY=True), pred, target)
            cells["psnr_y_lw0.5"] = run(ref.PSNRLoss(loss_weight=0.5, toY=True), pred, target)
        for cell, (loss, grad) in cells.items():
            out[f"{s}.{cell}.loss"], out[f"{s}.{cell}.grad"] = loss, grad
    path = os.path.join(OUT, "g12_losses.npz")
    np.savez_compressed(path, **{k: v.numpy() for k, v in out.items()})
    print(f"wrote g12_losses.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
