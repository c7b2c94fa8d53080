"""Training batches cut on the device: ``torch.ops.vmambair.pairs_draw`` and ``pairs_gather`` (and their Deraining forms
``pairs_draw_window`` / ``pairs_gather_padded``: ``padding()``, utils/img_util.py:148-164, and the progressive window of
train.py:213-271) on ``oss_pairs.hip`` -- the reference's ``paired_random_crop`` / ``augment`` / ``random_augmentation`` (Deraining/basicsr/data/transforms.py:24-83, :136-200,
:223-275), ``img2tensor`` of ``img / 255.`` (utils/img_util.py:9-40) and ``EnlargedSampler`` on a pool of decoded pairs that lives
in device memory.  ``vmambair_amd.data.DevicePairPool`` is the public face; layouts and the draw as in include/vmambair_oss.h."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _capi
from ._common import _LIB, _check

HFLIP, ROT = _capi.PAIRS_HFLIP, _capi.PAIRS_ROT


def pairs_ok(channels: int, scale: int, patch_h: int, patch_w: int, batch: int) -> bool:
    """whether ``pairs_gather`` takes this shape (a host query of the library)"""
    return bool(_capi.load().oss_pairs_ok(int(channels), int(scale), int(patch_h), int(patch_w), int(batch)))


def _dev(t: torch.Tensor, dtype, what: str) -> None:
    _check(t.is_cuda and t.dtype == dtype and t.is_contiguous(), f"{what} must be a contiguous {dtype} CUDA/HIP tensor")


def _draw_args(what: str, table: torch.Tensor, counter: torch.Tensor, batch: int, patch: int, seed: int, rank: int, world: int,
               out: Optional[torch.Tensor]) -> torch.Tensor:
    _dev(table, torch.int64, f"{what}: table")
    _dev(counter, torch.int64, f"{what}: counter")
    _check(table.dim() == 2 and table.shape[1] == 4 and table.shape[0] >= 1 and counter.numel() == 1,
           f"{what}: table must be (pairs, 4) and counter one element")
    _check(batch >= 1 and patch >= 1 and world >= 1 and 0 <= rank < world, f"{what}: batch, patch >= 1 and 0 <= rank < world")
    if out is None:
        out = torch.empty((batch, 4), dtype=torch.int32, device=table.device)
    _dev(out, torch.int32, f"{what}: out")
    _check(tuple(out.shape) == (batch, 4) and out.device == table.device == counter.device, f"{what}: out must be (batch, 4) on the table's device")
    _check(0 <= int(seed) < 1 << 63, f"{what}: 0 <= seed < 2^63")
    return out


def pairs_draw(table: torch.Tensor, counter: torch.Tensor, batch: int, patch: int, seed: int, rank: int, world: int, flags: int,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """table (pairs, 4) int64, counter (1,) int64 -> (batch, 4) int32 on the device: pair_index, top, left, code of the samples at
    per-rank positions counter .. counter + batch - 1; the counter is advanced by ``batch`` in the same launch.  Runs on the current
    stream, reads nothing back, allocates nothing when ``out`` is given: capturable."""
    out = _draw_args("pairs_draw", table, counter, batch, patch, seed, rank, world, out)
    with torch.cuda.device(table.device):
        _capi.check(_capi.load().oss_pairs_draw(table.data_ptr(), table.shape[0], counter.data_ptr(), out.data_ptr(), int(batch),
                                                int(patch), int(seed), int(rank), int(world),
                                                int(flags), torch.cuda.current_stream().cuda_stream), "oss_pairs_draw")
    return out


def pairs_draw_window(table: torch.Tensor, counter: torch.Tensor, batch: int, patch: int, full_patch: int, pad_to: int, seed: int,
                      rank: int, world: int, flags: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``pairs_draw`` in two stages (Deraining's loader and training loop): a crop of side ``full_patch`` from every image extended to
    ``max(side, pad_to)``, then ONE window of side ``patch`` per call inside the augmented crops, stored as ordinary samples of side
    ``patch`` (LQ pixels throughout).  ``full_patch == patch`` and ``pad_to == 0``: the samples of ``pairs_draw``."""
    out = _draw_args("pairs_draw_window", table, counter, batch, patch, seed, rank, world, out)
    _check(patch <= full_patch <= 1 << 20 and 0 <= pad_to <= 1 << 20, "pairs_draw_window: patch <= full_patch <= 2^20 and 0 <= pad_to <= 2^20")
    with torch.cuda.device(table.device):
        _capi.check(_capi.load().oss_pairs_draw_window(table.data_ptr(), table.shape[0], counter.data_ptr(), out.data_ptr(), int(batch),
                                                       int(patch), int(full_patch), int(pad_to), int(seed), int(rank), int(world),
                                                       int(flags), torch.cuda.current_stream().cuda_stream), "oss_pairs_draw_window")
    return out


def _gather_args(what: str, pool, table, samples, lq, gt, clamped, scale: int):
    _dev(pool, torch.uint8, f"{what}: pool")
    _dev(table, torch.int64, f"{what}: table")
    _dev(samples, torch.int32, f"{what}: samples")
    _dev(lq, torch.float32, f"{what}: lq")
    _dev(gt, torch.float32, f"{what}: gt")
    _dev(clamped, torch.int32, f"{what}: clamped")
    _check(lq.dim() == 4 and gt.dim() == 4 and samples.dim() == 2 and table.dim() == 2 and table.shape[1] == 4 and clamped.numel() == 1,
           f"{what}: lq, gt (batch, C, H, W), samples (batch, 4), table (pairs, 4), clamped one element")
    B, C, h, w = lq.shape
    _check(tuple(samples.shape) == (B, 4) and tuple(gt.shape) == (B, C, h * scale, w * scale),
           f"{what}: samples must be ({B}, 4) and gt {(B, C, h * scale, w * scale)} for lq {tuple(lq.shape)} at scale {scale}")
    _check(len({t.device for t in (pool, table, samples, lq, gt, clamped)}) == 1, f"{what}: all tensors on one device")
    _check(pool.numel() >= 1 and table.shape[0] >= 1 and pairs_ok(C, scale, h, w, B),
           f"{what}: batch {B}, {C} channels, patch {h} x {w}, scale {scale} is not supported (1 or 3 channels, "
           "batch <= 65535, at most 65535 tiles of 32 x 32 pixels per sample)")
    return B, C, h, w


def pairs_gather(pool: torch.Tensor, table: torch.Tensor, samples: torch.Tensor, lq: torch.Tensor, gt: torch.Tensor,
                 clamped: torch.Tensor, scale: int, swap_rb: bool) -> None:
    """pool flat uint8, table (pairs, 4) int64, samples (batch, 4) int32 -> fills lq (batch, C, h, w) and gt (batch, C, scale h,
    scale w), fp32 contiguous, in one launch on the current stream; ``clamped`` (1,) int32 is set to 1 by the kernel when a
    rectangle did not fit its image (the callers in ``vmambair_amd.data`` validate on the host, so it stays 0)."""
    B, C, h, w = _gather_args("pairs_gather", pool, table, samples, lq, gt, clamped, scale)
    with torch.cuda.device(pool.device):
        _capi.check(_capi.load().oss_pairs_gather(pool.data_ptr(), pool.numel(), table.data_ptr(), table.shape[0], samples.data_ptr(),
                                                  lq.data_ptr(), gt.data_ptr(), clamped.data_ptr(), B, C, h, w, int(scale),
                                                  int(bool(swap_rb)), torch.cuda.current_stream().cuda_stream), "oss_pairs_gather")


def pairs_gather_padded(pool: torch.Tensor, table: torch.Tensor, samples: torch.Tensor, lq: torch.Tensor, gt: torch.Tensor,
                        clamped: torch.Tensor, scale: int, swap_rb: bool, pad_to: int) -> None:
    """``pairs_gather`` on images extended at the bottom and right to ``max(side, pad_to)`` by ``cv2.BORDER_REFLECT`` (index
    ``i >= n`` reads ``r = i mod 2n; r if r < n else 2n - 1 - r``), the reference's ``padding()``; nothing is stored.  ``pad_to > 0``
    needs ``scale == 1``: the reference pads LQ and GT by the same pixel count."""
    B, C, h, w = _gather_args("pairs_gather_padded", pool, table, samples, lq, gt, clamped, scale)
    _check(0 <= pad_to <= 1 << 20 and (pad_to == 0 or scale == 1), "pairs_gather_padded: 0 <= pad_to <= 2^20, and pad_to > 0 only at scale 1")
    with torch.cuda.device(pool.device):
        _capi.check(_capi.load().oss_pairs_gather_padded(pool.data_ptr(), pool.numel(), table.data_ptr(), table.shape[0],
                                                         samples.data_ptr(), lq.data_ptr(), gt.data_ptr(), clamped.data_ptr(), B, C, h,
                                                         w, int(scale), int(bool(swap_rb)), int(pad_to),
                                                         torch.cuda.current_stream().cuda_stream), "oss_pairs_gather_padded")


def _pairs_draw_op(table, counter, batch, patch, seed, rank, world, flags):
    return pairs_draw(table, counter, batch, patch, seed, rank, world, flags)


def _pairs_draw_window_op(table, counter, batch, patch, full_patch, pad_to, seed, rank, world, flags):
    return pairs_draw_window(table, counter, batch, patch, full_patch, pad_to, seed, rank, world, flags)


_LIB.define("pairs_draw(Tensor table, Tensor(a!) counter, int batch, int patch, int seed, int rank, int world, int flags) -> Tensor")
_LIB.impl("pairs_draw", _pairs_draw_op, "CUDA")
_LIB.define("pairs_gather(Tensor pool, Tensor table, Tensor samples, Tensor(a!) lq, Tensor(b!) gt, Tensor(c!) clamped, int scale, "
            "bool swap_rb) -> ()")
_LIB.impl("pairs_gather", pairs_gather, "CUDA")
_LIB.define("pairs_draw_window(Tensor table, Tensor(a!) counter, int batch, int patch, int full_patch, int pad_to, int seed, int rank, "
            "int world, int flags) -> Tensor")
_LIB.impl("pairs_draw_window", _pairs_draw_window_op, "CUDA")
_LIB.define("pairs_gather_padded(Tensor pool, Tensor table, Tensor samples, Tensor(a!) lq, Tensor(b!) gt, Tensor(c!) clamped, int scale, "
            "bool swap_rb, int pad_to) -> ()")
_LIB.impl("pairs_gather_padded", pairs_gather_padded, "CUDA")
