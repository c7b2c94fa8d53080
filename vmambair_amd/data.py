"""Training batches from a pool of decoded image pairs that lives in device memory.

The reference feeds its step from CPU ``DataLoader`` workers: ``paired_random_crop`` (Deraining/basicsr/data/transforms.py:24-83),
``augment`` (:136-200, the SR trees) or ``random_augmentation`` (:223-275, Deraining), ``img2tensor(bgr2rgb=True, float32=True)``
of ``img.astype(np.float32) / 255.`` (utils/img_util.py:9-40), ``EnlargedSampler``'s ``perm[rank::world]`` per epoch.  A whole
training set fits an MI355X as decoded bytes (DIV2K sub-images with their x4 LQ: 23 GB of 288), so here it is uploaded once and a
batch costs two small launches (``oss_pairs.hip``): a counter-based draw -- a keyed permutation of the pairs per epoch, crop
origin and one of the 8 flips / transposes per sample, Philox4x32-10 -- and one gather that crops, flips, reorders the channels
and converts LQ and GT together.  No host work per batch, nothing is copied from the host, and both launches can be captured.

Both of the reference's augmentations are the uniform distribution over the dihedral group; ``code`` names its elements: bit 0
horizontal flip, bit 1 vertical flip, bit 2 transpose, applied in that order.

The Deraining tree's loader and loop do two more things, both behind the keyword ``dataset_gt_size`` (the option file's ``gt_size``,
``G``): ``padding()`` (utils/img_util.py:148-164) extends images smaller than ``G`` at the bottom and right by
``cv2.BORDER_REFLECT`` before the crop of side ``G`` -- read through the index map by the gather, never stored, scale 1 only as in
the reference -- and train.py:213-271 cuts one window of the stage's size, common to the batch, out of the augmented ``G`` patches;
crop and window are folded into one ordinary sample by the draw.  ``ProgressiveSchedule`` is the stage table of train.py:219-250 and
``pool.progressive_batches(schedule)`` feeds ``checkpoint.train_loop`` from it.  ``None`` (the default) is the SR trees' loader.

Not here: ``mixup`` / ``Mixing_Augment`` (``mixup: false`` in every option file), ``mean`` / ``std``
normalisation (unset everywhere), padding at a scale above 1 (the reference's own crop raises there), decoding, RealSR's
degradations.
"""
from __future__ import annotations

from typing import Iterator, Optional, Sequence, Tuple, Union

import numpy as np
import torch

_FORMAT = 1


def _default_rank_world(rank: Optional[int], world: Optional[int]) -> Tuple[int, int]:
    import torch.distributed as dist
    up = dist.is_available() and dist.is_initialized()
    rank = (dist.get_rank() if up else 0) if rank is None else int(rank)
    world = (dist.get_world_size() if up else 1) if world is None else int(world)
    if not (world >= 1 and 0 <= rank < world):
        raise ValueError(f"rank {rank} is not in [0, world = {world})")
    return rank, world


def _as_hwc(img, what: str) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(img)) if isinstance(img, np.ndarray) else img.detach().cpu().contiguous()
    if t.dtype != torch.uint8 or t.dim() not in (2, 3):
        raise ValueError(f"{what}: a uint8 (H, W, C) or (H, W) image is needed, got {t.dtype} {tuple(t.shape)}")
    return t.unsqueeze(2) if t.dim() == 2 else t


class ProgressiveSchedule:
    """The progressive-learning table of Deraining/basicsr/train.py:213-250: ``iters[j]`` iterations at ``mini_batch_sizes[j]``
    samples of side ``gt_sizes[j]``, cut out of loader patches of side ``gt_size``; ``batch_size`` is the loader's
    ``batch_size_per_gpu`` (kept for the record: the pool draws only the samples a stage uses)."""

    def __init__(self, iters: Sequence[int], mini_batch_sizes: Sequence[int], gt_sizes: Sequence[int], gt_size: int, batch_size: int):
        self.iters, self.mini_batch_sizes, self.gt_sizes = [int(v) for v in iters], [int(v) for v in mini_batch_sizes], [int(v) for v in gt_sizes]
        self.gt_size, self.batch_size = int(gt_size), int(batch_size)
        if not self.iters or not len(self.iters) == len(self.mini_batch_sizes) == len(self.gt_sizes):
            raise ValueError(f"iters, mini_batch_sizes and gt_sizes must be non-empty lists of one length, got {len(self.iters)}, "
                             f"{len(self.mini_batch_sizes)}, {len(self.gt_sizes)}")
        if min(self.iters) < 0 or min(self.mini_batch_sizes) < 1 or min(self.gt_sizes) < 1:
            raise ValueError("iters >= 0, mini_batch_sizes >= 1 and gt_sizes >= 1 are needed")
        if max(self.gt_sizes) > self.gt_size:
            raise ValueError(f"a stage's patch ({max(self.gt_sizes)}) is larger than the gt_size {self.gt_size} it is cut from")
        self.groups = np.cumsum(self.iters).tolist()

    @classmethod
    def from_options(cls, train_opt: dict) -> "ProgressiveSchedule":
        """from ``opt['datasets']['train']`` of a Deraining option file"""
        return cls(train_opt["iters"], train_opt["mini_batch_sizes"], train_opt["gt_sizes"], train_opt["gt_size"],
                   train_opt["batch_size_per_gpu"])

    def stage(self, current_iter: int) -> Tuple[int, int, int]:
        """-> ``(index, mini_batch, mini_gt)`` of the first stage ``j`` with ``current_iter <= sum(iters[:j + 1])``, else the last"""
        j = next((j for j, end in enumerate(self.groups) if current_iter <= end), len(self.groups) - 1)
        return j, self.mini_batch_sizes[j], self.gt_sizes[j]


class DevicePairPool:
    """Decoded (GT, LQ) image pairs in one flat ``uint8`` device buffer (HWC rows, 1 or 3 channels) with an ``int64`` table, one
    row per pair: ``gt_offset, lq_offset, lq_h, lq_w`` (bytes; GT is ``scale`` x LQ).  Build it once with ``from_arrays`` (or
    ``load`` what ``save`` wrote) and hand ``pool.batches(batch, gt_patch)`` to ``checkpoint.train_loop``.

    The draw is a pure function of ``(seed, rank, world, samples drawn so far)``: ``state_dict()`` is ``{'seed', 'samples_drawn'}``.
    ``checkpoint.save_training_state`` keeps its file format; store the pool's state beside its ``<iter>.state`` file, e.g.
    ``torch.save(pool.state_dict(), os.path.join(states_dir, f"{it}.pairs"))`` from ``train_loop``'s ``on_iter`` (or after it
    returns), and on resume ``pool.load_state_dict(torch.load(...))`` before ``pool.batches(...)`` is called again."""

    def __init__(self, data: torch.Tensor, table: torch.Tensor, scale: int, channels: int, swap_rb: bool = True, seed: int = 0,
                 rank: Optional[int] = None, world: Optional[int] = None):
        table_host = table.detach().cpu().to(torch.int64).contiguous()
        if data.dtype != torch.uint8 or data.dim() != 1 or table_host.dim() != 2 or table_host.shape[1] != 4 or not len(table_host):
            raise ValueError("data must be a flat uint8 tensor and table a non-empty (pairs, 4) integer tensor")
        if channels not in (1, 3) or scale < 1:
            raise ValueError(f"channels must be 1 or 3 and scale >= 1 (got {channels}, {scale})")
        if not 0 <= int(seed) < 1 << 63:
            raise ValueError("0 <= seed < 2^63")
        self.scale, self.channels, self.swap_rb, self.seed = int(scale), int(channels), bool(swap_rb), int(seed)
        self.rank, self.world = _default_rank_world(rank, world)
        self.table_host = table_host.numpy()
        gt_off, lq_off, h, w = (self.table_host[:, i] for i in range(4))
        if (h < 1).any() or (w < 1).any() or (gt_off < 0).any() or (lq_off < 0).any() or \
                (gt_off + h * w * scale * scale * channels > data.numel()).any() or (lq_off + h * w * channels > data.numel()).any():
            raise ValueError("the table names an image that does not lie inside the buffer")
        self.data = data.contiguous()
        dev = self.data.device
        self.table = table_host.to(dev)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self.clamped = torch.zeros(1, dtype=torch.int32, device=dev)
        self._samples = {}   # batch -> (batch, 4) int32 table the draw fills (kept: a captured graph replays into it)

    # ---- construction ---------------------------------------------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, gts: Sequence, lqs: Sequence, scale: int, device, swap_rb: bool = True, seed: int = 0,
                    rank: Optional[int] = None, world: Optional[int] = None) -> "DevicePairPool":
        """``gts`` / ``lqs``: lists of ``uint8`` HWC (or HW) arrays or tensors as the decoder returns them (BGR for cv2: keep
        ``swap_rb=True``, the reference's ``bgr2rgb``); sizes may differ from pair to pair.  Every GT must be exactly ``scale`` x its
        LQ (``paired_random_crop`` raises on anything else) with the same channel count, 1 or 3, for the whole pool."""
        if len(gts) != len(lqs) or not len(gts):
            raise ValueError(f"{len(gts)} GT images for {len(lqs)} LQ images")
        scale = int(scale)
        rows, parts, at, channels = [], [], 0, None
        for i, (g, l) in enumerate(zip(gts, lqs)):
            g, l = _as_hwc(g, f"gts[{i}]"), _as_hwc(l, f"lqs[{i}]")
            channels = g.shape[2] if channels is None else channels
            if g.shape[2] != l.shape[2] or g.shape[2] != channels or channels not in (1, 3):
                raise ValueError(f"pair {i}: GT has {g.shape[2]} channels, LQ {l.shape[2]}; the pool holds {channels} (1 or 3)")
            if g.shape[0] != l.shape[0] * scale or g.shape[1] != l.shape[1] * scale:
                raise ValueError(f"pair {i}: scale mismatches. GT {tuple(g.shape[:2])} is not {scale}x multiplication of LQ {tuple(l.shape[:2])}")
            rows.append((at, at + g.numel(), l.shape[0], l.shape[1]))
            parts += [g.reshape(-1), l.reshape(-1)]
            at += g.numel() + l.numel()
        data = torch.cat(parts).to(device)
        return cls(data, torch.tensor(rows, dtype=torch.int64), scale, channels, swap_rb, seed, rank, world)

    def save(self, path: str) -> None:
        """the packed pool (bytes, table, scale, channels, channel swap) as one ``torch.save`` file; the draw's state is not part of it"""
        torch.save({"format": _FORMAT, "data": self.data.cpu(), "table": torch.from_numpy(self.table_host.copy()), "scale": self.scale,
                    "channels": self.channels, "swap_rb": self.swap_rb}, path)

    @classmethod
    def load(cls, path: str, device, seed: int = 0, rank: Optional[int] = None, world: Optional[int] = None) -> "DevicePairPool":
        d = torch.load(path, map_location="cpu", weights_only=True)
        if d.get("format") != _FORMAT:
            raise ValueError(f"{path}: not a pair pool of format {_FORMAT}")
        return cls(d["data"].to(device), d["table"], d["scale"], d["channels"], d["swap_rb"], seed, rank, world)

    def __len__(self) -> int:
        return len(self.table_host)

    # ---- state ------------------------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """``{'seed', 'samples_drawn'}``: samples this rank has drawn (reads the device counter: one synchronisation)"""
        return {"seed": self.seed, "samples_drawn": int(self.counter.item())}

    def load_state_dict(self, state: dict) -> None:
        if not (0 <= int(state["seed"]) < 1 << 63 and int(state["samples_drawn"]) >= 0):
            raise ValueError(f"not a pool state: {state}")
        self.seed = int(state["seed"])
        self.counter.fill_(int(state["samples_drawn"]))

    # ---- checks (host) ----------------------------------------------------------------------------------------------------------
    def _lq_patch(self, gt_patch: Union[int, Tuple[int, int]]) -> Tuple[int, int]:
        gh, gw = (gt_patch, gt_patch) if isinstance(gt_patch, int) else (int(gt_patch[0]), int(gt_patch[1]))
        if gh < 1 or gw < 1 or gh % self.scale or gw % self.scale:
            raise ValueError(f"GT patch {gh} x {gw} must be a positive multiple of the scale {self.scale}")
        return gh // self.scale, gw // self.scale

    def _check_shape(self, batch: int, ph: int, pw: int) -> None:
        from .ops.pairs import pairs_ok
        if batch < 1 or not pairs_ok(self.channels, self.scale, ph, pw, batch):
            raise ValueError(f"batch {batch} of {ph} x {pw} LQ patches at scale {self.scale} is not supported (1 <= batch <= 65535, "
                             "at most 65535 tiles of 32 x 32 pixels per sample)")

    def _check_fits(self, batch: int, ph: int, pw: int, pad: int = 0) -> None:
        """a drawn patch must fit EVERY pair (extended to ``pad`` LQ pixels where ``dataset_gt_size`` pads)"""
        hmin, wmin = int(np.maximum(self.table_host[:, 2], pad).min()), int(np.maximum(self.table_host[:, 3], pad).min())
        if ph > hmin or pw > wmin:
            raise ValueError(f"LQ patch {ph} x {pw} is larger than the smallest image of the pool ({hmin} x {wmin}): the reference "
                             "pads such images; this pool rejects them unless dataset_gt_size is given")
        self._check_shape(batch, ph, pw)

    def _pad_lq(self, gt_side: int, what: str) -> Tuple[int, int]:
        """``gt_side`` (GT pixels: ``dataset_gt_size`` / ``pad_to``) -> ``(side in LQ pixels, pad)``: ``pad`` is that side when an
        image of the pool is smaller -- the reference's ``padding()``, defined at scale 1 only -- else 0"""
        g = int(gt_side)
        if g < 1 or g % self.scale:
            raise ValueError(f"{what} {g} must be a positive multiple of the scale {self.scale}")
        gl = g // self.scale
        if gl > 1 << 20:
            raise ValueError(f"{what} {g} is not supported (at most 2^20 LQ pixels)")
        if int(self.table_host[:, 2].min()) >= gl and int(self.table_host[:, 3].min()) >= gl:
            return gl, 0
        if self.scale != 1:
            raise ValueError(f"{what} {g}: the pool holds images smaller than that, and padding is defined at scale 1 only (the "
                             f"reference pads LQ and GT by the same pixel count, which its own paired_random_crop rejects at scale {self.scale})")
        return gl, gl

    def _window(self, dataset_gt_size: int, batch: int, ph: int) -> Tuple[int, int]:
        """the checks of a two-stage draw -> ``(full crop in LQ pixels, pad)``"""
        gl, pad = self._pad_lq(dataset_gt_size, "dataset_gt_size")
        if gl < ph:
            raise ValueError(f"dataset_gt_size {int(dataset_gt_size)} is smaller than the GT patch {ph * self.scale} cut out of it")
        self._check_fits(batch, ph, ph, pad)       # every image, extended where _pad_lq found one smaller, holds the crop
        return gl, pad

    def validate_table(self, table, ph: int, pw: int, pad: int = 0) -> np.ndarray:
        """-> the (n, 4) ``pair_index, top, left, code`` table as int32, or ``ValueError`` naming the first row that does not fit
        its image (extended to ``pad`` LQ pixels where it is smaller)"""
        t = np.asarray(table.cpu() if isinstance(table, torch.Tensor) else table)
        if t.ndim != 2 or t.shape[1] != 4 or not len(t) or t.dtype.kind not in "iu":
            raise ValueError("a sample table is a non-empty (n, 4) integer array: pair_index, top, left, code")
        t = t.astype(np.int64)
        for i, (pair, top, left, code) in enumerate(t.tolist()):
            if not 0 <= pair < len(self):
                raise ValueError(f"sample {i}: pair index {pair} is not in [0, {len(self)})")
            h, w = max(int(self.table_host[pair, 2]), pad), max(int(self.table_host[pair, 3]), pad)
            if not 0 <= top <= h - ph:
                raise ValueError(f"sample {i}: top {top} with {ph} rows does not fit the {h} rows of pair {pair}")
            if not 0 <= left <= w - pw:
                raise ValueError(f"sample {i}: left {left} with {pw} columns does not fit the {w} columns of pair {pair}")
            if not 0 <= code <= 7:
                raise ValueError(f"sample {i}: code {code} is not in [0, 7]")
            if code & 4 and ph != pw:
                raise ValueError(f"sample {i}: the transpose bit needs a square patch, not {ph} x {pw}")
        return t.astype(np.int32)

    # ---- batches ----------------------------------------------------------------------------------------------------------------
    def _outputs(self, batch: int, ph: int, pw: int):
        s, dev = self.scale, self.data.device
        return (torch.empty((batch, self.channels, ph, pw), dtype=torch.float32, device=dev),
                torch.empty((batch, self.channels, ph * s, pw * s), dtype=torch.float32, device=dev))

    def gather(self, table, gt_patch: Union[int, Tuple[int, int]], lq_out: Optional[torch.Tensor] = None,
               gt_out: Optional[torch.Tensor] = None, pad_to: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """explicit samples: ``table`` (n, 4) on the host -- ``pair_index, top, left, code`` in LQ pixels -- is checked against the
        pool HERE (``ValueError``) and only then uploaded.  -> ``(lq (n, C, h, w), gt (n, C, scale h, scale w))`` fp32 in [0, 1].
        ``pad_to`` (GT pixels, the option file's ``gt_size``): images smaller than that count as extended to it at the bottom and
        right by ``cv2.BORDER_REFLECT``, as the reference's ``padding()`` leaves them; rows are checked against the extended sizes."""
        from .ops.pairs import pairs_gather, pairs_gather_padded
        ph, pw = self._lq_patch(gt_patch)
        pad = None if pad_to is None else self._pad_lq(pad_to, "pad_to")[1]
        t = self.validate_table(table, ph, pw, pad or 0)
        self._check_shape(len(t), ph, pw)
        if lq_out is None or gt_out is None:
            lq_out, gt_out = self._outputs(len(t), ph, pw)
        samples = torch.from_numpy(t).to(self.data.device)
        if pad is None:
            pairs_gather(self.data, self.table, samples, lq_out, gt_out, self.clamped, self.scale, self.swap_rb)
        else:
            pairs_gather_padded(self.data, self.table, samples, lq_out, gt_out, self.clamped, self.scale, self.swap_rb, pad)
        return lq_out, gt_out

    def pair(self, i: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """the whole pair ``i`` as ``(lq (1, C, h, w), gt (1, C, H, W))`` floats, for validation"""
        if not 0 <= int(i) < len(self):
            raise ValueError(f"pair index {i} is not in [0, {len(self)})")
        h, w = int(self.table_host[i, 2]), int(self.table_host[i, 3])
        return self.gather([[int(i), 0, 0, 0]], (h * self.scale, w * self.scale))

    def next_into(self, lq_out: torch.Tensor, gt_out: torch.Tensor, use_hflip: bool = True, use_rot: bool = True,
                  dataset_gt_size: Optional[int] = None) -> None:
        """the next batch into caller-owned ``lq_out (batch, C, p, p)`` / ``gt_out (batch, C, scale p, scale p)``: draw + gather on
        the current stream, no host read-back.  Capturable into a graph once a call with this batch size has run eagerly (the
        sample table of a batch size is allocated on its first use); every replay then yields the following batch.
        ``dataset_gt_size`` (``G``, GT pixels): Deraining's rule -- pad to ``G`` (scale 1), crop ``G``, augment, then one window of
        side ``scale p`` common to the batch (``G == scale p``: no window) -- still two launches, which read only the window."""
        from .ops.pairs import HFLIP, ROT, pairs_draw, pairs_draw_window, pairs_gather, pairs_gather_padded
        batch, ph, pw = int(lq_out.shape[0]), int(lq_out.shape[2]), int(lq_out.shape[3])
        if ph != pw:
            raise ValueError(f"training patches are square, not {ph} x {pw}")
        if dataset_gt_size is None:
            self._check_fits(batch, ph, pw)
        else:
            full, pad = self._window(dataset_gt_size, batch, ph)
        samples = self._samples.get(batch)
        if samples is None:
            samples = self._samples[batch] = torch.empty((batch, 4), dtype=torch.int32, device=self.data.device)
        flags = (HFLIP if use_hflip else 0) | (ROT if use_rot else 0)
        if dataset_gt_size is None:
            pairs_draw(self.table, self.counter, batch, ph, self.seed, self.rank, self.world, flags, out=samples)
            pairs_gather(self.data, self.table, samples, lq_out, gt_out, self.clamped, self.scale, self.swap_rb)
        else:
            pairs_draw_window(self.table, self.counter, batch, ph, full, pad, self.seed, self.rank, self.world, flags, out=samples)
            pairs_gather_padded(self.data, self.table, samples, lq_out, gt_out, self.clamped, self.scale, self.swap_rb, pad)

    def batches(self, batch: int, gt_patch: int, iters: Optional[int] = None, use_hflip: bool = True, use_rot: bool = True,
                dataset_gt_size: Optional[int] = None) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        """-> an iterator of ``(lq, gt)`` for ``checkpoint.train_loop``: ``iters`` batches (``None``: without end) of ``batch`` square
        GT patches of side ``gt_patch``, each in fresh tensors.  The arguments are checked when this is CALLED (``ValueError`` for a
        patch larger than the smallest image); a later call may use another ``(batch, gt_patch)`` and continues the same sample
        sequence.  ``dataset_gt_size``: as in ``next_into``; Deraining's whole schedule is ``progressive_batches``."""
        ph, pw = self._lq_patch(int(gt_patch))
        if dataset_gt_size is None:
            self._check_fits(int(batch), ph, pw)
        else:
            self._window(dataset_gt_size, int(batch), ph)

        def gen():
            n = 0
            while iters is None or n < iters:
                lq, gt = self._outputs(int(batch), ph, pw)
                self.next_into(lq, gt, use_hflip, use_rot, dataset_gt_size)
                n += 1
                yield lq, gt
        return gen()

    def progressive_batches(self, schedule: ProgressiveSchedule, start_iter: int = 0, total_iters: Optional[int] = None,
                            use_hflip: bool = True, use_rot: bool = True) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        """-> an iterator of ``(lq, gt)`` for ``checkpoint.train_loop(step, batches, lr, start_iter, total_iters)``: the batch of
        iteration ``start_iter + 1, start_iter + 2, ...`` (as ``train_loop`` counts) has the ``(mini_batch, mini_gt)`` shape of
        ``schedule.stage(iteration)`` and is drawn by Deraining's rule from ``schedule.gt_size`` (``next_into``'s
        ``dataset_gt_size``); ends after iteration ``total_iters`` (``None``: without end).  Every stage is checked when this is
        CALLED.  The reference's loader cuts ``batch_size_per_gpu`` patches per iteration and train.py:259-262 throws all but
        ``mini_batch`` of them away; here only ``mini_batch`` samples are drawn.  The samples are i.i.d. either way; an epoch of the
        pool therefore lasts more iterations than one of the reference's loader.  ``state_dict`` stays ``{'seed', 'samples_drawn'}``:
        resume with ``load_state_dict`` and the ``start_iter`` the checkpoint was written at."""
        shapes = sorted({(mb, self._lq_patch(mg)[0]) for mb, mg in zip(schedule.mini_batch_sizes, schedule.gt_sizes)})
        for mb, ph in shapes:
            self._window(schedule.gt_size, mb, ph)

        def gen():
            it = int(start_iter)
            while total_iters is None or it < total_iters:
                it += 1
                _, mb, mg = schedule.stage(it)
                ph = mg // self.scale
                lq, gt = self._outputs(mb, ph, ph)
                self.next_into(lq, gt, use_hflip, use_rot, schedule.gt_size)
                yield lq, gt
        return gen()
