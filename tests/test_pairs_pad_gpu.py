"""The pair pool's Deraining forms on the GPU (oss_pairs.hip's ``oss_pairs_gather_padded`` / ``oss_pairs_draw_window`` through
vmambair_amd/data.py): the padded gather against the arrays the reference's own ``padding`` / crop / augmentation / ``img2tensor``
/ window slicing produce (tests/golden/g13_pairs_pad.npz) and against the NumPy twin of test_pairs_pad_host.py where a tile meets
the image's edge, the device-side defence, the two-stage draw against the host twin and against ``pairs_draw``, graph capture,
resumable state, and ``checkpoint.train_loop`` fed by ``pool.progressive_batches`` across stage boundaries.

Every comparison is EXACT (``np.array_equal``): bytes moved through index maps, one correctly rounded fp32 division, integer draws."""
import numpy as np
import pytest
import torch

from test_pairs_host import random_pairs, twin_gather
from test_pairs_pad_host import CASES, EDGE_G, EDGE_P, EDGE_SIZES, edge_table, golden_case, golden_table, twin_draw_window, twin_gather_padded
from vmambair_amd import DevicePairPool, ProgressiveSchedule, checkpoint, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLAGS = ops.pairs.HFLIP | ops.pairs.ROT


def host(t):
    return t if isinstance(t, np.ndarray) else t.cpu().numpy()


def assert_batch(got, want, what):
    for g, w, name in zip(got, want, ("lq", "gt")):
        g = host(g)
        assert g.shape == w.shape and g.dtype == np.float32, (what, name, g.shape, w.shape)
        assert np.array_equal(g, w), f"{what}: {name} differs in {int((g != w).sum())} of {g.size} elements"


# ---- the reference's arrays -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("swap_rb", [True, False], ids=["rgb", "bgr"])
@pytest.mark.parametrize("name", CASES)
def test_padded_gather_reproduces_the_golden_arrays_bit_exact(name, swap_rb):
    """all 8 modes of a G13 case in one ``gather(..., pad_to=G)``: what the reference pads, crops at G, augments, converts and
    windows is one folded sample read through the reflect map; with ``swap_rb`` off the planes come out reversed"""
    z, G, m, _, _, _, _ = golden_case(name)
    table, modes = golden_table(name)
    pool = DevicePairPool.from_arrays([z[f"{name}.gt"]], [z[f"{name}.lq"]], 1, DEV, swap_rb=swap_rb)
    lq, gt = (host(t) for t in pool.gather(table, m, pad_to=G))
    order = slice(None) if swap_rb else slice(None, None, -1)
    for code, mode in enumerate(modes):
        assert np.array_equal(lq[code], z[f"{name}.modes.lq"][mode].numpy()[order]), (code, mode)
        assert np.array_equal(gt[code], z[f"{name}.modes.gt"][mode].numpy()[order]), (code, mode)
    assert int(pool.clamped.item()) == 0


# ---- geometry -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
def test_padded_gather_edge_geometry_equals_the_cpu_twin(channels):
    """patches of side 40 (two tiles across) from 33 x 70, 5 x 7 and 40 x 41 images extended to 96: the image's last column on the
    first, a middle and the last column of a tile, tiles wholly inside, astride and wholly beyond the edge in x and in y, several
    reflection periods, every byte alignment of a row's first pixel, all 8 codes; then the whole 96 x 96 extension, three tiles
    across"""
    gts, lqs = random_pairs(EDGE_SIZES, 1, channels, seed=13)
    table = edge_table()
    if channels == 3:
        assert {(row[2] * 3) % 4 for row in table} == {0, 1, 2, 3}
    assert {(EDGE_SIZES[0][1] - 1 - row[2]) % 32 for row in table if row[0] == 0 and row[2] < EDGE_SIZES[0][1]} >= {0, 15, 31}
    assert {row[3] for row in table} == set(range(8))
    pool = DevicePairPool.from_arrays(gts, lqs, 1, DEV)
    assert_batch(pool.gather(table, EDGE_P, pad_to=EDGE_G), twin_gather_padded(gts, lqs, table, EDGE_P, EDGE_P, EDGE_G), "patch 40")
    assert_batch(pool.gather(table[3:4], EDGE_P, pad_to=EDGE_G), twin_gather_padded(gts, lqs, table[3:4], EDGE_P, EDGE_P, EDGE_G), "batch 1")
    whole = [[i, 0, 0, (3 * i + 1) % 8] for i in range(len(EDGE_SIZES))]
    assert_batch(pool.gather(whole, EDGE_G, pad_to=EDGE_G), twin_gather_padded(gts, lqs, whole, EDGE_G, EDGE_G, EDGE_G), "whole extension")
    rect = [[0, 50, 3, 1], [1, 0, 60, 2], [2, 7, 9, 3]]      # rectangular, codes without the transpose bit
    assert_batch(pool.gather(rect, (37, 33), pad_to=EDGE_G), twin_gather_padded(gts, lqs, rect, 37, 33, EDGE_G), "37 x 33")
    assert int(pool.clamped.item()) == 0


def test_pad_to_on_a_pool_that_needs_none_is_the_plain_gather():
    """every image holds ``pad_to``: nothing is extended (scale 4 is admitted then), and the padded kernel is the plain one"""
    sizes = [(37, 45), (33, 40)]
    gts, lqs = random_pairs(sizes, 4, 3, seed=3)
    pool = DevicePairPool.from_arrays(gts, lqs, 4, DEV)
    table = [[0, 4, 12, 5], [1, 0, 7, 2], [0, 1, 0, 7]]
    want = twin_gather(gts, lqs, table, 33, 33, 4)
    assert_batch(pool.gather(table, 132, pad_to=132), want, "pad_to 132")
    assert_batch(pool.gather(table, 132), want, "plain")
    assert int(pool.clamped.item()) == 0


def test_rows_beyond_the_padded_image_are_clamped_zero_filled_and_flagged():
    """the device-side defence below the host validation, on explicit tables: a 5 x 7 image extended to 16.  (i) a 4 x 4 patch at
    top 14 does not fit 16 rows: it is moved back to row 12 and flagged; (ii) a 20 x 20 patch does not fit at all: the 16 x 16 that
    exist are delivered, the rest is written as zeros, flagged"""
    gts, lqs = random_pairs([(5, 7)], 1, 3, seed=2)
    pool = DevicePairPool.from_arrays(gts, lqs, 1, DEV)

    def run(row, p):
        samples = torch.tensor([row], dtype=torch.int32, device=DEV)
        lq, gt = torch.full((1, 3, p, p), -1.0, device=DEV), torch.full((1, 3, p, p), -1.0, device=DEV)
        pool.clamped.zero_()
        torch.ops.vmambair.pairs_gather_padded(pool.data, pool.table, samples, lq, gt, pool.clamped, 1, True, 16)
        return (lq, gt), int(pool.clamped.item())

    got, flag = run([0, 12, 3, 0], 4)
    assert flag == 0
    assert_batch(got, twin_gather_padded(gts, lqs, [[0, 12, 3, 0]], 4, 4, 16), "fits")
    got, flag = run([0, 14, 3, 0], 4)
    assert flag == 1
    assert_batch(got, twin_gather_padded(gts, lqs, [[0, 12, 3, 0]], 4, 4, 16), "clamped to row 12")
    got, flag = run([0, 0, 0, 0], 20)
    assert flag == 1
    for g, w in zip(got, twin_gather_padded(gts, lqs, [[0, 0, 0, 0]], 16, 16, 16)):
        g = host(g)
        assert np.array_equal(g[:, :, :16, :16], w) and not g[:, :, 16:, :].any() and not g[:, :, :, 16:].any()
    pool.clamped.zero_()


# ---- the draw -------------------------------------------------------------------------------------------------------------------------
DRAW_SIZES = [(5 + 3 * (i % 11), 7 + 5 * (i % 13)) for i in range(37)]         # 5 x 7 .. 35 x 67


def draw_pool(seed=0, **kw):
    gts, lqs = random_pairs(DRAW_SIZES, 1, 3, seed=1)
    return gts, lqs, DevicePairPool.from_arrays(gts, lqs, 1, DEV, seed=seed, **kw)


@pytest.mark.parametrize("batch", [1, 8, 300])
@pytest.mark.parametrize("rank, world", [(0, 1), (2, 3)])
def test_draw_window_equals_the_host_twin(rank, world, batch):
    """the folded sample table bit for bit -- 300 samples are two passes of the workgroup and 8 epochs -- for G = 16 / m = 4 and
    G = 40 / m = 24 with padding, from a small counter and from one behind 2^38; the counter advances by ``batch``"""
    _, _, pool = draw_pool()
    seed = 0x1234567 + (1 << 45)
    for (G, m), c0 in (((16, 4), 5), ((40, 24), (1 << 38) + 11), ((16, 16), 9)):
        counter = torch.tensor([c0], dtype=torch.int64, device=DEV)
        got = torch.ops.vmambair.pairs_draw_window(pool.table, counter, batch, m, G, G, seed, rank, world, FLAGS)
        assert got.dtype == torch.int32 and np.array_equal(host(got), twin_draw_window(DRAW_SIZES, c0, batch, m, G, G, seed, rank, world))
        assert int(counter.item()) == c0 + batch
    if batch == 8:
        for hf, rot in ((False, True), (True, False), (False, False)):
            counter = torch.tensor([77], dtype=torch.int64, device=DEV)
            got = ops.pairs_draw_window(pool.table, counter, batch, 4, 16, 16, seed, rank, world, (ops.pairs.HFLIP if hf else 0) | (ops.pairs.ROT if rot else 0))
            assert np.array_equal(host(got), twin_draw_window(DRAW_SIZES, 77, batch, 4, 16, 16, seed, rank, world, hf, rot))


@pytest.mark.parametrize("batch", [1, 300])
def test_draw_window_without_window_or_padding_is_pairs_draw(batch):
    """``full_patch == patch`` on a pool that needs no padding (``pad_to`` 0, or a ``pad_to`` no image is below): the samples of
    ``pairs_draw``, device against device"""
    _, _, pool = draw_pool()
    for c0, pad in ((3, 0), ((1 << 38) + 7, 5)):
        a, b = (torch.tensor([c0], dtype=torch.int64, device=DEV) for _ in range(2))
        plain = torch.ops.vmambair.pairs_draw(pool.table, a, batch, 5, 42, 1, 2, FLAGS)
        window = torch.ops.vmambair.pairs_draw_window(pool.table, b, batch, 5, 5, pad, 42, 1, 2, FLAGS)
        assert torch.equal(plain, window) and int(a.item()) == int(b.item()) == c0 + batch


def twin_batches(gts, lqs, c, batch, m, G, seed, count, rank=0, world=1):
    return [twin_gather_padded(gts, lqs, twin_draw_window(DRAW_SIZES, c + k * batch, batch, m, G, G, seed, rank, world), m, m, G)
            for k in range(count)]


def test_captured_next_into_with_dataset_gt_size_walks_on():
    """``next_into(..., dataset_gt_size=G)`` inside ``torch.cuda.graph``: three replays are the batches an eager pool yields at
    counters c, c + B, c + 2 B, which are the twin's; the counter walks on"""
    gts, lqs, pool = draw_pool(seed=21, rank=1, world=2)
    _, _, eager = draw_pool(seed=21, rank=1, world=2)
    B, m, G = 3, 8, 40
    lq, gt = torch.zeros(B, 3, m, m, device=DEV), torch.zeros(B, 3, m, m, device=DEV)
    pool.next_into(lq, gt, dataset_gt_size=G)            # eager once: allocates the sample table of this batch size
    c = pool.state_dict()["samples_drawn"]
    assert c == B
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pool.next_into(lq, gt, dataset_gt_size=G)
    want = twin_batches(gts, lqs, c, B, m, G, 21, 3, rank=1, world=2)
    eager_batches = [(host(a), host(b)) for a, b in eager.batches(B, m, iters=4, dataset_gt_size=G)][1:]
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert_batch((lq, gt), want[k], f"replay {k} against the twin")
        assert_batch((lq, gt), eager_batches[k], f"replay {k} against the eager sequence")
    assert pool.state_dict()["samples_drawn"] == c + 3 * B and int(pool.clamped.item()) == 0


def test_state_dict_resumes_the_padded_sequence():
    """4 batches in one go == 2 batches, ``state_dict`` into a NEW pool, 2 more, the last at another stage's shape"""
    gts, lqs, pool = draw_pool(seed=9)
    G = 40
    straight = [(host(a), host(b)) for a, b in pool.batches(4, 8, iters=3, dataset_gt_size=G)]
    straight.append(tuple(host(t) for t in next(pool.batches(2, 24, dataset_gt_size=G))))
    assert pool.state_dict() == {"seed": 9, "samples_drawn": 14}
    _, _, first = draw_pool(seed=9)
    head = [(host(a), host(b)) for a, b in first.batches(4, 8, iters=2, dataset_gt_size=G)]
    state = first.state_dict()
    assert state == {"seed": 9, "samples_drawn": 8}
    _, _, second = draw_pool(seed=1)
    second.load_state_dict(state)
    tail = [tuple(host(t) for t in next(second.batches(4, 8, dataset_gt_size=G))), tuple(host(t) for t in next(second.batches(2, 24, dataset_gt_size=G)))]
    for (a, b), (c, d) in zip(straight, head + tail):
        assert np.array_equal(a, c) and np.array_equal(b, d)
    assert_batch(straight[2], twin_batches(gts, lqs, 8, 4, 8, G, 9, 1)[0], "third batch")
    assert_batch(straight[3], twin_batches(gts, lqs, 12, 2, 24, G, 9, 1)[0], "after the change of stage")


class RecordingStep:
    """what ``train_loop`` needs of a step: ``set_lr`` and a call that returns a loss"""

    def __init__(self):
        self.lrs, self.batches = [], []

    def set_lr(self, lr):
        self.lrs.append(lr)

    def __call__(self, lq, gt):
        self.batches.append((host(lq), host(gt)))
        return lq.mean()


def test_train_loop_fed_by_progressive_batches_across_stage_boundaries():
    """``checkpoint.train_loop`` over ``pool.progressive_batches`` with stages of 2, 2 and 1 iterations (then the last stage goes on):
    iteration by iteration the shapes are the schedule's and the contents the twin's at the walking counter; a loop resumed at
    ``start_iter`` 3 from the saved state yields the same tail"""
    gts, lqs, pool = draw_pool(seed=5)
    G = 40
    sched = ProgressiveSchedule([2, 2, 1], [3, 2, 1], [8, 24, 40], G, 4)
    step = RecordingStep()
    states = {}
    last = checkpoint.train_loop(step, pool.progressive_batches(sched), lambda it: 1e-4 * it, total_iters=7,
                                 on_iter=lambda it, loss: states.update({it: pool.state_dict()}))
    assert last == 7 and step.lrs == [1e-4 * it for it in range(1, 8)]
    want_shapes = [(3, 8), (3, 8), (2, 24), (2, 24), (1, 40), (1, 40), (1, 40)]
    assert [(a.shape[0], a.shape[2]) for a, _ in step.batches] == want_shapes
    c = 0
    for it, (mb, m) in enumerate(want_shapes, start=1):
        assert sched.stage(it)[1:] == (mb, m)
        assert_batch(step.batches[it - 1], twin_batches(gts, lqs, c, mb, m, G, 5, 1)[0], f"iteration {it}")
        c += mb
        assert states[it] == {"seed": 5, "samples_drawn": c}
    assert int(pool.clamped.item()) == 0
    _, _, resumed = draw_pool(seed=0)
    resumed.load_state_dict(states[3])
    again = RecordingStep()
    assert checkpoint.train_loop(again, resumed.progressive_batches(sched, start_iter=3, total_iters=7), lambda it: 1e-4, start_iter=3, total_iters=7) == 7
    assert len(again.batches) == 4
    for (a, b), (c_, d) in zip(again.batches, step.batches[3:]):
        assert np.array_equal(a, c_) and np.array_equal(b, d)
