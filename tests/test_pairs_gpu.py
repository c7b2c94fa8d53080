"""The device-resident pair sampler on the GPU (oss_pairs.hip through vmambair_amd/data.py): the gather against the arrays the
reference's own crop / augmentation / ``img2tensor`` produce (tests/golden/g11_pairs.npz) and against the NumPy restatement of
test_pairs_host.py at the shapes where tiling can go wrong, the draw against the CPU twin, byte offsets past 4 GiB, graph capture,
resumable state, and ``train_loop`` fed by ``pool.batches``.

Every comparison is EXACT (``np.array_equal``): the kernels move bytes, divide once (a correctly rounded fp32 division on both
sides) and evaluate integer arithmetic; there is nothing to round differently."""
import numpy as np
import pytest
import torch

from test_pairs_host import CASES, golden_case, random_pairs, twin_draw, twin_gather
from vmambair_amd import DevicePairPool, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODE_TO_CODE = {0: 0, 1: 2, 2: 5, 3: 4, 4: 3, 5: 1, 6: 6, 7: 7}   # data_augmentation's modes (test_pairs_host.py derives the map)


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
def test_gather_reproduces_the_golden_arrays_bit_exact(name, swap_rb):
    """all 8 codes of both G11 cases in one call each: ``augment``'s triples and ``data_augmentation``'s modes, bit for bit; with
    ``swap_rb`` off the channels come out in file order, i.e. the reference's planes reversed"""
    z, scale, patch, top, left = golden_case(name)
    pool = DevicePairPool.from_arrays([z[f"{name}.gt"]], [z[f"{name}.lq"]], scale, DEV, swap_rb=swap_rb)
    lq, gt = pool.gather([[0, top, left, code] for code in range(8)], patch * scale)
    lq, gt = host(lq), host(gt)
    order = slice(None) if swap_rb else slice(None, None, -1)
    for code in range(8):
        h, v, t = code & 1, (code >> 1) & 1, code >> 2
        assert np.array_equal(lq[code], z[f"{name}.aug{h}{v}{t}.lq"].numpy()[order]), code
        assert np.array_equal(gt[code], z[f"{name}.aug{h}{v}{t}.gt"].numpy()[order]), code
    for mode, code in MODE_TO_CODE.items():
        assert np.array_equal(lq[code], z[f"{name}.mode{mode}.lq"].numpy()[order]), mode
        assert np.array_equal(gt[code], z[f"{name}.mode{mode}.gt"].numpy()[order]), mode
    assert int(pool.clamped.item()) == 0


@pytest.mark.parametrize("channels", [1, 3])
def test_all_byte_values_convert_bit_exact(channels):
    """float(v) / 255.0f correctly rounded, for every byte value, in every channel"""
    img = ((np.arange(256).reshape(16, 16, 1) + 85 * np.arange(channels)) % 256).astype(np.uint8)
    pool = DevicePairPool.from_arrays([img], [img[::-1].copy()], 1, DEV, swap_rb=False)
    lq, gt = pool.pair(0)
    want = (img.astype(np.float32) / np.float32(255)).transpose(2, 0, 1)[None]
    for c in range(channels):
        assert set(img[..., c].reshape(-1).tolist()) == set(range(256))
    assert np.array_equal(host(gt), want) and np.array_equal(host(lq), want[:, :, ::-1])


# ---- geometry -----------------------------------------------------------------------------------------------------------------------
def edge_case(p, scale, channels):
    """three pairs of different sizes with odd widths (the third exactly one patch), 9 samples over all 8 codes whose ``left``
    values put the first byte of a row at every alignment"""
    sizes = [(p + 2, (p + 3) | 1), (p + 6, (p + 8) | 1), (p, p)]
    gts, lqs = random_pairs(sizes, scale, channels, seed=p)
    table = [[i % 3, (5 * i) % (sizes[i % 3][0] - p + 1), (3 * (i + 1)) % (sizes[i % 3][1] - p + 1), i % 8] for i in range(9)]
    return sizes, gts, lqs, table


@pytest.mark.parametrize("p, scale, channels", [(1, 4, 3), (5, 4, 3), (33, 4, 3), (64, 4, 3), (31, 1, 3), (5, 4, 1), (33, 4, 1), (31, 1, 1)],
                         ids=lambda v: str(v))
def test_gather_edge_geometry_equals_the_cpu_twin(p, scale, channels):
    """LQ patch sides 1, 5, 33, 64 (x4) and 31 (x1): below one tile, one tile plus one pixel, whole tiles; GT sides 4 .. 256"""
    sizes, gts, lqs, table = edge_case(p, scale, channels)
    if channels == 3:
        assert {(row[2] * 3) % 4 for row in table} >= {1, 2, 3} and all(w % 2 for _, w in sizes[:2])
    pool = DevicePairPool.from_arrays(gts, lqs, scale, DEV)
    assert_batch(pool.gather(table, p * scale), twin_gather(gts, lqs, table, p, p, scale), f"batch 9, patch {p}")
    assert_batch(pool.gather(table[6:7], p * scale), twin_gather(gts, lqs, table[6:7], p, p, scale), f"batch 1, patch {p}")
    assert int(pool.clamped.item()) == 0


@pytest.mark.parametrize("channels", [1, 3])
def test_whole_rectangular_pairs_equal_the_cpu_twin(channels):
    """``pair(i)``: rectangular output for validation, and rectangular crops with the two flips"""
    sizes = [(37, 45), (5, 71), (66, 3)]
    gts, lqs = random_pairs(sizes, 2, channels, seed=3)
    pool = DevicePairPool.from_arrays(gts, lqs, 2, DEV)
    for i, (h, w) in enumerate(sizes):
        assert_batch(pool.pair(i), twin_gather(gts, lqs, [[i, 0, 0, 0]], h, w, 2), f"pair {i}")
    table = [[0, 3, 5, 0], [0, 0, 1, 1], [0, 4, 2, 2], [0, 1, 3, 3]]
    assert_batch(pool.gather(table, (2 * 33, 2 * 40)), twin_gather(gts, lqs, table, 33, 40, 2), "33 x 40 crops")
    assert int(pool.clamped.item()) == 0


def test_offsets_past_4_gib():
    """a pool whose only pair lies behind byte 2^32 of the buffer (which is not filled: milliseconds)"""
    gts, lqs = random_pairs([(6, 7)], 2, 3, seed=8)
    buf = torch.empty(2 ** 32 + 8192, dtype=torch.uint8, device=DEV)
    at = 2 ** 32 + 5
    g, l = torch.from_numpy(gts[0]).reshape(-1), torch.from_numpy(lqs[0]).reshape(-1)
    buf[at:at + g.numel()] = g.to(DEV)
    buf[at + g.numel() + 3:at + g.numel() + 3 + l.numel()] = l.to(DEV)
    pool = DevicePairPool(buf, torch.tensor([[at, at + g.numel() + 3, 6, 7]]), 2, 3)
    assert_batch(pool.pair(0), twin_gather(gts, lqs, [[0, 0, 0, 0]], 6, 7, 2), "whole pair")
    table = [[0, 2, 3, 5], [0, 0, 1, 6]]
    assert_batch(pool.gather(table, 8), twin_gather(gts, lqs, table, 4, 4, 2), "crops")
    assert int(pool.clamped.item()) == 0


# ---- the draw -------------------------------------------------------------------------------------------------------------------------
def draw_pool(seed=0, **kw):
    sizes = [(8 + i % 5, 9 + i % 7) for i in range(37)]
    gts, lqs = random_pairs(sizes, 2, 3, seed=1)
    return sizes, gts, lqs, DevicePairPool.from_arrays(gts, lqs, 2, DEV, seed=seed, **kw)


@pytest.mark.parametrize("batch", [1, 8, 1500])
@pytest.mark.parametrize("rank, world", [(0, 1), (1, 4)])
def test_draw_equals_the_cpu_twin(rank, world, batch):
    """the sample table bit for bit -- 1500 samples are six passes of the workgroup and 40 epochs of the 37 pairs -- from a small
    counter and from one behind 2^38 (64-bit positions, epochs past 2^32); the counter advances by ``batch``"""
    sizes, _, _, pool = draw_pool()
    seed = 0x1234567 + (1 << 45)
    for c0 in (5, (1 << 38) + 11):
        counter = torch.tensor([c0], dtype=torch.int64, device=DEV)
        got = torch.ops.vmambair.pairs_draw(pool.table, counter, batch, 4, seed, rank, world, ops.pairs.HFLIP | ops.pairs.ROT)
        assert got.dtype == torch.int32 and np.array_equal(host(got), twin_draw(sizes, c0, batch, 4, seed, rank, world))
        assert int(counter.item()) == c0 + batch
    if batch == 8:
        for hf, rot in ((False, True), (True, False), (False, False)):
            counter = torch.tensor([77], dtype=torch.int64, device=DEV)
            got = ops.pairs_draw(pool.table, counter, batch, 4, seed, rank, world, (ops.pairs.HFLIP if hf else 0) | (ops.pairs.ROT if rot else 0))
            assert np.array_equal(host(got), twin_draw(sizes, 77, batch, 4, seed, rank, world, hf, rot))


def twin_batches(sizes, gts, lqs, c, batch, p, seed, count, scale=2, rank=0, world=1):
    return [twin_gather(gts, lqs, twin_draw(sizes, c + k * batch, batch, p, seed, rank, world), p, p, scale) for k in range(count)]


def test_captured_next_into_walks_on_with_every_replay():
    """``next_into`` inside ``torch.cuda.graph``: three replays are the twin's batches at counters c, c + B, c + 2 B"""
    sizes, gts, lqs, pool = draw_pool(seed=21, rank=1, world=2)
    B, p = 3, 4
    lq = torch.zeros(B, 3, p, p, device=DEV)
    gt = torch.zeros(B, 3, 2 * p, 2 * p, device=DEV)
    pool.next_into(lq, gt)                              # eager once: allocates the sample table of this batch size
    c = pool.state_dict()["samples_drawn"]
    assert c == B
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pool.next_into(lq, gt)
    want = twin_batches(sizes, gts, lqs, c, B, p, 21, 3, rank=1, world=2)
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert_batch((lq, gt), want[k], f"replay {k}")
    assert pool.state_dict()["samples_drawn"] == c + 3 * B and int(pool.clamped.item()) == 0


def test_state_dict_resumes_the_sequence():
    """5 batches in one go == 2 batches, ``state_dict`` into a NEW pool, 3 more; and the patch may change between ``batches`` calls"""
    sizes, gts, lqs, pool = draw_pool(seed=9)
    straight = [(host(a), host(b)) for a, b in pool.batches(4, 8, iters=5)]
    assert pool.state_dict() == {"seed": 9, "samples_drawn": 20}
    _, _, _, first = draw_pool(seed=9)
    head = [(host(a), host(b)) for a, b in first.batches(4, 8, iters=2)]
    state = first.state_dict()
    assert state == {"seed": 9, "samples_drawn": 8}
    _, _, _, second = draw_pool(seed=1)
    second.load_state_dict(state)
    tail = [(host(a), host(b)) for a, b in second.batches(4, 8, iters=3)]
    for (a, b), (c, d) in zip(straight, head + tail):
        assert np.array_equal(a, c) and np.array_equal(b, d)
    assert_batch(straight[4], twin_batches(sizes, gts, lqs, 16, 4, 4, 9, 1)[0], "fifth batch")
    lq, gt = next(second.batches(2, 12))                  # progressive schedule: another (batch, patch), same sequence
    assert_batch((lq, gt), twin_batches(sizes, gts, lqs, 20, 2, 6, 9, 1)[0], "after the change of patch")


def test_train_loop_fed_by_the_pool():
    """``train_loop`` over a ``GraphedTrainStep`` for 3 iterations, fed by ``pool.batches(2, 32)``: the losses are bit-identical to
    those of the same step (same initial weights) fed tensors built from the twin"""
    from vmambair_amd import checkpoint
    from vmambair_amd.archs import MambaSISR6
    from vmambair_amd.train_graph import GraphedTrainStep
    sizes = [(10, 13), (12, 9), (8, 8), (9, 15)]
    gts, lqs = random_pairs(sizes, 4, 3, seed=5)
    pool = DevicePairPool.from_arrays(gts, lqs, 4, DEV, seed=3)

    def run(batches):
        torch.manual_seed(0)
        net = MambaSISR6(dim=8, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1).to(DEV)
        step = GraphedTrainStep(net, autocast_dtype=None, warmup=1)
        losses = []
        last = checkpoint.train_loop(step, batches, lambda it: 2e-4, total_iters=3, on_iter=lambda it, loss: losses.append(float(loss)))
        assert last == 3
        return losses

    from_pool = run(pool.batches(2, 32))
    twin = [(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)) for a, b in twin_batches(sizes, gts, lqs, 0, 2, 8, 3, 3, scale=4)]
    from_twin = run(twin)
    print("losses", from_pool, from_twin)
    assert len(from_pool) == 3 and all(np.isfinite(from_pool)) and from_pool == from_twin
