"""Host side of the device-resident pair sampler (vmambair_amd/data.py on oss_pairs.hip): the generator's known answers through the
library's host entry point, a NumPy restatement of the draw and of the gather -- the twin the GPU tests (test_pairs_gpu.py) compare
the kernels with bit for bit -- checked for the properties the sampler promises, the reference's fixture G11
(tests/golden/make_golden_pairs.py) against the twin, and the host validation of ``DevicePairPool``.  No GPU needed."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from vmambair_amd import DevicePairPool, _capi

M32 = 0xFFFFFFFF
TAG_PERM, TAG_CROP = 0x7065726D, 0x63726F70   # include/vmambair_oss.h: oss_pairs_draw


# ---- the twin -----------------------------------------------------------------------------------------------------------------
def philox4x32_10(ctr, key):
    """Salmon et al., "Parallel random numbers: as easy as 1, 2, 3" (SC'11), Philox4x32 with 10 rounds, on Python integers"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def twin_perm(x, n, epoch, key):
    """the keyed bijection of [0, n): 4 Feistel rounds over 2 * half bits (4^half >= n), walked back into [0, n)"""
    half = 1
    while half < 16 and (1 << (2 * half)) < n:
        half += 1
    mask = (1 << half) - 1
    while True:
        l, r = x >> half, x & mask
        for rnd in range(4):
            f = philox4x32_10((r, rnd | (((epoch >> 32) << 8) & M32), epoch & M32, TAG_PERM), key)[0]
            l, r = r, l ^ (f & mask)
        x = (l << half) | r
        if x < n:
            return x


def twin_draw(sizes, c, batch, patch, seed, rank=0, world=1, use_hflip=True, use_rot=True):
    """sizes: (n, 2) LQ heights / widths -> (batch, 4) int32: pair_index, top, left, code of per-rank positions c .. c + batch - 1"""
    n, key = len(sizes), (seed & M32, seed >> 32)
    code_mask = (1 if use_hflip else 0) | (6 if use_rot else 0)
    out = np.zeros((batch, 4), dtype=np.int32)
    for b in range(batch):
        g = (c + b) * world + rank
        epoch = g // n
        pair = twin_perm(g - epoch * n, n, epoch, key)
        r = philox4x32_10((g & M32, g >> 32, TAG_CROP, 0), key)
        mh, mw = max(1, int(sizes[pair][0]) - patch + 1), max(1, int(sizes[pair][1]) - patch + 1)
        out[b] = (pair, (r[0] * mh) >> 32, (r[1] * mw) >> 32, (r[2] >> 29) & code_mask)
    return out


def twin_patch(img, top, left, ph, pw, code, swap_rb):
    """crop, hflip (bit 0), vflip (bit 1), transpose (bit 2) in that order, channel swap, / 255 in fp32, HWC -> CHW"""
    v = img[top:top + ph, left:left + pw]
    if code & 1:
        v = v[:, ::-1]
    if code & 2:
        v = v[::-1]
    if code & 4:
        v = v.transpose(1, 0, 2)
    if swap_rb and v.shape[2] == 3:
        v = v[..., ::-1]
    return np.ascontiguousarray((v.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))


def twin_gather(gts, lqs, table, ph, pw, scale, swap_rb=True):
    """-> (lq (n, C, ph, pw), gt (n, C, scale ph, scale pw)) float32 for the rows pair_index, top, left, code of ``table``"""
    lq = np.stack([twin_patch(lqs[p], t, l, ph, pw, c, swap_rb) for p, t, l, c in np.asarray(table).tolist()])
    gt = np.stack([twin_patch(gts[p], t * scale, l * scale, ph * scale, pw * scale, c, swap_rb) for p, t, l, c in np.asarray(table).tolist()])
    return lq, gt


def random_pairs(sizes, scale, channels=3, seed=0):
    rng = np.random.RandomState(seed)
    lqs = [rng.randint(0, 256, (h, w, channels)).astype(np.uint8) for h, w in sizes]
    gts = [rng.randint(0, 256, (h * scale, w * scale, channels)).astype(np.uint8) for h, w in sizes]
    return gts, lqs


# ---- the generator ------------------------------------------------------------------------------------------------------------
def lib_philox(ctr, key):
    c, k, o = (ctypes.c_uint32 * 4)(*ctr), (ctypes.c_uint32 * 2)(*key), (ctypes.c_uint32 * 4)()
    assert _capi.load().oss_pairs_philox(c, k, o) == 0
    return tuple(o)


KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
         ((M32,) * 4, (M32,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


def test_philox_known_answers():
    """the three known-answer vectors of Philox4x32-10 (Random123's kat_vectors), from the text the kernels are compiled from"""
    for ctr, key, want in KNOWN:
        assert lib_philox(ctr, key) == want
        assert philox4x32_10(ctr, key) == want
    rng = np.random.RandomState(1)
    for _ in range(50):
        w = [int(v) for v in rng.randint(0, 1 << 32, 6, dtype=np.uint64)]
        assert lib_philox(w[:4], w[4:]) == philox4x32_10(w[:4], w[4:])
    assert _capi.load().oss_pairs_philox(None, None, None) == _capi._K["OSS_ERR_NULL"]


# ---- the draw -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 4])
@pytest.mark.parametrize("n", [1, 2, 7, 64, 1000])
def test_twin_epoch_visits_every_pair_once(n, world):
    """over one epoch the union over the ranks is every pair exactly once, whatever the batch size; the next epoch is another order"""
    sizes, seed, batch = [(12, 20)] * n, 1234, 3
    assert n % batch
    per_rank = -(-2 * n // world)                       # enough positions for two epochs
    seen = {}
    for rank in range(world):
        rows, c = [], 0
        while c < per_rank:
            rows.append(twin_draw(sizes, c, batch, 4, seed, rank, world))
            c += batch
        for q, row in enumerate(np.concatenate(rows)):
            seen[q * world + rank] = int(row[0])
    first, second = [seen[g] for g in range(n)], [seen[g] for g in range(n, 2 * n)]
    assert sorted(first) == list(range(n)) and sorted(second) == list(range(n))
    if n >= 7:
        assert first != second


def test_twin_is_a_function_of_seed_and_counter():
    sizes = [(12, 20), (9, 33), (40, 8)] * 5
    a = twin_draw(sizes, 100, 16, 4, 99)
    assert np.array_equal(a, twin_draw(sizes, 100, 16, 4, 99))
    assert np.array_equal(a[4:], twin_draw(sizes, 104, 12, 4, 99))              # the batch boundary does not matter
    assert not np.array_equal(a, twin_draw(sizes, 100, 16, 4, 98))
    assert not np.array_equal(a[:, 1:], twin_draw(sizes, 100, 16, 4, 99 + (1 << 40))[:, 1:])   # the high key word counts


def _chi2(counts):
    e = sum(counts) / len(counts)
    return sum((c - e) ** 2 / e for c in counts)


def test_twin_crops_and_codes_are_in_range_and_uniform():
    """8192 draws from LQ 12 x 20 images at patch 4: top in [0, 8], left in [0, 16], code in [0, 7], each uniform: Pearson's
    statistic of k cells has mean k - 1 and variance 2 (k - 1); the limit is the mean plus 6 standard deviations.  The seed is
    fixed, so this is one deterministic evaluation, not a flaky one."""
    sizes = [(12, 20)] * 7
    t = twin_draw(sizes, 0, 8192, 4, 2024)
    assert t[:, 1].min() >= 0 and t[:, 1].max() <= 8 and t[:, 2].min() >= 0 and t[:, 2].max() <= 16
    for col, k in ((3, 8), (1, 9), (2, 17)):
        counts = np.bincount(t[:, col], minlength=k)
        assert len(counts) == k and counts.min() > 0
        assert _chi2(counts.tolist()) <= (k - 1) + 6 * math.sqrt(2 * (k - 1)), (col, counts)
    mixed = [(4, 4), (5, 30), (64, 7)]                   # top / left ranges follow each pair's own size, down to one position
    t = twin_draw(mixed, 0, 600, 4, 3)
    for pair, top, left, _ in t.tolist():
        assert 0 <= top <= mixed[pair][0] - 4 and 0 <= left <= mixed[pair][1] - 4


def test_twin_masked_bits_are_never_set():
    sizes = [(12, 20)] * 5
    both = twin_draw(sizes, 0, 512, 4, 7)
    assert set(both[:, 3].tolist()) == set(range(8))
    assert set(twin_draw(sizes, 0, 512, 4, 7, use_hflip=False)[:, 3].tolist()) == {0, 2, 4, 6}
    assert set(twin_draw(sizes, 0, 512, 4, 7, use_rot=False)[:, 3].tolist()) == {0, 1}
    assert set(twin_draw(sizes, 0, 512, 4, 7, use_hflip=False, use_rot=False)[:, 3].tolist()) == {0}
    assert np.array_equal(both[:, :3], twin_draw(sizes, 0, 512, 4, 7, use_hflip=False, use_rot=False)[:, :3])


# ---- the reference's fixture --------------------------------------------------------------------------------------------------
CASES = ("s1_12x20", "s4_6x10")


def golden_case(name):
    z = load_golden("g11_pairs.npz")
    scale, patch, top, left = (int(v) for v in z[f"{name}.meta"])
    return z, scale, patch, top, left


@pytest.mark.parametrize("name", CASES)
def test_golden_codes_are_the_reference_augmentations(name):
    """G11: ``augment``'s (hflip, vflip, transpose) triple is code h | v << 1 | t << 2, and every mode of the Deraining tree's
    ``data_augmentation`` is exactly one code -- the map is a bijection of the 8 modes onto the 8 codes (NumPy twin == reference)"""
    z, scale, patch, top, left = golden_case(name)
    gts, lqs = [z[f"{name}.gt"]], [z[f"{name}.lq"]]
    by_code = [twin_gather(gts, lqs, [[0, top, left, code]], patch, patch, scale) for code in range(8)]
    for code in range(8):
        h, v, t = code & 1, (code >> 1) & 1, code >> 2
        assert np.array_equal(by_code[code][0][0], z[f"{name}.aug{h}{v}{t}.lq"].numpy())
        assert np.array_equal(by_code[code][1][0], z[f"{name}.aug{h}{v}{t}.gt"].numpy())
    mode_to_code = {}
    for m in range(8):
        hits = [c for c in range(8) if np.array_equal(by_code[c][0][0], z[f"{name}.mode{m}.lq"].numpy())
                and np.array_equal(by_code[c][1][0], z[f"{name}.mode{m}.gt"].numpy())]
        assert len(hits) == 1, (m, hits)
        mode_to_code[m] = hits[0]
    assert sorted(mode_to_code.values()) == list(range(8))
    assert mode_to_code == {0: 0, 1: 2, 2: 5, 3: 4, 4: 3, 5: 1, 6: 6, 7: 7}


# ---- host validation ------------------------------------------------------------------------------------------------------------
def small_pool(scale=2):
    gts, lqs = random_pairs([(12, 20), (9, 10)], scale)
    return DevicePairPool.from_arrays(gts, lqs, scale, "cpu")


@pytest.mark.parametrize("row, patch, what", [
    ([2, 0, 0, 0], 8, "pair index"), ([-1, 0, 0, 0], 8, "pair index"),
    ([0, 9, 0, 0], 8, "top"), ([0, -1, 0, 0], 8, "top"), ([1, 6, 0, 0], 8, "top"),
    ([0, 0, 17, 0], 8, "left"), ([1, 0, 7, 0], 8, "left"), ([0, 0, -2, 0], 8, "left"),
    ([0, 0, 0, 8], 8, "code"), ([0, 0, 0, 4], (8, 12), "transpose"), ([0, 0, 0, 7], (4, 8), "transpose"),
])
def test_gather_validates_the_table_on_the_host(row, patch, what):
    """an index, top or left out of range, or the transpose bit on a non-square patch, raises before anything reaches a device"""
    pool = small_pool()
    with pytest.raises(ValueError, match=what):
        pool.gather([[0, 0, 0, 0], row], patch)
    with pytest.raises(ValueError, match="multiple of the scale"):
        pool.gather([[0, 0, 0, 0]], 7)


def test_pool_construction_rejects_mismatched_pairs():
    gts, lqs = random_pairs([(12, 20), (9, 10)], 2)
    with pytest.raises(ValueError, match="scale mismatches"):
        DevicePairPool.from_arrays(gts, lqs, 4, "cpu")
    with pytest.raises(ValueError, match="scale mismatches"):
        DevicePairPool.from_arrays([gts[0], gts[1][:-1]], lqs, 2, "cpu")
    with pytest.raises(ValueError, match="channels"):
        DevicePairPool.from_arrays([gts[0], gts[1][..., :1]], lqs, 2, "cpu")
    with pytest.raises(ValueError, match="channels"):
        DevicePairPool.from_arrays([g[..., :2] for g in gts], [l[..., :2] for l in lqs], 2, "cpu")
    with pytest.raises(ValueError, match="uint8"):
        DevicePairPool.from_arrays([g.astype(np.float32) for g in gts], lqs, 2, "cpu")
    with pytest.raises(ValueError):
        DevicePairPool.from_arrays(gts, lqs[:1], 2, "cpu")
    pool = DevicePairPool.from_arrays([torch.from_numpy(g) for g in gts], lqs, 2, "cpu")   # tensors and arrays alike
    assert len(pool) == 2 and pool.channels == 3 and pool.table_host.tolist() == [[0, 2880, 12, 20], [3600, 4680, 9, 10]]
    assert pool.data.numel() == 4680 + 270 and (pool.rank, pool.world) == (0, 1)


def test_batches_rejects_a_patch_larger_than_the_smallest_image():
    pool = small_pool()
    with pytest.raises(ValueError, match="smallest image"):
        pool.batches(4, 20)            # LQ patch 10 > the 9 rows of pair 1, raised by the call, not by the first next()
    with pytest.raises(ValueError, match="multiple of the scale"):
        pool.batches(4, 9)
    with pytest.raises(ValueError, match="not supported"):
        pool.batches(0, 8)
    assert pool.batches(4, 18) is not None      # fits: 9 x 9 LQ; nothing is drawn before the first next()
    assert pool.state_dict() == {"seed": 0, "samples_drawn": 0}


def test_pool_file_and_state_round_trip(tmp_path):
    pool = small_pool()
    pool.save(str(tmp_path / "pool.pt"))
    again = DevicePairPool.load(str(tmp_path / "pool.pt"), "cpu", seed=5)
    assert torch.equal(again.data, pool.data) and np.array_equal(again.table_host, pool.table_host)
    assert (again.scale, again.channels, again.swap_rb) == (2, 3, True)
    again.load_state_dict({"seed": 77, "samples_drawn": 1 << 40})
    assert again.state_dict() == {"seed": 77, "samples_drawn": 1 << 40}
    with pytest.raises(ValueError):
        again.load_state_dict({"seed": -1, "samples_drawn": 0})


def test_pairs_ok_is_a_pure_host_query():
    lib = _capi.load()
    assert lib.oss_pairs_ok(3, 4, 64, 64, 8) == 1 and lib.oss_pairs_ok(1, 1, 1, 1, 1) == 1 and lib.oss_pairs_ok(3, 1, 128, 128, 65535) == 1
    assert lib.oss_pairs_ok(2, 4, 64, 64, 8) == 0 and lib.oss_pairs_ok(3, 0, 64, 64, 8) == 0 and lib.oss_pairs_ok(3, 4, 0, 64, 8) == 0
    assert lib.oss_pairs_ok(3, 4, 64, 64, 0) == 0 and lib.oss_pairs_ok(3, 4, 64, 64, 65536) == 0
    assert lib.oss_pairs_ok(3, 4, 510, 339, 1) == 1        # a whole DIV2K validation pair: 16 * 11 + 64 * 43 tiles
    assert lib.oss_pairs_ok(3, 1, 8192, 8192, 1) == 0      # 2 * 256 * 256 tiles
