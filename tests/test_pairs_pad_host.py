"""Host side of the pair pool's Deraining forms (vmambair_amd/data.py ``dataset_gt_size`` / ``pad_to`` / ``ProgressiveSchedule`` on
oss_pairs.hip's ``oss_pairs_draw_window`` / ``oss_pairs_gather_padded``): the NumPy twin of the reflect map, of the folded sample and
of the two-stage draw -- the twin test_pairs_pad_gpu.py compares the kernels with bit for bit -- against the arrays the reference's
own ``padding`` / ``paired_random_crop`` / ``data_augmentation`` / ``img2tensor`` and window slicing produce
(tests/golden/make_golden_pairs_pad.py, G13), the folding identity, the stage table and the host validation.  No GPU needed.

Pixel data is compared with ``np.array_equal``: one correctly rounded ``byte / 255`` per value plus index maps on both sides."""
import itertools

import numpy as np
import pytest

from conftest import load_golden
from test_pairs_host import M32, TAG_CROP, lib_philox, philox4x32_10, random_pairs, twin_draw, twin_patch, twin_perm
from vmambair_amd import DevicePairPool, ProgressiveSchedule

TAG_WIND = 0x77696E64                                            # include/vmambair_oss.h: oss_pairs_draw_window
MODE_TO_CODE = {0: 0, 1: 2, 2: 5, 3: 4, 4: 3, 5: 1, 6: 6, 7: 7}   # data_augmentation's modes (test_pairs_host.py derives the map)
CASES = ("p5x7_g16_m16", "p5x7_g16_m4", "p15x16_g16", "p12x20_g16_m8", "p33x70_g96_m96", "p33x70_g96_m40", "p31x31_c1_g32")
OPTION_FILES = ("Deraining_mamber28", "Deraining_mamber32", "Deraining_mamber33", "Deraining_mamber34")


# ---- the twin -----------------------------------------------------------------------------------------------------------------
def reflect(i, n):
    """cv2.BORDER_REFLECT past the far edge (fedcba|abcdefgh|hgfedcb): r = i mod 2n; r < n ? r : 2n - 1 - r"""
    r = np.asarray(i) % (2 * n)
    return np.where(r < n, r, 2 * n - 1 - r)


def twin_padded_patch(img, top, left, ph, pw, code, swap_rb, pad):
    """``twin_patch`` on the image extended to ``max(side, pad)``: rows and columns go through the reflect map, nothing is built"""
    h, w = img.shape[:2]
    assert 0 <= top <= max(h, pad) - ph and 0 <= left <= max(w, pad) - pw
    v = img[reflect(np.arange(top, top + ph), h)][:, reflect(np.arange(left, left + pw), w)]
    return twin_patch(v, 0, 0, ph, pw, code, swap_rb)


def twin_gather_padded(gts, lqs, table, ph, pw, pad, swap_rb=True):
    """scale 1 -> (lq, gt), each (n, C, ph, pw) float32, for the rows pair_index, top, left, code of ``table``"""
    rows = np.asarray(table).tolist()
    return (np.stack([twin_padded_patch(lqs[p], t, l, ph, pw, c, swap_rb, pad) for p, t, l, c in rows]),
            np.stack([twin_padded_patch(gts[p], t, l, ph, pw, c, swap_rb, pad) for p, t, l, c in rows]))


def fold(top, left, G, m, x0, y0, code):
    """crop (top, left) of side G, augmentation ``code``, window rows x0 / columns y0 of side m -> the (top, left) of the ONE sample
    of side m with the same code"""
    wr, wc = (y0, x0) if code & 4 else (x0, y0)
    return top + (G - m - wr if code & 2 else wr), left + (G - m - wc if code & 1 else wc)


def twin_window(c, patch, full, seed, rank, world, philox=philox4x32_10):
    """the call's window offsets (x0 rows, y0 columns): words 0, 1 of the block keyed by the seed at the first sample's position"""
    g0 = c * world + rank
    r = philox((g0 & M32, g0 >> 32, TAG_WIND, 0), (seed & M32, seed >> 32))
    return (r[0] * (full - patch)) >> 32, (r[1] * (full - patch)) >> 32


def twin_draw_window(sizes, c, batch, patch, full, pad, seed, rank=0, world=1, use_hflip=True, use_rot=True, philox=philox4x32_10):
    """sizes: (n, 2) LQ heights / widths -> (batch, 4) int32 folded samples of per-rank positions c .. c + batch - 1"""
    n, key = len(sizes), (seed & M32, seed >> 32)
    code_mask = (1 if use_hflip else 0) | (6 if use_rot else 0)
    x0, y0 = twin_window(c, patch, full, seed, rank, world, philox)
    out = np.zeros((batch, 4), dtype=np.int32)
    for b in range(batch):
        g = (c + b) * world + rank
        epoch = g // n
        pair = twin_perm(g - epoch * n, n, epoch, key)
        r = philox((g & M32, g >> 32, TAG_CROP, 0), key)
        mh, mw = max(1, max(int(sizes[pair][0]), pad) - full + 1), max(1, max(int(sizes[pair][1]), pad) - full + 1)
        code = (r[2] >> 29) & code_mask
        out[b] = (pair, *fold((r[0] * mh) >> 32, (r[1] * mw) >> 32, full, patch, x0, y0, code), code)
    return out


def golden_case(name):
    z = load_golden("g13_pairs_pad.npz")
    G, m, top, left, x0, y0 = (int(v) for v in z[f"{name}.meta"])
    return z, G, m, top, left, x0, y0


def golden_table(name):
    """the 8 folded samples of a G13 case, by code -> (table, mode of every code)"""
    _, G, m, top, left, x0, y0 = golden_case(name)
    mode_of = {code: mode for mode, code in MODE_TO_CODE.items()}
    return [[0, *fold(top, left, G, m, x0, y0, code), code] for code in range(8)], [mode_of[code] for code in range(8)]


# the shapes of the GPU edge-geometry test (test_pairs_pad_gpu.py): patches of side 40 -- two tiles of 32 across -- from images
# extended to 96
EDGE_SIZES, EDGE_G, EDGE_P = [(33, 70), (5, 7), (40, 41)], 96, 40


def edge_table():
    """pair, top, left, code.  On the 33 x 70 image the last column (69) falls on patch column 69 - left: 32 (first of the second
    tile), 31 (last of the first), 15 and 47 (middles), 14, 13, and beyond the patch (wholly inside); rows wholly inside, astride row
    33 and wholly beyond it; 5 x 7: up to 19 periods; 40 x 41: columns wholly beyond the image, and its last column on patch
    column 0 and 31.  3 * left mod 4 takes all four values; all 8 codes"""
    return [[0, 0, 37, 0], [0, 20, 38, 1], [0, 56, 54, 2], [0, 10, 55, 3], [0, 1, 56, 4], [0, 33, 22, 5], [0, 2, 6, 6],
            [1, 0, 0, 7], [1, 56, 56, 0], [1, 13, 30, 5], [2, 0, 50, 1], [2, 30, 9, 6], [2, 56, 40, 3]]


# ---- the reflect map ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 7])
def test_reflect_is_numpy_symmetric_padding_over_several_periods(n):
    """``np.pad(mode="symmetric")``, the fixture's stand-in for ``copyMakeBorder(BORDER_REFLECT)``, is the stated index rule, for an
    extension of 0 .. 5 n elements"""
    a = np.arange(100, 100 + n)
    for extra in range(5 * n + 1):
        assert np.array_equal(np.pad(a, (0, extra), mode="symmetric"), a[reflect(np.arange(n + extra), n)])


# ---- the reference's fixture --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_twin_reproduces_the_golden_arrays(name):
    """G13: pad, crop at G, ``data_augmentation`` mode, ``img2tensor``, window -- the reference -- equals ONE folded sample of side m
    read through the reflect map -- the twin -- for all 8 modes, LQ and GT"""
    z, G, m, top, left, x0, y0 = golden_case(name)
    gt, lq = z[f"{name}.gt"], z[f"{name}.lq"]
    assert 0 <= x0 <= max(G - m - 1, 0) and 0 <= y0 <= max(G - m - 1, 0)
    table, modes = golden_table(name)
    got_lq, got_gt = twin_gather_padded([gt], [lq], table, m, m, G)
    for code, mode in enumerate(modes):
        assert np.array_equal(got_lq[code], z[f"{name}.modes.lq"][mode].numpy()), (name, mode)
        assert np.array_equal(got_gt[code], z[f"{name}.modes.gt"][mode].numpy()), (name, mode)


@pytest.mark.parametrize("m", [1, 4, 6])
def test_folding_identity(m):
    """pad -> crop -> augment -> slice equals the folded sample, for all 8 codes, every crop origin and every window offset (the
    closed range 0 .. G - m: one more than the reference ever draws), on a 9 x 5 image padded to G = 6 in x"""
    G = 6
    img = np.random.RandomState(m).randint(0, 256, (9, 5, 3)).astype(np.uint8)
    padded = np.pad(img, ((0, 0), (0, 1), (0, 0)), mode="symmetric")
    for code, top, x0, y0 in itertools.product(range(8), range(9 - G + 1), range(G - m + 1), range(G - m + 1)):
        want = twin_patch(padded, top, 0, G, G, code, True)[:, x0:x0 + m, y0:y0 + m]
        t, l = fold(top, 0, G, m, x0, y0, code)
        assert np.array_equal(twin_padded_patch(img, t, l, m, m, code, True, G), want), (code, top, x0, y0)


# ---- the two-stage draw -------------------------------------------------------------------------------------------------------
SIZES = [(5, 7), (15, 16), (12, 20), (33, 70), (16, 16)]


def test_window_block_comes_from_the_library_generator():
    """the twin's window offsets through ``oss_pairs_philox`` (the text the kernels are compiled from) and through the Python
    generator agree, at small and at 64-bit positions"""
    for c, rank, world in ((0, 0, 1), (7, 2, 3), ((1 << 38) + 5, 1, 4)):
        assert twin_window(c, 4, 16, 0x1234567 + (1 << 45), rank, world, lib_philox) == twin_window(c, 4, 16, 0x1234567 + (1 << 45), rank, world)
        assert np.array_equal(twin_draw_window(SIZES, c, 9, 4, 16, 16, 99, rank, world, philox=lib_philox),
                              twin_draw_window(SIZES, c, 9, 4, 16, 16, 99, rank, world))


@pytest.mark.parametrize("G, m", [(16, 4), (16, 15), (16, 16), (96, 40)])
def test_window_offsets_are_in_range_common_to_a_call_and_vary(G, m):
    """x0, y0 in {0 .. G - m - 1} ({0} at G == m), one pair per call, another per call and per rank; crop origins within
    max(side, G) - G: recovered from the folded samples by undoing the fold"""
    seed, batch, seen = 77, 6, set()
    for call, (rank, world) in itertools.product(range(40), ((0, 1), (0, 3), (2, 3))):
        c = call * batch
        x0, y0 = twin_window(c, m, G, seed, rank, world, lib_philox)
        assert 0 <= x0 <= max(G - m - 1, 0) and 0 <= y0 <= max(G - m - 1, 0)
        seen.add((rank, world, x0, y0))
        t = twin_draw_window(SIZES, c, batch, m, G, G, seed, rank, world, philox=lib_philox)
        plain = twin_draw([(max(h, G), max(w, G)) for h, w in SIZES], c, batch, G, seed, rank, world)    # the crop at G alone
        assert np.array_equal(t[:, [0, 3]], plain[:, [0, 3]])
        for (pair, top, left, code), (_, ctop, cleft, _) in zip(t.tolist(), plain.tolist()):
            assert 0 <= ctop <= max(SIZES[pair][0], G) - G and 0 <= cleft <= max(SIZES[pair][1], G) - G
            assert (top, left) == fold(ctop, cleft, G, m, x0, y0, code)              # the SAME window for every sample of the call
            assert 0 <= top <= max(SIZES[pair][0], G) - m and 0 <= left <= max(SIZES[pair][1], G) - m
    if G - m <= 1:
        assert {s[2:] for s in seen} == {(0, 0)}          # int((G - m) * random()) never reaches G - m
    else:
        for rank, world in ((0, 1), (0, 3), (2, 3)):
            assert len({s[2:] for s in seen if s[:2] == (rank, world)}) > 10                             # differs across calls
        assert {s[2:] for s in seen if s[:2] == (0, 3)} != {s[2:] for s in seen if s[:2] == (2, 3)}      # and across ranks


def test_draw_window_without_window_or_padding_is_the_plain_draw():
    sizes = [(20 + i % 5, 17 + i % 7) for i in range(11)]
    for c in (0, 13, (1 << 38) + 1):
        assert np.array_equal(twin_draw_window(sizes, c, 50, 8, 8, 0, 5, 1, 2), twin_draw(sizes, c, 50, 8, 5, 1, 2))
        assert np.array_equal(twin_draw_window(sizes, c, 50, 8, 8, 0, 5, 1, 2, use_rot=False), twin_draw(sizes, c, 50, 8, 5, 1, 2, use_rot=False))


# ---- the stage table ----------------------------------------------------------------------------------------------------------
def golden_schedule(name):
    z = load_golden("g13_pairs_pad.npz")
    opt = {k: z[f"options.{name}.{k}"].tolist() for k in ("iters", "mini_batch_sizes", "gt_sizes", "gt_size", "batch_size_per_gpu")}
    return opt, ProgressiveSchedule.from_options(opt)


def test_progressive_schedule_stages_of_the_option_files():
    """``groups = cumsum(iters)``, the first j with ``current_iter <= groups[j]``, else the last stage (train.py:219-250), for the
    lists of Deraining_mamber33 / 34: boundaries at 92000, 156000, 220000, 284000, 348000 and the end at 396000.

    The issue that asked for this test lists the iterations 1, 92000, 92001, 156000, 156001, 352000, 352001, 396000, 400000 with the
    stages 0, 0, 1, 1, 2, 4, 5, 5, 5.  Its fifth boundary is a slip of addition: 92000 + 4 * 64000 = 348000, not 352000, so under the
    rule it states itself 352000 is already stage 5.  All nine iterations are kept, with the stage the rule gives, and the boundary
    the list was after (348000 -> 4, 348001 -> 5) is added, as are all boundaries of every option file against an independent
    evaluation of the rule."""
    for name in ("Deraining_mamber33", "Deraining_mamber34"):
        opt, sched = golden_schedule(name)
        assert sched.groups == [92000, 156000, 220000, 284000, 348000, 396000] and (sched.gt_size, sched.batch_size) == (384, 8)
        its = [1, 92000, 92001, 156000, 156001, 348000, 348001, 352000, 352001, 396000, 400000]
        assert [sched.stage(it)[0] for it in its] == [0, 0, 1, 1, 2, 4, 5, 5, 5, 5, 5]
        assert sched.stage(1) == (0, 8, 128) and sched.stage(156001) == (2, 3, 192) and sched.stage(400000) == (5, 1, 384)
    for name in OPTION_FILES:
        opt, sched = golden_schedule(name)
        groups = np.cumsum(opt["iters"])
        for it in sorted({1, *groups.tolist(), *(groups + 1).tolist(), *(groups - 1).tolist(), int(groups[-1]) + 5000}):
            j = min(int(np.searchsorted(groups, it, side="left")), len(groups) - 1)
            assert sched.stage(it) == (j, opt["mini_batch_sizes"][j], opt["gt_sizes"][j]), (name, it)


def test_progressive_schedule_rejects_bad_tables():
    with pytest.raises(ValueError, match="one length"):
        ProgressiveSchedule([10, 10], [4], [8, 16], 16, 4)
    with pytest.raises(ValueError, match="one length"):
        ProgressiveSchedule([10, 10], [4, 2], [8], 16, 4)
    with pytest.raises(ValueError, match="one length"):
        ProgressiveSchedule([], [], [], 16, 4)
    with pytest.raises(ValueError, match="larger than the gt_size"):
        ProgressiveSchedule([10, 10], [4, 2], [8, 24], 16, 4)
    with pytest.raises(ValueError):
        ProgressiveSchedule([10, 10], [4, 0], [8, 16], 16, 4)
    assert ProgressiveSchedule([10, 10], [4, 2], [8, 16], 16, 4).stage(11) == (1, 2, 16)


# ---- host validation ------------------------------------------------------------------------------------------------------------
def pad_pool(scale=1, sizes=((5, 7), (12, 20))):
    gts, lqs = random_pairs(list(sizes), scale)
    return DevicePairPool.from_arrays(gts, lqs, scale, "cpu")


def test_dataset_gt_size_is_validated_when_called():
    pool = pad_pool()
    assert pool.batches(4, 8, dataset_gt_size=16) is not None             # 5 x 7 and 12 x 20 padded to 16: nothing drawn yet
    assert pool.batches(4, 16, dataset_gt_size=16) is not None
    with pytest.raises(ValueError, match="smaller than the GT patch"):
        pool.batches(4, 16, dataset_gt_size=8)                              # G < patch
    with pytest.raises(ValueError, match="not supported"):
        pool.batches(0, 8, dataset_gt_size=16)
    with pytest.raises(ValueError, match="scale 1 only"):
        pad_pool(4).batches(4, 16, dataset_gt_size=64)                      # LQ 5 x 7 would need padding to 16 at scale 4
    with pytest.raises(ValueError, match="multiple of the scale"):
        pad_pool(4).batches(4, 16, dataset_gt_size=18)                      # G is no multiple of the scale
    big = pad_pool(4, ((16, 18), (20, 16)))
    assert big.batches(4, 16, dataset_gt_size=64) is not None               # every image holds G: the two-stage draw at scale 4
    with pytest.raises(ValueError, match="scale 1 only"):
        big.batches(4, 16, dataset_gt_size=68)
    sched = ProgressiveSchedule([2, 2], [3, 1], [8, 16], 16, 4)
    assert pool.progressive_batches(sched) is not None
    with pytest.raises(ValueError, match="scale 1 only"):
        pad_pool(4).progressive_batches(ProgressiveSchedule([2, 2], [3, 1], [32, 64], 64, 4))
    assert pool.state_dict() == {"seed": 0, "samples_drawn": 0}


def test_without_dataset_gt_size_the_pool_still_rejects_small_images():
    pool = pad_pool()
    with pytest.raises(ValueError, match="smallest image"):
        pool.batches(4, 8)
    with pytest.raises(ValueError, match="smallest image"):
        pool.batches(4, 8, dataset_gt_size=None)
    with pytest.raises(ValueError, match="top"):
        pool.gather([[0, 1, 0, 0]], 5)                                      # 5 rows from row 1 of a 5-row image, no padding


@pytest.mark.parametrize("row, what", [([0, 13, 0, 0], "top"), ([0, 0, 13, 0], "left"), ([1, 0, 17, 0], "left"), ([1, 13, 0, 0], "top"),
                                       ([0, -1, 0, 0], "top"), ([2, 0, 0, 0], "pair index")])
def test_gather_validates_rows_against_the_padded_bounds(row, what):
    """patch 4 with pad_to 16: 5 x 7 counts as 16 x 16 (top, left <= 12), 12 x 20 as 16 x 20 (top <= 12, left <= 16)"""
    pool = pad_pool()
    with pytest.raises(ValueError, match=what):
        pool.gather([[0, 12, 12, 0], row], 4, pad_to=16)
    with pytest.raises(ValueError, match="scale 1 only"):
        pad_pool(4).gather([[0, 0, 0, 0]], 4, pad_to=64)
    with pytest.raises(ValueError, match="multiple of the scale"):
        pad_pool(4).gather([[0, 0, 0, 0]], 4, pad_to=18)


def test_edge_table_of_the_gpu_test_fits_the_padded_bounds():
    gts, lqs = random_pairs(EDGE_SIZES, 1)
    pool = DevicePairPool.from_arrays(gts, lqs, 1, "cpu")
    t = pool.validate_table(edge_table(), EDGE_P, EDGE_P, EDGE_G)
    assert t.dtype == np.int32 and len(t) == 13
    with pytest.raises(ValueError, match="top"):
        pool.validate_table(edge_table(), EDGE_P, EDGE_P, 0)
