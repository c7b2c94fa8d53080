"""The host plan of the 1x1-convolution launches (csrc/oss_conv1x1_plan.h) through ``oss_conv1x1_describe`` (no GPU): which
kernel, which template arguments, which grid a forward / input-gradient call would launch is integer arithmetic on the shape, the
strides and the low address bits.  The calls carry stand-in addresses; nothing is launched and nothing is dereferenced."""
import ctypes
import itertools

import pytest

from conv1x1_plan_cases import (EXPECTED, F32_SPLITK, F32_TILE64, FIELDS, PAIR, PAIRK, PAIRW, REUSE, SMALLEST, UNREACHABLE, WG)
from vmambair_amd import _capi

OK, ERR_SHAPE, ERR_NULL = 0, _capi._K["OSS_ERR_SHAPE"], _capi._K["OSS_ERR_NULL"]
Launch = _capi._HDR.structs["oss_conv1x1_launch"]
LDS_MAX = 160 * 1024
BASE = 0x100000        # a stand-in address, 16-byte aligned

IOS = {"bf16": _capi.OSS_BF16, "f16": _capi.OSS_F16, "f32": _capi.OSS_F32, "f32_split": _capi.OSS_F32_BF16X3}
BATCHES = (1, 2, 8, 65535, 65536)
ROWS = (1, 31, 33, 40, 96, 192, 254, 510, 765)
# (32 and 64 added to the issue's list: the workgroup-level kernel is built for K / 16 = 2 and 4 as well)
CHANNELS = (1, 16, 30, 32, 40, 48, 64, 80, 96, 127, 128, 176, 192, 255, 510, 520)
PIXELS = (1, 63, 64, 128, 256, 4096, 16384)
ALIGN = (0, 4, 2)      # address & 15 of a 16-, 4- and 2-byte aligned tensor
OVERRIDES = ((1, 0), (0, 0), (1, 64), (1, 128))
WG_BUILT = (16, 32, 48, 64, 96, 128, 192)


@pytest.fixture
def lib():
    lib = _capi.load()
    yield lib
    lib.oss_conv1x1_set_wg(1, 0)


def key(o):
    return tuple(getattr(o, f) for f in FIELDS)


def wg_takes(io, M, K, P, xsb, xsk, xa, wa, res):
    """conv1x1_wg_ok, written out again (y and the residual sit at aligned addresses here)"""
    return (io in ("bf16", "f16") and not res and K in WG_BUILT and P % 128 == 0 and xsb % 8 == 0 and xsk % 8 == 0 and xa == 0 and
            wa == 0)


def walk(lib, io, dgrad, reached):
    """every call of the grid for one element type and direction; -> accepted calls"""
    desc, o = lib.oss_conv1x1_describe, Launch()
    ref, code, sixteen = ctypes.byref(o), IOS[io], io in ("bf16", "f16")
    accepted = 0
    for on, pixels in OVERRIDES:
        lib.oss_conv1x1_set_wg(on, pixels)
        for B, M, K, P in itertools.product(BATCHES, ROWS, CHANNELS, PIXELS):
            cout, cin = (K, M) if dgrad else (M, K)
            for res, img, wa, xa, pad in itertools.product((0, 1), (0, 1), ALIGN, ALIGN, (0, 1)):
                xsk = P + pad
                xsb = K * xsk
                rc = desc(dgrad, code, BASE + xa, BASE + wa, BASE if img else None, None, BASE if res else None, BASE, B, cout, cin, P,
                          xsb, xsk, ref)
                if rc != OK:
                    assert rc == ERR_SHAPE
                    # a 16-bit call is refused for its grid alone
                    assert not sixteen or B > 65535, (io, dgrad, B, M, K, P)
                    continue
                accepted += 1
                fam, per = o.family, o.per
                t = (fam, o.ks, o.mt, o.wt, o.wvec, o.res, o.pf, o.wimg, o.pt, o.x3)
                if t not in reached:
                    reached[t] = (io, dgrad, B, M, K, P, res, img, wa, xa, pad, (on, pixels))
                where = (t, io, dgrad, B, M, K, P, res, img, wa, xa, pad, on, pixels)
                assert o.grid_x * o.pt >= P and o.grid_x >= 1, where
                assert 1 <= o.grid_y <= 65535 and 1 <= o.grid_z <= 65535 and o.lds_bytes <= LDS_MAX, where
                if sixteen:
                    assert fam < F32_TILE64 and o.grid_y == B and o.grid_z * per * 32 >= M and o.block == 256, where
                else:
                    assert fam >= F32_TILE64 and o.grid_z == B and o.grid_y * o.mt * 32 >= M and o.mt == per, where
                    assert o.block == (256 if fam == F32_SPLITK else 64) and o.x3 == (io == "f32_split"), where
                if fam in (WG, PAIR, REUSE):
                    assert o.ks * 16 >= K, where
                takes = wg_takes(io, M, K, P, xsb, xsk, xa, wa, res and not dgrad)
                assert (fam == WG) == bool(on and takes), where
                if fam == WG:
                    assert not o.res and o.nz == o.grid_z and o.ks * 16 == K and o.pt in (64, 128), where
                    assert not pixels or o.pt == pixels, where
                if o.wvec or fam == PAIRW:
                    assert wa == 0 and not dgrad, where
                if fam in (PAIR, PAIRW, PAIRK):
                    assert P % 2 == 0 and xsk % 2 == 0 and xsb % 2 == 0 and xa in (0, 4), where
                if o.wimg:
                    assert img and sixteen, where
                if o.res:
                    assert res and not dgrad, where
                if o.wt:
                    assert dgrad or M == K == 1, where
    return accepted


REACHED, WALKED = {}, set()


@pytest.mark.parametrize("dgrad", (0, 1), ids=("forward", "input_gradient"))
@pytest.mark.parametrize("io", list(IOS))
def test_every_plan_of_the_grid_covers_its_call(lib, io, dgrad):
    assert walk(lib, io, dgrad, REACHED) > 0
    WALKED.add((io, dgrad))


def test_the_grid_reaches_every_instantiation_and_nothing_else(lib):
    """zero missing, zero extra against the hand-written set; the smallest-call table names the same tuples"""
    for io, dgrad in itertools.product(IOS, (0, 1)):
        if (io, dgrad) not in WALKED:   # (this test selected alone)
            walk(lib, io, dgrad, REACHED)
            WALKED.add((io, dgrad))
    got = set(REACHED)
    assert not (EXPECTED - got), sorted(EXPECTED - got)
    assert not (got - EXPECTED), sorted((t, REACHED[t]) for t in got - EXPECTED)
    assert not (got & UNREACHABLE) and set(SMALLEST) == EXPECTED


@pytest.mark.parametrize("t", sorted(SMALLEST), ids=lambda t: "-".join(map(str, t)))
def test_smallest_calls_reach_their_tuple(lib, t):
    io, dgrad, B, M, K, P, res, img, wa, xa, pad, ov = SMALLEST[t]
    o = Launch()
    lib.oss_conv1x1_set_wg(*ov)
    cout, cin = (K, M) if dgrad else (M, K)
    assert lib.oss_conv1x1_describe(dgrad, IOS[io], BASE + xa, BASE + wa, BASE if img else None, None, BASE if res else None, BASE, B, cout,
                                    cin, P, K * (P + pad), P + pad, ctypes.byref(o)) == OK
    assert key(o) == t


def test_shapes_read_from_the_launchers(lib):
    """the dispatch as DESIGN.md tells it, at the shapes of the training step"""
    o = Launch()

    def d(dgrad, io, B, cout, cin, P, res=False, img=False, wa=0):
        assert lib.oss_conv1x1_describe(dgrad, IOS[io], BASE, BASE + wa, BASE if img else None, None, BASE if res else None, BASE, B, cout,
                                        cin, P, (cout if dgrad else cin) * P, P, ctypes.byref(o)) == OK
        return o

    assert (d(0, "bf16", 8, 192, 96, 4096).family, o.pt, o.grid_x, o.grid_y, o.grid_z) == (WG, 128, 32, 8, 1)
    assert (d(0, "bf16", 2, 192, 96, 16384).pt, d(0, "bf16", 1, 192, 96, 16384).pt) == (128, 64)     # a workgroup per CU
    assert (d(0, "bf16", 8, 96, 48, 4096).pt, d(0, "bf16", 8, 96, 48, 16384).pt) == (64, 128)        # K <= 48: 64 up to 1024 tiles
    assert d(0, "bf16", 4, 192, 96, 1024).nz == 2 and o.lds_bytes == 96 * 2 * 96 + 4 * 32 * 2 * 80 + 2 * 96 * 4
    assert (d(0, "bf16", 8, 96, 96, 4096, res=True).family, o.ks, o.res, o.pf, o.wvec) == (PAIR, 6, 1, 1, 1)
    assert (d(0, "bf16", 8, 96, 127, 4096).family, d(0, "bf16", 8, 96, 127, 4096, img=True).family, o.ks, o.pf) == (PAIRW, PAIR, 8, 1)
    assert (d(1, "bf16", 8, 127, 48, 4096).family, o.ks, o.wt, o.pf) == (PAIR, 8, 1, 0)
    assert (d(0, "bf16", 8, 48, 255, 64).family, d(0, "bf16", 8, 48, 255, 4096).family) == (PAIRW, PAIRW)
    assert (d(1, "bf16", 8, 255, 96, 4096).family, o.mt, o.wt) == (PAIRK, 1, 1)
    # (K = 255 with 16-byte aligned rows of the matrix as a whole stays on pairw at every size: the K-chunk kernel needs an image,
    # a weight matrix off the 16-byte grid, or K > 512)
    assert (d(0, "bf16", 8, 765, 255, 4096, img=True).mt, d(0, "bf16", 8, 510, 255, 4096, wa=4).mt) == (3, 2)
    assert (d(0, "bf16", 8, 510, 520, 4096).family, o.mt, o.wvec) == (PAIRK, 2, 1)
    assert (d(0, "f32", 8, 96, 96, 4096).family, d(0, "f32", 8, 192, 96, 16384).family, d(0, "f32_split", 8, 96, 16, 4096).family) == (8, 6, 7)
    # the overrides
    lib.oss_conv1x1_set_wg(0, 128)
    assert d(0, "bf16", 8, 192, 96, 4096).family == PAIR
    lib.oss_conv1x1_set_wg(1, 0)
    # the plan owns the grid limits: one-tile workgroups (K = 255 at an odd pixel count: the generic kernel) beyond 65535 row tiles are
    # refused on the input gradient too; kernels that deal several tiles to a workgroup reach further
    big = 32 * 65535
    for dgrad, cout, cin in ((0, big + 1, 255), (1, 255, big + 1)):
        assert lib.oss_conv1x1_describe(dgrad, IOS["bf16"], BASE, BASE, None, None, None, BASE, 1, cout, cin, 63, (cout if dgrad else cin) * 63, 63,
                                        ctypes.byref(o)) == ERR_SHAPE
    assert lib.oss_conv1x1_describe(1, IOS["bf16"], BASE, BASE, None, None, None, BASE, 1, 255, big, 63, 255 * 63, 63, ctypes.byref(o)) == OK
    assert o.grid_z == 65535 and o.per == 1
    assert lib.oss_conv1x1_describe(1, IOS["bf16"], BASE, BASE, None, None, None, BASE, 1, 30, big + 1, 63, 30 * 63, 63, ctypes.byref(o)) == OK
    assert (o.family, o.grid_z, o.per) == (REUSE, 1024, 64)
    # argument rules of the entry points
    assert lib.oss_conv1x1_describe(0, IOS["bf16"], None, BASE, None, None, None, BASE, 1, 8, 8, 64, 512, 64, ctypes.byref(o)) == ERR_NULL
    assert lib.oss_conv1x1_describe(0, IOS["bf16"], BASE, BASE, BASE + 8, None, None, BASE, 1, 8, 8, 64, 512, 64, ctypes.byref(o)) == ERR_SHAPE
    assert lib.oss_conv1x1_describe(0, 7, BASE, BASE, None, None, None, BASE, 1, 8, 8, 64, 512, 64, ctypes.byref(o)) == ERR_SHAPE
    assert o.family == -1
    assert lib.oss_conv1x1_describe(0, IOS["bf16"], BASE, BASE, None, None, None, BASE, 1, 8, 8, 64, 512, 64, None) == ERR_NULL
