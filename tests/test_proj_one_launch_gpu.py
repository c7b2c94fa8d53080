"""x_proj and dt_proj as ONE launch (oss_proj_fwd_dt_kernel, csrc/oss_proj.hip) against the two launches it replaces
(oss_proj_fwd_mfma_kernel + oss_dt_fwd_kernel): bit-identical xdbl and dts for bf16 and f16, at every tile form, at the shapes that stay
on the two launches, at the tile edges, and against a float64 product.  The dispatch is switched with ``oss_proj_set_one_launch``.

Which shapes the one launch takes: 16-bit I/O, dts wanted, R <= 8, D % 16 == 0, D <= 192, L a multiple of the tile (128 steps, 64
when the grid is small -- so L = 192 runs as three 64-step tiles, L = 130 stays on the two launches), 16-byte aligned tensors."""
import functools

import pytest
import torch

from conftest import assert_close
from vmambair_amd import _capi, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "f16"]
IO = {torch.bfloat16: _capi.OSS_BF16, torch.float16: _capi.OSS_F16}
SENTINEL = 777.0   # exactly representable in bf16 and f16; no projection of unit-scale operands produces it in every element

TAKEN = [  # (B, D, R, N, L)
    (1, 96, 6, 16, 128),    # one tile
    (2, 96, 6, 16, 256),    # two tiles, batch stride
    (1, 48, 3, 16, 128),    # KS 3, 70 rows: the third row tile is ragged
    (1, 96, 8, 16, 128),    # R at the limit
    (1, 96, 1, 16, 128),
    (1, 192, 8, 16, 128),   # D at the limit
    (3, 32, 2, 4, 384),     # small N: 2C = 12, a single short row tile
]
FALLBACK = [
    (1, 96, 12, 16, 128),   # R = 12
    (1, 96, 6, 16, 192),    # no multiple of 128 (three 64-step tiles)
    (1, 96, 6, 16, 130),    # no multiple of any tile
    (1, 40, 3, 16, 128),    # D % 16 != 0
]


def _ids(shapes):
    return [f"B{s[0]}D{s[1]}R{s[2]}N{s[3]}L{s[4]}" for s in shapes]


@pytest.fixture
def one_launch():
    """call with 0 (two launches), 1 (as shipped), 64 | 128 (tile forced); the library is back at 1 afterwards"""
    lib = _capi.load()
    yield lib.oss_proj_set_one_launch
    lib.oss_proj_set_one_launch(1)


@functools.lru_cache(maxsize=None)
def _operands(shape, dt, kind="random"):
    B, D, R, N, L = shape
    Cc = R + 2 * N
    g = torch.Generator().manual_seed(11 + D + 7 * R + L)
    if kind == "random":
        x2 = torch.randn(B, 2, D, L, generator=g).to(dt)
        wx = torch.randn(4, Cc, D, generator=g) / D ** 0.5
        wdt = torch.randn(4, D, R, generator=g) / R ** 0.5
    else:   # integers: every product and every partial sum of xdbl is exact in fp32 and |xdbl| <= D < 256 exact in both types
        x2 = torch.randint(-1, 2, (B, 2, D, L), generator=g).to(dt)
        wx = torch.randint(-1, 2, (4, Cc, D), generator=g).float()
        wdt = torch.randint(-2, 3, (4, D, R), generator=g).float()
    return x2.to(DEV), wx.to(DEV), wdt.to(DEV)


@functools.lru_cache(maxsize=None)
def _two_launches(shape, dt, kind="random"):
    """the reference side of every equality below, computed once per case; never modified"""
    lib = _capi.load()
    lib.oss_proj_set_one_launch(0)
    try:
        xdbl, dts = ops.proj_fwd(*_operands(shape, dt, kind))
        torch.cuda.synchronize()
    finally:
        lib.oss_proj_set_one_launch(1)
    return xdbl, dts


def _raw_fwd(dt, x2, wx, wdt, xdbl, dts, shape):
    """the C entry point on buffers of the test's own (views, guard rows, dts omitted)"""
    B, D, R, N, L = shape
    with torch.cuda.device(x2.device):
        _capi.check(_capi.load().oss_proj_fwd(IO[dt], x2.data_ptr(), wx.data_ptr(), wdt.data_ptr(), xdbl.data_ptr(),
                                              dts.data_ptr() if dts is not None else None, B, D, R + 2 * N, R, L,
                                              torch.cuda.current_stream().cuda_stream), "oss_proj_fwd")
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", [1, 64, 128], ids=["by_grid", "tile64", "tile128"])
@pytest.mark.parametrize("shape", TAKEN, ids=_ids(TAKEN))
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_one_launch_equals_two_launches(shape, dt, mode, one_launch):
    ref_x, ref_d = _two_launches(shape, dt)
    one_launch(mode)
    xdbl, dts = ops.proj_fwd(*_operands(shape, dt))
    assert torch.equal(xdbl, ref_x), "xdbl"
    assert torch.equal(dts, ref_d), "dts"


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_integer_operands_are_exact_and_equal(dt, one_launch):
    shape = (2, 96, 6, 16, 256)
    B, D, R, N, L = shape
    x2, wx, wdt = _operands(shape, dt, "integer")
    ref_x, ref_d = _two_launches(shape, dt, "integer")
    one_launch(1)
    xdbl, dts = ops.proj_fwd(x2, wx, wdt)
    assert torch.equal(xdbl, ref_x) and torch.equal(dts, ref_d)
    x64, w64 = x2.double().cpu(), wx.double().cpu()
    z = torch.cat([torch.einsum("bjdl,jcd->bjcl", x64, w64[0:2]), torch.einsum("bjdl,jcd->bjcl", x64, w64[2:4])], dim=1)
    assert torch.equal(xdbl.double().cpu(), z), "xdbl: integer sums below 256 are exact"
    d64 = torch.einsum("bkrl,kdr->bkdl", z[:, :, :R], wdt.double().cpu()).reshape(B, 4 * D, L)
    assert torch.equal(dts.cpu(), d64.float().to(dt)), "dts: exact fp32 sums, one rounding"


@pytest.mark.parametrize("shape", FALLBACK, ids=_ids(FALLBACK))
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_shapes_outside_the_rule_are_unchanged(shape, dt, one_launch):
    ref_x, ref_d = _two_launches(shape, dt)
    one_launch(1)
    xdbl, dts = ops.proj_fwd(*_operands(shape, dt))
    assert torch.equal(xdbl, ref_x) and torch.equal(dts, ref_d)


@pytest.mark.parametrize("which", ["x2", "xdbl", "dts"])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_views_off_the_16_byte_grid_are_unchanged(which, dt, one_launch):
    shape = (1, 96, 6, 16, 128)
    B, D, R, N, L = shape
    x2, wx, wdt = _operands(shape, dt)
    ref_x, ref_d = _two_launches(shape, dt)

    def buf(n, off):
        flat = torch.full((n + 16,), SENTINEL, dtype=dt, device=DEV)
        return flat, flat[off:off + n]

    one_launch(1)
    xflat, xv = buf(x2.numel(), 2 if which == "x2" else 0)
    xv.copy_(x2.reshape(-1))
    zflat, zv = buf(ref_x.numel(), 2 if which == "xdbl" else 0)
    dflat, dv = buf(ref_d.numel(), 2 if which == "dts" else 0)
    _raw_fwd(dt, xv, wx, wdt, zv, dv, shape)
    assert torch.equal(zv.view_as(ref_x), ref_x) and torch.equal(dv.view_as(ref_d), ref_d)
    for flat, off, n in ((zflat, 2 if which == "xdbl" else 0, ref_x.numel()), (dflat, 2 if which == "dts" else 0, ref_d.numel())):
        assert bool((flat[:off] == SENTINEL).all()) and bool((flat[off + n:] == SENTINEL).all())


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_dts_omitted_writes_xdbl_only(dt, one_launch):
    shape = (1, 96, 6, 16, 128)
    B, D, R, N, L = shape
    assert _capi.load().oss_proj_rows_optional_ok(IO[dt], B, D, R + 2 * N, R, L) == 1
    x2, wx, wdt = _operands(shape, dt)
    ref_x, ref_d = _two_launches(shape, dt)
    one_launch(1)
    # xdbl and, right behind it where a dts of this call would lie, a canary of that size
    flat = torch.full((ref_x.numel() + ref_d.numel(),), SENTINEL, dtype=dt, device=DEV)
    _raw_fwd(dt, x2, wx, wdt, flat[:ref_x.numel()], None, shape)
    assert torch.equal(flat[:ref_x.numel()].view_as(ref_x), ref_x)
    assert bool((flat[ref_x.numel():] == SENTINEL).all()), "nothing may be written where dts would be"


@pytest.mark.parametrize("mode", [64, 128], ids=["tile64", "tile128"])
@pytest.mark.parametrize("shape", [(2, 96, 6, 16, 256), (1, 48, 3, 16, 128)], ids=_ids([(2, 96, 6, 16, 256), (1, 48, 3, 16, 128)]))
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_guard_rows_around_the_outputs_stay_untouched(shape, dt, mode, one_launch):
    B, D, R, N, L = shape
    x2, wx, wdt = _operands(shape, dt)
    ref_x, ref_d = _two_launches(shape, dt)
    guard = 4 * L   # four rows before and after
    zflat = torch.full((ref_x.numel() + 2 * guard,), SENTINEL, dtype=dt, device=DEV)
    dflat = torch.full((ref_d.numel() + 2 * guard,), SENTINEL, dtype=dt, device=DEV)
    one_launch(mode)
    _raw_fwd(dt, x2, wx, wdt, zflat[guard:guard + ref_x.numel()], dflat[guard:guard + ref_d.numel()], shape)
    for flat, ref in ((zflat, ref_x), (dflat, ref_d)):
        assert bool((flat[:guard] == SENTINEL).all()) and bool((flat[guard + ref.numel():] == SENTINEL).all()), "guard rows"
        assert torch.equal(flat[guard:guard + ref.numel()].view_as(ref), ref)   # (so every element inside was written)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_against_float64_product_of_the_rounded_operands(dt, one_launch):
    shape = (2, 96, 6, 16, 256)
    B, D, R, N, L = shape
    x2, wx, wdt = _operands(shape, dt)
    one_launch(1)
    xdbl, dts = ops.proj_fwd(x2, wx, wdt)
    x64, w64 = x2.double().cpu(), wx.to(dt).double().cpu()   # the matrix cores multiply the weights narrowed to the I/O type
    z = torch.cat([torch.einsum("bjdl,jcd->bjcl", x64, w64[0:2]), torch.einsum("bjdl,jcd->bjcl", x64, w64[2:4])], dim=1)
    d = torch.einsum("bkrl,kdr->bkdl", z.to(dt).double()[:, :, :R], wdt.double().cpu()).reshape(B, 4 * D, L)
    # the tolerances of tests/test_proj_gpu.py::test_projections_forward_backward for 16-bit I/O
    assert_close(xdbl, z, 1.2e-2, 1e-2 * float(z.abs().max()), "xdbl")
    assert_close(dts, d, 2e-2, 3e-2 * float(d.abs().max()), "dts")


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_reruns_are_bit_identical(dt, one_launch):
    shape = (2, 96, 6, 16, 256)
    one_launch(1)
    a = ops.proj_fwd(*_operands(shape, dt))
    b = ops.proj_fwd(*_operands(shape, dt))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
