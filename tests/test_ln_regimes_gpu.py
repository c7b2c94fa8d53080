"""The three LayerNorm implementations -- the stand-alone kernels of oss_layernorm.hip, the LayerNorm stage of the workgroup-level
1x1 convolution (oss_conv1x1_wg_kernel<.., LN = true>) and the LayerNorm backward behind the input gradient
(oss_conv1x1_dgrad_lnbwd_kernel) -- against the FLOAT64 reference in the input regimes of tests/ln_regimes.py, where the
statistics are hard: every output INCLUDING the kernels' own mean and rstd, with limits tied to the fp32 twin's own error
(ln_regimes.compare; what that limit catches is shown on the CPU in test_ln_regimes_host.py).  One forward and one backward per
case; every launch form the host code can choose is the stated target of a case."""
import pytest
import torch

import ln_regimes as lr
from vmambair_amd import _capi, ops
from vmambair_amd.ops import pointwise
from vmambair_amd.ops._common import _DT
from vmambair_amd.ops.layernorm import _LN_PAIRS

pytestmark = [pytest.mark.gpu, pytest.mark.tier(0)]
DEV = "cuda:0"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
CODE = {F32: 0, F16: 1, BF16: 2}
TESTED_BEFORE = [(F32, F32), (F32, BF16), (BF16, BF16)]                      # the pairs of test_glue_gpu.py
UNTESTED_BEFORE = [(F32, F16), (F16, F16), (F16, F32), (BF16, F32)]
assert set(TESTED_BEFORE + UNTESTED_BEFORE) == set(_LN_PAIRS)


def _dev(t, shape=None):
    return None if t is None else (t if shape is None else t.view(shape)).to(DEV)


# ---- which instantiation of OSS_LN_LAUNCH a call takes (oss_layernorm.hip: ln_waves, ln_cached, ln_pairs) -----------------------
def _ln_form(B, C, P, pairs_possible=True):
    """-> "<CPW, V, MAXT>/waves" as the host code chooses it; ``pairs_possible``: even strides and 8-byte aligned pointers"""
    nw = 4 if C <= 96 else (8 if C <= 192 else 16)
    pairs = C <= 384 and nw <= 8 and P % 2 == 0 and pairs_possible
    if nw == 4 and C >= 48 and B * ((P + 127) // 128) * 4 < 4096:
        nw = 8
    if C > 384:
        return f"<0, 1, 1024>/{nw}"
    if not pairs:
        return f"<24, 1, 1024>/{nw}"
    half = C <= nw * 12
    return f"<{12 if half else 24}, 2, {256 if nw == 4 else 512}>/{nw}"


def _standalone(label, regime, shape, xdt, ydt, bias, gate, skip, affine=None, place=None, pairs_possible=True, form=None, seed=0):
    """ln_nchw_fwd + ln_nchw_bwd (the backward on the kernel's own mean / rstd) against float64: y, mean, rstd, dx, dgate, dw, db.
    ``place``: how x and the gate get to the device (misaligned, strided views); default: a contiguous copy."""
    B, C, H, W = shape
    P = H * W
    if form is not None:
        assert _ln_form(B, C, P, pairs_possible) == form, (_ln_form(B, C, P, pairs_possible), form)
    inp = lr.make_inputs(regime, B, C, P, xdt, ydt, seed, bias, gate, skip, affine)
    ref64, ref32 = lr.references(inp)
    place = place or (lambda t: t.to(DEV))
    x = place(inp["x"].view(shape))
    g = place(inp["gate"].view(shape)) if gate else None
    assert torch.equal(x.cpu(), inp["x"].view(shape))
    w, b = _dev(inp["w"]), _dev(inp["b"])
    y, mean, rstd = torch.ops.vmambair.ln_nchw_fwd(x, w, b, g, CODE[ydt])
    dx, dgate, dw, db = torch.ops.vmambair.ln_nchw_bwd(x, w, b, g, _dev(inp["dy"], shape), mean, rstd, _dev(inp["skip"], shape), None,
                                                       _dev(inp["dy_mul"]), _dev(inp["dy_add"]), inp["add_scale"])
    torch.cuda.synchronize()
    assert y.dtype == ydt and dx.dtype == xdt and mean.dtype == F32 and rstd.dtype == F32
    got = {"y": y, "mean": mean, "rstd": rstd, "dx": dx, "dw": dw, "db": db if bias else None, "dgate": dgate if gate else None}
    lr.compare(got, ref64, ref32, (xdt, ydt), f"{label}:{regime} {'WithBias' if bias else 'BiasFree'} gate={int(gate)} "
               f"skip={int(skip)} {B}x{C}x{H}x{W}")


# ---- a. the stand-alone kernels: every regime, both forms, every dtype pair ---------------------------------------------------
# (2, 96, 9, 14): P = 126 is even (pixel pairs) with a ragged last 128-pixel tile; C = 96 at a small grid is <12, 2, 512>/8
_A_CASES = [(r, p) for p in UNTESTED_BEFORE for r in lr.REGIMES] + [(r, p) for p in TESTED_BEFORE for r in ("offset", "flat", "wide")]


@pytest.mark.parametrize("gate", [True, False], ids=["gate", "nogate"])
@pytest.mark.parametrize("bias", [True, False], ids=["WithBias", "BiasFree"])
@pytest.mark.parametrize("regime,pair", _A_CASES, ids=[f"{r}-{NAME[p[0]]}-{NAME[p[1]]}" for r, p in _A_CASES])
def test_standalone_kernels_vs_float64(regime, pair, bias, gate):
    _standalone("a", regime, (2, 96, 9, 14), pair[0], pair[1], bias, gate, skip=False, form="<12, 2, 512>/8")


# ---- b. every launch form of OSS_LN_LAUNCH ------------------------------------------------------------------------------------
def _off_grid(t):
    """the same values at a base pointer one element off the 8-byte grid"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 8 != 0
    return v


def _channel_slice(t):
    """a channel slice of a tensor twice as wide whose planes are one element longer: channel stride H W + 1"""
    B, C, H, W = t.shape
    wide = torch.zeros(B, 2 * C, H * W + 1, dtype=t.dtype, device=DEV)
    v = wide[:, C // 2:C // 2 + C, :H * W].view(B, C, H, W)
    v.copy_(t)
    assert v.stride(1) == H * W + 1 and v.stride(3) == 1 and v.stride(2) == W
    return v


_B_CASES = [
    # shape, expected form, placement, pairs possible
    ((2, 385, 7, 10), "<0, 1, 1024>/16", None, True),            # streaming: C > 16 x 24
    ((2, 384, 7, 10), "<24, 1, 1024>/16", None, True),           # 16 waves, every slot used: no pixel pairs
    ((2, 193, 7, 10), "<24, 1, 1024>/16", None, True),           # 16 waves, 13 slots in wave 0 and 12 in the others
    ((2, 96, 5, 7), "<24, 1, 1024>/8", None, True),              # odd P
    ((2, 96, 9, 14), "<24, 1, 1024>/8", _off_grid, False),       # even P, base pointer off the 8-byte grid
    ((2, 96, 9, 14), "<24, 1, 1024>/8", _channel_slice, False),  # even P, odd channel stride
    ((2, 48, 9, 14), "<12, 2, 512>/8", None, True),              # small grid: 8 waves, 6 slots
    ((2, 96, 9, 14), "<12, 2, 512>/8", None, True),              # ... 12 slots, all used
    ((2, 97, 9, 14), "<24, 2, 512>/8", None, True),
    ((2, 192, 9, 14), "<24, 2, 512>/8", None, True),
    ((2, 24, 9, 14), "<12, 2, 256>/4", None, True),              # C < 48: four waves whatever the grid
    ((2, 40, 9, 14), "<12, 2, 256>/4", None, True),
    ((128, 48, 32, 32), "<12, 2, 256>/4", None, True),           # 128 x 8 x 4 = 4096: the grid term keeps four waves
    ((128, 56, 32, 32), "<24, 2, 256>/4", None, True),           # the four-wave, 24-slot form
    ((128, 96, 32, 32), "<24, 2, 256>/4", None, True),
    ((2, 1, 9, 14), "<12, 2, 256>/4", None, True),               # C = 1: every slot but one is a clamped duplicate
    ((2, 2, 9, 14), "<12, 2, 256>/4", None, True),
]


@pytest.mark.parametrize("xdt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("regime", ["offset", "wide"])
@pytest.mark.parametrize("shape,form,place,pairs_ok", _B_CASES,
                         ids=[f"{'x'.join(map(str, c[0]))}-{c[2].__name__ if c[2] else 'plain'}" for c in _B_CASES])
def test_every_launch_form_vs_float64(shape, form, place, pairs_ok, regime, xdt):
    _standalone("b", regime, shape, xdt, xdt, bias=True, gate=True, skip=True, place=place, pairs_possible=pairs_ok, form=form)


# ---- c. the backward with the channel gate folded into its load ----------------------------------------------------------------
@pytest.mark.parametrize("affine", ["mul", "add"], ids=["mul+add", "add"])
@pytest.mark.parametrize("regime", ["offset", "flat"])
@pytest.mark.parametrize("shape,form", [((2, 96, 9, 14), "<12, 2, 512>/8"), ((1, 600, 4, 6), "<0, 1, 1024>/16")], ids=["C96", "C600"])
def test_affine_backward_vs_float64(shape, form, regime, affine):
    """oss_ln_nchw_bwd_affine: the gradient dy (1 + dy_mul[b, c]) + dy_add[b, c] / (H W) formed on load, register-resident and
    streaming, as out_norm issues it (fp32 x, bf16 gate / dy)"""
    _standalone("c", regime, shape, F32, BF16, bias=True, gate=True, skip=False, affine=affine, form=form)


# ---- d. the LayerNorm stage of the fused forward -------------------------------------------------------------------------------
def _wg_pixels(B, K, P):
    """pixels per workgroup by shape (oss_conv1x1_wg.hip: wg_shape)"""
    t128 = B * (P // 128)
    return 64 if (K <= 48 and t128 < 1024) or t128 < 256 else 128


def _conv_weights(Cin, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(Cout, Cin, 1, 1, generator=g) * Cin ** -0.5, torch.randn(Cout, generator=g)


def _fused_forward(label, regime, dt, shape, Cout, bias, pts, seed=0):
    """ln_conv1x1_fwd at the pixel-tile sizes ``pts`` (0: by shape): n, mean, rstd against float64; y against the float64
    convolution of the kernel's OWN stored n with the weights rounded to the I/O type, so that each stage is measured on the
    inputs it actually had -> (inputs, the last call's outputs)"""
    B, Cin, H, W = shape
    P = H * W
    inp = lr.make_inputs(regime, B, Cin, P, dt, dt, seed, bias, dy=False)
    ref64, ref32 = lr.references(inp)
    wc, bc = _conv_weights(Cin, Cout, seed + 7)
    x, lw, lb = _dev(inp["x"], shape), _dev(inp["w"]), _dev(inp["b"])
    wd, bd = wc.to(DEV), bc.to(DEV)
    assert ops.ln_conv1x1_ok(x, wd)
    lib = _capi.load()
    out = None
    try:
        for pt in pts:
            lib.oss_conv1x1_set_wg(1, pt)
            out = torch.ops.vmambair.ln_conv1x1_fwd(x, lw, lb, wd, bd)
            torch.cuda.synchronize()
            y, n, mean, rstd = out
            tag = f"{label}:{regime} {'WithBias' if bias else 'BiasFree'} {B}x{Cin}->{Cout}x{H}x{W} pt={pt or _wg_pixels(B, Cin, P)}"
            lr.compare({"n": n, "mean": mean, "rstd": rstd}, ref64, ref32, (dt, dt), tag)
            c64, c32 = lr.conv_references(n.view(B, Cin, P), wc.view(Cout, Cin).to(dt), bc)
            lr.compare({"conv": y.view(B, Cout, P)}, c64, c32, (dt, dt), tag)
    finally:
        lib.oss_conv1x1_set_wg(1, 0)
    return inp, out


@pytest.mark.parametrize("Cout", [40, 254])                       # 254: eight row tiles over gridDim.z = 2
@pytest.mark.parametrize("Cin", [16, 32, 48, 64, 96, 128, 192])   # every built KS
@pytest.mark.parametrize("regime", ["offset", "flat", "wide", "outlier"])
@pytest.mark.parametrize("bias", [True, False], ids=["WithBias", "BiasFree"])
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_fused_forward_ln_stage_vs_float64(dt, bias, regime, Cin, Cout):
    _fused_forward("d", regime, dt, (2, Cin, 16, 16), Cout, bias, pts=(64, 128))


@pytest.mark.parametrize("dt,regime", [(BF16, "wide"), (F16, "offset")], ids=["bf16-wide", "f16-offset"])
def test_fused_forward_takes_128_pixel_tiles_by_shape(dt, regime):
    """the headline step's shape: 8 x 32 tiles of 128 pixels >= 256 and K = 96 > 48"""
    assert _wg_pixels(8, 96, 64 * 64) == 128
    _fused_forward("d", regime, dt, (8, 96, 64, 64), 40, True, pts=(0,))


# ---- e. the input gradient + LayerNorm backward in one launch ------------------------------------------------------------------
def _exact_dn(Cin, Cout, B, P, dt, seed):
    """conv weights in {-1, 0, 1} with 8 non-zeros per input channel and dy of integers in [-4, 4]: dn = W^T dy is an integer
    with |dn| <= 32, exact in bf16 and fp16 in any summation order, so the LayerNorm stage is what is measured"""
    g = torch.Generator().manual_seed(seed)
    w = torch.zeros(Cout, Cin)
    for k in range(Cin):
        rows = torch.randperm(Cout, generator=g)[:8]
        w[rows, k] = torch.where(torch.rand(8, generator=g) < 0.5, -1.0, 1.0)
    dy = torch.randint(-4, 5, (B, Cout, P), generator=g).float()
    dn = torch.einsum("mk,bmp->bkp", w.double(), dy.double())
    assert float(dn.abs().max()) <= 32 and torch.equal(dn.to(dt).double(), dn)
    return w.view(Cout, Cin, 1, 1), dy.to(dt), dn


_E_SHAPES = [(16, 32), (16, 48), (32, 64), (48, 96), (64, 128), (96, 192), (32, 96)]      # (Cin, Cout): KS = Cout / 16


@pytest.mark.parametrize("size", [(2, 16, 16), (32, 32, 32)], ids=["pt64", "pt128"])
@pytest.mark.parametrize("Cin,Cout", _E_SHAPES)
@pytest.mark.parametrize("regime", ["offset", "flat"])
@pytest.mark.parametrize("skip", [True, False], ids=["skip", "noskip"])
@pytest.mark.parametrize("bias", [True, False], ids=["WithBias", "BiasFree"])
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_fused_input_gradient_and_ln_backward_vs_float64(dt, bias, skip, regime, Cin, Cout, size, monkeypatch):
    """x, mean and rstd as the fused forward left them; the fused kernel (64-pixel tiles at 2 x 256 pixels, 128-pixel tiles at
    32 x 8 tiles of 128 = 256) and the two-kernel fallback on the same tensors, both against float64"""
    B, H, W = size
    P, shape = H * W, (size[0], Cin, H, W)
    inp = lr.make_inputs(regime, B, Cin, P, dt, dt, 0, bias, skip=skip, dy=False)
    wc, dy, dn = _exact_dn(Cin, Cout, B, P, dt, 11)
    inp["dy"] = dn
    ref64, ref32 = lr.references(inp)
    x, lw, lb, wd = _dev(inp["x"], shape), _dev(inp["w"]), _dev(inp["b"]), wc.to(DEV)
    y, n, mean, rstd = torch.ops.vmambair.ln_conv1x1_fwd(x, lw, lb, wd, None)
    lib = _capi.load()
    assert lib.oss_conv1x1_dgrad_ln_bwd_ok(_DT[dt], Cout, Cin, P, B), "the fused kernel does not take this shape"
    assert (B * (P // 128) >= 256) == (size[0] == 32)            # oss_conv1x1_wg.hip, lnbwd_launch: 128-pixel tiles from 256 on
    dyd, sk = _dev(dy, (B, Cout, H, W)), _dev(inp["skip"], shape)
    for fused in (True, False):
        monkeypatch.setattr(pointwise, "LN_BWD_FUSED", fused)
        dx, dlw, dlb, dw, db = torch.ops.vmambair.ln_conv1x1_bwd(x, lw, lb, n, mean, rstd, wd, dyd, sk, False)
        torch.cuda.synchronize()
        lr.compare({"dx": dx, "dw": dlw, "db": dlb if bias else None}, ref64, ref32, (dt, dt),
                   f"e:{regime} {'fused' if fused else 'two kernels'} {'WithBias' if bias else 'BiasFree'} skip={int(skip)} "
                   f"{B}x{Cin}<-{Cout}x{H}x{W}")
