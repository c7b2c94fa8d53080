"""The opt-in "high" precision mode of the fp32 GEMM-shaped products on the GPU (csrc/oss_conv1x1_f32x3.h; include/vmambair_oss.h
``OSS_F32_BF16X3``; ``vmambair_amd.set_float32_matmul_precision``): fp32 tensors, products on v_mfma_f32_32x32x16_bf16 with both
operands split into two bfloat16 numbers.  All inputs fp32, all references float64 torch.

1. exactness -- integer operands in [-4, 4] are bf16-exact (every lo is 0) and all sums stay below 2^24: "high" must equal the
   float64 product and "highest", bit for bit.  Catches every index, tail and operand-map error with no tolerance.
2. bound -- random operands: every output element within
       (3 * 2^-16 + (K + 2) * 2^-23) * sum_k |w_k||x_k|        (tests/test_f32_matmul_precision.py has the emulation)
   plus one fp32 rounding (2^-24 of the magnitudes involved) per epilogue addend / per partial of the weight gradient's slab sum;
   and for K >= 48 "high" is NOT bit-equal to "highest" (the route was taken).
3. an infinity and a NaN among the activations come out where "highest" puts them.
4. the selector is rejected by every entry point outside the six.
5. block and net fixtures of the reference under "high", at the limits tests/test_block_gpu.py uses for the exact path.
6. a hipGraph captured under "high" keeps the mode on replay.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

import vmambair_amd
from conftest import assert_close, load_golden
from vmambair_amd import _capi
from vmambair_amd.ops import core as core_ops
from vmambair_amd.ops import pointwise as pw

pytestmark = [pytest.mark.gpu, pytest.mark.tier(1)]   # one op against float64 PyTorch (and against the exact path of this repo)
DEV = "cuda:0"
U16, U23, U24 = 2.0 ** -16, 2.0 ** -23, 2.0 ** -24
high = functools.partial(vmambair_amd.float32_matmul_precision, "high")

# (B, Cin, Cout, H, W, bias + residual, channel-slice view)
CONV_CASES = {
    "p96":        (2, 48, 96, 8, 12, False, False),    # P = 96: less than one 128-pixel tile
    "ktail":      (1, 127, 48, 4, 8, False, False),    # K = 127: a half-empty last round of 16; the four-wave (split-K) form
    "mtail":      (1, 48, 254, 8, 8, False, False),    # M = 254: the last 32-row tile has 30 rows
    "longk":      (1, 510, 96, 8, 8, False, False),    # long K over four waves, few tiles
    "bias_res":   (1, 96, 48, 16, 16, True, False),    # bias and residual in the epilogue ...
    "view":       (2, 32, 40, 8, 8, True, True),       # ... and a channel-slice view: batch stride != C * P
    # one further shape per launch form of the dispatch.  Forward / input gradient (gemm_f32): 64-row tiles (>= 3072 waves, M > 32:
    # here M = 33, the second 32 rows of the tile hold ONE row), 32-row tiles one wave each (K < 64: p96, mtail, the input
    # gradients of ktail / bias_res), 32-row tiles with K over four waves (ktail, longk).  Weight gradient (rows_f32_wgrad):
    # 64 x 32 tiles (>= 1024 tiles, M > 32: here 64 images x 16 slabs) and 32 x 32 tiles (every other case).
    "wide_tiles": (64, 8, 33, 64, 128, True, False),
}


def _rand(shape, kind, gen):
    if kind == "int":
        return torch.randint(-4, 5, shape, generator=gen).float()
    t = torch.randn(shape, generator=gen)
    return t.abs() if kind == "pos" else t


@functools.lru_cache(maxsize=None)
def conv_case(name, kind):
    """inputs on the GPU and the float64 results, computed once per (shape, operand kind) and shared by the tests; read-only"""
    B, Cin, Cout, H, W, epi, view = CONV_CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name + kind)))
    scale = 1.0 if kind == "int" else Cin ** -0.5
    w = (_rand((Cout, Cin, 1, 1), kind, g) * scale).to(DEV)
    if view:
        big = _rand((B, 2 * Cin, H, W), kind, g).to(DEV)
        x = big[:, Cin // 2:Cin // 2 + Cin]
        assert not x.is_contiguous() and pw.f32_ok(x)
    else:
        x = _rand((B, Cin, H, W), kind, g).to(DEV)
    dy = _rand((B, Cout, H, W), kind, g).to(DEV)
    b = _rand((Cout,), kind, g).to(DEV) if epi else None
    res = _rand((B, Cout, H, W), kind, g).to(DEV) if epi else None
    x64, w64, dy64 = x.double(), w.double().view(Cout, Cin), dy.double()
    ref = {"y": torch.einsum("mk,bkhw->bmhw", w64, x64), "dx": torch.einsum("mk,bmhw->bkhw", w64, dy64),
           "dw": torch.einsum("bmhw,bkhw->mk", dy64, x64), "db": dy64.sum((0, 2, 3))}
    mag = {"y": torch.einsum("mk,bkhw->bmhw", w64.abs(), x64.abs()), "dx": torch.einsum("mk,bmhw->bkhw", w64.abs(), dy64.abs()),
           "dw": torch.einsum("bmhw,bkhw->mk", dy64.abs(), x64.abs()), "db": dy64.abs().sum((0, 2, 3))}
    if epi:
        ref["y"] = ref["y"] + b.double().view(1, -1, 1, 1) + res.double()
    return dict(x=x, w=w, dy=dy, b=b, res=res, ref=ref, mag=mag)


def run_conv(c):
    y = pw.conv1x1_fwd(c["x"], c["w"], c["b"], c["res"])
    dx, dw, db = pw.conv1x1_bwd(c["x"], c["w"], c["dy"], c["b"] is not None)
    torch.cuda.synchronize()
    return {"y": y, "dx": dx, "dw": dw.view(dw.shape[0], dw.shape[1]), "db": db}


def check_bound(got, ref, bound, what):
    err = (got.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"[f32 matmul high] {what}: worst error {ratio:.3f} of the bound")
    assert bool((err <= bound).all()), f"{what}: {ratio:.3f} of the bound"


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv1x1_high_is_bit_exact_on_integer_operands(name):
    c = conv_case(name, "int")
    with high():
        hi = run_conv(c)
    exact = run_conv(c)
    for k in ("y", "dx", "dw") + (("db",) if c["b"] is not None else ()):
        assert float(c["ref"][k].abs().max()) < 2 ** 24
        assert torch.equal(hi[k], c["ref"][k].float()), f"{name} {k}: high differs from the float64 product"
        assert torch.equal(hi[k], exact[k]), f"{name} {k}: high differs from highest"


# random normal operands at every shape, all-positive ones (no cancellation: the error terms add up) once per epilogue form
@pytest.mark.parametrize("name,kind", [(n, "normal") for n in CONV_CASES] + [("p96", "pos"), ("bias_res", "pos")])
def test_conv1x1_high_obeys_the_bound_and_takes_the_route(name, kind):
    B, Cin, Cout, H, W, epi, _ = CONV_CASES[name]
    P = H * W
    c = conv_case(name, kind)
    with high():
        hi = run_conv(c)
    exact = run_conv(c)
    mag = c["mag"]
    coef = lambda K: 3 * U16 + (K + 2) * U23   # noqa: E731
    # forward: K = Cin; the epilogue forms bias + residual, then accumulator + that: one rounding each
    by = coef(Cin) * mag["y"]
    if epi:
        by = by + 2 * U24 * (mag["y"] + c["b"].double().abs().view(1, -1, 1, 1) + c["res"].double().abs())
    check_bound(hi["y"], c["ref"]["y"], by, f"{name} {kind} y (K {Cin})")
    check_bound(hi["dx"], c["ref"]["dx"], coef(Cout) * mag["dx"], f"{name} {kind} dx (K {Cout})")
    # weight gradient: the bound holds per 512-pixel slab (K <= 512); the finishing sum then adds the B * slabs partial
    # products one after the other in fp32: (n - 1) roundings of at most 2^-24 of the magnitude so far (1 % for second order)
    nparts = B * ((P + 511) // 512)
    wcoef = coef(min(P, 512)) + 1.01 * (nparts - 1) * U24
    check_bound(hi["dw"], c["ref"]["dw"], wcoef * mag["dw"], f"{name} {kind} dw (K {min(P, 512)} x {nparts} partials)")
    if epi:
        check_bound(hi["db"], c["ref"]["db"], wcoef * mag["db"], f"{name} {kind} db")
    if Cin >= 48:
        assert not torch.equal(hi["y"], exact["y"]), "y: high is bit-equal to highest -- the split-bf16 route was not taken"
    if Cout >= 48:
        assert not torch.equal(hi["dx"], exact["dx"]), "dx: high is bit-equal to highest"
    if B * P >= 48:
        assert not torch.equal(hi["dw"], exact["dw"]), "dw: high is bit-equal to highest"


# ---- x_proj / dt_proj -----------------------------------------------------------------------------------------------------------
PROJ_CASES = {"d48": (2, 48, 35, 3, 64), "d96": (1, 96, 38, 6, 100)}   # (B, D, C, R, L): K tails 35 / 38 / 3 / 6, L = 100: a partial pixel tile


@functools.lru_cache(maxsize=None)
def proj_case(name, kind):
    B, D, Cc, R, L = PROJ_CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name + kind)))
    s = 1.0 if kind == "int" else 0.2
    t = lambda *shape: (_rand(shape, kind, g) * s).to(DEV)   # noqa: E731
    return dict(x2=t(B, 2, D, L), Wx=t(4, Cc, D), Wdt=t(4, D, R), ddts=t(B, 4 * D, L), dxdbl=t(B, 4, Cc, L), du=t(B, 4 * D, L),
                xdbl=t(B, 4, Cc, L))


def run_proj(c):
    """-> the kernels' outputs.  dts is the product of the kernel's OWN xdbl rows, dx2 of its OWN dt rows of dxdbl (returned too)."""
    xdbl, dts = core_ops.proj_fwd(c["x2"], c["Wx"], c["Wdt"])
    dxdbl = c["dxdbl"].clone()
    dx2 = core_ops.proj_dgrad(c["ddts"], dxdbl, c["du"], c["Wx"], c["Wdt"])
    R = c["Wdt"].shape[2]
    dwx, dwdt = core_ops.proj_wgrad(c["x2"], c["xdbl"], c["dxdbl"], c["ddts"], R)
    torch.cuda.synchronize()
    return dict(xdbl=xdbl, dts=dts, dxdbl=dxdbl, dx2=dx2, dwx=dwx, dwdt=dwdt)


def proj_refs(c, out, absolute=False):
    """float64 products (or, absolute: the sums of |w||x| of the same products) of the inputs the kernels read"""
    f = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
    B, _, D, L = c["x2"].shape
    Cc, R = c["Wx"].shape[1], c["Wdt"].shape[2]
    x2, Wx, Wdt = f(c["x2"]), f(c["Wx"]), f(c["Wdt"])
    r = {}
    r["xdbl"] = torch.einsum("kcd,bkdl->bkcl", Wx, x2[:, [0, 1, 0, 1]])
    r["dts"] = torch.einsum("kdr,bkrl->bkdl", Wdt, f(out["xdbl"])[:, :, :R]).reshape(B, 4 * D, L)
    ddts = f(c["ddts"]).view(B, 4, D, L)
    r["dt_rows"] = torch.einsum("kdr,bkdl->bkrl", Wdt, ddts)
    dz = f(out["dxdbl"])
    per_k = torch.einsum("kcd,bkcl->bkdl", Wx, dz)
    du = f(c["du"]).view(B, 4, D, L)
    r["dx2"] = (per_k[:, :2] + du[:, :2]) + (per_k[:, 2:] + du[:, 2:])
    r["dwx"] = torch.einsum("bkcl,bkdl->kcd", f(c["dxdbl"]), x2[:, [0, 1, 0, 1]])
    r["dwdt"] = torch.einsum("bkdl,bkrl->kdr", ddts, f(c["xdbl"])[:, :, :R])
    return r


@pytest.mark.parametrize("name", list(PROJ_CASES))
def test_proj_high_is_bit_exact_on_integer_operands(name):
    c = proj_case(name, "int")
    R = c["Wdt"].shape[2]
    with high():
        hi = run_proj(c)
    exact = run_proj(c)
    ref = proj_refs(c, hi)
    got = dict(hi, dt_rows=hi["dxdbl"][:, :, :R])
    for k, v in ref.items():
        assert float(v.abs().max()) < 2 ** 24
        assert torch.equal(got[k], v.float()), f"{name} {k}: high differs from the float64 product"
    for k in hi:
        assert torch.equal(hi[k], exact[k]), f"{name} {k}: high differs from highest"


@pytest.mark.parametrize("kind", ["normal", "pos"])
@pytest.mark.parametrize("name", list(PROJ_CASES))
def test_proj_high_obeys_the_bound_and_takes_the_route(name, kind):
    B, D, Cc, R, L = PROJ_CASES[name]
    c = proj_case(name, kind)
    with high():
        hi = run_proj(c)
    exact = run_proj(c)
    ref, mag = proj_refs(c, hi), proj_refs(c, hi, absolute=True)
    got = dict(hi, dt_rows=hi["dxdbl"][:, :, :R])
    coef = lambda K: 3 * U16 + (K + 2) * U23   # noqa: E731
    nparts = B * ((L + 511) // 512)
    wcoef = coef(min(L, 512)) + 1.01 * (nparts - 1) * U24
    # dx2: two passes of K = C, each adding its du rows (and the second the first's result) in the fp32 epilogue: four roundings
    bounds = {"xdbl": coef(D) * mag["xdbl"], "dts": coef(R) * mag["dts"], "dt_rows": coef(D) * mag["dt_rows"],
              "dx2": (coef(Cc) + 4 * U24) * mag["dx2"], "dwx": wcoef * mag["dwx"], "dwdt": wcoef * mag["dwdt"]}
    for k in bounds:
        check_bound(got[k], ref[k], bounds[k], f"proj {name} {kind} {k}")
    for k, K in (("xdbl", D), ("dt_rows", D), ("dwx", B * L), ("dwdt", B * L)):
        if K >= 48:
            ex = exact["dxdbl"][:, :, :R] if k == "dt_rows" else exact[k]
            assert not torch.equal(got[k], ex), f"{k}: high is bit-equal to highest -- the split-bf16 route was not taken"


# ---- non-finite values ------------------------------------------------------------------------------------------------------------
def test_infinity_and_nan_come_out_where_highest_puts_them():
    c = dict(conv_case("p96", "normal"))
    x = c["x"].clone()
    x[0, 5, 2, 3] = float("inf")
    x[1, 40, 7, 11] = float("nan")
    c["x"] = x
    with high():
        hi = run_conv(c)
    exact = run_conv(c)
    for k in ("y", "dw"):
        assert torch.equal(torch.isnan(hi[k]), torch.isnan(exact[k])), f"{k}: NaNs in other places than on the exact path"
        assert torch.equal(torch.isinf(hi[k]), torch.isinf(exact[k])), f"{k}: infinities in other places than on the exact path"
        inf = torch.isinf(exact[k])
        assert torch.equal(hi[k][inf], exact[k][inf]), f"{k}: an infinity of the other sign"
    assert bool(torch.isinf(exact["y"][0, :, 2, 3]).all()) and bool(torch.isnan(exact["y"][1, :, 7, 11]).all())
    assert int(torch.isinf(exact["y"]).sum()) == exact["y"].shape[1]


# ---- the selector belongs to six entry points -----------------------------------------------------------------------------------
def test_other_entry_points_reject_the_selector():
    lib = _capi.load()
    X3, F32 = _capi.OSS_F32_BF16X3, _capi.OSS_F32
    ERR_SHAPE = -2   # include/vmambair_oss.h: OSS_ERR_SHAPE, the entry points' answer to an I/O type they do not take
    B, Cn, H, W = 1, 8, 16, 16
    x = torch.randn(B, Cn, H, W, device=DEV)
    y = torch.full_like(x, 7.0)
    w9, wc = torch.randn(Cn, 9, device=DEV), torch.ones(Cn, device=DEV)
    mean, rstd = torch.zeros(B, H * W, device=DEV), torch.zeros(B, H * W, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    dw = lambda io: lib.oss_dwconv3x3_fwd(io, x.data_ptr(), w9.data_ptr(), None, y.data_ptr(), None, B, Cn, H, W, Cn * H * W, H * W,  # noqa: E731
                                          Cn * H * W, H * W, 0, s)
    ln = lambda xt, yt: lib.oss_ln_nchw_fwd(xt, yt, x.data_ptr(), wc.data_ptr(), None, None, y.data_ptr(), mean.data_ptr(),  # noqa: E731
                                            rstd.data_ptr(), B, Cn, H * W, Cn * H * W, H * W, 0, 0, 1e-5, s)
    assert dw(X3) == ERR_SHAPE and ln(X3, F32) == ERR_SHAPE and ln(F32, X3) == ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()), "a rejected call wrote its output"
    assert dw(F32) == 0 and ln(F32, F32) == 0   # the same arguments with a real element type are taken
    # the *_ok queries answer 0 (proj_rows_optional reads every value but OSS_F32 as a 16-bit type unless it is told otherwise)
    assert lib.oss_dwconv3x3_fused_ok(F32, 16, 16, 1) == 1 and lib.oss_dwconv3x3_fused_ok(X3, 16, 16, 1) == 0
    assert lib.oss_proj_rows_optional_ok(_capi.OSS_BF16, 1, 48, 35, 3, 64) == 1
    assert lib.oss_proj_rows_optional_ok(X3, 1, 48, 35, 3, 64) == 0
    assert lib.oss_scan_fused_dt_ok(X3, 1, 48, 35, 3, 16, 4096) == 0
    torch.cuda.synchronize()


# ---- block and net fixtures of the reference under "high" ----------------------------------------------------------------------
def _state(z):
    return {k[3:]: v for k, v in z.items() if k.startswith("sd.")}


def test_block_matches_reference_under_high():
    """the limits of tests/test_block_gpu.py for the exact path; the bound above (4.6e-5 of sum |w||x|) leaves ~20x below them"""
    from vmambair_amd.oss_block import MamberBlock
    z = load_golden("g3_block_srgan_mamber_d48.npz")
    m = MamberBlock(48, variant="srgan")
    m.load_state_dict(_state(z), strict=True)
    m.to(DEV)
    x = z["x"].to(DEV).requires_grad_()
    assert x.dtype == torch.float32
    with high():
        y = m(x)
        y.backward(z["dy"].to(DEV))
        torch.cuda.synchronize()
    assert_close(y, z["y"], 1e-3, 1e-3, "block output")
    assert_close(x.grad, z["dx"], 3e-3, 3e-3, "input grad")
    for k, p in m.named_parameters():
        ref = z["grad." + k]
        if k.endswith("conv_cout.bias"):
            continue  # exact gradient is 0 (constant before a LayerNorm); both sides return noise
        scale = max(1.0, float(ref.abs().max()))
        assert_close(p.grad, ref, 5e-3, 1e-3 * scale, f"grad {k}")


def test_net_matches_reference_under_high():
    from vmambair_amd.archs import MambaSISR6
    z = load_golden("g4_net_mambasisr6_d8.npz")
    net = MambaSISR6(dim=8, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1)
    net.load_state_dict(_state(z), strict=True)
    net.to(DEV)
    with torch.no_grad(), high():
        y = net(z["x"].to(DEV))
        exact_mode = vmambair_amd.get_float32_matmul_precision()
    assert exact_mode == "high" and vmambair_amd.get_float32_matmul_precision() == "highest"
    assert_close(y, z["y"], 1e-3, 1e-3, "net output")


# ---- a captured graph keeps the mode it was captured under --------------------------------------------------------------------
def test_captured_training_step_keeps_its_mode_on_replay():
    """GraphedTrainStep in fp32 (no autocast), captured under "high", replayed twice under "highest": the losses and a parameter
    equal two eager "high" steps bit for bit and differ from two eager "highest" steps.  (Two steps and a rate of 1e-2: the first
    Adam update is lr * g / (|g| + eps) = +-lr whatever the mode; from the second on the update depends on the ratio of the two
    gradients, whose relative difference between the modes (~1e-5) times the rate is above the parameters' last bit.)"""
    from vmambair_amd.archs import MambaSISR6
    from vmambair_amd.train_graph import GraphedTrainStep
    torch.manual_seed(30)
    net0 = MambaSISR6(dim=48, num_blocks=(1, 1, 1, 1), num_refinement_blocks=1, bias=False).to(DEV)
    g = torch.Generator().manual_seed(30)
    gt = torch.rand(2, 3, 128, 128, generator=g).to(DEV)
    lq = F.interpolate(gt, scale_factor=0.25, mode="area")
    name = "encoder_level1.0.attn.in_conv.weight" if "encoder_level1.0.attn.in_conv.weight" in dict(net0.named_parameters()) else \
        next(n for n, p in net0.named_parameters() if n.endswith("in_conv.weight"))

    def eager(mode):
        """two optimizer steps run eagerly: the step's own forward + backward + optimizer, as its warm-up runs them"""
        step = GraphedTrainStep(copy.deepcopy(net0), lr=1e-2, autocast_dtype=None, warmup=1)
        step.static_lq, step.static_gt = lq.clone(), gt.clone()
        losses = []
        with vmambair_amd.float32_matmul_precision(mode):
            for _ in range(2):
                losses.append(step._fwd_bwd().clone())
                step._opt_ema()
                torch.cuda.synchronize()
        return torch.stack(losses), dict(step.net.named_parameters())[name].detach().clone()

    step = GraphedTrainStep(copy.deepcopy(net0), lr=1e-2, autocast_dtype=None, warmup=1)
    with high():
        step.capture(lq, gt)
    assert vmambair_amd.get_float32_matmul_precision() == "highest"
    losses = torch.stack([step(lq, gt).clone() for _ in range(2)])
    torch.cuda.synchronize()
    param = dict(step.net.named_parameters())[name].detach().clone()
    loss_high, param_high = eager("high")
    loss_exact, param_exact = eager("highest")
    print(f"[f32 matmul high] captured step: losses {losses.tolist()}, eager high {loss_high.tolist()}, eager highest {loss_exact.tolist()}")
    assert torch.isfinite(losses).all()
    assert torch.equal(losses, loss_high), "the replayed graph did not keep the mode it was captured under"
    assert torch.equal(param, param_high), f"{name}: replay under highest differs from two eager high steps"
    assert not torch.equal(losses, loss_exact), "the losses equal the exact mode's"
    assert not torch.equal(param, param_exact), f"{name}: equals two eager highest steps"
