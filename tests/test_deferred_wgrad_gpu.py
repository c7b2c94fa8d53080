"""The deferred forms of the backward's reductions -- what a training step inside ``ops.deferred_finishes()`` runs -- against
float64 references of the same operations:

* the grouped weight-gradient launch (``oss_flush_wgrads`` -> ``oss_conv1x1_wgrad_grouped_kernel``) for the 1x1 product and the two
  projection products, at the pixel counts where ``wgrad_body`` changes path inside ONE partial product (several LDS-staged
  512-pixel pieces, then 64-pixel steps, then a 16-pixel tail), in both 16-bit I/O types and at spans 1 / 4 / 64;
* ``oss_sum_partials_kernel`` (``oss_flush_finishes``) on partial vectors the test writes itself: K below / at / above its groups
  of 16, the 16-byte and the scalar path, chunks at the dw / db boundary;
* every other registered reduction (LayerNorm, depth-wise convolution, thin 3x3, channel branch, fused dgrad + LN backward) run
  deferred, against the reference and the tolerances of that op's own kernel test;
* the tables: partial flushes, tables that are too small, two I/O types in one flush.

Two kinds of input.  INTEGER operands in {-3 .. 3}: every product is an integer of magnitude <= 9 and with B * P <= 1e5 terms every
partial and final sum stays below 2^24, so ANY fp32 summation order (MFMA accumulation included) is exact and the result must EQUAL
the float64 contraction -- one dropped, doubled or misplaced pixel, slab, span or output element fails.  RANDOM operands (unit
normal, rounded to the I/O type): the limit is measured, not chosen: ``e32`` = the Frobenius error of the same contraction done in
plain float32 on the CPU (``torch.einsum``: an unrelated summation order), and the kernel's error must stay within ``4 * e32``
(three fp32 blockings of 7800 terms differ by less than 1.5 x among themselves; one lost pixel is four orders of magnitude more).
The measured ratio is printed (``pytest -s`` / the captured output of a failure)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close
from vmambair_amd import _capi, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
IO = [torch.bfloat16, torch.float16]
IO_IDS = ["bf16", "f16"]


def _lib():
    return _capi.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _restore_span():
    _lib().oss_conv1x1_wgrad_set_span(4)   # the library's start value


def _flush():
    """the recorded products as one grouped launch, then every registered sum as one launch (inside the open context)"""
    wt = ft = None
    if ops.pending_wgrads():
        wt = ops.WgradTable(DEV, ops.pending_wgrad_table_bytes())
        ops.flush_wgrads(wt)
    assert ops.pending_wgrads() == 0
    if ops.pending_finish_chunks():
        ft = ops.FinishTable(DEV, ops.pending_finish_chunks())
        ops.flush_finishes(ft)
    assert ops.pending_finish_chunks() == 0
    torch.cuda.synchronize()   # the pinned tables stay alive until their copies have run


def _draw(shape, kind, dt, gen):
    if kind == "int":
        return torch.randint(-3, 4, shape, generator=gen).to(dt)   # exact in bf16 / f16 / fp32
    return torch.randn(shape, generator=gen).to(dt)


def _exact(got, ref, what):
    got = got.double().cpu()
    assert got.shape == ref.shape, what
    if not torch.equal(got, ref):
        bad = (got != ref) | got.isnan()
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())}/{ref.numel()} elements differ from the exact sum; first at flat index {i}: "
                             f"got {got.flatten()[i].item()}, want {ref.flatten()[i].item()}")


def _within_fp32_roundoff(got, ref64, cpu32, what):
    """``||got - ref64||_F <= 4 ||cpu32 - ref64||_F`` and no NaN; prints the measured ratio"""
    got = got.double().cpu()
    assert got.shape == ref64.shape, what
    assert not bool(got.isnan().any()), f"{what}: {int(got.isnan().sum())} NaN (an element nobody wrote, or a partial nobody wrote)"
    e32 = float((cpu32.double() - ref64).norm())
    err = float((got - ref64).norm())
    print(f"[{what}] |got - ref64|_F = {err:.3e}, e32 = {e32:.3e}, ratio = {err / e32 if e32 > 0 else (0.0 if err == 0 else float('inf')):.3f}")
    assert err <= 4.0 * e32, f"{what}: |got - ref64|_F = {err:.3e} > 4 e32 = {4 * e32:.3e}"


def _check(kind, got, ref64, cpu32, what):
    if kind == "int":
        _exact(got, ref64, what)
    else:
        _within_fp32_roundoff(got, ref64, cpu32, what)


def _same_up_to_order(got, want, what):
    """the project's "same up to the summation order" limit (test_conv1x1_wgrad_tiles_per_wave)"""
    assert_close(got, want, 1e-5, 1e-5 * max(1.0, float(want.abs().max())), what)


# =====================================================================================================================
# A. the grouped 1x1 product at kernel level
# =====================================================================================================================
# (B, Cout, Cin, H, W): each the smallest shape that reaches the named edge of wgrad_body / defer_sum
WGRAD_SHAPES = [
    (3, 33, 193, 8, 325),   # P = 2600, 16-byte rows: span 4 = four staged pieces | one staged piece + 40-pixel tail; K % 4 != 0 weights,
                            # ragged row tile, B > 1 (partial index with the reduced slab count), pvec = 6402 (scalar finishing path)
    (2, 48, 96, 41, 50),    # P = 2050, P % 8 != 0: element-wise loads everywhere, spans 2048 + 2, the bias column alone in a 4th column tile,
                            # pvec and nw multiples of 4 (vector finishing path, several 1024-chunks)
    (1, 8, 32, 8, 125),     # P = 1000 < one span: one staged piece, seven 64-pixel steps, 40-pixel tail
    (2, 97, 127, 64, 64),   # two full spans; M = three tiles + one row; K % 4 != 0
    (1, 40, 64, 8, 576),    # P = 4608: the third span is exactly one staged piece
    (5, 7, 5, 3, 5),        # everything smaller than one tile and one k-step
]


@functools.lru_cache(maxsize=None)
def _wgrad_case(shape, dt, kind):
    """operands (CPU, I/O type), the float64 contraction and the same contraction in plain float32 -- computed once per
    (shape, type, kind) and shared by every span / bias / form that uses it.  The bias gradient is the column of an all-ones row
    appended to x (what the kernel does), so both references come out of ONE contraction."""
    B, Cout, Cin, H, W = shape
    gen = torch.Generator().manual_seed(1000 + 7 * WGRAD_SHAPES.index(shape) + (1 if kind == "int" else 0))
    dy = _draw((B, Cout, H * W), kind, dt, gen)
    x = _draw((B, Cin, H * W), kind, dt, gen)
    x1 = torch.cat([x.float(), torch.ones(B, 1, H * W)], dim=1)
    ref64 = torch.einsum("bmp,bnp->mn", dy.double(), x1.double())
    cpu32 = torch.einsum("bmp,bnp->mn", dy.float(), x1)
    return dy, x, ref64, cpu32


def _wgrad_call(dt, dy, x, has_bias):
    """``oss_conv1x1_wgrad`` on buffers the test owns, all pre-filled with NaN: an output element or a partial vector that is read
    but was never written shows up as NaN.  dy (B, Cout, P), x (B, Cin, P): pixel-contiguous views with any batch / channel stride"""
    lib = _lib()
    B, Cout, P = dy.shape
    Cin = x.shape[1]
    assert dy.stride(2) == 1 and x.stride(2) == 1
    dw = torch.full((Cout, Cin), NAN, device=DEV)
    db = torch.full((Cout,), NAN, device=DEV) if has_bias else None
    part = torch.full((int(lib.oss_conv1x1_wgrad_partial_floats(B, Cout, Cin, P)),), NAN, device=DEV)
    _capi.check(lib.oss_conv1x1_wgrad(ops._DT[dt], dy.data_ptr(), x.data_ptr(), dw.data_ptr(), ops._ptr(db), part.data_ptr(), B, Cout, Cin,
                                      P, dy.stride(0), dy.stride(1), x.stride(0), x.stride(1), _stream()), "oss_conv1x1_wgrad")
    return dw, db, part


def _wgrad_both_forms(dt, dy, x, has_bias):
    """-> ((dw, db) one launch + its own finishing kernel, (dw, db) recorded + grouped launch + deferred sum)"""
    now = _wgrad_call(dt, dy, x, has_bias)
    torch.cuda.synchronize()
    with ops.deferred_finishes(wgrads=True):
        rec = _wgrad_call(dt, dy, x, has_bias)
        assert ops.pending_wgrads() == 1, "a 16-bit product inside deferred_finishes(wgrads=True) is recorded, not launched"
        _flush()
    return now[:2], rec[:2]


def _check_wgrad(kind, got, ref64, cpu32, Cin, what):
    """integer operands: dw and db each equal the exact sums; random operands: the 4 * e32 rule on the product as the kernel forms it,
    ONE (Cout, Cin + 1) matrix whose last column is db (seven bias sums alone are too few roundings to be a statistic)"""
    dw, db = got
    if kind == "int":
        _exact(dw, ref64[:, :Cin], what + " dw")
        if db is not None:
            _exact(db, ref64[:, Cin], what + " db")
    elif db is None:
        _within_fp32_roundoff(dw, ref64[:, :Cin], cpu32[:, :Cin], what + " dw")
    else:
        _within_fp32_roundoff(torch.cat([dw, db[:, None]], dim=1), ref64, cpu32, what + " dw|db")


@pytest.mark.parametrize("span", [1, 4, 64])
@pytest.mark.parametrize("has_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", IO, ids=IO_IDS)
def test_grouped_1x1_product_vs_float64(dt, shape, has_bias, span):
    """``oss_conv1x1_wgrad`` as one launch with its own finishing kernel, and recorded -> ``oss_flush_wgrads`` -> ``oss_flush_finishes``,
    on the same operands: both forms against the float64 contraction, at every span"""
    Cin = shape[2]
    try:
        _lib().oss_conv1x1_wgrad_set_span(span)
        for kind in ("int", "randn"):
            dy, x, ref64, cpu32 = _wgrad_case(shape, dt, kind)
            now, rec = _wgrad_both_forms(dt, dy.to(DEV), x.to(DEV), has_bias)
            _check_wgrad(kind, now, ref64, cpu32, Cin, f"{kind} one-launch")
            _check_wgrad(kind, rec, ref64, cpu32, Cin, f"{kind} grouped span {span}")
            if span == 1:   # include/vmambair_oss.h: span 1 reproduces the one-problem launches bit for bit
                assert torch.equal(now[0], rec[0]), "dw: grouped launch at span 1 != one launch per product"
                assert has_bias is False or torch.equal(now[1], rec[1]), "db: grouped launch at span 1 != one launch per product"
    finally:
        _restore_span()


@pytest.mark.parametrize("shape", WGRAD_SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", IO, ids=IO_IDS)
def test_grouped_1x1_product_on_channel_strided_operands(dt, shape):
    """x and dy are the middle channels of wider buffers (what ``chunk(2, dim=1)`` hands the block's convolutions): the real batch
    and channel strides go to the kernel; the rest of the buffers holds NaN, so a row read from outside the view poisons the result"""
    B, Cout, Cin, H, W = shape
    P = H * W
    for kind in ("int", "randn"):
        dy, x, ref64, cpu32 = _wgrad_case(shape, dt, kind)
        dy_big = torch.full((B, Cout + 5, P), NAN, dtype=dt, device=DEV)
        x_big = torch.full((B, Cin + 8, P), NAN, dtype=dt, device=DEV)
        dyv, xv = dy_big[:, 3:3 + Cout], x_big[:, 5:5 + Cin]
        dyv.copy_(dy)
        xv.copy_(x)
        assert dyv.stride(0) == (Cout + 5) * P and xv.stride(0) == (Cin + 8) * P
        now, rec = _wgrad_both_forms(dt, dyv, xv, True)
        _check_wgrad(kind, now, ref64, cpu32, Cin, f"{kind} strided one-launch")
        _check_wgrad(kind, rec, ref64, cpu32, Cin, f"{kind} strided grouped")


# =====================================================================================================================
# B. oss_sum_partials_kernel on partials the test chooses
# =====================================================================================================================
SUM_SHAPES = [   # (Cout, Cin, bias)
    (3, 5, True),       # pvec 18, nw 15: the db chunk starts unaligned
    (32, 33, True),     # nw = 1056 = 1024 + 32, db in a chunk of its own, everything aligned
    (4, 1025, False),   # four full chunks + a chunk of 4
    (5, 41, False),     # odd stride
    (1, 1, True),
    (2, 1027, False),   # the last chunk ends in a partial quad: one lane on the scalar path beside vector lanes
]


@pytest.mark.parametrize("K", [1, 2, 15, 16, 17, 31, 33, 48])
@pytest.mark.parametrize("Cout,Cin,has_bias", SUM_SHAPES, ids=[f"{c}x{n}{'b' if b else ''}" for c, n, b in SUM_SHAPES])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_finishing_sum_of_chosen_partials(dt, Cout, Cin, has_bias, K):
    """``oss_conv1x1_wgrad`` with one 8-pixel slab per image and batch = K runs its product at once (wgrads=False; an fp32 product
    is never recorded anyway) and registers the finishing sum; the test then REPLACES the partials before the flush.
    Layout (conv1x1_wgrad / rows_f32_wgrad: ``defer_sum(part, slabs * B, pvec, pvec, dw, nw, db)`` with slabs = 1): K vectors of
    pvec = Cout Cin (+ Cout) floats at stride pvec; outputs j < nw = Cout Cin go to dw, the rest to db, in chunks of <= 1024 that do
    not straddle that boundary."""
    lib = _lib()
    P = 8
    nw = Cout * Cin
    pvec = nw + (Cout if has_bias else 0)
    x = torch.zeros(K, Cin, P, dtype=dt, device=DEV)
    dy = torch.zeros(K, Cout, P, dtype=dt, device=DEV)
    gen = torch.Generator().manual_seed(2000 + 64 * K + pvec % 61)

    def finish(vals):
        dw = torch.full((Cout, Cin), NAN, device=DEV)
        db = torch.full((Cout,), NAN, device=DEV) if has_bias else None
        n_part = int(lib.oss_conv1x1_wgrad_partial_floats(K, Cout, Cin, P))
        assert n_part >= K * pvec
        part = torch.full((n_part,), NAN, device=DEV)
        with ops.deferred_finishes(wgrads=False):
            _capi.check(lib.oss_conv1x1_wgrad(ops._DT[dt], dy.data_ptr(), x.data_ptr(), dw.data_ptr(), ops._ptr(db), part.data_ptr(), K, Cout,
                                              Cin, P, dy.stride(0), dy.stride(1), x.stride(0), x.stride(1), _stream()), "oss_conv1x1_wgrad")
            assert ops.pending_wgrads() == 0
            assert ops.pending_finish_chunks() == (nw + 1023) // 1024 + (1 if has_bias else 0)
            part[:K * pvec].copy_(vals.flatten())   # stream order: after the product kernel that wrote (zeros) here
            _flush()
        return (dw.flatten() if db is None else torch.cat([dw.flatten(), db])).cpu()

    ints = torch.randint(-1000, 1001, (K, pvec), generator=gen).float()
    _exact(finish(ints), ints.double().sum(0), f"int K={K} pvec={pvec}")
    # random partials, magnitudes 2^-10 .. 2^10.  The 4 * e32 rule compares two sums of round-off, so it needs enough of them: an
    # output vector of 2 or 18 elements is drawn (and summed on the GPU) several times and the rule applied to all draws together
    # (at K = 17, pvec = 2 the plain CPU sum of one draw happens to be ten times more accurate than a faithful float32 emulation of
    # this kernel's order -- two samples are no estimate of a round-off level)
    got, ref64, cpu32 = [], [], []
    for _ in range((63 + pvec) // pvec if pvec < 64 else 1):
        vals = torch.randn(K, pvec, generator=gen) * torch.exp2(torch.rand(K, pvec, generator=gen) * 20.0 - 10.0)
        got.append(finish(vals))
        ref64.append(vals.double().sum(0))
        cpu32.append(vals.sum(0))
    _within_fp32_roundoff(torch.cat(got), torch.cat(ref64), torch.cat(cpu32), f"randn K={K} pvec={pvec}")


# =====================================================================================================================
# C. the projection products through the grouped launch
# =====================================================================================================================
PROJ_SHAPES = [(2, 12, 16, 3, 2600), (3, 5, 4, 1, 2050), (1, 48, 1, 3, 1000)]   # (B, D, N, R, L)


@functools.lru_cache(maxsize=None)
def _proj_case(shape, dt, kind):
    B, D, N, R, L = shape
    Cc = R + 2 * N
    gen = torch.Generator().manual_seed(3000 + 7 * PROJ_SHAPES.index(shape) + (1 if kind == "int" else 0))
    x2 = _draw((B, 2, D, L), kind, dt, gen)
    xdbl = _draw((B, 4, Cc, L), kind, dt, gen)
    dxdbl = _draw((B, 4, Cc, L), kind, dt, gen)
    ddts = _draw((B, 4 * D, L), kind, dt, gen)
    refs = []
    for cast in (torch.double, torch.float32):   # the two einsums ops.core.proj_wgrad spells out for its fallback
        dz = dxdbl.to(cast).view(B, 2, 2, Cc, L)   # [b, kk, j]: direction k = j + 2 kk
        dwx = torch.einsum("bhjcl,bjdl->hjcd", dz, x2.to(cast)).reshape(4, Cc, D)
        dwdt = torch.einsum("bkdl,bkrl->kdr", ddts.to(cast).view(B, 4, D, L), xdbl.to(cast)[:, :, :R])
        refs.append((dwx, dwdt))
    return (x2, xdbl, dxdbl, ddts), refs[0], refs[1]


def _check_proj(dt, shape, with_ddts, span):
    R = shape[3]
    try:
        if span is not None:
            _lib().oss_conv1x1_wgrad_set_span(span)
        for kind in ("int", "randn"):
            (x2, xdbl, dxdbl, ddts), ref64, cpu32 = _proj_case(shape, dt, kind)
            x2, xdbl, dxdbl = x2.to(DEV), xdbl.to(DEV), dxdbl.to(DEV)
            ddts = ddts.to(DEV) if with_ddts else None
            now = ops.core.proj_wgrad(x2, xdbl, dxdbl, ddts, R)
            torch.cuda.synchronize()
            with ops.deferred_finishes(wgrads=True):
                rec = ops.core.proj_wgrad(x2, xdbl, dxdbl, ddts, R)
                assert ops.pending_wgrads() == (2 if with_ddts else 1)
                _flush()
            assert (rec[1] is None) == (not with_ddts)
            for form, got in (("one-launch", now), ("grouped", rec)):
                _check(kind, got[0], ref64[0], cpu32[0], f"{kind} {form} dx_proj_weight")
                if with_ddts:
                    _check(kind, got[1], ref64[1], cpu32[1], f"{kind} {form} ddt_projs_weight")
            if span == 1:
                assert torch.equal(now[0], rec[0]) and (not with_ddts or torch.equal(now[1], rec[1])), "span 1 != one launch per product"
    finally:
        _restore_span()


@pytest.mark.parametrize("span", [None, 1], ids=["span-default", "span1"])
@pytest.mark.parametrize("shape", PROJ_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", IO, ids=IO_IDS)
def test_projection_products_through_the_grouped_launch(dt, shape, span):
    """x_proj (G = 2 problems whose 2 C rows come from two places: ``Mh`` / ``gs_hi``) and dt_proj (G = 4), against the two float64
    einsums ``ops.core.proj_wgrad`` spells out for its fallback"""
    _check_proj(dt, shape, True, span)


def test_projection_x_proj_product_alone_without_ddts():
    """``ddts=None`` (the fused-delta scan backward made the dt_proj gradient itself): only the x_proj product is recorded"""
    _check_proj(torch.bfloat16, PROJ_SHAPES[0], False, None)


# =====================================================================================================================
# D. every other registered reduction, deferred
# =====================================================================================================================
def ln_ref(x, w, b, gate):
    """the reference's LayerNorm (MambaSISR6_arch.py:144-195), as tests/test_glue_gpu.py states it"""
    xf = x.float().permute(0, 2, 3, 1)
    sig = xf.var(-1, keepdim=True, unbiased=False)
    if b is not None:
        y = (xf - xf.mean(-1, keepdim=True)) / torch.sqrt(sig + 1e-5) * w + b
    else:
        y = xf / torch.sqrt(sig + 1e-5) * w
    y = y.permute(0, 3, 1, 2)
    return y if gate is None else y * F.silu(gate.float())


def _twice(run, leaves_of=None):
    """``run()`` -> tuple of parameter gradients, once immediately and once inside deferred_finishes() + flush.  ``leaves_of``:
    run() went through an autograd Function with fresh leaves -- every deferred output must have been ADOPTED as a leaf's .grad"""
    now = run()
    torch.cuda.synchronize()
    now = [None if t is None else t.clone() for t in now]
    with ops.deferred_finishes():
        got = run()
        assert ops.pending_finish_chunks() > 0, "nothing was registered: the op did not defer its reduction"
        if leaves_of is not None:
            assert ops.orphaned_deferred_outputs(leaves_of()) == 0
        _flush()
    return now, got


@pytest.mark.parametrize("shape", [(2, 7, 3, 5), (2, 768, 8, 8), (1, 100, 16, 16)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
def test_layernorm_parameter_gradients_deferred(shape, dt, with_bias):
    """limits of test_layernorm_nchw"""
    torch.manual_seed(0)
    B, C, H, W = shape
    x = (torch.randn(shape) * 2 + 0.5).to(dt)
    w = torch.randn(C) * 0.5 + 1
    b = torch.randn(C) if with_bias else None
    dy = torch.randn(shape).to(dt)
    wr = w.clone().requires_grad_()
    br = b.clone().requires_grad_() if with_bias else None
    ln_ref(x, wr, br, None).backward(dy.float())
    xd, dyd = x.to(DEV), dy.to(DEV)
    leaves = []

    def run():
        leaves[:] = [w.to(DEV).requires_grad_()] + ([b.to(DEV).requires_grad_()] if with_bias else [])
        ops.layer_norm_nchw(xd, leaves[0], leaves[1] if with_bias else None, None, dt).backward(dyd)
        return [p.grad for p in leaves]

    now, got = _twice(run, lambda: leaves)
    lo = dt == torch.float32
    for g, n, r, name in zip(got, now, [wr.grad] + ([br.grad] if with_bias else []), ("dw", "db")):
        assert_close(g, r, 1e-3 if lo else 3e-2, (1e-4 if lo else 2e-2) * max(1.0, float(r.abs().max())), name)
        _same_up_to_order(g, n, name + " deferred vs immediate")


@pytest.mark.parametrize("with_mul", [True, False], ids=["mul", "nomul"])
def test_layernorm_with_the_channel_gate_folded_in_deferred(with_mul):
    """``oss_ln_nchw_bwd_affine`` (dy * (1 + mul) + s * add formed on load): reference and limits of
    test_layernorm_backward_with_the_channel_gate_folded_into_its_load"""
    torch.manual_seed(21)
    shape = (3, 48, 16, 24)
    B, C, H, W = shape
    x = torch.randn(shape, device=DEV)
    w, b = torch.randn(C, device=DEV), torch.randn(C, device=DEV)
    gate = torch.randn(shape, device=DEV).to(torch.bfloat16)
    dy = torch.randn(shape, device=DEV).to(torch.bfloat16)
    mul = torch.randn(B, C, device=DEV) * 0.3 if with_mul else None
    add = torch.randn(B, C, device=DEV)
    scale = 1.0 / (H * W)
    _, mean, rstd = ops.ln_nchw_fwd(x, w, b, gate, 2)
    dy_eff = dy.float() * ((1.0 + mul)[:, :, None, None] if with_mul else 1.0) + scale * add[:, :, None, None]
    xr, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    yr = (xr - xr.mean(1, keepdim=True)) * (xr.var(1, keepdim=True, unbiased=False) + 1e-5).rsqrt() * wr.view(1, -1, 1, 1) + br.view(1, -1, 1, 1)
    (yr * F.silu(gate.float())).backward(dy_eff)
    now, got = _twice(lambda: torch.ops.vmambair.ln_nchw_bwd(x, w, b, gate, dy, mean, rstd, None, None, mul, add, scale)[2:])
    for g, n, r, name in zip(got, now, (wr.grad, br.grad), ("dw", "db")):
        assert_close(g, r, 2e-3, 2e-3 * float(r.abs().max()), name)
        _same_up_to_order(g, n, name + " deferred vs immediate")


def _dw_ref(x, w, b, dy, act, cast=torch.float32):
    xx, ww = x.to(cast).cpu(), w.to(cast).cpu().requires_grad_()
    bb = None if b is None else b.to(cast).cpu().requires_grad_()
    y = F.conv2d(xx, ww, bb, padding=1, groups=xx.shape[1])
    (F.silu(y) if act else y).backward(dy.to(cast).cpu())
    return ww.grad, None if bb is None else bb.grad


DW_SHAPE = (17, 5, 7, 9)   # K = 17 partial vectors, stride 50, the db chunk starts at 45


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_depthwise_conv_parameter_gradients_deferred(dt):
    """plain depth-wise convolution (``oss_dwconv3x3_wgrad``): limits of test_dwconv_matches_torch; the weight gradient is linear in
    both operands, so integer operands must give the exact sums"""
    B, C, H, W = DW_SHAPE
    gen = torch.Generator().manual_seed(41)
    w, b = torch.randn(C, 1, 3, 3, generator=gen) * 0.3, torch.randn(C, generator=gen)
    for kind in ("int", "randn"):
        x, dy = _draw(DW_SHAPE, kind, dt, gen), _draw(DW_SHAPE, kind, dt, gen)
        xd, dyd = x.to(DEV), dy.to(DEV)
        leaves = []

        def run():
            leaves[:] = [w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()]
            ops.DWConv3x3Fn.apply(xd, leaves[0], leaves[1]).backward(dyd)
            return [p.grad for p in leaves]

        now, got = _twice(run, lambda: leaves)
        if kind == "int":
            for grads, form in ((now, "immediate"), (got, "deferred")):
                for g, r, name in zip(grads, _dw_ref(x, w, b, dy, False, torch.double), ("dw", "db")):
                    _exact(g, r, f"{form} {name}")
            continue
        lo = dt == torch.float32
        for g, n, r, name in zip(got, now, _dw_ref(x, w, b, dy, False), ("dw", "db")):
            assert_close(g, r, 1e-4 if lo else 2e-2, (1e-5 if lo else 5e-3) * max(float(r.abs().max()), 1.0), name)
            _same_up_to_order(g, n, name + " deferred vs immediate")


@pytest.mark.parametrize("form,shape", [("silu", (17, 5, 7, 16)), ("flat2", (17, 5, 8, 8))])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_fused_depthwise_conv_silu_backward_deferred(form, shape, dt):
    """the one-launch backward of silu(conv(x)) and its flat2 form (the merge of the two flattenings' gradients in its load): reference
    and limits of test_fused_conv_silu_one_launch_backward (the flat2 form on the merged, I/O-rounded gradient ``cross_merge2`` gives)"""
    torch.manual_seed(11)
    B, C, H, W = shape
    x = torch.randn(shape, device=DEV).to(dt)
    w, b = torch.randn(C, 1, 3, 3, device=DEV) * 0.3, torch.randn(C, device=DEV) * 0.1
    assert ops.dwconv.fused_ok(x, 1) and (form != "flat2" or ops.flat2_ok(x))
    if form == "flat2":
        g2 = torch.randn(B, 2, C, H * W, device=DEV).to(dt)
        dy = ops.cross_merge2(g2, H, W)
        run = lambda: torch.ops.vmambair.dwconv3x3_silu_flat2_bwd(x, w, b, g2, None)[1:]   # noqa: E731
    else:
        dy = torch.randn(shape, device=DEV).to(dt)
        run = lambda: torch.ops.vmambair.dwconv3x3_silu_bwd(x, w, b, dy, None)[1:]   # noqa: E731
    now, got = _twice(run)
    rt = {torch.bfloat16: 1e-2, torch.float32: 1e-4}[dt]
    for g, n, r, name in zip(got, now, _dw_ref(x, w, b, dy, True), ("dw", "db")):
        assert_close(g, r, 2 * rt, 2 * rt * float(r.abs().max()), name)
        _same_up_to_order(g, n, name + " deferred vs immediate")


def _thin_ref(x, w, b, dy, cast=torch.float32):
    ww = w.to(cast).requires_grad_()
    bb = None if b is None else b.to(cast).requires_grad_()
    F.conv2d(x.to(cast), ww, bb, padding=1).backward(dy.to(cast))
    return [ww.grad] + ([] if bb is None else [bb.grad])


@pytest.mark.parametrize("shape,cout,has_bias", [((17, 5, 3, 8), 1, True), ((17, 1, 3, 8), 5, False)], ids=["5to1", "1to5"])
@pytest.mark.parametrize("dt", IO, ids=IO_IDS)
def test_thin_conv3x3_parameter_gradients_deferred(shape, cout, has_bias, dt):
    """one partial vector per image, K = 17: limits of test_thin_conv_matches_torch; linear, so integer operands give the exact sums"""
    B, Cin, H, W = shape
    gen = torch.Generator().manual_seed(51)
    w = torch.randn(cout, Cin, 3, 3, generator=gen) / (3.0 * Cin ** 0.5)
    b = torch.randn(cout, generator=gen) * 0.1 if has_bias else None
    for kind in ("int", "randn"):
        x, dy = _draw(shape, kind, dt, gen), _draw((B, cout, H, W), kind, dt, gen)
        xd, dyd = x.to(DEV), dy.to(DEV)
        leaves = []

        def run():
            leaves[:] = [w.to(DEV).requires_grad_()] + ([b.to(DEV).requires_grad_()] if has_bias else [])
            assert ops.conv3x3.thin_ok(xd, leaves[0])
            ops.ThinConv3x3Fn.apply(xd, leaves[0], leaves[1] if has_bias else None).backward(dyd)
            return [p.grad for p in leaves]

        now, got = _twice(run, lambda: leaves)
        if kind == "int":
            for grads, form in ((now, "immediate"), (got, "deferred")):
                for g, r, name in zip(grads, _thin_ref(x, w, b, dy, torch.double), ("dw", "db")):
                    _exact(g, r, f"{form} {name}")
            continue
        for g, n, r, name in zip(got, now, _thin_ref(x, w, b, dy), ("dw", "db")):
            assert_close(g, r, 2e-4, 2e-4 * float(r.abs().max()) + 1e-6, name)
            _same_up_to_order(g, n, name + " deferred vs immediate")


_CHAN_NAMES = ["conv_cin.weight", "conv_cin.bias", "xc_proj_weight", "dtc_projs_weight", "dtc_projs_bias", "Ac_logs", "Dsc",
               "conv_cout.weight", "conv_cout.bias", "channel_norm.body.weight", "channel_norm.body.bias"]


@pytest.mark.parametrize("variant", ["srgan", "realsr"])
def test_channel_branch_parameter_gradients_deferred(variant, oracle_cpu_kernel):
    """``oss_chan_bwd`` leaves one gradient vector per image (K = 17): the deferred sums against the literal reference data flow on
    the CPU (oracle/cpu_twins.py), limits of test_fused_channel_branch_against_oracle_twin"""
    from vmambair_amd.oss_block import SS2D_1
    torch.manual_seed(2)
    m = SS2D_1(d_model=16, variant=variant)
    with torch.no_grad():
        m.Ac_logs.mul_(0.5)
    lift = m.dc_inner is not None
    y2 = torch.randn(17, m.d_inner, 6, 5)
    g = torch.randn(17, m.d_inner, 6, 5)
    pr = dict(m.named_parameters())
    used = [n for n in _CHAN_NAMES if lift or not n.startswith("conv_c")]
    cpu = {n: pr[n].detach().clone().requires_grad_() for n in used}
    ops.ChannelGateFn.apply(y2, *[cpu.get(n) for n in _CHAN_NAMES], m.gate != "add").backward(g)
    y2d, gd = y2.to(DEV), g.to(DEV)
    leaves = {}

    def run():
        leaves.clear()
        leaves.update({n: pr[n].detach().to(DEV).requires_grad_() for n in used})
        ops.ChannelGateFn.apply(y2d, *[leaves.get(n) for n in _CHAN_NAMES], m.gate != "add").backward(gd)
        return [leaves[n].grad for n in used]

    now, got = _twice(run, lambda: list(leaves.values()))
    for n, gi, ni in zip(used, got, now):
        if n.endswith("conv_cout.bias"):
            continue   # exact gradient 0 (a constant in front of a LayerNorm): rounding noise on both sides
        r = cpu[n].grad
        assert_close(gi, r, 5e-3, 1e-3 * max(float(r.abs().max()), 1e-6), n)
        _same_up_to_order(gi, ni, n + " deferred vs immediate")


@pytest.mark.parametrize("B,Cin,Cout,H,W,ln_bias", [(3, 48, 96, 8, 16, True), (5, 16, 32, 8, 16, False), (3, 48, 254, 8, 16, True)],
                         ids=["fused-bwd", "fused-bwd-biasfree", "separate-bwd"])
@pytest.mark.parametrize("dt", IO, ids=IO_IDS)
def test_layernorm_1x1_conv_backward_deferred(dt, B, Cin, Cout, H, W, ln_bias):
    """LNConv1x1Fn: the weight gradient is a recorded product, the LayerNorm parameter gradients come out of the fused dgrad + LN
    backward (``oss_conv1x1_dgrad_ln_bwd``, per-workgroup partials) or of the two separate kernels.  Limits of
    test_layernorm_fused_into_the_1x1_convolution: dW against plain PyTorch fp32, the LayerNorm gradients against the two separate
    nodes (LayerNormNCHWFn -> Conv1x1Fn) run immediately"""
    torch.manual_seed(5)
    x = (torch.randn(B, Cin, H, W, device=DEV) * 1.5 + 0.3).to(dt)
    lw = torch.randn(Cin, device=DEV) * 0.2 + 1.0
    lb = torch.randn(Cin, device=DEV) * 0.1 if ln_bias else None
    w = torch.randn(Cout, Cin, 1, 1, device=DEV) * (Cin ** -0.5)
    b = torch.randn(Cout, device=DEV)
    dy = torch.randn(B, Cout, H, W, device=DEV).to(dt)
    dskip = torch.randn(B, Cin, H, W, device=DEV).to(dt)
    conv = torch.nn.Conv2d(Cin, Cout, 1).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    assert ops.ln_conv1x1_ok(x, conv.weight)
    assert bool(_lib().oss_conv1x1_dgrad_ln_bwd_ok(ops._DT[dt], Cout, Cin, H * W, B)) == (Cout <= 192)
    leaves = []

    def run(fused=True):
        conv.zero_grad(set_to_none=True)
        lwi = lw.clone().requires_grad_()
        lbi = lb.clone().requires_grad_() if ln_bias else None
        leaves[:] = [lwi, conv.weight, conv.bias] + ([lbi] if ln_bias else [])
        xi = x.clone().requires_grad_()
        if fused:
            y, skip = ops.ln_conv1x1(xi, lwi, lbi, conv)
        else:
            n, skip = ops.layer_norm_nchw(xi, lwi, lbi, None, dt, True)
            y = ops.conv1x1(n, conv)
        torch.autograd.backward([y, skip], [dy, dskip])
        return [lwi.grad, lbi.grad if ln_bias else None, conv.weight.grad, conv.bias.grad]

    sep = [None if t is None else t.clone() for t in run(fused=False)]
    now, got = _twice(run, lambda: leaves)
    # plain PyTorch fp32 on the same 16-bit inputs
    xr, lwr, wr = x.float(), lw.clone(), w.clone().requires_grad_()
    rs = (xr.var(1, keepdim=True, unbiased=False) + 1e-5).rsqrt()
    n = (xr - xr.mean(1, keepdim=True)) * rs * lwr.view(1, -1, 1, 1) + lb.view(1, -1, 1, 1) if ln_bias else xr * rs * lwr.view(1, -1, 1, 1)
    F.conv2d(n, wr, b).backward(dy.float())
    rt = 2e-2 if dt == torch.bfloat16 else 3e-3
    assert_close(got[2], wr.grad, 2 * rt, 2 * rt * float(wr.grad.abs().max()), "dW vs torch")
    assert_close(got[0], sep[0], rt, rt * float(sep[0].abs().max()), "d ln weight")
    if ln_bias:
        assert_close(got[1], sep[1], rt, rt * float(sep[1].abs().max()), "d ln bias")
    assert_close(got[2], sep[2], rt, rt * float(sep[2].abs().max()), "dW")
    assert_close(got[3], sep[3], 1e-4, 1e-4 * float(sep[3].abs().max()), "db")
    for gi, ni, name in zip(got, now, ("d ln weight", "d ln bias", "dW", "db")):
        if gi is not None:
            _same_up_to_order(gi, ni, name + " deferred vs immediate")


# =====================================================================================================================
# E. table handling
# =====================================================================================================================
def _record_int_product(shape, dt, has_bias=True):
    """record one integer product inside an open context -> (outputs, everything that must stay alive, float64 reference)"""
    dy, x, ref64, _ = _wgrad_case(shape, dt, "int")
    dyd, xd = dy.to(DEV), x.to(DEV)
    dw, db, part = _wgrad_call(dt, dyd, xd, has_bias)
    return (dw, db), (dyd, xd, part), ref64


def _exact_product(out, ref64, Cin, what):
    _exact(out[0], ref64[:, :Cin], what + " dw")
    if out[1] is not None:
        _exact(out[1], ref64[:, Cin], what + " db")


def test_partial_flush_finishes_the_first_recorded_product_only():
    """``flush_wgrads(count=1)`` + ``flush_finishes(count=chunks registered by then)``: the first product's gradients are complete
    and nothing of the other two has been written; the rest follows with the next flush"""
    shapes = [WGRAD_SHAPES[0], WGRAD_SHAPES[5], WGRAD_SHAPES[2]]
    dt = torch.bfloat16
    with ops.deferred_finishes(wgrads=True):
        recs = [_record_int_product(shapes[0], dt)]
        chunks_first = ops.pending_finish_chunks()
        recs += [_record_int_product(s, dt, has_bias) for s, has_bias in ((shapes[1], False), (shapes[2], True))]
        assert ops.pending_wgrads() == 3 and ops.pending_finish_chunks() > chunks_first > 0
        wt = ops.WgradTable(DEV, ops.pending_wgrad_table_bytes())
        ft = ops.FinishTable(DEV, ops.pending_finish_chunks())
        chunks_all = ops.pending_finish_chunks()
        ops.flush_wgrads(wt, count=1)
        ops.flush_finishes(ft, count=chunks_first)
        torch.cuda.synchronize()
        assert ops.pending_wgrads() == 2 and ops.pending_finish_chunks() == chunks_all - chunks_first
        _exact_product(recs[0][0], recs[0][2], shapes[0][2], "first product after the partial flush")
        for (dw, db), _, _ in recs[1:]:
            assert bool(dw.isnan().all()) and (db is None or bool(db.isnan().all())), "a later product's output was written early"
        ops.flush_wgrads(wt)
        ops.flush_finishes(ft)
        torch.cuda.synchronize()
        assert ops.pending_wgrads() == 0 and ops.pending_finish_chunks() == 0
    for (out, _, ref64), s in zip(recs, shapes):
        _exact_product(out, ref64, s[2], f"product {s}")


def test_tables_one_entry_too_small_raise_and_keep_the_recordings():
    """OSS_ERR_WORKSPACE comes back before anything is launched or dropped: the same recordings flush correctly afterwards.  (The
    short tables are full-sized buffers whose stated capacity is one entry short.)"""
    shape, dt = WGRAD_SHAPES[1], torch.float16
    with ops.deferred_finishes(wgrads=True):
        out, keep, ref64 = _record_int_product(shape, dt)
        need_w, need_f = ops.pending_wgrad_table_bytes(), ops.pending_finish_chunks()
        assert need_w > 256 and need_f > 1
        wt, ft = ops.WgradTable(DEV, need_w), ops.FinishTable(DEV, need_f)
        wt.capacity = need_w - 2    # one 16-bit block-to-problem entry short
        with pytest.raises(RuntimeError, match="OSS_ERR_WORKSPACE"):
            ops.flush_wgrads(wt)
        assert ops.pending_wgrads() == 1 and ops.pending_wgrad_table_bytes() == need_w
        wt.capacity = need_w
        ops.flush_wgrads(wt)
        assert ops.pending_wgrads() == 0
        ft.capacity = need_f - 1
        with pytest.raises(RuntimeError, match="OSS_ERR_WORKSPACE"):
            ops.flush_finishes(ft)
        assert ops.pending_finish_chunks() == need_f
        ft.capacity = need_f
        ops.flush_finishes(ft)
        torch.cuda.synchronize()
        assert ops.pending_finish_chunks() == 0
    _exact_product(out, ref64, shape[2], "after the refused flushes")
    del keep


def test_two_io_types_in_one_flush_raise():
    """the grouped kernel is instantiated per I/O type: a flush over a bf16 and an f16 product is refused, and switching the
    recording off drops both"""
    lib = _lib()
    try:
        with ops.deferred_finishes(wgrads=True):
            a = _record_int_product(WGRAD_SHAPES[5], torch.bfloat16)
            b = _record_int_product(WGRAD_SHAPES[5], torch.float16)
            assert ops.pending_wgrads() == 2
            wt = ops.WgradTable(DEV, ops.pending_wgrad_table_bytes())
            with pytest.raises(RuntimeError, match="oss_flush_wgrads: OSS_ERR_SHAPE"):
                ops.flush_wgrads(wt)
            assert ops.pending_wgrads() == 2, "a refused flush drops nothing"
            lib.oss_set_defer_wgrad(0)
            assert ops.pending_wgrads() == 0 and ops.pending_wgrad_table_bytes() == 0
            torch.cuda.synchronize()
            for (dw, db), _, _ in (a, b):
                assert bool(dw.isnan().all()) and bool(db.isnan().all()), "a refused flush must not have launched anything"
    finally:
        lib.oss_set_defer_wgrad(0)
        lib.oss_set_defer_finish(0)
