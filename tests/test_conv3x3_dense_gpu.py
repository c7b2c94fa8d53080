"""The GEMM-shaped dense 3x3 convolutions of the UNet skeleton on the in-tree MFMA kernels (oss_conv3x3_dense.hip; Cin % 16 == 0,
Cout >= 5; opt-in through VMAMBAIR_CONV3X3_DENSE / ops.set_dense) against float64 references of the same operations on the same
rounded operands: F.conv2d, F.conv_transpose2d, torch.nn.grad.conv2d_weight.

INTEGER operands (x, dy in {-3 .. 3}, w in {-2 .. 2}, bias in {-4 .. 4}): every partial and final sum is an integer below 2^24, so
any fp32 summation order is exact; y and dx must EQUAL the float64 result rounded once to the I/O type, dW and db the float64 result.
RANDOM operands (unit normal, w / (3 sqrt(Cin))): y and dx element-wise within
    1/2 ulp_dt(max(|ref64|, |got|)) + K 2^-23 S
(one correct rounding + the standard bound of a K-term fp32 sum with unit round-off 2^-23, which a matrix unit that chops instead of
rounding still meets; K = 9 Cin forward, 9 Cout input gradient; S = the same convolution of absolute values, plus |bias|; ulp_dt has
8 significant bits for bf16, 11 for fp16).  dW and db: the rule of tests/test_deferred_wgrad_gpu.py -- Frobenius error at most 4 x the
error of the same contraction in plain float32 on the CPU, no NaN.  The worst ratios are printed (``pytest -s``)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from vmambair_amd import _capi, ops
from vmambair_amd.ops.conv3x3 import DenseConv3x3Fn, conv3x3, dense_ok, set_dense

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IO = [torch.bfloat16, torch.float16]
IO_IDS = ["bf16", "f16"]

# (B, Cin, H, W) -> Cout
SHAPES = [
    ((2, 16, 5, 7), 24), ((1, 48, 9, 33), 40), ((2, 96, 8, 16), 192), ((1, 192, 3, 5), 96), ((3, 32, 1, 1), 8), ((1, 384, 4, 6), 33),
    ((1, 16, 17, 70), 100), ((2, 64, 2, 40), 64),
    # edges of this kernel's own tiling that the table above does not reach: the weight gradient's row bands hold ONE row unless
    # batch * (co, ci) tiles * H > 512 -- here 18 tiles and 41 rows give 20 bands of two rows and a last band of one; 8-pixel rows
    # (16-byte path) that fill half a 16-pixel k-step; Cout = 192 = three 64-wide workgroup tiles, Cin = 128 = one 4-wave tile
    ((3, 128, 41, 8), 192),
]
IDS = ["x".join(map(str, s)) + f"-{c}" for s, c in SHAPES]


def _conv_w(dy, x):
    return torch.nn.grad.conv2d_weight(x, (dy.shape[1], x.shape[1], 3, 3), dy, padding=1)


@functools.lru_cache(maxsize=None)
def _case(idx, dt, kind):
    """operands (CPU; activations in the I/O type, fp32 masters) and every reference, computed once and shared"""
    shape, cout = SHAPES[idx]
    B, Cin, H, W = shape
    gen = torch.Generator().manual_seed(4000 + 10 * idx + (1 if kind == "int" else 0))
    if kind == "int":
        x = torch.randint(-3, 4, shape, generator=gen).to(dt)
        dy = torch.randint(-3, 4, (B, cout, H, W), generator=gen).to(dt)
        w = torch.randint(-2, 3, (cout, Cin, 3, 3), generator=gen).float()
        b = torch.randint(-4, 5, (cout,), generator=gen).float()
    else:
        x = torch.randn(shape, generator=gen).to(dt)
        dy = torch.randn((B, cout, H, W), generator=gen).to(dt)
        w = torch.randn((cout, Cin, 3, 3), generator=gen) / (3.0 * Cin ** 0.5)
        b = torch.randn((cout,), generator=gen) * 0.1
    x64, dy64, w64, b64 = x.double(), dy.double(), w.to(dt).double(), b.to(dt).double()
    ref = dict(
        y0=F.conv2d(x64, w64, None, padding=1),
        dx=F.conv_transpose2d(dy64, w64, None, padding=1),
        dw=_conv_w(dy64, x64), db=dy64.sum(dim=(0, 2, 3)),
        sy=F.conv2d(x64.abs(), w64.abs(), None, padding=1),
        sdx=F.conv_transpose2d(dy64.abs(), w64.abs(), None, padding=1),
        dw32=_conv_w(dy.float(), x.float()), db32=dy.float().sum(dim=(0, 2, 3)), b64=b64)
    return x, dy, w, b, ref


def _run(x, dy, w, b):
    """forward and backward through the operators on fresh device copies -> y, dx, dw, db"""
    xd, dyd, wd = x.to(DEV), dy.to(DEV), w.to(DEV)
    bd = None if b is None else b.to(DEV)
    assert dense_ok(xd, wd)
    y = torch.ops.vmambair.conv3x3_dense_fwd(xd, wd, bd)
    dx, dw, db = torch.ops.vmambair.conv3x3_dense_bwd(xd, wd, dyd, b is not None, True)
    torch.cuda.synchronize()
    return y, dx, dw, (db if b is not None else None)


def _ulp(v, dt):
    """spacing of the I/O type at magnitude v (float64 tensor)"""
    p, emin = (8, -125) if dt == torch.bfloat16 else (11, -13)
    _, e = torch.frexp(v.abs())
    e = torch.where(v == 0, torch.full_like(e, emin), e).clamp(min=emin)
    return torch.ldexp(torch.ones_like(v), e - p)


def _within(got, ref64, S, K, dt, what):
    got = got.double().cpu()
    assert got.shape == ref64.shape and not bool(got.isnan().any()), what
    lim = 0.5 * _ulp(torch.maximum(ref64.abs(), got.abs()), dt) + K * 2.0 ** -23 * S
    ratio = float(((got - ref64).abs() / lim).max())
    print(f"[{what}] worst |got - ref64| / limit = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: worst |got - ref64| / limit = {ratio:.3f}"


def _fro(got, ref64, cpu32, what):
    got = got.double().cpu()
    assert got.shape == ref64.shape, what
    assert not bool(got.isnan().any()), f"{what}: NaN (an element or a partial vector nobody wrote)"
    e32, err = float((cpu32.double() - ref64).norm()), float((got - ref64).norm())
    print(f"[{what}] |got - ref64|_F = {err:.3e}, e32 = {e32:.3e}, ratio = {err / e32 if e32 > 0 else (0.0 if err == 0 else float('inf')):.3f}")
    assert err <= 4.0 * e32, f"{what}: |got - ref64|_F = {err:.3e} > 4 e32 = {4 * e32:.3e}"


def _exact(got, ref, what):
    got, ref = got.cpu(), ref.to(got.dtype)
    assert got.shape == ref.shape, what
    if not torch.equal(got, ref):
        bad = (got != ref) | got.isnan()
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())}/{ref.numel()} elements differ; first at flat index {i}: "
                             f"got {got.flatten()[i].item()}, want {ref.flatten()[i].item()}")


@pytest.mark.parametrize("idx", range(len(SHAPES)), ids=IDS)
@pytest.mark.parametrize("dt", IO, ids=IO_IDS)
@pytest.mark.parametrize("has_bias", [True, False], ids=["bias", "nobias"])
def test_integer_operands_are_exact(idx, dt, has_bias):
    x, dy, w, b, ref = _case(idx, dt, "int")
    y, dx, dw, db = _run(x, dy, w, b if has_bias else None)
    y64 = ref["y0"] + (ref["b64"].view(1, -1, 1, 1) if has_bias else 0.0)
    assert float(y64.abs().max()) < 2 ** 24 and float(ref["dw"].abs().max()) < 2 ** 24
    assert y.dtype == dt and dx.dtype == dt and dw.dtype == torch.float32
    _exact(y, y64.to(dt), "y")
    _exact(dx, ref["dx"].to(dt), "dx")
    _exact(dw.double(), ref["dw"], "dw")
    if has_bias:
        _exact(db.double(), ref["db"], "db")


@pytest.mark.parametrize("idx", range(len(SHAPES)), ids=IDS)
@pytest.mark.parametrize("dt", IO, ids=IO_IDS)
@pytest.mark.parametrize("has_bias", [True, False], ids=["bias", "nobias"])
def test_random_operands(idx, dt, has_bias):
    (shape, cout) = SHAPES[idx]
    x, dy, w, b, ref = _case(idx, dt, "rand")
    y, dx, dw, db = _run(x, dy, w, b if has_bias else None)
    bias = ref["b64"].view(1, -1, 1, 1) if has_bias else torch.zeros(1, 1, 1, 1, dtype=torch.float64)
    _within(y, ref["y0"] + bias, ref["sy"] + bias.abs(), 9 * shape[1], dt, "y")
    _within(dx, ref["dx"], ref["sdx"], 9 * cout, dt, "dx")
    _fro(dw, ref["dw"], ref["dw32"], "dw")
    if has_bias:
        _fro(db, ref["db"], ref["db32"], "db")


@pytest.mark.parametrize("idx", [7, 0], ids=[IDS[7], IDS[0]])   # 16-byte rows / odd rows (element-wise loaders)
def test_reruns_are_bit_identical_and_strided_inputs_work(idx):
    (shape, cout) = SHAPES[idx]
    B, Cin, H, W = shape
    x, dy, w, b, _ = _case(idx, torch.bfloat16, "rand")
    big = torch.randn(B, Cin + 40, H, W).to(torch.bfloat16).to(DEV)
    xv = big[:, 8:8 + Cin]                    # a channel slice: batch stride != Cin * H * W
    xv.copy_(x.to(DEV))
    gbig = torch.randn(B, cout + 9, H, W).to(torch.bfloat16).to(DEV)
    gv = gbig[:, 3:3 + cout]
    gv.copy_(dy.to(DEV))
    wd, bd = w.to(DEV), b.to(DEV)
    outs = []
    for xx, gg in ((xv, gv), (xv, gv), (xv.contiguous(), gv.contiguous())):
        y = torch.ops.vmambair.conv3x3_dense_fwd(xx, wd, bd)
        outs.append([y] + list(torch.ops.vmambair.conv3x3_dense_bwd(xx, wd, gg, True, True)))
    torch.cuda.synchronize()
    for other in outs[1:]:
        for a, c in zip(outs[0], other):
            assert a.numel() and torch.equal(a, c)


def test_refused_shapes_fall_back_to_the_module():
    prev = set_dense(True)
    try:
        for cin, cout, dt in ((24, 24, torch.bfloat16), (32, 24, torch.float32), (32, 3, torch.bfloat16)):
            conv = torch.nn.Conv2d(cin, cout, 3, padding=1).to(DEV).to(dt)
            x = torch.randn(2, cin, 6, 5, device=DEV).to(dt)   # width 5: the thin kernels refuse the Cout = 3 layer too
            assert not dense_ok(x, conv.weight)
            y = conv3x3(x, conv)
            assert not y.grad_fn.__class__.__name__.startswith("DenseConv3x3Fn")
            assert torch.equal(y, conv(x))
        conv = torch.nn.Conv2d(32, 24, 3, padding=1).to(DEV)
        x = torch.randn(2, 32, 6, 5, device=DEV).to(torch.bfloat16)
        assert dense_ok(x, conv.weight)
        assert conv3x3(x, conv).grad_fn.__class__.__name__.startswith("DenseConv3x3Fn")
        set_dense(False)
        assert torch.equal(conv3x3(x.float(), conv), conv(x.float()))
    finally:
        set_dense(prev)


@pytest.mark.parametrize("idx", [2, 8], ids=[IDS[2], IDS[8]])
def test_deferred_finishing_is_bit_identical(idx):
    x, dy, w, b, _ = _case(idx, torch.bfloat16, "rand")
    xd, dyd, wd = x.to(DEV), dy.to(DEV), w.to(DEV)
    _, dw, db = torch.ops.vmambair.conv3x3_dense_bwd(xd, wd, dyd, True, False)
    torch.cuda.synchronize()
    with ops.deferred_finishes():
        _, dw2, db2 = torch.ops.vmambair.conv3x3_dense_bwd(xd, wd, dyd, True, False)
        n = ops.pending_finish_chunks()
        assert n > 0 and ops.pending_wgrads() == 0
        table = ops.FinishTable(DEV, n)
        ops.flush_finishes(table)
        assert ops.pending_finish_chunks() == 0
        torch.cuda.synchronize()
    assert torch.equal(dw, dw2) and torch.equal(db, db2) and not bool(dw.isnan().any())


def test_forward_and_backward_capture_into_a_graph():
    x, dy, w, b, _ = _case(2, torch.bfloat16, "rand")
    xd, dyd = x.to(DEV).requires_grad_(), dy.to(DEV)
    wd, bd = w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()

    def run():
        y = DenseConv3x3Fn.apply(xd, wd, bd)
        return (y,) + torch.autograd.grad(y, (xd, wd, bd), dyd)

    eager = [t.detach().clone() for t in run()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for _ in range(2):
        for t in outs:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, c in zip(eager, outs):
            assert torch.equal(a, c.detach())


# ---- the nets -------------------------------------------------------------------------------------------------------------------
def _net():
    from vmambair_amd.archs import MambaSISR6
    torch.manual_seed(0)
    return MambaSISR6(dim=16, num_blocks=(1, 1, 1, 1), num_refinement_blocks=1).to(DEV)


def _skeleton_convs(net):
    """the Conv2d modules of Downsample / Upsample / the x4 tail's two up-convolutions, by parameter-owning module name"""
    from vmambair_amd.archs import Downsample, Upsample
    names = [f"{n}.body.0" for n, m in net.named_modules() if isinstance(m, (Downsample, Upsample))]
    return names + ["tail.0.0", "tail.0.2"]


def _dense_nodes(out):
    seen, todo, n = set(), [out.grad_fn], 0
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        n += f.__class__.__name__.startswith("DenseConv3x3Fn")
        todo.extend(g for g, _ in f.next_functions)
    return n


def test_net_runs_its_skeleton_on_the_dense_kernels():
    torch.manual_seed(3)
    lq = torch.rand(2, 3, 16, 16, device=DEV)
    prev = set_dense(False)
    try:
        net = _net()
        keys_off = list(net.state_dict().keys())
        with torch.no_grad():
            ref32 = net(lq).double()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out_off = net(lq)
        assert _dense_nodes(out_off) == 0
        set_dense(True)
        net_on = _net()
        assert list(net_on.state_dict().keys()) == keys_off
        net_on.load_state_dict(net.state_dict(), strict=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out_on = net_on(lq)
        skeleton = _skeleton_convs(net_on)
        assert len(skeleton) == 8 and _dense_nodes(out_on) == len(skeleton)   # 3 down, 3 up, 2 in the tail
        e_off = float((out_off.detach().double() - ref32).abs().max())
        e_on = float((out_on.detach().double() - ref32).abs().max())
        print(f"[net bf16 vs fp32] max error: vendor 3x3 {e_off:.3e}, dense kernels {e_on:.3e}")
        assert e_on <= 2.0 * e_off
        out_on.float().sum().backward()
        mods = dict(net_on.named_modules())
        for n in skeleton:
            g = mods[n].weight.grad
            assert g is not None and g.dtype == torch.float32 and bool(g.isfinite().all()) and float(g.abs().max()) > 0
    finally:
        set_dense(prev)


def test_graphed_step_with_the_dense_kernels_matches_eager():
    """one GraphedTrainStep step (bf16 autocast) against the eager step, at the limits of
    test_train_step_selfcheck_gpu.test_graphed_train_step_matches_eager; the skeleton's weights have no 16-bit shadow"""
    from vmambair_amd.train_graph import GraphedTrainStep
    prev = set_dense(True)
    try:
        torch.manual_seed(5)
        lq = torch.rand(2, 3, 16, 16, device=DEV)
        gt = torch.rand(2, 3, 64, 64, device=DEV)
        net_g = _net()
        init = [p.detach().clone() for p in net_g.parameters()]
        step = GraphedTrainStep(net_g, autocast_dtype=torch.bfloat16, warmup=1)
        for n in _skeleton_convs(net_g):
            assert f"{n}.weight" not in step.shadow and f"{n}.bias" not in step.shadow
        net_e = _net()
        lr = 2e-4
        opt = torch.optim.Adam(net_e.parameters(), lr=lr, betas=(0.9, 0.99))
        loss_g = float(step(lq, gt))
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = net_e(lq)
        assert _dense_nodes(out) == 8
        loss = F.l1_loss(out.float(), gt)
        loss.backward()
        opt.step()
        ug = torch.cat([(p.detach() - i).flatten() for p, i in zip(net_g.parameters(), init)]).double()
        ue = torch.cat([(p.detach() - i).flatten() for p, i in zip(net_e.parameters(), init)]).double()
        cos = float((ug * ue).sum() / (ug.norm() * ue.norm()))
        print(f"[graphed step, dense 3x3] loss graph {loss_g} eager {float(loss)}; first-update cosine {cos:.5f}")
        assert float(ug.abs().max()) <= 1.01 * lr and float(ue.abs().max()) <= 1.01 * lr
        assert loss_g == pytest.approx(float(loss), rel=1e-2)
        assert cos >= 0.85, cos
    finally:
        set_dense(prev)
