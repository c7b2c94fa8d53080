"""Which route a module takes and what state that route reads: the two forward-only fast paths behind Python predicates.

* the one-launch EFFN forward (``FeedForward.forward`` -> ``effn_fwd``, csrc/oss_effn.hip) reads 16-bit copies of the weights made by
  ``FeedForward._rounded``.  A: after the weights change between two eager ``no_grad`` forwards -- by the fused optimizer step (raw
  pointers, no version bump), by ``p.data`` updates (the reference's ``model_ema``, Deraining/basicsr/models/base_model.py:54-62), by
  torch in-place ops, ``load_state_dict`` or a new ``nn.Parameter``, and between graphed training steps of a whole net -- the second
  forward must compute with the weights as they are THEN;
* B: a partly frozen module (a detached stream, ``project_in`` or the gate's weight frozen, something else trainable) must build the
  autograd chain and hand every trainable parameter its gradient, where the fast path (no autograd) would leave ``.grad = None``.

Every test proves its route: a spy counts the calls of ``torch.ops.vmambair.effn_fwd`` / ``dwgate_fwd``.  The references are fp64
PyTorch built from the parameters as they are when the forward runs (tests/test_effn_gpu.py: reference(), in double precision);
the single-module tests never use the chain as the reference (under a stale-copy defect it would be compared with itself)."""
import contextlib

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import assert_close
from vmambair_amd import ops, oss_block
from vmambair_amd.ops import dwconv as dw_ops
from vmambair_amd.ops import ffn as ffn_ops
from vmambair_amd.optim import FusedAdamEMA

pytestmark = [pytest.mark.gpu, pytest.mark.tier(1)]   # one op / module against fp64 PyTorch (the whole-net case: against the chain)
DEV = "cuda:0"
DTS = [torch.float16, torch.bfloat16]
DT_IDS = ["f16", "bf16"]
#: elementwise forward tolerance of test_effn_gpu.py (x the output's largest magnitude), relative-L2 limit of a parameter gradient
RT = {torch.float16: 2e-3, torch.bfloat16: 1.6e-2}
GRAD_RL2 = {torch.float16: 5e-3, torch.bfloat16: 2e-2}


@pytest.fixture
def spy(monkeypatch):
    """records the stream shape of every call of the two forward-only ops"""
    calls = {"effn_fwd": [], "dwgate_fwd": []}
    for name, log in calls.items():
        real = getattr(torch.ops.vmambair, name)

        def counted(*args, _real=real, _log=log):
            _log.append(tuple(args[0].shape))
            return _real(*args)
        monkeypatch.setattr(torch.ops.vmambair, name, counted)
    return calls


@contextlib.contextmanager
def chain():
    """the launch-per-layer chain: every kernel of it reads the live fp32 parameters"""
    ffn_ops.EFFN_FUSED = False
    try:
        yield
    finally:
        ffn_ops.EFFN_FUSED = True


def _q(t, dt):
    """``t`` rounded to ``dt`` in the forward, the gradient passed through in fp64"""
    t = t.double()
    return t + (t.to(dt).double() - t).detach()


def ffn64(x, ln_w, ln_b, w_in, w_dw, w_out):
    """``x + project_out(gelu(x1) * x2)`` in fp64 on the values the kernels read: x and the two 1x1 weights rounded to the I/O type,
    norm2(x), project_in's output and the gate's output rounded where the chain stores them (the depth-wise weight stays fp32)"""
    dt = x.dtype
    xd = x.double()
    mu = xd.mean(1, keepdim=True)
    var = xd.var(1, keepdim=True, unbiased=False)
    if ln_b is not None:
        n = (xd - mu) / torch.sqrt(var + 1e-5) * ln_w.double().view(1, -1, 1, 1) + ln_b.double().view(1, -1, 1, 1)
    else:
        n = xd / torch.sqrt(var + 1e-5) * ln_w.double().view(1, -1, 1, 1)
    t = _q(F.conv2d(_q(n, dt), _q(w_in, dt)), dt)
    t = F.conv2d(t, w_dw.double(), padding=1, groups=t.shape[1])
    x1, x2 = t.chunk(2, dim=1)
    return xd + F.conv2d(_q(F.gelu(x1) * x2, dt), _q(w_out, dt))


def reference(x, norm, ff):
    """fp64 from the parameters as they are NOW"""
    with torch.no_grad():
        return ffn64(x, norm.body.weight, norm.body.bias, ff.project_in.weight, ff.dwconv.weight, ff.project_out.weight)


def _modules(D, seed):
    torch.manual_seed(seed)
    norm = oss_block.LayerNorm(D, "WithBias").to(DEV)
    ff = oss_block.FeedForward(D, 2.66, False).to(DEV)
    with torch.no_grad():
        norm.body.weight.uniform_(0.5, 1.5)
        norm.body.bias.normal_(0, 0.3)
        ff.dwconv.weight.mul_(2.0)
    return norm, ff


def _stream(shape, dt, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * 1.5 + 0.2).to(DEV).to(dt)


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm())


def check_forward(got, want, chain_out, what):
    """test_effn_gpu.py's rule: elementwise rtol of the I/O type scaled by the output's largest magnitude, and a mean |error| no worse
    than 1.5 x the chain's on the same input"""
    rt = RT[got.dtype]
    assert_close(got, want, rt, rt * float(want.abs().max()) * 0.5, what)
    e = float((got.double() - want).abs().mean()), float((chain_out.double() - want).abs().mean())
    assert e[0] <= 1.5 * e[1] + 1e-6, f"{what}: mean |error| {e[0]:.3e} vs the chain's {e[1]:.3e}"


# ---------------------------------------------------------------------------------------------------------------------------------
# A. the weights change between two eager no_grad forwards of the one-launch EFFN
# ---------------------------------------------------------------------------------------------------------------------------------
def _adam_step(norm, ff, x):
    """one FusedAdamEMA step (a raw-pointer write of the parameters) with the gradients of one forward/backward of the chain"""
    g = torch.Generator().manual_seed(21)
    out = ff(x.clone().requires_grad_(), pre_norm=norm)
    out.backward(torch.randn(out.shape, generator=g).to(DEV).to(out.dtype))
    opt = FusedAdamEMA(list(ff.parameters()), lr=0.05)
    opt.step()
    torch.cuda.synchronize()   # (the step's pointer table is copied asynchronously out of the optimizer's pinned buffer)


def _ema_update(name):
    def update(norm, ff, x):
        """``model_ema``: ``ema.data.mul_(decay).add_(net.data, alpha=1 - decay)`` -- ``.data`` has a version counter of its own"""
        p = getattr(ff, name).weight
        src = torch.randn(p.shape, generator=torch.Generator().manual_seed(22)).to(DEV) * float(p.detach().std())
        p.data.mul_(0.5).add_(src.data, alpha=0.5)
    return update


def _in_place(norm, ff, x):
    with torch.no_grad():
        ff.project_in.weight.mul_(1.5)
        ff.dwconv.weight.add_(0.05)
        ff.project_out.weight.mul_(-1.0)


def _load_state_dict(norm, ff, x):
    _, other = _modules(ff.project_out.out_channels, 23)
    ff.load_state_dict(other.state_dict())


def _new_parameter(norm, ff, x):
    w = ff.project_out.weight
    ff.project_out.weight = nn.Parameter(torch.randn(w.shape, generator=torch.Generator().manual_seed(24)).to(DEV) * float(w.detach().std()))


UPDATES = {
    "fused_adam_ema_step": _adam_step,
    "data_ema_project_in": _ema_update("project_in"),
    "data_ema_dwconv": _ema_update("dwconv"),
    "data_ema_project_out": _ema_update("project_out"),
    "in_place_no_grad": _in_place,          # (version-bumping updates: regression guards)
    "load_state_dict": _load_state_dict,
    "new_parameter": _new_parameter,
}
SHAPES = [(1, 48, 24, 32), (2, 96, 16, 48)]   # hidden 127; hidden 255: the last 16-channel chunk ragged


@pytest.mark.parametrize("update", list(UPDATES))
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}x{s[3]}" for s in SHAPES])
def test_fused_effn_reads_the_live_weights_after_an_update(shape, dt, update, spy):
    norm, ff = _modules(shape[1], 20)
    x = _stream(shape, dt, 20)
    assert ffn_ops.effn_fwd_ok(x, ff.project_out.in_channels)
    with torch.no_grad():
        first = ff(x, pre_norm=norm)
    UPDATES[update](norm, ff, x)
    with torch.no_grad():
        second = ff(x, pre_norm=norm)
        want = reference(x, norm, ff)
        with chain():
            chain_out = ff(x, pre_norm=norm)
    assert spy["effn_fwd"] == [shape, shape], "both eager no_grad forwards took the one-launch EFFN"
    assert not torch.equal(first, second), "the update changed the output"
    check_forward(second, want, chain_out, f"one-launch EFFN after {update}")


def test_validation_between_graphed_bf16_training_steps_uses_the_trained_weights(spy):
    """the headline training workflow: GraphedTrainStep (bf16 autocast, the reference's Adam rate 2e-4; the fused Adam + EMA step is
    replayed from a graph and bumps no version counter) with an eager bf16-autocast no_grad validation of the net before, between and
    after two replays.  Each validation against the same net at the same instant through the chain, which reads the live fp32
    parameters: every one-launch EFFN (it must run at d 48 and d 96) against the chain of the same module on the same input, and the
    whole output against the net run with ``EFFN_FUSED = False``"""
    from vmambair_amd.archs import MambaSISR6
    from vmambair_amd.train_graph import GraphedTrainStep
    torch.manual_seed(30)
    net = MambaSISR6(dim=48, num_blocks=(1, 1, 1, 1), num_refinement_blocks=1, bias=False).to(DEV)
    g = torch.Generator().manual_seed(30)
    gt = torch.rand(2, 3, 128, 128, generator=g).to(DEV)
    lq = F.interpolate(gt, scale_factor=0.25, mode="area")
    lq_val = F.interpolate(torch.rand(1, 3, 128, 128, generator=g).to(DEV), scale_factor=0.25, mode="area")
    up = F.interpolate(lq_val, scale_factor=4, mode="nearest")
    step = GraphedTrainStep(net, autocast_dtype=torch.bfloat16, warmup=1)
    ffs = [m for m in net.modules() if isinstance(m, oss_block.FeedForward)]
    earlier = {}   # per module: the rounded weights its one-launch forward read at the previous validation
    tol = 1e-2     # rel-L2 of one EFFN's branch (output - input), one-launch vs chain (measured <= 1.8e-3)

    def validate(tag):
        n0 = len(spy["effn_fwd"])
        rows = []

        def against_the_chain(m, args, kwargs, out):
            x, pn = args[0], kwargs.get("pre_norm")
            if pn is None or not ffn_ops.effn_fwd_ok(x, m.project_out.in_channels):
                return   # (d 192 / 384: no instantiation, the chain anyway)
            with chain():
                ref = m.forward(x, pre_norm=pn)
            e = _rel(out.float() - x.float(), ref.float() - x.float())
            stale = None
            if m in earlier:   # what the previous validation's weight copies would give now
                old = torch.ops.vmambair.effn_fwd(x, pn.body.weight, pn.body.bias, *earlier[m], m.project_out.in_channels)
                stale = _rel(old.float() - x.float(), ref.float() - x.float())
            earlier[m] = [w.clone() for w in m._rounded(x.dtype)]
            rows.append((x.shape[1], e, stale))

        hooks = [m.register_forward_hook(against_the_chain, with_kwargs=True) for m in ffs]
        try:
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                out = step.net(lq_val).float()
                for h in hooks:
                    h.remove()
                with chain():
                    ref = step.net(lq_val).float()
        finally:
            for h in hooks:
                h.remove()
        dims = {s[1] for s in spy["effn_fwd"][n0:]}
        assert {48, 96} <= dims, f"{tag}: the one-launch EFFN ran at d {sorted(dims)}"
        assert torch.isfinite(out).all() and torch.isfinite(ref).all()
        # the body's residual (the output minus the upsampled input), where every EFFN of the net lands
        e_net = _rel(out - up, ref - up)
        print(f"[graphed training] {tag}: rel-L2 one-launch vs chain: per EFFN " +
              ", ".join(f"d{d} {e:.1e}" + (f" (stale copies {st:.1e})" if st is not None else "") for d, e, st in rows) +
              f"; residual of the net {e_net:.2e}")
        for d, e, _ in rows:
            assert e <= tol, f"{tag}: an EFFN at d {d}, rel-L2 {e:.3e} against the chain on the live weights"
        assert e_net <= 2e-2, f"{tag}: the net's residual, rel-L2 {e_net:.3e} against the chain"
        return rows

    validate("before training")
    step(lq, gt)
    after = [validate("after replay 1"), None]
    step(lq, gt)
    after[1] = validate("after replay 2")
    # each replay moved the weights far enough that the copies of the previous validation would fail the check above
    assert all(st is not None and st > tol for rows in after for _, _, st in rows), after


# ---------------------------------------------------------------------------------------------------------------------------------
# B. gradients under partial freezing: grad mode on, a detached 16-bit stream
# ---------------------------------------------------------------------------------------------------------------------------------
_NAMES = ("norm2.weight", "norm2.bias", "project_in.weight", "dwconv.weight", "project_out.weight")
FROZEN_CASES = {"norm2.weight": ("norm2.weight",), "norm2.bias": ("norm2.bias",), "dwconv.weight": ("dwconv.weight",),
                "project_out.weight": ("project_out.weight",),
                "all_but_project_in": tuple(n for n in _NAMES if n != "project_in.weight")}


def _named(norm, ff):
    return dict(zip(_NAMES, (norm.body.weight, norm.body.bias, ff.project_in.weight, ff.dwconv.weight, ff.project_out.weight)))


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("case", list(FROZEN_CASES))
def test_partly_frozen_effn_keeps_the_gradients_of_its_trainable_parameters(case, dt, spy):
    shape = (1, 48, 24, 32)
    norm, ff = _modules(48, 40)
    x = _stream(shape, dt, 40)
    params = _named(norm, ff)
    trainable = FROZEN_CASES[case]
    for name, p in params.items():
        p.requires_grad_(name in trainable)
    with torch.no_grad():   # the same setup without grad mode: on the fast path's side of the predicate
        ff(x, pre_norm=norm)
    assert len(spy["effn_fwd"]) == 1, "no_grad takes the one-launch EFFN"
    out = ff(x, pre_norm=norm)
    assert len(spy["effn_fwd"]) == 1, "a trainable parameter under grad mode: the autograd chain, not the one-launch forward"
    assert out.grad_fn is not None
    dy = torch.randn(shape, generator=torch.Generator().manual_seed(41)).to(DEV).to(dt)
    out.backward(dy)
    grads = {}
    for name in trainable:
        assert params[name].grad is not None, f"{name}: no gradient"
        grads[name] = params[name].grad.clone()
    want_out = reference(x, norm, ff)
    # fp64 autograd from the same parameters, same upstream gradient
    leaves = {name: p.detach().double().requires_grad_() for name, p in params.items()}
    y64 = ffn64(x, leaves["norm2.weight"], leaves["norm2.bias"], leaves["project_in.weight"], leaves["dwconv.weight"],
                leaves["project_out.weight"])
    (y64 * dy.double()).sum().backward()
    # the yardstick: the training chain with every parameter trainable
    for p in params.values():
        p.requires_grad_(True)
        p.grad = None
    out_c = ff(x, pre_norm=norm)
    out_c.backward(dy)
    check_forward(out.detach(), want_out, out_c.detach(), f"{case} forward")
    for name in trainable:
        e, ec = _rel(grads[name], leaves[name].grad), _rel(params[name].grad, leaves[name].grad)
        print(f"[partly frozen] {case} {dt}: {name} rel-L2 {e:.2e} (chain {ec:.2e})")
        assert e <= GRAD_RL2[dt] and e <= 1.5 * ec + 1e-7, f"{name}: rel-L2 {e:.3e} vs fp64 (chain {ec:.3e})"


def test_streaming_gate_with_only_the_bias_trainable_keeps_its_gradient(spy):
    """``dwconv3x3_gelu_gate`` on a plane only the streaming forward takes (272 x 272 fp16: too large for the LDS-resident form)"""
    torch.manual_seed(50)
    dt = torch.float16
    conv = nn.Conv2d(6, 6, 3, padding=1, groups=6, bias=True).to(DEV)
    with torch.no_grad():
        conv.bias.normal_(0, 0.5)
    t = _stream((1, 6, 272, 272), dt, 50)
    assert not dw_ops.fused_ok(t, 2) and dw_ops.gate_fwd_ok(t)
    conv.weight.requires_grad_(False)

    def ref64(w, b):
        x1, x2 = F.conv2d(t.double(), w.double(), b.double(), padding=1, groups=6).chunk(2, dim=1)
        return F.gelu(x1) * x2

    with torch.no_grad():
        fast = ops.dwconv3x3_gelu_gate(t, conv)
    assert len(spy["dwgate_fwd"]) == 1, "no_grad takes the streaming forward"
    out = ops.dwconv3x3_gelu_gate(t, conv)
    assert len(spy["dwgate_fwd"]) == 1, "a trainable bias under grad mode: the autograd chain, not the streaming forward"
    assert out.grad_fn is not None
    dy = torch.randn(out.shape, generator=torch.Generator().manual_seed(51)).to(DEV).to(dt)
    out.backward(dy)
    assert conv.bias.grad is not None, "bias: no gradient"
    got = conv.bias.grad.clone()
    w64, b64 = conv.weight.detach().double(), conv.bias.detach().double().requires_grad_()
    want = ref64(w64, b64)
    (want * dy.double()).sum().backward()
    conv.weight.requires_grad_(True)
    conv.bias.grad = None
    out_c = ops.dwconv3x3_gelu_gate(t, conv)
    out_c.backward(dy)
    want = want.detach()
    rt = RT[dt]
    assert_close(fast, want, rt, rt * float(want.abs().max()) * 0.5, "streaming gate forward")
    assert_close(out, want, rt, rt * float(want.abs().max()) * 0.5, "gate forward under grad mode")
    e, ec = _rel(got, b64.grad), _rel(conv.bias.grad, b64.grad)
    print(f"[partly frozen] streaming gate: bias rel-L2 {e:.2e} (chain {ec:.2e})")
    assert e <= GRAD_RL2[dt] and e <= 1.5 * ec + 1e-7, (e, ec)


def test_block_with_only_project_out_trainable_gets_the_chain_gradient(spy):
    """fine-tuning the output projection of a pretrained block: one MamberBlock, everything frozen but ffn.project_out, on a bf16 stream
    under autocast (as the nets run it) -- the gradient equals the one with the one-launch EFFN switched off"""
    torch.manual_seed(60)
    blk = oss_block.MamberBlock(48).to(DEV)
    for p in blk.parameters():
        p.requires_grad_(False)
    w = blk.ffn.project_out.weight
    w.requires_grad_(True)
    x = _stream((1, 48, 24, 32), torch.bfloat16, 60)
    dy = torch.randn(x.shape, generator=torch.Generator().manual_seed(61)).to(DEV).to(torch.bfloat16)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with torch.no_grad():
            blk(x)
        assert len(spy["effn_fwd"]) == 1, "no_grad takes the one-launch EFFN"
        out = blk(x)
        assert len(spy["effn_fwd"]) == 1, "a trainable project_out under grad mode: the autograd chain"
        assert out.grad_fn is not None
        out.backward(dy.to(out.dtype))
        assert w.grad is not None, "project_out: no gradient"
        got = w.grad.clone()
        w.grad = None
        with chain():
            out_c = blk(x)
            out_c.backward(dy.to(out_c.dtype))
    assert float(got.abs().max()) > 0
    assert torch.equal(got, w.grad), f"max |diff| {float((got - w.grad).abs().max()):.3e}"
