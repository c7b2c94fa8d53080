"""``vmambair_amd.losses`` on the device (``oss_pixel_loss.hip`` through ``torch.ops.vmambair.pixel_loss_fwd`` / ``_bwd``): the
reference's float64 losses and gradients of tests/golden/g12_losses.npz, the launch geometry against the float64 restatement,
reproducibility, graph capture, argument checks and the captured training step with the device loss.

Tolerances (set by the arithmetic, not by what the kernels give):
  loss      |got - want| <= 1e-6 |want| for L1, MSE, Charbonnier: every positive term carries at most about 4 fp32 roundings of 2^-24,
            the sums are fp64, the result is rounded once to fp32.  PSNR additionally atol 5e-6: a relative error of mse_b is an
            absolute one of its logarithm, times 10 / ln 10.
  gradient  fp32 pred: rtol 1e-6, atol 1e-6 max|want|.  16-bit pred: one unit in the last place of that type -- rtol 2^-10 (fp16) /
            2^-7 (bf16) and the same fraction of max|want| as atol -- of the float64 formula on the widened 16-bit inputs.  Where the
            shapes of this file push an fp16 gradient below fp16's smallest normal number (2^-14) the spacing is 2^-24 whatever the
            value, so half of that is added for fp16.
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from test_losses_host import cell_inputs, cell_module, golden_cells
from vmambair_amd import losses, ops

pytestmark = pytest.mark.gpu
selfcheck = pytest.mark.selfcheck
DEV = "cuda:0"
#: (pred dtype, target dtype); the last one is the training step's
DTYPES = ((torch.float32, torch.float32), (torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32))
GRAD_RTOL = {torch.float32: 1e-6, torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}


def check(what, psnr, pred_dtype, loss, grad, want_loss, want_grad):
    assert loss.dtype == torch.float32 and loss.dim() == 0 and grad.dtype == pred_dtype and grad.shape == want_grad.shape
    got, want = float(loss), float(want_loss)
    tol = 1e-6 * abs(want) + (5e-6 if psnr else 0.0)
    print(f"[{what}] loss {got:.9g} want {want:.9g} |diff| {abs(got - want):.2e} (tol {tol:.2e})")
    assert abs(got - want) <= tol, what
    rtol = GRAD_RTOL[pred_dtype]
    g, w = grad.double(), want_grad.double().to(grad.device)
    lim = rtol * w.abs() + rtol * float(w.abs().max()) + (2.0 ** -25 if pred_dtype == torch.float16 else 0.0)
    over = ((g - w).abs() - lim).max()
    print(f"[{what}] grad max|diff| {float((g - w).abs().max()):.2e} max|want| {float(w.abs().max()):.2e} worst excess {float(over):.2e}")
    assert float(over) <= 0.0, what


def run(module, pred, target, w):
    pred = pred.detach().requires_grad_(True)
    loss = module(pred, target, *w)
    grad, = torch.autograd.grad(loss, pred)
    return loss.detach(), grad


def want64(module, pred, target, w):
    """the float64 restatement on the widened inputs, on the device (float64 tensors are not the kernels')"""
    return run(module, pred.double(), target.double(), [x.double() for x in w])


@pytest.mark.tier(0)
@pytest.mark.parametrize("s, cell", golden_cells())
def test_kernels_match_the_reference_golden(s, cell):
    z = load_golden("g12_losses.npz")
    module, weight = cell_module(cell)
    for pd, td in DTYPES:
        pred, target, w = cell_inputs(z, s, weight, torch.float32, DEV)
        pred, target = pred.to(pd), target.to(td)
        assert ops.pixel_loss_ok(pred, target, 0, 0)
        loss, grad = run(module, pred, target, w)
        if pd == torch.float32:
            want_loss, want_grad = z[f"{s}.{cell}.loss"], z[f"{s}.{cell}.grad"]
        else:   # G12's formula (tests/test_losses_host.py pins the restatement to it at 1e-12) on the widened 16-bit inputs
            want_loss, want_grad = want64(module, pred, target, w)
        check(f"{s}.{cell} {pd}/{td}", cell.startswith("psnr"), pd, loss, grad, want_loss, want_grad)
        if cell.startswith("l1"):
            assert bool((grad[pred.float() == target.float()] == 0).all()), "sign(0) = 0"


SHAPES = ((1, 3, 1, 1), (2, 3, 5, 7), (3, 1, 4, 8), (2, 3, 33, 65), (2, 3, 67, 129))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_launch_geometry_against_the_float64_restatement(shape):
    """one lane, one workgroup, several workgroups with a ragged tail, images that start off a 16-byte boundary (the element-wise
    loads) and per-image sums whose workgroups end inside the tensor (2048 elements per workgroup: 25,929 per image is 13)"""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(n * 1000 + h * w)
    target = torch.rand(shape, generator=g)
    pred = target + 0.1 * torch.randn(shape, generator=g)
    pred = torch.where(torch.rand(shape, generator=g) < 0.1, target, pred)
    w4, w1 = torch.rand(shape, generator=g).to(DEV), torch.rand((n, 1, h, w), generator=g).to(DEV)
    cells = [("l1 mean", losses.L1Loss(), []), ("l1 sum w4", losses.L1Loss(reduction="sum"), [w4]),
             ("mse mean w1", losses.MSELoss(loss_weight=0.5), [w1]), ("mse sum", losses.MSELoss(reduction="sum"), []),
             ("l1 mean w1", losses.L1Loss(), [w1]), ("charb", losses.CharbonnierLoss(), []), ("psnr", losses.PSNRLoss(), [])]
    if c == 3:
        cells.append(("psnr y", losses.PSNRLoss(loss_weight=2.0, toY=True), []))
    for pd, td in DTYPES:
        p, t = pred.to(DEV).to(pd), target.to(DEV).to(td)
        for name, module, wt in cells:
            loss, grad = run(module, p, t, wt)
            check(f"{shape} {name} {pd}/{td}", name.startswith("psnr"), pd, loss, grad, *want64(module, p, t, wt))


def _inputs(shape=(2, 3, 33, 65), dtype=torch.bfloat16, seed=0):
    g = torch.Generator().manual_seed(seed)
    target = torch.rand(shape, generator=g).to(DEV)
    pred = (target + 0.1 * torch.randn(shape, generator=g).to(DEV)).to(dtype)
    return pred, target


def _modules():
    return (losses.L1Loss(), losses.MSELoss(reduction="sum"), losses.CharbonnierLoss(), losses.PSNRLoss(), losses.PSNRLoss(toY=True))


def test_reruns_are_bit_identical():
    pred, target = _inputs()
    w1 = torch.rand(2, 1, 33, 65, device=DEV)
    for module, wt in [(m, []) for m in _modules()] + [(losses.L1Loss(), [w1])]:
        first = run(module, pred, target, wt)
        for _ in range(3):
            again = run(module, pred, target, wt)
            assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])


def test_grad_output_scales_dpred():
    pred, target = _inputs(dtype=torch.float32)
    for module in _modules():
        _, one = run(module, pred, target, [])
        p = pred.detach().requires_grad_(True)
        (2.5 * module(p, target)).backward()
        torch.testing.assert_close(p.grad, 2.5 * one, rtol=1e-6, atol=0.0)   # a few fp32 roundings apart (the factor is rounded once per side)


def test_no_backward_without_requires_grad():
    pred, target = _inputs()
    for module in _modules():
        with_grad, _ = run(module, pred, target, [])
        plain = module(pred, target)
        assert not plain.requires_grad and plain.grad_fn is None and torch.equal(plain, with_grad)
        with torch.no_grad():
            assert torch.equal(module(pred.detach().requires_grad_(True), target), with_grad)


def test_non_contiguous_inputs_and_fallbacks():
    pred, target = _inputs(dtype=torch.float32)
    base = torch.zeros(2, 3, 33, 70, device=DEV)
    base[..., :65] = pred
    view = base[..., :65]
    assert not view.is_contiguous()
    m = losses.MSELoss()
    want = run(m, pred, target, [])
    got = run(m, view, target, [])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # what the kernels do not take is the restatement's: reduction 'none', a target that needs a gradient, a 16-bit target next to fp32
    assert losses.L1Loss(reduction="none")(pred, target).shape == pred.shape
    t = target.clone().requires_grad_(True)
    m(pred, t).backward()
    torch.testing.assert_close(t.grad, -2 * (pred - target) / pred.numel())
    assert not ops.pixel_loss_ok(pred, target.half(), 1, 0)
    torch.testing.assert_close(m(pred, target.half()), F.mse_loss(pred, target.half().float()))


def test_forward_and_backward_inside_a_captured_graph():
    for module in (losses.L1Loss(), losses.PSNRLoss(toY=True)):
        a, b = _inputs(seed=1), _inputs(seed=2)
        sp, st = a[0].clone().requires_grad_(True), a[1].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            torch.autograd.grad(module(sp, st), sp)   # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            loss = module(sp, st)
            grad, = torch.autograd.grad(loss, sp)
        for pred, target in (a, b, a):
            with torch.no_grad():
                sp.copy_(pred)
                st.copy_(target)
            g.replay()
            torch.cuda.synchronize()
            fresh = run(module, pred, target, [])
            assert torch.equal(loss, fresh[0]) and torch.equal(grad, fresh[1])
        assert not torch.equal(run(module, *a, [])[0], run(module, *b, [])[0])


def test_raw_ops_refuse_bad_arguments():
    fwd, bwd = torch.ops.vmambair.pixel_loss_fwd, torch.ops.vmambair.pixel_loss_bwd
    pred, target = _inputs(dtype=torch.float32)
    loss, stats = fwd(pred, target, None, 0, 0, 1.0, 0.0)
    one = torch.ones((), device=DEV)
    assert bwd(pred, target, None, stats, one, 0, 0, 1.0, 0.0).shape == pred.shape
    with pytest.raises(RuntimeError):
        fwd(pred.cpu(), target.cpu(), None, 0, 0, 1.0, 0.0)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        ops.pixel_loss_fwd(pred, target.cpu(), None, 0, 0, 1.0, 0.0)
    with pytest.raises(RuntimeError, match="one shape"):
        fwd(pred, target[:, :, :32], None, 0, 0, 1.0, 0.0)
    with pytest.raises(RuntimeError, match="contiguous"):
        fwd(pred.transpose(2, 3), target.transpose(2, 3), None, 0, 0, 1.0, 0.0)
    w = torch.ones_like(pred)
    with pytest.raises(RuntimeError, match="fp32"):
        fwd(pred, target, w.half(), 0, 4, 1.0, 0.0)
    with pytest.raises(RuntimeError, match="weight"):
        fwd(pred, target, w, 0, 8, 1.0, 0.0)          # a (N, C, H, W) weight under the one-channel flag
    with pytest.raises(RuntimeError, match="weight"):
        fwd(pred, target, w, 0, 0, 1.0, 0.0)          # a weight without a flag
    with pytest.raises(RuntimeError, match="not supported"):
        fwd(pred, target, w, 3, 4, 1.0, 0.0)          # PSNR takes no weight
    with pytest.raises(RuntimeError, match="not supported"):
        fwd(pred[:, :1].contiguous(), target[:, :1].contiguous(), None, 3, 2, 1.0, 0.0)   # toY needs three channels
    with pytest.raises(RuntimeError, match="stats"):
        bwd(pred, target, None, stats.float(), one, 0, 0, 1.0, 0.0)
    with pytest.raises(RuntimeError, match="grad_output"):
        bwd(pred, target, None, stats, torch.ones(2, device=DEV), 0, 0, 1.0, 0.0)


def make_net(seed=0, dim=8):
    from vmambair_amd.archs import Mamber32
    torch.manual_seed(seed)
    return Mamber32(dim=dim, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1).to(DEV)


@selfcheck
@pytest.mark.parametrize("autocast", [None, torch.bfloat16], ids=["fp32", "bf16"])
def test_graphed_step_with_the_device_loss_matches_the_default_loss(autocast):
    """the net, the inputs and the tolerances of tests/test_train_graph_gpu.py::test_graphed_deraining_step_matches_eager"""
    from vmambair_amd.train_graph import GraphedTrainStep
    torch.manual_seed(3)
    lq, gt = torch.rand(2, 3, 32, 32, device=DEV), torch.rand(2, 3, 32, 32, device=DEV)
    net_d, net_t = make_net(), make_net()
    kw = dict(lr=3e-4, betas=(0.9, 0.999), ema_decay=0.0, autocast_dtype=autocast, warmup=1, weight_decay=1e-4, clip_grad_norm=0.01)
    step_d = GraphedTrainStep(net_d, loss_fn=losses.L1Loss(), **kw)
    step_t = GraphedTrainStep(net_t, loss_fn=F.l1_loss, **kw)
    for i in range(3):
        ld, lt = float(step_d(lq, gt)), float(step_t(lq, gt))
        print(f"step {i}: device loss {ld:.9g}, torch loss {lt:.9g}")
        assert ld == pytest.approx(lt, rel=2e-3), i
    same = True
    for (k, p), q in zip(net_d.named_parameters(), net_t.parameters()):
        same = same and torch.equal(p, q)
        assert float((p - q).abs().max()) <= 2 * 3e-4 * 3 + 1e-5, k
    print(f"parameters bit-identical after 3 steps ({'fp32' if autocast is None else 'bf16 autocast'}): {same}")
