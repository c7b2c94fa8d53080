"""``vmambair_amd.losses`` without a GPU: the plain-torch restatement of the reference's pixel losses against
tests/golden/g12_losses.npz (tests/golden/make_golden_losses.py runs the reference's classes on float64 copies of the stored inputs),
the reference's argument errors, ``from_options`` and the library's support query.  The kernels: tests/test_losses_gpu.py."""
import pytest
import torch

from conftest import load_golden
from vmambair_amd import _capi, losses

BF16, F16, F32 = _capi.OSS_BF16, _capi.OSS_F16, _capi.OSS_F32
K = _capi.LOSS


def golden_cells():
    """-> [(set name, cell name)] of g12_losses.npz"""
    z = load_golden("g12_losses.npz")
    return sorted({tuple(k.split(".", 1)[0:1] + [k.split(".", 1)[1][:-len(".loss")]]) for k in z if k.endswith(".loss")})


def cell_module(cell):
    """the module and the name of the weight ('none', 'w4', 'w1') a G12 cell name stands for"""
    parts = cell.split("_")
    kw, weight = {}, "none"
    for p in list(parts):
        if p.startswith("lw"):
            kw["loss_weight"] = float(p[2:])
            parts.remove(p)
        elif p.startswith("eps"):
            kw["eps"] = float(p[3:])
            parts.remove(p)
    if parts[0] in ("l1", "mse"):
        weight = parts[2]
        return (losses.L1Loss if parts[0] == "l1" else losses.MSELoss)(reduction=parts[1], **kw), weight
    if parts[0] == "charb":
        return losses.CharbonnierLoss(**kw), weight
    assert parts[0] == "psnr"
    return losses.PSNRLoss(toY=parts[1:] == ["y"], **kw), weight


def cell_inputs(z, s, weight, dtype=torch.float64, device="cpu"):
    pred, target = z[f"{s}.pred"].to(device=device, dtype=dtype), z[f"{s}.target"].to(device=device, dtype=dtype)
    return pred, target, ([] if weight == "none" else [z[f"{s}.{weight}"].to(device=device, dtype=dtype)])


def test_fixture_covers_the_grid():
    z = load_golden("g12_losses.npz")
    cells = golden_cells()
    assert tuple(z["a.pred"].shape) == (2, 3, 5, 7) and tuple(z["b.pred"].shape) == (3, 1, 4, 8)
    assert tuple(z["a.w4"].shape) == (2, 3, 5, 7) and tuple(z["a.w1"].shape) == (2, 1, 5, 7)
    for s in ("a", "b", "c"):
        assert z[f"{s}.pred"].dtype == torch.float32
        assert int((z[f"{s}.pred"] == z[f"{s}.target"]).sum()) >= 3, "tied elements pin sign(0) = 0"
        names = {c for t, c in cells if t == s}
        for kind in ("l1", "mse"):
            for red in ("mean", "sum"):
                for w in ("none", "w4", "w1"):
                    assert f"{kind}_{red}_{w}" in names
        assert {"charb", "psnr", "l1_mean_w1_lw0.5", "mse_sum_none_lw2.5", "charb_lw3.0", "psnr_lw0.5"} <= names
    assert ("a", "psnr_y") in cells and ("c", "psnr_y") in cells and ("b", "psnr_y") not in cells


@pytest.mark.parametrize("s, cell", golden_cells())
def test_restatement_reproduces_the_reference_golden(s, cell):
    z = load_golden("g12_losses.npz")
    module, weight = cell_module(cell)
    pred, target, w = cell_inputs(z, s, weight)
    pred.requires_grad_(True)
    loss = module(pred, target, *w)
    grad, = torch.autograd.grad(loss, pred)
    torch.testing.assert_close(loss.detach(), z[f"{s}.{cell}.loss"], rtol=1e-12, atol=0.0)
    want = z[f"{s}.{cell}.grad"]
    torch.testing.assert_close(grad, want, rtol=1e-12, atol=1e-12 * float(want.abs().max()))
    if cell.startswith("l1"):
        assert bool((grad[pred.detach() == target] == 0).all())


def test_reduction_none_and_target_gradients_are_the_restatement():
    z = load_golden("g12_losses.npz")
    pred, target, (w1,) = cell_inputs(z, "a", "w1", torch.float32)
    out = losses.L1Loss(reduction="none")(pred, target, w1)
    assert out.shape == pred.shape and torch.equal(out, (pred - target).abs() * w1)
    out = losses.MSELoss(loss_weight=2.0, reduction="none")(pred, target)
    assert torch.equal(out, 2.0 * (pred - target) ** 2)
    target.requires_grad_(True)
    losses.MSELoss()(pred, target).backward()
    torch.testing.assert_close(target.grad, -2 * (pred - target.detach()) / pred.numel())


def test_argument_errors_match_the_reference():
    for cls in (losses.L1Loss, losses.MSELoss):
        with pytest.raises(ValueError, match="Unsupported reduction mode: avg"):
            cls(reduction="avg")
        assert cls(reduction="none").reduction == "none"
    with pytest.raises(AssertionError):
        losses.PSNRLoss(reduction="sum")
    with pytest.raises(AssertionError):
        losses.PSNRLoss()(torch.zeros(3, 4, 4), torch.zeros(3, 4, 4))
    with pytest.raises(TypeError):
        losses.PSNRLoss()(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), torch.ones(1, 3, 4, 4))   # no weight argument there
    with pytest.raises(AssertionError):
        losses.L1Loss()(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), torch.ones(1, 2, 4, 4))   # loss_util.py:40
    c = losses.CharbonnierLoss(loss_weight=3.0, reduction="sum", eps=1e-2)   # accepted and unused, as in the reference
    assert c.eps == 1e-2 and not hasattr(c, "loss_weight")
    for m in (losses.L1Loss(), losses.MSELoss(), losses.PSNRLoss(), c):
        assert m.takes_network_dtype is True and isinstance(m, torch.nn.Module)


def test_from_options():
    opt = {"type": "L1Loss", "loss_weight": 1, "reduction": "mean"}
    m = losses.from_options(opt)
    assert type(m) is losses.L1Loss and m.loss_weight == 1 and m.reduction == "mean"
    assert opt == {"type": "L1Loss", "loss_weight": 1, "reduction": "mean"}
    m = losses.from_options({"type": "PSNRLoss", "loss_weight": 0.5, "toY": True})
    assert type(m) is losses.PSNRLoss and m.toY is True and m.loss_weight == 0.5
    assert type(losses.from_options({"type": "MSELoss", "reduction": "sum"})) is losses.MSELoss
    assert losses.from_options({"type": "CharbonnierLoss", "eps": 1e-2}).eps == 1e-2
    with pytest.raises(ValueError, match="PerceptualLoss"):
        losses.from_options({"type": "PerceptualLoss"})
    with pytest.raises(ValueError):
        losses.from_options({"type": "L1Loss", "reduction": "avg"})


def test_support_query_is_a_pure_host_function():
    lib = _capi.load()
    q, st = lib.oss_pixel_loss_partial_doubles, lib.oss_pixel_loss_stat_doubles
    L1, MSE, CH, PSNR = K["L1"], K["MSE"], K["CHARBONNIER"], K["PSNR"]
    SUM, TOY, W4, W1 = K["SUM"], K["TOY"], K["WEIGHT"], K["WEIGHT_1CH"]
    assert (L1, MSE, CH, PSNR, SUM, TOY, W4, W1) == (0, 1, 2, 3, 1, 2, 4, 8)
    # one double per 2048 elements (of an image for PSNR), two with a weight
    assert q(L1, 0, BF16, F32, 8, 3, 256 * 256) == 8 * 3 * 256 * 256 // 2048
    assert q(MSE, SUM | W1, F32, F32, 2, 3, 67 * 129) == 2 * 26 and q(L1, W4, F16, F16, 1, 3, 1) == 2
    assert q(PSNR, 0, F32, F32, 2, 3, 67 * 129) == 2 * 13 and q(PSNR, TOY, BF16, BF16, 2, 3, 67 * 129) == 2 * 5
    assert q(CH, 0, F16, F32, 3, 1, 32) == 1
    assert st(L1, 0, 8, 3, 65536) == 1 and st(PSNR, TOY, 8, 3, 65536) == 8 and st(PSNR, TOY, 8, 1, 65536) == 0
    # toY needs three channels and PSNR
    assert q(PSNR, TOY, F32, F32, 2, 1, 64) == 0 and q(PSNR, TOY, F32, F32, 2, 4, 64) == 0 and q(MSE, TOY, F32, F32, 2, 3, 64) == 0
    # a weight or a sum goes with L1 and MSE only
    for kind in (PSNR, CH):
        assert q(kind, W4, F32, F32, 2, 3, 64) == 0 and q(kind, W1, F32, F32, 2, 3, 64) == 0 and q(kind, SUM, F32, F32, 2, 3, 64) == 0
    assert q(L1, W4 | W1, F32, F32, 2, 3, 64) == 0
    # dtypes: no element type (3 = OSS_F32_BF16X3, 7, -1), or a 16-bit target that is not pred's type
    for bad in (3, 7, -1):
        assert q(L1, 0, bad, F32, 2, 3, 64) == 0 and q(L1, 0, F32, bad, 2, 3, 64) == 0 and q(PSNR, 0, bad, bad, 2, 3, 64) == 0
    assert q(L1, 0, F32, BF16, 2, 3, 64) == 0 and q(L1, 0, F16, BF16, 2, 3, 64) == 0 and q(L1, 0, BF16, BF16, 2, 3, 64) == 1
    # unknown kinds and flags, empty shapes, more workgroups than a grid holds
    assert q(4, 0, F32, F32, 2, 3, 64) == 0 and q(-1, 0, F32, F32, 2, 3, 64) == 0 and q(L1, 16, F32, F32, 2, 3, 64) == 0
    assert q(L1, 0, F32, F32, 0, 3, 64) == 0 and q(L1, 0, F32, F32, 2, 0, 64) == 0 and q(L1, 0, F32, F32, 2, 3, 0) == 0
    assert q(L1, 0, F32, F32, 1 << 20, 1 << 10, 1 << 12) == 0 and q(L1, 0, F32, F32, 1, 1, 1 << 41) == 0   # 64-bit counts, capped at 2^40
    assert q(L1, 0, F32, F32, 1, 1, 1 << 40) == 1 << 29 and q(PSNR, 0, F32, F32, 1 << 20, 1, 1 << 20) == 1 << 29
    # the entry points refuse the same without touching the device: NULL pointers first, then the shape
    assert lib.oss_pixel_loss_fwd(L1, 0, F32, F32, None, None, None, None, None, None, 2, 3, 64, 1.0, 0.0, None) == _capi._K["OSS_ERR_NULL"]
    assert lib.oss_pixel_loss_bwd(L1, 0, F32, F32, None, None, None, None, None, None, 2, 3, 64, 1.0, 0.0, None) == _capi._K["OSS_ERR_NULL"]


def test_raw_ops_have_no_cpu_kernel():
    cpu = torch.zeros(1, 3, 4, 4)
    with pytest.raises(RuntimeError):
        torch.ops.vmambair.pixel_loss_fwd(cpu, cpu, None, 0, 0, 1.0, 0.0)
    with pytest.raises(RuntimeError):
        torch.ops.vmambair.pixel_loss_bwd(cpu, cpu, None, torch.zeros(1, dtype=torch.float64), torch.ones(()), 0, 0, 1.0, 0.0)
    # CPU tensors are the restatement's
    assert float(losses.L1Loss()(cpu + 1, cpu)) == 1.0
