"""The reference's pixel losses -- ``L1Loss``, ``MSELoss``, ``PSNRLoss`` (with ``toY``) and ``CharbonnierLoss``
(Deraining/basicsr/models/losses/losses.py:26-122) with ``weight_reduce_loss`` (losses/loss_util.py:25-54) -- as modules with the
reference's constructor and ``forward`` signatures and its argument errors, and ``from_options`` for the ``pixel_opt`` entry of an
options file (Deraining/Deraining/Options/*.yml:99-102; image_restoration_model.py:103-107).

Device tensors go through one ``torch.autograd.Function`` over ``torch.ops.vmambair.pixel_loss_fwd`` / ``pixel_loss_bwd``
(``oss_pixel_loss.hip``): two launches forward, one backward, every element widened to fp32, every sum in fp64 in a fixed order, the
loss one fp32 scalar, ``dpred`` in ``pred``'s dtype and only computed when ``pred`` needs a gradient.  The modules take the network's
own output dtype (``takes_network_dtype``: ``GraphedTrainStep`` then hands over ``out`` instead of ``out.float()``), with a target in
fp32 or in that dtype.

A plain-torch restatement of the same formulas, differentiated by autograd, serves CPU tensors, ``reduction='none'``, a ``target``
or ``weight`` that requires a gradient and whatever the library's query does not take (``ops.pixel_loss_ok``) -- as ``metrics.py``
does for CPU inputs.  Pinned by tests/golden/g12_losses.npz (tests/golden/make_golden_losses.py runs the reference's classes).
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import nn
from torch.nn import functional as F

from . import ops as _ops

_reduction_modes = ['none', 'mean', 'sum']
_TOY_COEF = (65.481, 128.553, 24.966)   # losses.py:92, held in a float32 tensor there
_PSNR_SCALE = 10 / math.log(10)         # losses.py:90


# ---------------------------------------------------------------------------------------------
# the restatement (dtype-preserving, like the reference: on float64 inputs it is the reference's arithmetic)
# ---------------------------------------------------------------------------------------------
def _weight_reduce(loss: torch.Tensor, weight: Optional[torch.Tensor], reduction: str) -> torch.Tensor:
    """loss_util.py:25-54"""
    if weight is not None:
        assert weight.dim() == loss.dim()
        assert weight.size(1) == 1 or weight.size(1) == loss.size(1)
        loss = loss * weight
    if weight is None or reduction == 'sum':
        return loss if reduction == 'none' else (loss.mean() if reduction == 'mean' else loss.sum())
    if reduction == 'mean':
        den = weight.sum() if weight.size(1) > 1 else weight.sum() * loss.size(1)
        loss = loss.sum() / den
    return loss


def restate_l1(pred, target, weight=None, reduction='mean', loss_weight=1.0):
    return loss_weight * _weight_reduce((pred - target).abs(), weight, reduction)


def restate_mse(pred, target, weight=None, reduction='mean', loss_weight=1.0):
    return loss_weight * _weight_reduce((pred - target) ** 2, weight, reduction)


def restate_charbonnier(pred, target, eps=1e-3):
    diff = pred - target
    return torch.mean(torch.sqrt((diff * diff) + (eps * eps)))


def restate_psnr(pred, target, loss_weight=1.0, toY=False):
    assert len(pred.size()) == 4
    if toY:
        coef = torch.tensor(_TOY_COEF).reshape(1, 3, 1, 1).to(pred.device)
        pred = (pred * coef).sum(dim=1).unsqueeze(dim=1) + 16.
        target = (target * coef).sum(dim=1).unsqueeze(dim=1) + 16.
        pred, target = pred / 255., target / 255.
    return loss_weight * _PSNR_SCALE * torch.log(((pred - target) ** 2).mean(dim=(1, 2, 3)) + 1e-8).mean()


# ---------------------------------------------------------------------------------------------
# the device form
# ---------------------------------------------------------------------------------------------
class _PixelLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, weight, kind, flags, loss_weight, eps):
        p, t = pred.detach().contiguous(), target.detach().contiguous()
        loss, stats = torch.ops.vmambair.pixel_loss_fwd(p, t, weight, kind, flags, loss_weight, eps)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(p, t, weight, stats)
            ctx.call = (kind, flags, loss_weight, eps)
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        p, t, weight, stats = ctx.saved_tensors
        g = grad_output.detach().to(torch.float32).contiguous()
        dpred = torch.ops.vmambair.pixel_loss_bwd(p, t, weight, stats, g, *ctx.call)
        return dpred, None, None, None, None, None, None


def _device_loss(pred, target, weight, kind, flags, loss_weight, eps):
    """the loss by the kernels, or None when this call is the restatement's"""
    if not (torch.is_tensor(pred) and torch.is_tensor(target) and pred.is_cuda and target.is_cuda and pred.dim() == 4):
        return None
    grad = torch.is_grad_enabled()
    if grad and (target.requires_grad or (weight is not None and weight.requires_grad)):
        return None
    if weight is not None:
        N, C, H, W = pred.shape
        if not (weight.is_cuda and tuple(weight.shape) in ((N, C, H, W), (N, 1, H, W))):
            return None
        flags |= _ops.losses.weight_flag(pred, weight)
        weight = weight.detach().float().contiguous()
    if not _ops.pixel_loss_ok(pred, target, kind, flags):
        return None
    return _PixelLossFn.apply(pred, target, weight, kind, flags, float(loss_weight), float(eps))


class _PixelLoss(nn.Module):
    #: the modules widen 16-bit predictions themselves: GraphedTrainStep passes the network's output as it is
    takes_network_dtype = True


class L1Loss(_PixelLoss):
    """L1 (mean absolute error) loss, losses.py:26-53: ``loss_weight * reduce(|pred - target| [* weight])``"""

    def __init__(self, loss_weight=1.0, reduction='mean'):
        super().__init__()
        if reduction not in ['none', 'mean', 'sum']:
            raise ValueError(f'Unsupported reduction mode: {reduction}. '
                             f'Supported ones are: {_reduction_modes}')
        self.loss_weight = loss_weight
        self.reduction = reduction

    _kind, _restate = _ops.losses.L1, staticmethod(restate_l1)

    def forward(self, pred, target, weight=None, **kwargs):
        """pred, target (N, C, H, W); weight (N, C, H, W) or (N, 1, H, W), optional"""
        if self.reduction != 'none':
            out = _device_loss(pred, target, weight, self._kind, _ops.losses.SUM if self.reduction == 'sum' else 0, self.loss_weight, 0.0)
            if out is not None:
                return out
        return self._restate(pred, target, weight, self.reduction, self.loss_weight)


class MSELoss(L1Loss):
    """MSE (L2) loss, losses.py:55-82: ``loss_weight * reduce((pred - target)^2 [* weight])``"""
    _kind, _restate = _ops.losses.MSE, staticmethod(restate_mse)


class PSNRLoss(_PixelLoss):
    """losses.py:84-109: ``loss_weight * 10 / ln 10 * mean_b ln(mse_b + 1e-8)``; ``toY``: on the BT.601 luma of 3-channel images"""

    def __init__(self, loss_weight=1.0, reduction='mean', toY=False):
        super().__init__()
        assert reduction == 'mean'
        self.loss_weight = loss_weight
        self.scale = _PSNR_SCALE
        self.toY = toY

    def forward(self, pred, target):
        assert len(pred.size()) == 4
        out = _device_loss(pred, target, None, _ops.losses.PSNR, _ops.losses.TOY if self.toY else 0, self.loss_weight, 0.0)
        return out if out is not None else restate_psnr(pred, target, self.loss_weight, self.toY)


class CharbonnierLoss(_PixelLoss):
    """losses.py:111-122: ``mean(sqrt((x - y)^2 + eps^2))``; ``loss_weight`` and ``reduction`` are accepted and unused, as there"""

    def __init__(self, loss_weight=1.0, reduction='mean', eps=1e-3):
        super().__init__()
        self.eps = eps

    def forward(self, x, y):
        out = _device_loss(x, y, None, _ops.losses.CHARBONNIER, 0, 1.0, self.eps)
        return out if out is not None else restate_charbonnier(x, y, self.eps)


def from_options(opt: dict) -> nn.Module:
    """the loss a ``pixel_opt`` entry names (``{type: L1Loss, loss_weight: 1, reduction: mean}``), built as the reference's model
    does (image_restoration_model.py:103-107); ``opt`` is left as it was"""
    opt = dict(opt)
    name = opt.pop('type')
    cls = {c.__name__: c for c in (L1Loss, MSELoss, PSNRLoss, CharbonnierLoss)}.get(name)
    if cls is None:
        raise ValueError(f'Unsupported pixel loss type: {name}. Supported ones are: L1Loss, MSELoss, PSNRLoss, CharbonnierLoss')
    return cls(**opt)


__all__ = ["L1Loss", "MSELoss", "PSNRLoss", "CharbonnierLoss", "from_options"]
