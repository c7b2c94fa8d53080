"""Torch-facing boundary of the HIP selective scan: ``torch.ops.vmambair.selective_scan_fwd / _bwd``.

The host half of the reference's native module (Mamba/kernels/selective_scan/csrc/selective_scan/cus/selective_scan.cpp:157-349)
-- dtype / shape / stride checks raising ``RuntimeError``, outputs allocated by the callee, parameter structs, launch on the
current stream of ``u``'s device without host synchronisation -- is compiled: ``csrc_host/oss_torch_host.cpp``, loaded by
``_host.ops()`` as ``torch.ops.vmambair_host.scan_fwd / scan_bwd``.  It is the only host path; a missing or stale library is an
error.  This module keeps the reference's positional signatures in front of it: it encodes ``tune=`` / ``scan_tuning`` into the
per-call fields, asks the library for the optional scan forms, hands everything to the compiled operator and shapes the result
(``None`` for absent gradients, the ``dB`` / ``dC`` views of ``dbc_into``).  Differences from the reference, all invisible to
callers:
  * ``x`` holds one saved state every ``scan_chunk()`` = 256 steps instead of 2048;
  * ``bwd`` needs no zero-filled outputs and returns ``dB``/``dC`` already in the input dtype
    (the reference zero-fills five tensors and casts two, :319-327,347);
  * ``nrows`` is accepted and ignored (the reference archs always end up with 1,
    SRGAN/VmambaIR/archs/MambaSISR6_arch.py:57,69).
Beyond the reference's signature (keyword-only, used by the fused spatial core): ``dt_weight`` -- delta computed INSIDE the
scan from the rank-R rows of x_dbl (include/vmambair_oss.h), so the (batch, 4 D, L) delta / ddelta tensors never exist.

No CPU implementation exists: CPU tensors are rejected exactly as the reference rejects them
(``TORCH_CHECK(u.is_cuda())``, :174).
"""
from __future__ import annotations

import contextlib
import os
import threading
from typing import List, Optional

import torch

from .. import _capi, _host
from ._common import _DT, _LIB, _check

#: ``VMAMBAIR_SCAN_LANE_STATES=1``: the autograd nodes of this package ask the forward scan for lane states (the state entering
#: every 8-step block) and the backward loads them instead of re-running the forward recurrence from ``x``.  Default OFF: measured
#: slower on the headline (forward kernel +7 %, backward -1 %).  The C ABI and ``selective_scan_fwd(want_hs=True)``
#: take the form regardless of this switch.
LANE_STATES = os.environ.get("VMAMBAIR_SCAN_LANE_STATES", "0") == "1"

_TLS = threading.local()


@contextlib.contextmanager
def scan_tuning(fwd: Optional[tuple] = None, bwd: Optional[tuple] = None):
    """Per-thread DEFAULT launch shape of the scan calls issued inside the context by code that does not pass ``tune=`` itself (the
    block / net modules): ``fwd`` / ``bwd`` = ``(variant, segments, carry_split[, partials])`` as ``selective_scan_fwd / _bwd(tune=)``
    take them.  It ends up in the per-call fields of the params structs (include/vmambair_oss.h: tune_*), never in the library's
    process-global setters -- so it is safe next to other threads and streams, and a hipGraph captured inside keeps the shape.
    Used by infer.TiledSR(concurrent_shapes=True): four forwards side by side already fill the GPU, so their scans must not be cut
    into time segments (the heuristic only sees ONE call's workgroup count)."""
    old = (getattr(_TLS, "fwd", None), getattr(_TLS, "bwd", None))
    _TLS.fwd, _TLS.bwd = fwd, bwd
    try:
        yield
    finally:
        _TLS.fwd, _TLS.bwd = old


def _tune_fields(tune):
    """``(variant, segments, carry_split[, partials])`` with None = heuristic -> the C struct's encoding (0 = heuristic,
    variant + 1; partials "bf16" -> oss_scan_bwd_params.tune_partials = 2, backward only: bf16 row-tile partials, opt-in)"""
    if tune is None:
        return 0, 0, 0, 0
    v, s, c, f = (tuple(tune) + (None, None, None, None))[:4]
    return ((0 if v is None or v < 0 else int(v) + 1), (0 if s is None or s < 0 else max(1, int(s))), (0 if c is None or c <= 0 else int(c)),
            (2 if f == "bf16" else 0))


def selective_scan_fwd(u: torch.Tensor, delta: torch.Tensor, A: torch.Tensor, B: torch.Tensor, C: torch.Tensor,
                       D: Optional[torch.Tensor], delta_bias: Optional[torch.Tensor], delta_softplus: bool,
                       nrows: int = 1, rev_group_start: Optional[int] = None, u_row_mod: int = 0,
                       a_log_form: bool = False, dt_weight: Optional[torch.Tensor] = None,
                       want_hs: bool = False, tune: Optional[tuple] = None) -> List[torch.Tensor]:
    """``selective_scan_cuda_core.fwd`` (cus/selective_scan.cpp:157-239) -> ``[out, x]``.
    ``rev_group_start`` / ``u_row_mod``: omni-scan direction handling; ``dt_weight``: ``delta`` is the rank-R factor and the
    kernels evaluate delta themselves -- see include/vmambair_oss.h.  ``want_hs``: -> ``[out, x, hs]`` with the lane states
    (the state entering every 8-step block) for ``selective_scan_bwd(..., hs=hs)``.  ``tune``: per-call launch shape
    ``(variant or None, segments or None, carry_split or None)`` -> ``oss_scan_fwd_params.tune_*`` (None = heuristic)."""
    tv, ts, tc, _ = _tune_fields(tune if tune is not None else getattr(_TLS, "fwd", None))
    if want_hs:
        _capi.require_feature(_capi.FEATURE_LANE_STATES, "selective_scan_fwd(want_hs=True)")
    if dt_weight is not None:
        _capi.require_feature(_capi.FEATURE_FUSED_DT, "selective_scan_fwd(dt_weight=...)")
    _check(u.is_cuda, "u must be a CUDA/HIP tensor")
    return list(_host.ops().scan_fwd(u, delta, A, B, C, D, delta_bias, bool(delta_softplus),
                                     -1 if rev_group_start is None else int(rev_group_start), int(u_row_mod), bool(a_log_form), dt_weight,
                                     bool(want_hs), tv, ts, tc))


def selective_scan_bwd(u: torch.Tensor, delta: torch.Tensor, A: torch.Tensor, B: torch.Tensor, C: torch.Tensor,
                       D: Optional[torch.Tensor], delta_bias: Optional[torch.Tensor], dout: torch.Tensor,
                       x: Optional[torch.Tensor], delta_softplus: bool, nrows: int = 1,
                       rev_group_start: Optional[int] = None, u_row_mod: int = 0,
                       dout_row_mod: int = 0, a_log_form: bool = False,
                       dbc_into: Optional[torch.Tensor] = None,
                       dt_weight: Optional[torch.Tensor] = None,
                       hs: Optional[torch.Tensor] = None, tune: Optional[tuple] = None,
                       finish_dt_weight: Optional[torch.Tensor] = None) -> List[Optional[torch.Tensor]]:
    """``selective_scan_cuda_core.bwd`` (cus/selective_scan.cpp:241-349) ->
    ``[du, ddelta, dA, dB, dC, dD, ddelta_bias]`` (the last two ``None`` when absent).  In the omni
    form ``du`` has ``dim`` rows (one per direction); the caller adds the rows that share ``u``.
    With ``dt_weight`` (delta computed inside the scan; needs ``dbc_into``): ``ddelta`` is ``None``, the gradient of the rank
    factor lands in the first R rows of ``dbc_into`` and an eighth entry, the (dim, R) gradient of ``dt_weight``, is returned.
    ``finish_dt_weight`` (dim, R) fp32 (needs ``dbc_into``, not together with ``dt_weight``): ``ddelta`` is returned as usual AND the
    finishing launch fills the first R rows of ``dbc_into`` with ``dt_projs_weight^T . ddelta`` -- the dt rows of the gradient of
    x_dbl, which ``oss_proj_dgrad`` is then not asked for (include/vmambair_oss.h: oss_scan_bwd_params.finish_dt_weight)."""
    tv, ts, tc, tp = _tune_fields(tune if tune is not None else getattr(_TLS, "bwd", None))
    _check(u.is_cuda, "u must be a CUDA/HIP tensor")
    # -> [du, ddelta, dA, dB, dC, dD, dbias, ddt_weight], empty = absent
    du, ddelta, dA, dB, dC, dD, dbias, ddtw = _host.ops().scan_bwd(
        u, delta, A, B, C, D, delta_bias, dout, x, bool(delta_softplus), -1 if rev_group_start is None else int(rev_group_start),
        int(u_row_mod), int(dout_row_mod), bool(a_log_form), dbc_into, dt_weight, hs, tv, ts, tc, tp, finish_dt_weight)
    if dbc_into is not None:   # written in place (a mutated argument is not returned): the views are made here
        rows, N = dbc_into.shape[2], A.shape[1]
        dB, dC = dbc_into[:, :, rows - 2 * N:rows - N], dbc_into[:, :, rows - N:]
    fused = dt_weight is not None
    return [du, None if fused else ddelta, dA, dB, dC, dD if D is not None else None,
            dbias if delta_bias is not None else None] + ([ddtw] if fused else [])


_LIB.define("selective_scan_fwd(Tensor u, Tensor delta, Tensor A, Tensor B, Tensor C, Tensor? D, "
            "Tensor? delta_bias, bool delta_softplus, int nrows) -> Tensor[]")
_LIB.define("selective_scan_bwd(Tensor u, Tensor delta, Tensor A, Tensor B, Tensor C, Tensor? D, "
            "Tensor? delta_bias, Tensor dout, Tensor? x, bool delta_softplus, int nrows) -> Tensor[]")


def _fwd_op(u, delta, A, B, C, D, delta_bias, delta_softplus, nrows):
    return selective_scan_fwd(u, delta, A, B, C, D, delta_bias, delta_softplus, nrows)


def _bwd_op(u, delta, A, B, C, D, delta_bias, dout, x, delta_softplus, nrows):
    res = selective_scan_bwd(u, delta, A, B, C, D, delta_bias, dout, x, delta_softplus, nrows)
    # Tensor[] cannot hold None: absent dD / ddelta_bias come back as empty tensors, like the
    # reference's undefined at::Tensor (cus/selective_scan.cpp:323-326)
    return [t if t is not None else u.new_empty(0, dtype=torch.float32) for t in res]


_LIB.impl("selective_scan_fwd", _fwd_op, "CUDA")
_LIB.impl("selective_scan_bwd", _bwd_op, "CUDA")

# omni form: time-mirrored groups and shared u rows handled inside the kernels (no xs / flips)
_LIB.define("omni_scan_fwd(Tensor u, Tensor delta, Tensor A_log, Tensor B, Tensor C, Tensor? D, Tensor? delta_bias, "
            "bool delta_softplus, int rev_group_start, int u_row_mod) -> Tensor[]")
_LIB.define("omni_scan_bwd(Tensor u, Tensor delta, Tensor A_log, Tensor B, Tensor C, Tensor? D, Tensor? delta_bias, "
            "Tensor dout, Tensor? x, bool delta_softplus, int rev_group_start, int u_row_mod, int dout_row_mod) -> Tensor[]")
_LIB.define("merge4(Tensor out, int H, int W) -> Tensor")


def _omni_fwd_op(u, delta, A_log, B, C, D, delta_bias, delta_softplus, rev_group_start, u_row_mod):
    # the omni ops take A_log and evaluate A = -exp(A_log) inside the kernels
    return selective_scan_fwd(u, delta, A_log, B, C, D, delta_bias, delta_softplus, 1, rev_group_start, u_row_mod, True)


def _omni_bwd_op(u, delta, A_log, B, C, D, delta_bias, dout, x, delta_softplus, rev_group_start, u_row_mod, dout_row_mod):
    res = selective_scan_bwd(u, delta, A_log, B, C, D, delta_bias, dout, x, delta_softplus, 1, rev_group_start, u_row_mod,
                             dout_row_mod, True)
    return [t if t is not None else u.new_empty(0, dtype=torch.float32) for t in res]


def merge4(out: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """(B, 4, D, H*W) un-flipped omni-scan outputs -> (B, D, H, W) fp32, reference association order."""
    _check(out.is_cuda and out.dim() == 4 and out.shape[1] == 4 and out.shape[3] == H * W and out.dtype in _DT,
           "merge4: out must be a (B, 4, D, H*W) GPU tensor")
    out = out.contiguous()
    B, _, D, L = out.shape
    y = torch.empty((B, D, H, W), dtype=torch.float32, device=out.device)
    if out.numel() == 0:
        return y
    lib = _capi.load()
    with torch.cuda.device(out.device):
        _capi.check(lib.oss_merge4(_DT[out.dtype], out.data_ptr(), y.data_ptr(), B, D, H, W,
                                   torch.cuda.current_stream().cuda_stream), "oss_merge4")
    return y


_LIB.impl("omni_scan_fwd", _omni_fwd_op, "CUDA")
_LIB.impl("omni_scan_bwd", _omni_bwd_op, "CUDA")
_LIB.impl("merge4", merge4, "CUDA")
