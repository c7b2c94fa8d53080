"""Input regimes and the float64 comparison of the selective-scan tests (tests/test_scan_regimes_host.py, CPU only, and
tests/test_scan_regimes_gpu.py, the HIP kernels).  TEST INFRASTRUCTURE: plain helpers, no test in here.

Why: the reference's grid (``A = -0.5 rand``, ``delta = 0.5 rand``; test_scan_gpu.py: make_inputs) decays by about exp(-0.25) per
step, so whatever a kernel carries across a chunk, piece or segment boundary is multiplied by ~0 before anything is compared.
The regimes below keep the carries alive (``slow``, ``none``), mix live and dead states in every row the way the archs'
initialisation does (``arch``: oss_block.py, _dt_proj_init and the A_log initialiser) or underflow everything (``stiff``).

The comparison has no tolerance of its own: every limit is the error of the sequential fp32 oracle (oracle/oss_scan_oracle.c)
against its float64 twin ON THE SAME INPUTS, times one margin:

    MARGIN = 16          margin over the fp32 oracle's own error; must lie in [1, 32]
    largest measured ratio: 4.187 (saved states, fp32 I/O, regime `stiff`, L = 1541), MI355X run of 2026-10-20;
    the table per quantity, regime and type is profiles/scan_regimes_error.txt

MARGIN is the next power of two above twice the largest ratio ``max|got - ref64| / (E32 * max|ref64|)`` that the HIP kernels
showed over all cases of test_scan_regimes_gpu.py; MARGIN_CAP = 32 is the most any kernel may need (a quantity that needs more
is a finding about that kernel) and is what the host file proves to be sharp enough to catch a 1 % error of ONE slot's carry.
"""
import math

import torch

from oracle import oss_oracle

MARGIN = 16
MARGIN_CAP = 32

REGIMES = ("arch", "slow", "none", "stiff")
SOFTPLUS = {"arch": True, "slow": False, "none": False, "stiff": True}

#: one unit of the 16-bit output types: the largest relative error of ONE round-to-nearest to the type (2^-8 at the bottom of a
#: bfloat16 binade, 2^-9 at its top; the fp32 error that moves a value across a rounding boundary is inside MARGIN's term).
#: Every kernel rounds out / du / ddelta / dB / dC to the I/O type ONCE, in its final store (the row-tile partials
#: of dB / dC are fp32 by default), so the count that multiplies it is 1 for every quantity.
UNIT = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
ROUNDED = ("out", "du", "ddelta", "dB", "dC", "dz")          # stored in the I/O type; everything else is fp32
GRADS = ("du", "ddelta", "dA", "dB", "dC", "dD", "ddelta_bias")
TINY = 1e-30

#: every compare() appends (label, itype, quantity, ratio) here: what profiles/scan_regimes_error.txt is made from
RATIOS = []


def make_regime(name, batch, dim, N, G, L, itype, seed=0):
    """-> ``(u, delta, A, B, C, D, bias, dout)`` like test_scan_gpu.make_inputs (CPU generator; u / delta / B / C / dout rounded to
    ``itype``, the weights fp32); ``bias`` is None where the regime has none.  SOFTPLUS[name] says how delta is to be read."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g)
    steps = torch.arange(1, N + 1, dtype=torch.float32)
    bias = None
    if name == "arch":        # A = -(1..N), softplus(delta + bias) around dt ~ logU[1e-3, 0.1] per row
        A = -steps.repeat(dim, 1)
        delta = rnd(batch, dim, L) - 0.5
        dt = torch.exp(rnd(dim) * (math.log(0.1) - math.log(1e-3)) + math.log(1e-3))
        bias = dt + torch.log(-torch.expm1(-dt))              # softplus^-1
    elif name == "slow":      # every state keeps e^-0.25 .. e^-4 over the WHOLE sequence
        A = -(0.25 + 3.75 * rnd(dim, N))
        delta = (0.5 + rnd(batch, dim, L)) / L
    elif name == "none":      # a = 1: running sums
        A = torch.zeros(dim, N)
        delta = 0.02 * (0.5 + rnd(batch, dim, L))
    elif name == "stiff":     # delta A down to about -100: decay factors and products underflow
        A = -steps.repeat(dim, 1)
        delta = 2.0 + 4.0 * rnd(batch, dim, L)
        bias = 0.5 * rnd(dim)
    else:
        raise ValueError(name)
    B = torch.randn(batch, G, N, L, generator=g).to(itype)
    C = torch.randn(batch, G, N, L, generator=g).to(itype)
    D = torch.randn(dim, generator=g)
    u = torch.randn(batch, dim, L, generator=g).to(itype)
    dout = torch.randn(batch, dim, L, generator=g).to(itype)
    return u, delta.to(itype), A, B, C, D, bias, dout


def mirror(t, per):
    """flip the time axis of rows / groups ``2 * per ..`` (the mirrored directions of the omni form; its own inverse)"""
    t = t.clone()
    t[:, 2 * per:] = t[:, 2 * per:].flip(-1)
    return t


def _oracle(inputs, softplus, chunk, real, lane_states):
    cast = (lambda t: None if t is None else t.double()) if real == "f64" else (lambda t: None if t is None else t.float())
    u, delta, A, B, C, D, bias, dout = (cast(t) for t in inputs)
    out, x = oss_oracle.scan_fwd(u, delta, A, B, C, D, bias, softplus, chunk=chunk, real=real)
    res = {"out": out, "x": x}
    if lane_states:           # the state entering block k > 0 = the state after step 8k - 1
        L8 = (u.shape[-1] + 7) // 8
        _, x8 = oss_oracle.scan_fwd(u, delta, A, B, C, D, bias, softplus, chunk=8, real=real)
        res["hs"] = x8[:, :, :L8 - 1, 1::2].permute(0, 1, 3, 2)
    res.update(zip(GRADS, oss_oracle.scan_bwd(u, delta, A, B, C, D, bias, dout, None, softplus, real=real)))
    return {k: (None if v is None else v.double()) for k, v in res.items()}


def references(inputs, softplus, chunk=256, lane_states=False):
    """-> ``(ref64, ref32)``: the float64 oracle on exactly ``inputs`` and the fp32 oracle on float32 copies of them (so that its
    error is fp32 arithmetic alone, no I/O rounding), as dicts of float64 CPU tensors: out, x, the seven gradients (None where
    absent) and, on request, the lane states ``hs`` (batch, dim, N, blocks - 1)."""
    return _oracle(inputs, softplus, chunk, "f64", lane_states), _oracle(inputs, softplus, chunk, "f32", lane_states)


def _scaled(err, ref, e32, unit, dims, extra=0.0):
    """per element: the margin this element needs, ``(|err| - unit |ref| - extra) / (E32 max|ref|)``, E32 and the maximum over
    ``dims``"""
    scale = ref.abs().amax(dim=dims, keepdim=True)
    lim1 = e32.abs().amax(dim=dims, keepdim=True)             # = E32 * scale
    excess = (err.abs() - unit * ref.abs() - extra).clamp_min(0.0)
    ratio = torch.where(excess > 0, excess / lim1, torch.zeros_like(excess))   # lim1 = 0 and excess > 0 -> inf
    return torch.nan_to_num(ratio, nan=math.inf, posinf=math.inf), scale


def measure(got, ref64, ref32, itype, extra=None):
    """-> {quantity: per-element tensor of the margin it needs} for every key of ``got`` (x is split into ``x states`` and
    ``x products``).  A non-finite entry of ``got`` needs an infinite margin.  ``extra``: {quantity: per-element absolute
    allowance} for a quantity with a documented limit of its own -- the caller states the arithmetic reason."""
    res, extra = {}, extra or {}
    for q, g in got.items():
        want, w32 = ref64[q], ref32[q]
        if want is None:
            assert g is None, f"{q}: the oracle has none"
            continue
        assert g is not None, f"{q} is missing"
        g = g.detach().double().cpu()
        assert g.shape == want.shape, f"{q}: shape {tuple(g.shape)} vs {tuple(want.shape)}"
        bad = ~torch.isfinite(g)
        g = torch.where(bad, torch.zeros_like(g), g)
        unit = UNIT[itype] if q in ROUNDED else 0.0
        if q == "x":
            # saved states, per state slot: scale and E32 over batch, row and chunk -- an error of one slot cannot hide behind
            # another slot's magnitude
            r, _ = _scaled(g[..., 1::2] - want[..., 1::2], want[..., 1::2], w32[..., 1::2] - want[..., 1::2], 0.0, (0, 1, 2))
            res["x states"] = torch.where(bad[..., 1::2], torch.full_like(r, math.inf), r)
            # running products: relative, against the fp32 oracle's largest relative error where the product is alive
            p, p32, gp = want[..., 0::2], w32[..., 0::2], g[..., 0::2]
            live = p > TINY
            e32 = float(((p32 - p).abs() / p)[live].max()) if live.any() else 0.0
            rel = (gp - p).abs() / p.clamp_min(TINY)
            r = torch.where(rel > 0, rel / e32, torch.zeros_like(rel)) if e32 > 0 else torch.where(rel > 0, math.inf, 0.0).double()
            # dead entries: finite and below 2e-30 (the hardware may flush what the oracle keeps as a denormal)
            r = torch.where(live, r, torch.where(gp.abs() < 2 * TINY, 0.0, math.inf).double())
            res["x products"] = torch.where(bad[..., 0::2], torch.full_like(r, math.inf), r)
            continue
        dims = (0, 1, 3) if q == "hs" else tuple(range(g.dim()))
        r, _ = _scaled(g - want, want, w32 - want, unit, dims, extra.get(q, 0.0))
        res[q] = torch.where(bad, torch.full_like(r, math.inf), r)
    return res


def compare(got, ref64, ref32, itype, margin=None, label="", extra=None):
    """assert that every quantity of ``got`` lies within ``margin`` (default MARGIN) times the fp32 oracle's own error of the
    float64 oracle -- plus one unit of the I/O type for what is stored in it -- and that everything is finite"""
    margin = MARGIN if margin is None else margin
    assert 1 <= MARGIN <= MARGIN_CAP
    wrong = []
    for q, r in measure(got, ref64, ref32, itype, extra).items():
        worst = float(r.max()) if r.numel() else 0.0
        RATIOS.append((label, str(itype).replace("torch.", ""), q, worst))
        if worst > margin:
            i = int(torch.argmax(r))
            wrong.append(f"{q}: {int((r > margin).sum())}/{r.numel()} beyond {margin} x the fp32 oracle's error; worst needs "
                         f"{worst:.3g} x at flat index {i}")
    assert not wrong, f"[{label} {itype}] " + "; ".join(wrong)
