"""Input regimes and the float64 comparison of the LayerNorm tests (tests/test_ln_regimes_host.py, CPU only, and
tests/test_ln_regimes_gpu.py, the HIP kernels).  TEST INFRASTRUCTURE: plain helpers, no test in here.

Why: the grid of test_glue_gpu.py (``randn * 2 + 0.5``, an fp32 PyTorch reference, absolute tolerances) has |mean| ~ std, a
variance far above eps and one scale for every pixel, and it never looks at the kernels' own ``mean`` / ``rstd``.  A one-pass
variance ``E[x^2] - mu^2``, a dropped eps or a wrong divisor pass there.  The regimes below put the statistics where those
mistakes show: a mean far above the std (``offset``), no variance at all (``flat``), pixels that span six decades (``wide``)
and one element that owns the statistics (``outlier``).

The comparison has no tolerance of its own: every limit is the error of an fp32 twin of the float64 reference ON THE SAME
INPUTS, relative to a scale per quantity, times one margin (plus one unit of a 16-bit type for what is stored in it):

    MARGIN = 8           margin over the fp32 twin's own error; must lie in [1, 32]
    largest measured ratio: 2.747 (dw, regime `outlier`, float16 -> float32, BiasFree and gated), MI355X run of 2026-10-20;
    the table per quantity, regime and type pair is profiles/ln_regimes_error.txt

MARGIN is the next power of two above twice the largest ratio that the HIP kernels showed over all cases of
test_ln_regimes_gpu.py; MARGIN_CAP = 32 is the most any kernel may need (a quantity that needs more is a finding about that
kernel) and is what the host file proves to be sharp enough to reject a one-pass variance, a dropped eps, a wrong divisor, a
centred BiasFree form, a dropped term of the backward and a 1 % error of one channel's weight gradient.

One such finding: dx of the BiasFree backward needed 24000 (`flat`, fp32 x) -- x - mean times rstd^3 mean(g w x) carried the
rounding of the stored fp32 mean, which autograd (the twin) cancels.  The kernels now subtract the mean of the residuals.
"""
import math

import torch

MARGIN = 8
MARGIN_CAP = 32
EPS = 1e-5

REGIMES = ("plain", "offset", "flat", "wide", "outlier")

#: ``offset``: (mean, std) per type of x.  The steps of the 16-bit types at the offset are 0.5 (fp16 at 1000) and 0.25 (bf16 at
#: 48), so the rounded rows keep a few distinct values.  bf16 48 is the value of the issue; test_ln_regimes_host.py shows that a
#: one-pass variance is beyond MARGIN_CAP there (had it not been, 64 or 96 were next: still exact bf16 steps).
OFFSET = {torch.float32: (100.0, 0.1), torch.float16: (1000.0, 2.0), torch.bfloat16: (48.0, 1.0)}

#: one unit of the 16-bit types: the largest relative error of ONE round-to-nearest to the type (in its normal range; below it the
#: error is absolute, see measure()).  The kernels round y / n / dgate (the output type) and dx (the type of x) ONCE, in their
#: final store; mean, rstd, dw and db are fp32.
UNIT = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
ROUNDED_Y = ("y", "n", "dgate", "conv")       # stored in the output type
ROUNDED_X = ("dx",)                           # stored in the type of x
WHOLE = ("y", "n", "dgate", "dw", "db", "conv")   # scale: max |ref64| of the tensor; mean / rstd / dx: per pixel, see _scale
FLOOR = 2.0 ** -23

#: every compare() appends (label, types, quantity, needed margin) here: what profiles/ln_regimes_error.txt is made from
RATIOS = []


def make_regime(name, B, C, P, xdt, seed=0):
    """-> x (B, C, P), already rounded to ``xdt`` (CPU generator); the references see exactly these values.

    plain    randn * 2 + 0.5: the old grid, for continuity
    offset   mean far above std, OFFSET[xdt] (fp32 100 + 0.1 randn, fp16 1000 + 2 randn, bf16 48 + randn -- at 48 a one-pass
             variance already needs 124 x the twin's error on y, so the offset was not raised): cancellation in the variance
             or in x - mu
    flat     every pixel constant over the channels (3 randn); the first half of the pixels exactly (var = 0), the second
             half + 1e-3 randn (var << eps): eps, the rstd ~ 316 amplification of the backward, NaN / Inf
    wide     s[p] randn, s log-uniform in [1e-3, 1e3] per pixel: errors that hide under a whole-tensor tolerance
    outlier  randn with channel C // 3 at +-1e4: statistics owned by one element; a channel-slot indexing error"""
    g = torch.Generator().manual_seed(seed)
    randn = lambda *s: torch.randn(*s, generator=g)
    if name == "plain":
        x = randn(B, C, P) * 2 + 0.5
    elif name == "offset":
        off, sd = OFFSET[xdt]
        x = off + sd * randn(B, C, P)
    elif name == "flat":
        x = (3 * randn(B, 1, P)).expand(B, C, P).clone()
        x[:, :, P // 2:] += 1e-3 * randn(B, C, P - P // 2)
    elif name == "wide":
        s = torch.exp((2 * torch.rand(B, 1, P, generator=g) - 1) * math.log(1e3))
        x = s * randn(B, C, P)
    elif name == "outlier":
        x = randn(B, C, P)
        x[:, C // 3] = torch.where(torch.rand(B, P, generator=g) < 0.5, -1e4, 1e4)
    else:
        raise ValueError(name)
    return x.to(xdt)


def make_inputs(regime, B, C, P, xdt, ydt, seed=0, bias=True, gate=False, skip=False, affine=None, dy=True):
    """-> dict of CPU tensors: x (B, C, P) in ``xdt``; w = 0.5 randn + 1 and b = randn or None (None: the BiasFree form), fp32;
    gate = 3 randn and dy = randn in ``ydt``; skip = randn in ``xdt``; ``affine`` in (None, "add", "mul"): dy_add = randn and
    dy_mul = 0.3 randn, (B, C) fp32, add_scale = 1 / P (the channel gate's backward folded into the load of dy)"""
    g = torch.Generator().manual_seed(seed + 1000)
    randn = lambda *s: torch.randn(*s, generator=g)
    inp = {"x": make_regime(regime, B, C, P, xdt, seed), "w": 0.5 * randn(C) + 1, "b": randn(C) if bias else None,
           "gate": (3 * randn(B, C, P)).to(ydt) if gate else None, "dy": randn(B, C, P).to(ydt) if dy else None,
           "skip": randn(B, C, P).to(xdt) if skip else None, "dy_mul": None, "dy_add": None, "add_scale": 1.0}
    if affine is not None:
        inp["dy_add"], inp["add_scale"] = randn(B, C), 1.0 / P
        if affine == "mul":
            inp["dy_mul"] = 0.3 * randn(B, C)
    return inp


# ---- the fp32 twin's sums: a stated sequential order, so that torch.sum's pairwise order does not flatter it ------------------
def _seq_sum_c(t):
    s = t[:, 0].clone()
    for c in range(1, t.shape[1]):
        s += t[:, c]
    return s


class _SumC(torch.autograd.Function):
    """(B, C, P) -> (B, P): the channels added one after the other"""

    @staticmethod
    def forward(ctx, t):
        ctx.C = t.shape[1]
        return _seq_sum_c(t)

    @staticmethod
    def backward(ctx, g):
        return g[:, None, :].expand(-1, ctx.C, -1)


class _OverC(torch.autograd.Function):
    """(B, P) -> (B, C, P); its backward is the sum over the channels, again one after the other"""

    @staticmethod
    def forward(ctx, v, C):
        return v[:, None, :].expand(-1, C, -1).contiguous()

    @staticmethod
    def backward(ctx, g):
        return _seq_sum_c(g), None


class _OverBP(torch.autograd.Function):
    """(C,) -> (B, C, P); its backward (dw, db) sums an image's pixels in blocks of 64 and adds the blocks one after the other:
    the plain blocked order of a sum too long for a Python loop (the sums over the CHANNELS are fully sequential)"""

    @staticmethod
    def forward(ctx, v, B, P):
        return v[None, :, None].expand(B, -1, P).contiguous()

    @staticmethod
    def backward(ctx, g):
        B, C, P = g.shape
        pad = (-P) % 64
        blocks = torch.nn.functional.pad(g, (0, pad)).view(B, C, -1, 64).sum(-1).permute(1, 0, 2).reshape(C, -1)
        s = blocks[:, 0].clone()
        for k in range(1, blocks.shape[1]):
            s += blocks[:, k]
        return s, None, None


def reference(x, w, b, gate, dy, skip=None, dy_mul=None, dy_add=None, add_scale=1.0, real="f64"):
    """The written-out LayerNorm over the channels of x (B, C, P) in float64 (``real = "f64"``) or as the fp32 twin (``"f32"``:
    float32 copies of the already rounded inputs, the sums in the sequential order above), torch autograd on the formula:

        mean = sum_c x / C;  var = sum_c (x - mean)^2 / C  (unbiased=False);  rstd = (var + 1e-5)^-1/2
        n = (x - mean) rstd w + b      b None (BiasFree): n = x rstd w  (the variance still about the mean)
        y = n silu(gate)
        backward of y with the gradient dy (1 + dy_mul[b, c]) + add_scale dy_add[b, c]; dx += skip

    -> dict of float64 tensors: x, mean, rstd (B, P); n, y (B, C, P); with ``dy``: dx, dgate, dw, db (None where absent)"""
    dt = torch.float64 if real == "f64" else torch.float32
    seq = real == "f32"
    cast = lambda t: None if t is None else t.detach().to(dt)
    x, w, b, gate, dy, skip, dy_mul, dy_add = (cast(t) for t in (x, w, b, gate, dy, skip, dy_mul, dy_add))
    B, C, P = x.shape
    leaves = [t.requires_grad_() for t in (x, w, b, gate) if t is not None]
    sum_c = _SumC.apply if seq else (lambda t: t.sum(1))
    over_c = (lambda v: _OverC.apply(v, C)) if seq else (lambda v: v[:, None, :])
    over_bp = (lambda v: _OverBP.apply(v, B, P)) if seq else (lambda v: v[None, :, None])
    mean = sum_c(x) / C
    d = x - over_c(mean)
    var = sum_c(d * d) / C
    rstd = 1.0 / torch.sqrt(var + EPS)
    n = d * over_c(rstd) * over_bp(w) + over_bp(b) if b is not None else x * over_c(rstd) * over_bp(w)
    y = n if gate is None else n * (gate * torch.sigmoid(gate))
    res = {"x": x, "mean": mean, "rstd": rstd, "n": n, "y": y}
    if dy is not None:
        g = dy
        if dy_add is not None:
            g = (dy * (1 + dy_mul)[:, :, None] if dy_mul is not None else dy) + add_scale * dy_add[:, :, None]
        names = [k for k, t in zip(("x", "w", "b", "gate"), (x, w, b, gate)) if t is not None]
        grads = dict(zip(names, torch.autograd.grad(y, leaves, g)))
        res["dx"] = grads["x"] + skip if skip is not None else grads["x"]
        res.update(dw=grads["w"], db=grads.get("b"), dgate=grads.get("gate"))
    return {k: (None if v is None else v.detach().double()) for k, v in res.items()}


def references(inp):
    """-> (ref64, ref32) of a make_inputs() dict"""
    return tuple(reference(inp["x"], inp["w"], inp["b"], inp["gate"], inp["dy"], inp["skip"], inp["dy_mul"], inp["dy_add"],
                           inp["add_scale"], real) for real in ("f64", "f32"))


def conv_references(n, weight, bias):
    """the 1x1 convolution behind the fused LayerNorm: y[b, m, p] = sum_k W[m, k] n[b, k, p] + bias[m] on the STORED n (B, K, P)
    and the weights as given (already rounded to the I/O type) -> (float64, fp32 twin: the k-steps added one after the other),
    each a dict with the one quantity ``conv``"""
    n64, w64 = n.detach().double().cpu(), weight.detach().double().cpu()
    ref = torch.einsum("mk,bkp->bmp", w64, n64) + bias.double().cpu()[None, :, None]
    n32, w32 = n64.float(), w64.float()
    acc = torch.zeros(ref.shape, dtype=torch.float32)
    for k in range(n32.shape[1]):
        acc += w32[None, :, k, None] * n32[:, None, k, :]
    acc += bias.float().cpu()[None, :, None]
    return {"conv": ref}, {"conv": acc.double()}


def _scale(q, ref64):
    """the scale an error of quantity ``q`` is measured against (broadcasts over the quantity)"""
    r = ref64[q].abs()
    if q in WHOLE:
        return r.max() if r.numel() else r.sum()
    if q == "mean":
        return ref64["x"].abs().amax(1)          # per pixel: the largest |x| over the channels
    if q == "rstd":
        return r                                  # per pixel: the value itself
    if q == "dx":
        return r.amax(1, keepdim=True)            # per pixel: the largest |dx| over the channels
    raise KeyError(q)


def _ratio(excess, lim):
    """excess / lim with 0 / 0 = 0 and anything / 0 = inf"""
    r = torch.where(excess > 0, excess / lim, torch.zeros_like(excess))
    return torch.nan_to_num(r, nan=math.inf, posinf=math.inf)


def measure(got, ref64, ref32, types):
    """-> {quantity: (per-element tensor of the margin it needs, E32)} for every key of ``got``; ``types`` = (type of x / dx,
    type of y / gate / dy).  E32(q) = max(2^-23, max |ref32 - ref64| / scale): the twin's own relative error on this case.  An
    element needs (|got - ref64| - UNIT max(|ref64|, smallest normal of the type)) / (E32 scale); a non-finite one needs an
    infinite margin, unless the reference itself lies beyond the type's range."""
    xdt, ydt = types
    res = {}
    for q, g in got.items():
        want, w32 = ref64[q], ref32[q]
        if want is None:
            assert g is None, f"{q}: the reference has none"
            continue
        assert g is not None, f"{q} is missing"
        g = g.detach().double().cpu().reshape(want.shape) if g.numel() == want.numel() else g
        assert g.shape == want.shape, f"{q}: shape {tuple(g.shape)} vs {tuple(want.shape)}"
        store = ydt if q in ROUNDED_Y else (xdt if q in ROUNDED_X else torch.float32)
        unit = UNIT[store]
        bad = ~torch.isfinite(g)
        if store != torch.float32:
            # beyond the largest finite value of the type the correct stored value IS an infinity (`flat` in the BiasFree form:
            # dx ~ xhat rstd^3 mean(g w x) reaches 3e5, float16 ends at 65504): accepted there, with the reference's sign
            over = (want.abs() > torch.finfo(store).max * (1 - 2 * unit)) & torch.isinf(g) & (torch.sign(g) == torch.sign(want))
            bad = bad & ~over
            g = torch.where(over, want, g)
        g = torch.where(bad, torch.zeros_like(g), g)
        scale = _scale(q, ref64)
        e32 = _ratio((w32 - want).abs(), scale.expand_as(want))
        assert bool(torch.isfinite(e32).all()), f"{q}: the fp32 twin is wrong where the reference is exactly 0"
        e32 = max(FLOOR, float(e32.max()) if e32.numel() else 0.0)
        # one rounding to the type: UNIT |ref64| in the normal range, half a subnormal step = UNIT x the smallest normal below it
        # (2^-25 in float16: dx of `outlier` and `wide` has elements near 1e-7 beside a per-pixel scale of 1e-3, and the float64
        # reference itself, rounded once to float16, needed 33 x without this; test_ln_regimes_host.py)
        floor = torch.finfo(store).tiny if store != torch.float32 else 0.0
        excess = ((g - want).abs() - unit * want.abs().clamp_min(floor)).clamp_min(0.0)
        r = _ratio(excess, (e32 * scale).expand_as(want))
        res[q] = (torch.where(bad, torch.full_like(r, math.inf), r), e32)
    return res


def compare(got, ref64, ref32, types, label="", margin=None):
    """assert that every quantity of ``got`` lies within ``margin`` (default MARGIN) times the fp32 twin's own error of the
    float64 reference -- plus one unit of a 16-bit type for what is stored in it -- and that everything is finite"""
    margin = MARGIN if margin is None else margin
    assert 1 <= MARGIN <= MARGIN_CAP
    wrong = []
    tname = "->".join(str(t).replace("torch.", "") for t in types)
    for q, (r, e32) in measure(got, ref64, ref32, types).items():
        worst = float(r.max()) if r.numel() else 0.0
        RATIOS.append((label, tname, q, worst))
        if not worst <= margin:
            i = int(torch.argmax(r))
            wrong.append(f"{q}: {int((~(r <= margin)).sum())}/{r.numel()} beyond {margin} x the fp32 twin's error (E32 = {e32:.3g}); "
                         f"worst needs {worst:.3g} x at flat index {i}")
    assert not wrong, f"[{label} {tname}] " + "; ".join(wrong)
