"""Cases, references and the float64 comparison of the one-launch EFFN forward (csrc/oss_effn.hip):
tests/test_effn_regimes_host.py (CPU only) and tests/test_effn_float64_gpu.py (the HIP kernel).  TEST INFRASTRUCTURE: plain
helpers, no test in here.

Why: test_effn_gpu.py compares ``x + project_out(gelu(x1) * x2)`` with an fp32 PyTorch reference under a tolerance tied to
``max |want|`` -- but the output is dominated by the skip connection (max |want| 7.1 against a branch of rms 0.17), and the bf16
tolerance is a third of the branch's rms: a dropped hidden pair passes in all but 3 of 46080 elements, a lost tap is invisible.
Here the limit is the error that ROUNDING THE THREE INTERMEDIATES to the I/O type causes on the same inputs, which does not
know about the skip connection:

    ref64   the formula in float64, nothing rounded but the inputs and the weights
    twin    the same in float64 with n = norm2(x), t = project_in(n) and the gate output rounded to the I/O type: the three
            places the kernel (and the launch-per-layer chain) rounds
    E       max |twin - ref64| over the tensor (floored at 2^-23 max |ref64|)
    an element needs  max(0, |got - ref64| - UNIT |ref64|) / E   (the subtracted term: the ONE rounding of the final store)

    MARGIN = 2           margin over the twin's own error; must lie in [1, 8]
    largest measured ratio: 0.995 (d-D48-h127-bf16-WithBias-2x9x24-dense-wide), MI355X run of 2026-10-21;
    the table per case is profiles/effn_float64_error.txt

MARGIN is the next power of two above twice the largest ratio that the HIP kernel showed over all cases of
test_effn_float64_gpu.py.  MARGIN_CAP = 8 is a condition, not a measurement: the fp32 chain twin needs under 1 everywhere, and the
host file shows that every mutant of MUTANTS -- a seam column or band row read as 0, a dropped pair, a dropped tap, a wrong value
outside the image, a one-pass variance, a dropped eps, a centred BiasFree form, the skip taken from the normalised tile -- needs
more than 8 in at least one case of the grid, in both 16-bit types (one exception, stated in the host file: with a bfloat16 x a
one-pass variance in fp32 is exact or nearly so and nothing can reject it).  A case that needs more than the cap is a finding
about the kernel.

No finding: the kernel needs under 1 in every case, i.e. it is as close to float64 as float64 arithmetic with the same three
roundings is.

What the measure cannot see: where |x| UNIT exceeds the branch, the one rounding of the final store swallows it -- `offset` in the
WithBias form (float16 x ~ 1000, steps of 0.5; bfloat16 x ~ 48, steps of 0.25; a branch of rms 0.2) needs 0 whatever the branch
holds, and so does the +-1e4 channel of `outlier`.  That is a property of ``x + branch`` in a 16-bit type, not of the comparison; those cases
check the skip connection, finiteness, and (outlier) the other channels.
"""
import math

import torch
import torch.nn.functional as F

import ln_regimes as lr
from ln_regimes import UNIT

MARGIN = 2
MARGIN_CAP = 8
EPS = 1e-5
F16, BF16 = torch.float16, torch.bfloat16
NAME = {F16: "f16", BF16: "bf16"}
TYPES = (F16, BF16)
DIMS = (32, 48, 64, 96)                      # KS = 2, 3, 4, 6: every instantiation
TILE_H, TILE_W, BAND = 8, 16, 2              # a workgroup's pixel tile; the rows of a wave's band (oss_effn.hip: TH, TW, RW)

#: every compare() appends (label, dtype, needed margin) here: what profiles/effn_float64_error.txt is made from
RATIOS = []


def hidden_of(D):
    return int(2.66 * D)                     # 85, 127, 170, 255: what the module builds


# ---- weights and inputs ---------------------------------------------------------------------------------------------------------
def dense(D, h, seed=0):
    """-> fp32 (w_in (2 h, D), w_dw (2 h, 9), w_out (D, h)): fan-in uniform 1x1 weights (nn.Conv2d's default, +-1 / sqrt(fan-in))
    and the depth-wise taps doubled, as test_effn_gpu.py draws them"""
    g = torch.Generator().manual_seed(1000 + seed)
    u = lambda *s: 2 * torch.rand(*s, generator=g) - 1
    return u(2 * h, D) / math.sqrt(D), 2 * u(2 * h, 9) / 3, u(D, h) / math.sqrt(h)


def probe(D, h, run, seed=0):
    """dense()'s w_in and w_dw, but w_out selects ONE hidden pair per output channel: w_out[d, run D + d] = 1 where run D + d < h.
    Then out[d] - x[d] is the gate output of pair run D + d, which GEMM 2 carries through exactly; runs 0 .. ceil(h / D) - 1
    show every pair alone"""
    w_in, w_dw, _ = dense(D, h, seed)
    w_out = torch.zeros(D, h)
    for d in range(D):
        if run * D + d < h:
            w_out[d, run * D + d] = 1.0
    return w_in, w_dw, w_out


def ln_params(D, bias, seed=0):
    g = torch.Generator().manual_seed(2000 + seed)
    w = 0.5 + torch.rand(D, generator=g)
    b = 0.3 * torch.randn(D, generator=g)
    return w, (b if bias else None)


def make_x(regime, shape, dt, seed=0):
    """``skip``: 1.5 randn + 0.2 (test_effn_gpu.py's input, the skip connection 40 x the branch); otherwise a regime of
    ln_regimes.make_regime reshaped to the plane"""
    B, D, H, W = shape
    if regime == "skip":
        g = torch.Generator().manual_seed(3000 + seed)
        return (1.5 * torch.randn(B, D, H, W, generator=g) + 0.2).to(dt)
    return lr.make_regime(regime, B, D, H * W, dt, seed).view(B, D, H, W)


# ---- the case grid (shared by the host and the GPU file) -------------------------------------------------------------------------
class Case:
    """one launch: section of test_effn_float64_gpu.py, D, hidden, type, LayerNorm form, shape (B, H, W), weights ("dense" or
    ("probe", run)) and the regime of x"""

    def __init__(self, sec, D, dt, bias=True, bhw=(1, 9, 24), weights="dense", regime="skip", hidden=None):
        self.sec, self.D, self.dt, self.bias, self.bhw, self.weights, self.regime = sec, D, dt, bias, bhw, weights, regime
        self.h = hidden_of(D) if hidden is None else hidden
        self.shape = (bhw[0], D, bhw[1], bhw[2])

    @property
    def id(self):
        w = "dense" if self.weights == "dense" else f"probe{self.weights[1]}"
        return (f"{self.sec}-D{self.D}-h{self.h}-{NAME[self.dt]}-{'WithBias' if self.bias else 'BiasFree'}-"
                f"{'x'.join(map(str, self.bhw))}-{w}-{self.regime}")

    def inputs(self):
        """-> CPU tensors: x in the I/O type, ln_w, ln_b (or None), and the UNROUNDED fp32 w_in (2 h, D), w_dw (2 h, 9), w_out (D, h)"""
        ws = dense(self.D, self.h) if self.weights == "dense" else probe(self.D, self.h, self.weights[1])
        return (make_x(self.regime, self.shape, self.dt),) + ln_params(self.D, self.bias) + ws


SHAPES_A = ((1, 8, 16),      # one full tile
            (1, 9, 24),      # ragged in both directions, a second tile row of ONE image row, W % 16 == 8
            (2, 17, 40))     # 3 x 3 tiles: interior seams and ragged edges in both directions; two images (blockIdx.y, batch stride)
SEAM_SHAPES = ((1, 9, 24), (2, 17, 40))      # a tile seam inside the image (every shape has band seams)

CASES_A = [Case("a", D, dt, bias, bhw) for D in DIMS for dt in TYPES for bias in (True, False) for bhw in SHAPES_A]
CASES_B = [Case("b", D, dt, weights=("probe", run)) for D in DIMS for dt in TYPES for run in range(3)]
CASES_C = ([Case("c", 48, dt, hidden=h) for dt in TYPES for h in (1, 16, 17, 32)] +
           [Case("c", 48, dt, hidden=h, weights=("probe", 0)) for dt in TYPES for h in (16, 17)])

#: section d, BiasFree: the un-centred form multiplies x ITSELF by rstd.  Left out (test_effn_regimes_host.py shows the overflow):
EXCLUDED_D = {
    ("offset", False, F16): "x ~ 1000 and rstd ~ 0.5: n ~ 500, x1 and x2 ~ 1e3, the gate output ~ 1e6 is beyond float16",
    ("flat", False, F16): "var = 0, rstd = 316: n ~ 1e3 on every channel, the gate output ~ 1e6 is beyond float16",
}
CASES_D = [Case("d", D, dt, bias, (2, 9, 24), regime=r) for D in (48, 96) for dt in TYPES for bias in (True, False)
           for r in lr.REGIMES if (r, bias, dt) not in EXCLUDED_D]
FLOAT64_CASES = CASES_A + CASES_B + CASES_C + CASES_D


# ---- the formula -----------------------------------------------------------------------------------------------------------------
def round_weights(w_in, w_dw, w_out, dt):
    """the values the kernel reads: the two 1x1 weights rounded to the I/O type, the taps fp32 (ops.effn_round_weights without the
    padding)"""
    return w_in.to(dt).float(), w_dw.float(), w_out.to(dt).float()


def unpad_weights(w_in_p, w_dw_p, w_out_p, h):
    """ops.effn_round_weights' padded tensors (read back from the device) -> (2 h, D), (2 h, 9), (D, h) fp32 on the CPU"""
    hp = w_out_p.shape[1]
    rows = torch.cat([torch.arange(h), hp + torch.arange(h)])
    return w_in_p.float().cpu()[rows], w_dw_p.float().cpu()[rows], w_out_p.float().cpu()[:, :h]


def reference(x, ln_w, ln_b, w_in, w_dw, w_out, dt, real="f64", rounded=False, mutate=None, parts=False):
    """``x + project_out(gelu(x1) * x2)``, ``x1, x2 = dwconv3x3(project_in(LayerNorm(x))).chunk(2, 1)`` written out on CPU tensors:

        LayerNorm over the channels, unbiased=False, eps 1e-5; ln_b None: the BiasFree form x rstd w (variance about the mean)
        t = W_in n with W_in rounded to ``dt``; zero-padded depth-wise 3x3 with fp32 taps; gelu in its erf form
        out = x + W_out (gelu(x1) x2) with W_out rounded to ``dt``

    ``real``: "f64" or "f32" arithmetic.  ``rounded``: n, t and the gate output are rounded to ``dt`` (the kernel's header names
    these three; the chain stores the same three tensors); the final sum is never rounded.
    (f64, False) = the float64 reference; (f64, True) = the twin; (f32, True) = the fp32 chain twin.
    ``mutate``: an entry of MUTANTS.  -> out as float64 (with ``parts``: out, {"n", "t", "gate"})"""
    m = mutate or {}
    rt = torch.float64 if real == "f64" else torch.float32
    rnd = (lambda v: v.to(dt).to(rt)) if rounded else (lambda v: v)
    B, D, H, W = x.shape
    h = w_out.shape[1]
    xr = x.to(rt)
    per_c = lambda v: v.to(rt).view(1, D, 1, 1)
    if m.get("one_pass"):                     # E[x^2] - mu^2 in fp32, the channels added one after the other as a thread would
        xf = x.float()
        s1, s2 = torch.zeros(B, 1, H, W), torch.zeros(B, 1, H, W)
        for c in range(D):
            s1 += xf[:, c:c + 1]
            s2 += xf[:, c:c + 1] * xf[:, c:c + 1]
        mu32 = s1 / D
        mu, var = mu32.to(rt), (s2 / D - mu32 * mu32).to(rt)
    else:
        mu = xr.mean(1, keepdim=True)
        var = ((xr - mu) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + (0.0 if m.get("no_eps") else EPS))
    if ln_b is not None:
        n = (xr - mu) * rstd * per_c(ln_w) + per_c(ln_b)
    elif m.get("centred_biasfree"):
        n = (xr - mu) * rstd * per_c(ln_w)
    else:
        n = xr * rstd * per_c(ln_w)
    n = rnd(n)
    # the pixels around the image are 0 AFTER the LayerNorm; without a project_in bias t = W 0 = 0 there: the zero padding of t
    if m.get("outside_bias") and ln_b is not None:
        npad = rnd(per_c(ln_b)).expand(B, D, H + 2, W + 2).clone()
        npad[:, :, 1:-1, 1:-1] = n
    else:
        npad = F.pad(n, (1, 1, 1, 1))
    t = rnd(torch.einsum("md,bdhw->bmhw", w_in.to(dt).to(rt), npad))
    k = w_dw.float().to(rt).reshape(2 * h, 3, 3).clone()
    if "drop_tap" in m:
        plane, tap = m["drop_tap"]
        k[plane * h + h // 2].view(9)[tap] = 0.0
    cols = (torch.arange(W) % TILE_W != 0).to(rt).view(1, 1, 1, W)
    rows = (torch.arange(H) % BAND != 0).to(rt).view(1, 1, H, 1)
    conv = torch.zeros(B, 2 * h, H, W, dtype=rt)
    for dr in range(3):
        for dc in range(3):
            term = k[:, dr, dc].view(1, -1, 1, 1) * t[:, :, dr:dr + H, dc:dc + W]
            if m.get("left_halo") and dc == 0:
                term = term * cols
            if m.get("top_halo") and dr == 0:
                term = term * rows
            conv += term
    x1, x2 = conv[:, :h], conv[:, h:]
    gate = rnd(0.5 * x1 * (1.0 + torch.erf(x1 / math.sqrt(2.0))) * x2)
    if m.get("drop_last_pair"):
        gate[:, h - 1] = 0.0
    branch = torch.einsum("dm,bmhw->bdhw", w_out.to(dt).to(rt), gate)
    out = ((n if m.get("skip_from_n") else xr) + branch).double()
    return (out, {"n": n, "t": t[:, :, 1:-1, 1:-1], "gate": gate}) if parts else out


#: reference-side modifications: what a wrong kernel would compute.  Applied to the CPU twin only, never to the kernel.
MUTANTS = {
    "left halo column of a 16-wide tile reads 0": {"left_halo": True},
    "halo row above a 2-row band reads 0": {"top_halo": True},
    "last hidden pair dropped": {"drop_last_pair": True},
    "one tap of one pair dropped": {"drop_tap": (0, 2)},          # pair h // 2, x1 plane, the top right tap
    "outside the image normalised to ln_b": {"outside_bias": True},
    "one-pass variance in fp32": {"one_pass": True},
    "eps dropped": {"no_eps": True},
    "BiasFree form centred": {"centred_biasfree": True},
    "skip taken from the normalised tile": {"skip_from_n": True},
}


def references(x, ln_w, ln_b, w_in, w_dw, w_out, dt):
    """-> (ref64, twin64)"""
    return (reference(x, ln_w, ln_b, w_in, w_dw, w_out, dt, "f64", False),
            reference(x, ln_w, ln_b, w_in, w_dw, w_out, dt, "f64", True))


# ---- the comparison ---------------------------------------------------------------------------------------------------------------
def needed(got, ref64, twin64, dt):
    """-> (per-element tensor of the margin ``got`` needs, E)"""
    g = got.detach().double().cpu()
    assert g.shape == ref64.shape, f"shape {tuple(g.shape)} vs {tuple(ref64.shape)}"
    E = max(float((twin64 - ref64).abs().max()), 2.0 ** -23 * float(ref64.abs().max()))
    bad = ~torch.isfinite(g)
    g = torch.where(bad, torch.zeros_like(g), g)
    r = ((g - ref64).abs() - UNIT[dt] * ref64.abs()).clamp_min(0.0) / E
    return torch.where(bad, torch.full_like(r, math.inf), r), E


def compare(got, ref64, twin64, dt, label, margin=None):
    """assert that every element of ``got`` lies within ``margin`` (default MARGIN) times the twin's own error of the float64
    reference, plus one unit of ``dt`` for the final store, and that everything is finite"""
    margin = MARGIN if margin is None else margin
    assert 1 <= MARGIN <= MARGIN_CAP
    r, E = needed(got, ref64, twin64, dt)
    worst = float(r.max())
    RATIOS.append((label, NAME[dt], worst))
    if not worst <= margin:
        i = int(torch.argmax(r))
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), r.shape))
        raise AssertionError(f"[{label} {NAME[dt]}] {int((~(r <= margin)).sum())}/{r.numel()} beyond {margin} x the twin's error "
                             f"(E = {E:.3g}); worst needs {worst:.3g} x at (b, d, row, col) = {idx}")
    return worst
