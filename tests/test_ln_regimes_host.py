"""The limit of tests/ln_regimes.py is a CONDITION, checked here without a GPU: at the cap of 32 x the fp32 twin's own error
(a) the twin itself and a correct closed-form fp32 LayerNorm pass, so the limit can be met, and (b) fp32 implementations of the
same formulas with ONE of the mistakes a kernel can make -- a one-pass variance, a divisor padded to the register slots, a
dropped eps, a centred BiasFree form, a dropped term of the backward, a dropped skip gradient, one channel's weight gradient off
by 1 %, an unbiased variance -- are rejected, with the quantity named in the message.  The outputs are taken as fp32 (the pairs
x -> float32 of the kernels), so that no 16-bit unit stands between the mistake and the limit."""
import pytest
import torch

import ln_regimes as lr

pytestmark = pytest.mark.tier(0)

B, C, P = 2, 96, 126
TYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
_CASES = {}


def _case(regime, xdt=torch.float32, bias=True, gate=True, skip=True, C=C):
    """inputs and both references of a case, computed once and shared (nothing below changes them)"""
    key = (regime, xdt, bias, gate, skip, C)
    if key not in _CASES:
        inp = lr.make_inputs(regime, B, C, P, xdt, torch.float32, seed=3, bias=bias, gate=gate, skip=skip)
        _CASES[key] = (inp,) + lr.references(inp)
    return _CASES[key]


def _fp32(inp, one_pass=False, pad24=False, no_eps=False, centred_biasfree=False, drop_m2=False, drop_skip=False, dw_off=False,
          unbiased=False, keep_mean_rounding=False):
    """closed-form fp32 LayerNorm forward and backward as the kernels write it (oss_layernorm.hip), with the named mistake"""
    f = lambda t: None if t is None else t.float()
    x, w, b, gate, dy, skip = (f(inp[k]) for k in ("x", "w", "b", "gate", "dy", "skip"))
    Cc = x.shape[1]
    div = float(-(-Cc // 24) * 24 if pad24 else Cc)
    mean = x.sum(1) / div
    xc = x - mean[:, None]
    var = (x * x).sum(1) / div - mean * mean if one_pass else (xc * xc).sum(1) / (div - 1 if unbiased else div)
    rstd = 1.0 / torch.sqrt(var + (0.0 if no_eps else lr.EPS))
    r, wb = rstd[:, None], w[None, :, None]
    xh = xc * r
    centred = b is not None or centred_biasfree
    n = xh * wb + (b[None, :, None] if b is not None else 0.0) if centred else x * r * wb
    got = {"mean": mean, "rstd": rstd, "n": n}
    g = dy
    if gate is not None:
        sg = torch.sigmoid(gate)
        got["dgate"] = dy * n * (sg + gate * sg * (1 - sg))
        g = dy * gate * sg
        got["y"] = n * gate * sg
    else:
        got["y"] = n
    gw = g * wb
    if b is not None:
        m1, m2 = gw.sum(1) / Cc, (gw * xh).sum(1) / Cc
        dx = r * (gw - m1[:, None] - xh * (0.0 if drop_m2 else m2[:, None]))
        got["dw"], got["db"] = (g * xh).sum((0, 2)), g.sum((0, 2))
    else:
        m2 = (gw * x).sum(1) / Cc
        if not keep_mean_rounding:       # x - mean - mean_c(x - mean): the rounding of the fp32 mean taken out again
            xh = (xc - (xc.sum(1) / Cc)[:, None]) * r
        dx = r * gw - xh * r * r * (0.0 if drop_m2 else m2[:, None])
        got["dw"] = (g * x * r).sum((0, 2))
    got["dx"] = dx + skip if skip is not None and not drop_skip else dx
    if dw_off:
        got["dw"][int(got["dw"].abs().argmax())] *= 1.01
    return got


def _rejected(case, types, match, **mistake):
    inp, ref64, ref32 = case
    with torch.no_grad():
        got = _fp32(inp, **mistake)
    needs = {q: float(r.max()) for q, (r, _) in lr.measure(got, ref64, ref32, types).items()}
    print(f"{mistake}: needs " + ", ".join(f"{q} {v:.3g}" for q, v in needs.items()))
    with pytest.raises(AssertionError, match=match):
        lr.compare(got, ref64, ref32, types, "mistake", margin=lr.MARGIN_CAP)


@pytest.mark.parametrize("regime", lr.REGIMES)
@pytest.mark.parametrize("bias", [True, False], ids=["WithBias", "BiasFree"])
def test_fp32_twin_and_closed_form_meet_the_limit(regime, bias):
    """the limit is reachable: the twin needs a margin of at most 1 by construction, and the kernels' closed form in fp32 passes
    at MARGIN and at the cap"""
    inp, ref64, ref32 = _case(regime, bias=bias)
    got = {q: v for q, v in ref32.items() if q != "x"}
    for q, (r, _) in lr.measure(got, ref64, ref32, (torch.float32, torch.float32)).items():
        assert float(r.max()) <= 1.0 + 1e-12, q
    with torch.no_grad():
        closed = _fp32(inp)
    for margin in (lr.MARGIN, lr.MARGIN_CAP):
        lr.compare(got, ref64, ref32, (torch.float32, torch.float32), f"twin {regime}", margin)
    for margin in (lr.MARGIN, lr.MARGIN_CAP):
        lr.compare(closed, ref64, ref32, (torch.float32, torch.float32), f"closed form {regime}", margin)


@pytest.mark.parametrize("regime", lr.REGIMES)
@pytest.mark.parametrize("xdt", list(TYPES), ids=list(TYPES))
@pytest.mark.parametrize("Cc", [1, 7, 96, 385])
def test_references_are_finite_in_every_regime(regime, xdt, Cc):
    inp = lr.make_inputs(regime, 2, Cc, 10, TYPES[xdt], TYPES[xdt], seed=5, gate=True, skip=True)
    assert inp["x"].dtype == TYPES[xdt] and bool(torch.isfinite(inp["x"].float()).all())
    for ref in lr.references(inp):
        for q, v in ref.items():
            assert v is not None and bool(torch.isfinite(v).all()), q


@pytest.mark.parametrize("xdt", list(TYPES), ids=list(TYPES))
def test_flat_constant_pixels_give_the_bias_exactly(xdt):
    inp, ref64, _ = _case("flat", TYPES[xdt], gate=False)
    x = inp["x"].float()
    const = (x == x[:, :1]).all(1)
    assert bool(const[:, :P // 2].all()) and not bool(const[:, P // 2:].all())
    assert float(ref64["rstd"][:, :P // 2].sub(lr.EPS ** -0.5).abs().max()) < 1e-10
    want = inp["b"].double()[None, :, None].expand(B, C, P // 2)
    assert torch.equal(ref64["y"][:, :, :P // 2], want)


@pytest.mark.parametrize("xdt", list(TYPES), ids=list(TYPES))
def test_one_pass_variance_is_rejected_on_offset(xdt):
    _rejected(_case("offset", TYPES[xdt]), (TYPES[xdt], torch.float32), "rstd:", one_pass=True)
    inp, ref64, ref32 = _case("offset", TYPES[xdt])
    with torch.no_grad():
        got = _fp32(inp, one_pass=True)
    needs = float(lr.measure({"y": got["y"]}, ref64, ref32, (TYPES[xdt], torch.float32))["y"][0].max())
    print(f"one-pass variance, offset, {xdt}: y needs {needs:.4g} x the twin's error")
    assert needs > lr.MARGIN_CAP


def test_one_pass_variance_is_rejected_on_flat():
    _rejected(_case("flat"), (torch.float32, torch.float32), "rstd:", one_pass=True)


def test_divisor_padded_to_the_register_slots_is_rejected():
    """C = 90 divided by 96: what a sum over 24-channel slots that counts its padding would do"""
    _rejected(_case("plain", C=90), (torch.float32, torch.float32), "mean:", pad24=True)


def test_dropped_eps_is_rejected_on_flat():
    _rejected(_case("flat"), (torch.float32, torch.float32), "rstd:", no_eps=True)


def test_centred_biasfree_form_is_rejected_on_offset():
    _rejected(_case("offset", bias=False), (torch.float32, torch.float32), "y:", centred_biasfree=True)


@pytest.mark.parametrize("bias", [True, False], ids=["WithBias", "BiasFree"])
def test_dropped_m2_term_is_rejected(bias):
    _rejected(_case("plain", bias=bias), (torch.float32, torch.float32), "dx:", drop_m2=True)


def test_rounding_of_the_stored_mean_is_rejected_in_the_biasfree_backward(regime="flat", xdt="f32"):
    """What the GPU tests found in the kernels (and why they now subtract the mean of the residuals): BiasFree dx multiplies
    x - mean by rstd^3 mean(g w x), which does not shrink with the variance, so the rounding of the fp32 mean alone -- |mean| 2^-24
    -- is 2 % of dx at var << eps (9400 x the twin's error on `flat`; 16 x on `offset` and 30 x on `flat` with float16 x, under the
    cap).  Autograd differentiates the computed function and cancels it, hence the twin does not have it."""
    _rejected(_case(regime, TYPES[xdt], bias=False), (TYPES[xdt], torch.float32), "dx:", keep_mean_rounding=True)


def test_dropped_skip_gradient_is_rejected():
    _rejected(_case("plain"), (torch.float32, torch.float32), "dx:", drop_skip=True)


def test_one_channel_of_dw_off_by_one_percent_is_rejected():
    _rejected(_case("plain"), (torch.float32, torch.float32), "dw:", dw_off=True)


def test_unbiased_variance_is_rejected():
    _rejected(_case("plain"), (torch.float32, torch.float32), "rstd:", unbiased=True)


def test_sixteen_bit_outputs_get_one_unit_and_no_more():
    inp, ref64, ref32 = _case("plain", torch.bfloat16)
    types = (torch.bfloat16, torch.bfloat16)
    lr.compare({"y": ref64["y"].to(torch.bfloat16), "dx": ref64["dx"].to(torch.bfloat16)}, ref64, ref32, types, "rounded once", 1)
    with pytest.raises(AssertionError, match="y:"):
        lr.compare({"y": ref64["y"] * (1 + 3 * 2.0 ** -8)}, ref64, ref32, types, "three units", lr.MARGIN_CAP)
    with pytest.raises(AssertionError, match="rstd:"):          # fp32 quantities get none
        lr.compare({"rstd": ref64["rstd"] * (1 + 2.0 ** -9)}, ref64, ref32, types, "rstd", lr.MARGIN_CAP)


@pytest.mark.parametrize("regime", lr.REGIMES)
@pytest.mark.parametrize("bias", [True, False], ids=["WithBias", "BiasFree"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_reference_rounded_once_meets_the_limit_without_any_margin(regime, bias, dt):
    """the unit term is what ONE rounding to the type costs, the subnormal range of float16 (dx of `outlier` and `wide` has
    elements near 1e-7) and its overflow (`flat` in the BiasFree form: dx beyond 65504) included: the float64 reference itself,
    stored in the type, needs no margin at all"""
    dt = TYPES[dt]
    inp = lr.make_inputs(regime, B, C, P, dt, dt, seed=3, bias=bias, gate=True, skip=True)
    ref64, ref32 = lr.references(inp)
    got = {q: ref64[q].to(dt) for q in ("y", "n", "dx", "dgate")}
    for q, (r, _) in lr.measure(got, ref64, ref32, (dt, dt)).items():
        assert float(r.max()) == 0.0, q


def test_non_finite_values_are_rejected():
    inp, ref64, ref32 = _case("plain")
    for poison in (float("nan"), float("inf")):
        wrong = ref64["y"].clone()
        wrong[1, 5, 17] = poison
        with pytest.raises(AssertionError, match="y:"):
            lr.compare({"y": wrong}, ref64, ref32, (torch.float32, torch.float32), "poisoned", lr.MARGIN_CAP)
