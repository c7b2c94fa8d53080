"""The limit of tests/scan_regimes.py is a CONDITION, checked here without a GPU: at the cap of 32 x the fp32 oracle's own error
(a) the fp32 oracle itself passes, so the limit can be met, and (b) a float64 result in which ONE state slot's carry across the
second chunk boundary is wrong by 1 % is rejected -- the error a wrong lane, a wrong pair of the two-states-at-a-time walk or a
wrong piece of the carry split would make, and which the suite's contract tolerance (6e-4 / 2e-3) does not see.  Everything is
built from the float64 oracle alone."""
import pytest
import torch

import scan_regimes as sr
from oracle import oss_oracle

pytestmark = pytest.mark.tier(0)

SHAPE = (2, 24, 16, 2, 1541)
CUT = 1024                    # the second boundary of 512-step chunks
_CASES = {}


def _case(regime):
    """inputs and both references of a regime, computed once and shared (nothing below changes them)"""
    if regime not in _CASES:
        inputs = sr.make_regime(regime, *SHAPE, torch.float32)
        _CASES[regime] = (inputs,) + sr.references(inputs, sr.SOFTPLUS[regime])
    return _CASES[regime]


def _needs(regime, q, value):
    inputs, ref64, ref32 = _case(regime)
    return sr.measure({q: value}, ref64, ref32, torch.float32)[q]


@pytest.mark.parametrize("regime", sr.REGIMES)
@pytest.mark.parametrize("itype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_references_are_finite_in_every_regime(regime, itype):
    inputs = sr.make_regime(regime, *SHAPE, itype)
    for ref in sr.references(inputs, sr.SOFTPLUS[regime], lane_states=True):
        for q, v in ref.items():
            assert v is None or bool(torch.isfinite(v).all()), q
    assert (inputs[6] is None) == (regime in ("slow", "none"))


def test_regimes_keep_the_carries_they_promise():
    """share of (row, state) pairs whose running product over a 512-step chunk is above 1e-3"""
    share = {}
    for regime in sr.REGIMES:
        u, delta, A, B, C, D, bias, dout = sr.make_regime(regime, *SHAPE, torch.float32)
        dt = delta.double() + (0 if bias is None else bias.double()[None, :, None])
        dt = torch.nn.functional.softplus(dt) if sr.SOFTPLUS[regime] else dt
        logp = dt[:, :, :512].sum(-1)[:, :, None] * A.double()[None]
        share[regime] = float((logp.exp() > 1e-3).double().mean())
    assert share["slow"] == 1.0 and share["none"] == 1.0 and share["stiff"] == 0.0
    assert 0.1 < share["arch"] < 0.4, share


@pytest.mark.parametrize("regime", ["arch", "slow", "none", "stiff"])
def test_fp32_oracle_meets_the_limit(regime):
    """the limit is reachable: the fp32 oracle needs a margin of exactly 1 by construction, hence passes at MARGIN and at 32"""
    inputs, ref64, ref32 = _case(regime)
    for margin in (sr.MARGIN, sr.MARGIN_CAP):
        sr.compare(dict(ref32), ref64, ref32, torch.float32, margin, f"fp32 oracle {regime}")
    for q, r in sr.measure(dict(ref32), ref64, ref32, torch.float32).items():
        assert float(r.max()) <= 1.0 + 1e-12, q


def _forward_mutant(regime, n):
    """float64 ``out`` with 1 % added to what state slot ``n`` carries across t = CUT"""
    (u, delta, A, B, C, D, bias, dout), ref64, _ = _case(regime)
    Cn = torch.zeros_like(C)
    Cn[:, :, n] = C[:, :, n]
    sp = sr.SOFTPLUS[regime]
    out_n, _ = oss_oracle.scan_fwd(u, delta, A, B, Cn, None, bias, sp, real="f64")
    tail = lambda t: t[..., CUT:].contiguous()
    restart_n, _ = oss_oracle.scan_fwd(tail(u), tail(delta), A, tail(B), tail(Cn), None, bias, sp, real="f64")
    mutant = ref64["out"].clone()
    mutant[..., CUT:] += 1e-2 * (out_n[..., CUT:] - restart_n)
    return mutant


# slot 15 of `arch` (A = -16) decays to nothing within a chunk by construction: it carries nothing to be wrong about
@pytest.mark.parametrize("regime,n", [("slow", 0), ("slow", 7), ("slow", 15), ("none", 0), ("none", 7), ("none", 15),
                                      ("arch", 0), ("arch", 7)])
def test_one_slot_carry_error_is_rejected(regime, n):
    mutant = _forward_mutant(regime, n)
    needs = _needs(regime, "out", mutant)
    for margin in (sr.MARGIN, sr.MARGIN_CAP):
        beyond = int((needs > margin).sum())
        print(f"{regime} slot {n}: {beyond}/{needs.numel()} outputs beyond {margin} x E32, worst needs {float(needs.max()):.3g}")
        assert beyond > 0
        with pytest.raises(AssertionError, match="out:"):
            _, ref64, ref32 = _case(regime)
            sr.compare(dict(ref64, out=mutant), ref64, ref32, torch.float32, margin, "mutant")


@pytest.mark.parametrize("n", [0, 7, 15])
def test_contract_tolerance_accepts_the_same_error(n):
    """what this file adds: the fp32 contract of test_scan_gpu.py (rtol 6e-4, atol 2e-3) flags none of the mutant's outputs"""
    ref = _case("slow")[1]["out"]
    diff = (_forward_mutant("slow", n) - ref).abs()
    assert float(diff.max()) > 0
    assert int((diff > 2e-3 + 6e-4 * ref.abs()).sum()) == 0


@pytest.mark.parametrize("regime", ["slow", "none"])
def test_reverse_carry_error_is_rejected(regime):
    """the part of du at t < 512 that comes from dout at t >= CUT (the backward's reverse carry across two boundaries), 1 % off"""
    (u, delta, A, B, C, D, bias, dout), ref64, ref32 = _case(regime)
    late = dout.clone()
    late[..., :CUT] = 0
    du_late = oss_oracle.scan_bwd(u, delta, A, B, C, D, bias, late, None, sr.SOFTPLUS[regime], real="f64")[0]
    mutant = ref64["du"].clone()
    mutant[..., :512] += 1e-2 * du_late[..., :512]
    needs = _needs(regime, "du", mutant)
    for margin in (sr.MARGIN, sr.MARGIN_CAP):
        print(f"{regime}: {int((needs > margin).sum())}/{needs.numel()} of du beyond {margin} x E32, worst {float(needs.max()):.3g}")
        with pytest.raises(AssertionError, match="du:"):
            sr.compare(dict(ref64, du=mutant), ref64, ref32, torch.float32, margin, "mutant")


def test_dead_running_products_may_be_flushed_but_not_wrong():
    """entries of the running product below 1e-30 must stay below 2e-30 and finite; live ones are compared relatively"""
    _, ref64, ref32 = _case("stiff")
    x = ref64["x"].clone()
    assert float(x[..., 0::2].max()) < sr.TINY
    flushed = x.clone()
    flushed[..., 0::2] = 0
    sr.compare({"x": flushed}, ref64, ref32, torch.float32, 1, "flushed")
    for poison in (1e-20, float("nan"), float("inf")):
        wrong = x.clone()
        wrong[0, 0, 0, 0] = poison
        with pytest.raises(AssertionError, match="x products"):
            sr.compare({"x": wrong}, ref64, ref32, torch.float32, sr.MARGIN_CAP, "poisoned")
    _, ref64, ref32 = _case("slow")
    wrong = ref64["x"].clone()
    wrong[1, 3, 2, 10] *= 1 + 1e-3          # a live product of slot 5
    with pytest.raises(AssertionError, match="x products"):
        sr.compare({"x": wrong}, ref64, ref32, torch.float32, sr.MARGIN_CAP, "product")
    wrong = ref64["x"].clone()
    wrong[1, 3, 2, 11] *= 1 + 1e-3          # the state of slot 5
    with pytest.raises(AssertionError, match="x states"):
        sr.compare({"x": wrong}, ref64, ref32, torch.float32, sr.MARGIN_CAP, "state")


def test_sixteen_bit_outputs_get_one_unit_and_no_more():
    inputs = sr.make_regime("slow", 1, 4, 16, 2, 600, torch.bfloat16)
    ref64, ref32 = sr.references(inputs, False)
    rounded = ref64["out"].to(torch.bfloat16)
    sr.compare({"out": rounded}, ref64, ref32, torch.bfloat16, 1, "rounded once")
    with pytest.raises(AssertionError, match="out:"):
        sr.compare({"out": ref64["out"] * (1 + 3 * 2.0 ** -8)}, ref64, ref32, torch.bfloat16, sr.MARGIN_CAP, "three units")
