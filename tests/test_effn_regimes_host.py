"""The limit of tests/effn_cases.py is a CONDITION, checked here without a GPU: at the cap of 8 x the twin's own error (a) the
fp32 chain twin -- fp32 arithmetic, the same three roundings -- passes with a margin of 2 in EVERY case of the GPU grid, so the
limit can be met, and (b) every mutant of effn_cases.MUTANTS needs more than the cap in at least one case of that grid, in both
16-bit types.  (c) decides which regime / form / type combinations the grid may hold: the twin's n, t and gate output stay below
half the largest finite value of the type."""
import pytest
import torch

import effn_cases as ec

pytestmark = pytest.mark.tier(0)

_REFS = {}


def _refs(case):
    """inputs (weights as the kernel reads them), float64 reference, twin and the twin's intermediates: computed once per case and
    shared (nothing below changes them)"""
    if case.id not in _REFS:
        x, lw, lb, w_in, w_dw, w_out = case.inputs()
        inp = (x, lw, lb) + ec.round_weights(w_in, w_dw, w_out, case.dt)
        ref64 = ec.reference(*inp, case.dt, "f64", False)
        twin64, parts = ec.reference(*inp, case.dt, "f64", True, parts=True)
        _REFS[case.id] = (inp, ref64, twin64, parts)
    return _REFS[case.id]


def _needs(case, mutate=None, real="f32"):
    inp, ref64, twin64, _ = _refs(case)
    got = ec.reference(*inp, case.dt, real, True, mutate=mutate)
    return float(ec.needed(got, ref64, twin64, case.dt)[0].max())


def test_the_grid_is_what_the_gpu_file_runs():
    ids = [c.id for c in ec.FLOAT64_CASES]
    assert len(set(ids)) == len(ids)
    assert len(ec.CASES_A) == 48 and len(ec.CASES_B) == 24 and len(ec.CASES_C) == 12
    assert {c.h for c in ec.CASES_A} == {85, 127, 170, 255} and all(-(-c.h // c.D) == 3 for c in ec.CASES_B)
    assert len(ec.CASES_D) == 2 * 2 * 2 * 5 - 2 * len(ec.EXCLUDED_D)


@pytest.mark.parametrize("case", ec.FLOAT64_CASES, ids=lambda c: c.id)
def test_fp32_chain_twin_meets_the_limit_and_the_intermediates_fit_the_type(case):
    """the fp32 chain twin (what the launch-per-layer chain computes, final sum unrounded) needs at most 2; and the case belongs
    in the grid: n, t and the gate output of the twin are finite and below half the largest finite value of the type"""
    inp, ref64, twin64, parts = _refs(case)
    lim = torch.finfo(case.dt).max / 2
    for q, v in parts.items():
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) < lim, f"{q}: max |.| = {float(v.abs().max()):.3g}"
    assert bool(torch.isfinite(ref64).all())
    got = ec.reference(*inp, case.dt, "f32", True)
    worst = ec.compare(got, ref64, twin64, case.dt, case.id, margin=2)
    print(f"[fp32 chain twin] {case.id}: needs {worst:.3f}")
    assert float(ec.needed(twin64, ref64, twin64, case.dt)[0].max()) <= 1.0     # the twin itself: at most 1 by construction


@pytest.mark.parametrize("regime,bias,dt", list(ec.EXCLUDED_D), ids=[f"{r}-{'WithBias' if b else 'BiasFree'}-{ec.NAME[d]}"
                                                                       for r, b, d in ec.EXCLUDED_D])
def test_excluded_combinations_do_overflow_the_type(regime, bias, dt):
    """what EXCLUDED_D leaves out of section d is left out for the stated reason, at both widths"""
    for D in (48, 96):
        case = ec.Case("d", D, dt, bias, (2, 9, 24), regime=regime)
        x, lw, lb, w_in, w_dw, w_out = case.inputs()
        _, parts = ec.reference(x, lw, lb, *ec.round_weights(w_in, w_dw, w_out, dt), dt, "f64", False, parts=True)
        peak = float(parts["gate"].abs().max())
        print(f"{case.id}: unrounded max |gate output| = {peak:.3g}")
        assert peak > torch.finfo(dt).max / 2


def test_probe_weights_select_each_pair_exactly_once():
    for D in ec.DIMS:
        h = ec.hidden_of(D)
        total = torch.zeros(h)
        for run in range(3):
            w_in, w_dw, w_out = ec.probe(D, h, run)
            d_in, d_dw, _ = ec.dense(D, h)
            assert torch.equal(w_in, d_in) and torch.equal(w_dw, d_dw)
            assert set(w_out.unique().tolist()) <= {0.0, 1.0} and bool((w_out.sum(1) <= 1).all())
            total += w_out.sum(0)
        assert torch.equal(total, torch.ones(h)), D


def test_probe_weights_show_one_gate_output_per_channel():
    """under the probe weights out - x of the twin IS the rounded gate output of the selected pair (GEMM 2 carries it exactly)"""
    case = ec.Case("b", 32, ec.BF16, weights=("probe", 2))
    inp, _, twin64, parts = _refs(case)
    got = twin64 - inp[0].double()
    for d in range(32):
        want = parts["gate"][:, 64 + d] if 64 + d < case.h else torch.zeros_like(got[:, d])
        assert torch.equal(got[:, d], want), d


# ---- the mutants: where each is looked for (cases of the GPU grid only) ----------------------------------------------------------
def _grid(**want):
    return [c for c in ec.FLOAT64_CASES if all(getattr(c, k) == v for k, v in want.items())]


_SEAMS = [c for c in ec.CASES_A if c.bhw in ec.SEAM_SHAPES and c.bias]
_WHERE = {
    "left halo column of a 16-wide tile reads 0": _SEAMS,
    "halo row above a 2-row band reads 0": _SEAMS,
    "last hidden pair dropped": [c for c in ec.CASES_A if c.bhw == (2, 17, 40) and c.bias] + _grid(sec="b", weights=("probe", 2)),
    "one tap of one pair dropped": _grid(sec="b", weights=("probe", 1)),        # pair h // 2 lies in run 1 for every width
    "outside the image normalised to ln_b": [c for c in ec.CASES_A if c.bias],
    "one-pass variance in fp32": list(ec.CASES_D),
    "eps dropped": _grid(sec="d", regime="flat", bias=True),
    "BiasFree form centred": [c for c in ec.CASES_A + ec.CASES_D if not c.bias],
    "skip taken from the normalised tile": _grid(sec="a", bhw=(1, 8, 16)),
}
assert set(_WHERE) == set(ec.MUTANTS)
#: NOT a mistake at this type, so no case can reject it: a bfloat16 x has 8-bit significands, x^2 has 16 and the sum of up to 96 of
#: them at one exponent is exact in fp32 -- on `flat` (constant pixels) E[x^2] - mu^2 is exactly 0 and on `offset` (48 + randn,
#: steps of 0.25) it is off by one rounding of the division.  Looked for in ALL of section d: the most it needs is 6.6 (D = 96,
#: BiasFree, `flat`, the pixels where the 1e-3 noise moves some channels by one bfloat16 step).  In float16 (11-bit significands,
#: x^2 ~ 1e6 on `offset`, ~ 9 against var + eps ~ 1e-5 on `flat`) the same code gives a negative variance on `flat`.
_EQUIVALENT = {("one-pass variance in fp32", ec.BF16)}


@pytest.mark.parametrize("dt", ec.TYPES, ids=[ec.NAME[d] for d in ec.TYPES])
@pytest.mark.parametrize("name", list(ec.MUTANTS))
def test_every_mutant_needs_more_than_the_cap_somewhere(name, dt):
    cases = [c for c in _WHERE[name] if c.dt == dt]
    assert cases
    needs = [(_needs(c, ec.MUTANTS[name]), c.id) for c in cases]
    best, least = max(needs), min(needs)
    print(f"[mutant] {name}, {ec.NAME[dt]}: caught in {best[1]} needing {best[0]:.3g}; least over the {len(needs)} cases looked at: "
          f"{least[0]:.3g} in {least[1]}")
    if (name, dt) in _EQUIVALENT:
        assert best[0] <= ec.MARGIN_CAP, "this mutant is caught after all: take it out of _EQUIVALENT"
    else:
        assert best[0] > ec.MARGIN_CAP


@pytest.mark.parametrize("dt", ec.TYPES, ids=[ec.NAME[d] for d in ec.TYPES])
def test_seam_mutants_are_caught_at_every_width(dt):
    """the two seam mutants at (2, D, 17, 40), per instantiation: each KS has its own LDS geometry"""
    for name in ("left halo column of a 16-wide tile reads 0", "halo row above a 2-row band reads 0"):
        for c in [c for c in ec.CASES_A if c.dt == dt and c.bhw == (2, 17, 40)]:
            need = _needs(c, ec.MUTANTS[name])
            print(f"[mutant] {name}: {c.id} needs {need:.3g}")
            assert need > ec.MARGIN_CAP


@pytest.mark.parametrize("dt", ec.TYPES, ids=[ec.NAME[d] for d in ec.TYPES])
def test_one_dropped_tap_hides_under_dense_weights(dt):
    """why the probe cases exist: under dense weights project_out spreads one pair over every output channel at 1 / sqrt(h)"""
    name = "one tap of one pair dropped"
    for D in ec.DIMS:
        dense = _needs(ec.Case("a", D, dt, True, (1, 9, 24)), ec.MUTANTS[name])
        alone = _needs(ec.Case("b", D, dt, weights=("probe", 1)), ec.MUTANTS[name])
        print(f"[mutant] {name}, D = {D}, {ec.NAME[dt]}: needs {dense:.3g} under dense weights, {alone:.3g} with the pair alone")
        assert alone > ec.MARGIN_CAP


def test_reference_rounded_once_needs_no_margin_and_non_finite_values_an_infinite_one():
    case = ec.CASES_A[0]
    _, ref64, twin64, _ = _refs(case)
    assert float(ec.needed(ref64.to(case.dt), ref64, twin64, case.dt)[0].max()) == 0.0
    for poison in (float("nan"), float("inf")):
        wrong = ref64.clone()
        wrong[0, 5, 3, 7] = poison
        with pytest.raises(AssertionError, match="beyond"):
            ec.compare(wrong, ref64, twin64, case.dt, "poisoned", ec.MARGIN_CAP)
