"""The one-launch EFFN forward (csrc/oss_effn.hip, ``torch.ops.vmambair.effn_fwd``) against the FLOAT64 reference of
tests/effn_cases.py: every instantiation with dense weights on the smallest planes that have the tile geometry (a), every hidden
pair alone through a selecting project_out (b), ``hidden`` at one chunk, one chunk + one pair and a single pair (c), the kernel's
own LayerNorm stage where the statistics are hard (d), strided inputs and a dirty output (e) and the G9 fixtures of the reference
(f).  The limit is effn_cases.compare: MARGIN x the error that rounding the three intermediates causes on the same inputs, plus
one unit of the type for the final store -- it does not know about the skip connection; what it rejects is shown on the CPU in
test_effn_regimes_host.py.  The weights the reference sees are the ones ops.effn_round_weights left on the device."""
import pytest
import torch

import effn_cases as ec
from conftest import golden_files, load_golden
from vmambair_amd import ops, oss_block
from vmambair_amd.ops import ffn as ffn_ops

pytestmark = [pytest.mark.gpu, pytest.mark.tier(0)]
DEV = "cuda:0"


def _launch(case):
    """one launch of the raw op on the case's inputs -> (out, x on the device, the device tensors of the call, the CPU inputs of the
    reference: x, ln_w, ln_b and the rounded weights read back from the device)"""
    x, lw, lb, w_in, w_dw, w_out = case.inputs()
    h, D = case.h, case.D
    padded = ops.effn_round_weights(w_in.view(2 * h, D, 1, 1).to(DEV), w_dw.view(2 * h, 1, 3, 3).to(DEV), w_out.view(D, h, 1, 1).to(DEV),
                                    case.dt)
    xd, lwd, lbd = x.to(DEV), lw.to(DEV), (None if lb is None else lb.to(DEV))
    assert ffn_ops.effn_fwd_ok(xd, h), case.id
    out = torch.ops.vmambair.effn_fwd(xd, lwd, lbd, *padded, h)
    torch.cuda.synchronize()
    assert out.dtype == case.dt and out.shape == x.shape
    return out, xd, (lwd, lbd) + tuple(padded), (x, lw, lb) + ec.unpad_weights(*padded, h)


def _vs_float64(case):
    out, xd, _, inp = _launch(case)
    if case.weights != "dense":   # output channels whose pair lies behind ``hidden`` have a zero row of project_out: x, bit for bit
        behind = [d for d in range(case.D) if case.weights[1] * case.D + d >= case.h]
        assert torch.equal(out[:, behind], xd[:, behind]), f"{case.id}: channels {behind[:1]}.. must return x itself"
    ref64, twin64 = ec.references(*inp, case.dt)
    print(f"[effn f64] {case.id}: needs {float(ec.needed(out, ref64, twin64, case.dt)[0].max()):.3f}")
    ec.compare(out, ref64, twin64, case.dt, case.id)


@pytest.mark.parametrize("case", ec.CASES_A, ids=lambda c: c.id)
def test_dense_weights_every_instantiation_vs_float64(case):
    """(1, D, 8, 16): one full tile; (1, D, 9, 24): ragged both ways; (2, D, 17, 40): 3 x 3 tiles, seams and ragged edges both ways"""
    _vs_float64(case)


@pytest.mark.parametrize("case", ec.CASES_B, ids=lambda c: c.id)
def test_every_hidden_pair_alone_vs_float64(case):
    """project_out selects pair run D + d for output channel d: out - x is that pair's gate output, the last ragged chunk included;
    the channels behind ``hidden`` return x itself"""
    _vs_float64(case)


@pytest.mark.parametrize("case", ec.CASES_C, ids=lambda c: c.id)
def test_hidden_edges_through_the_raw_op_vs_float64(case):
    """hidden = 1 (a single pair), 16 (one chunk exactly: ``more`` is never true), 17 (one chunk + one pair), 32 (two full chunks)"""
    _vs_float64(case)


@pytest.mark.parametrize("case", ec.CASES_D, ids=lambda c: c.id)
def test_layernorm_stage_in_hard_regimes_vs_float64(case):
    """stage 0b of the kernel (a fourth LayerNorm implementation) on ln_regimes' inputs; BiasFree where effn_cases.EXCLUDED_D admits"""
    _vs_float64(case)


# ---- e. strided inputs and a dirty output (an equivalence of two launches: no float64 needed) ---------------------------------
def _channel_slice(x):
    B, D, H, W = x.shape
    wide = torch.full((B, 2 * D, H, W), float("nan"), dtype=x.dtype, device=DEV)
    v = wide[:, D // 2:D // 2 + D]
    v.copy_(x)
    assert v.stride(1) == H * W and v.stride(0) == 2 * D * H * W and v.storage_offset() > 0
    return v


def _batch_slice(x):
    B, D, H, W = x.shape
    big = torch.full((2 * B, D, H, W), float("nan"), dtype=x.dtype, device=DEV)
    v = big[::2]
    v.copy_(x)
    assert v.stride(0) == 2 * D * H * W
    return v


def _offset(x, elements):
    buf = torch.full((x.numel() + 16,), float("nan"), dtype=x.dtype, device=DEV)
    v = buf[elements:elements + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() == buf.data_ptr() + 2 * elements
    return v


@pytest.mark.tier(2)
@pytest.mark.parametrize("dt", ec.TYPES, ids=[ec.NAME[d] for d in ec.TYPES])
@pytest.mark.parametrize("D", [48, 96])
def test_strided_inputs_and_a_dirty_output_equal_the_contiguous_launch(D, dt):
    """xsb / xsc of the kernel: a channel slice of a tensor twice as wide, every other image of a batch, a base pointer 16 bytes into
    an allocation -- each surrounded by NaN, each accepted, each bit-identical to the launch on a contiguous copy; and the op's
    output does not depend on what its allocation held before"""
    case = ec.Case("e", D, dt, True, (2, 17, 40))
    want, xd, rest, _ = _launch(case)
    for place in (_channel_slice, _batch_slice, lambda t: _offset(t, 8)):
        v = place(xd)
        assert not v.is_contiguous() or v.storage_offset() > 0
        assert torch.equal(v, xd) and ffn_ops.effn_fwd_ok(v, case.h)
        got = torch.ops.vmambair.effn_fwd(v, *rest, case.h)
        assert got.is_contiguous() and torch.equal(got, want)
    dirty = torch.full(want.shape, float("nan"), dtype=dt, device=DEV)
    ptr = dirty.data_ptr()
    del dirty
    again = torch.ops.vmambair.effn_fwd(xd, *rest, case.h)
    print(f"[effn e] the second output {'reused' if again.data_ptr() == ptr else 'did not reuse'} the NaN-filled allocation")
    assert torch.equal(again, want)


@pytest.mark.tier(2)
@pytest.mark.parametrize("dt", ec.TYPES, ids=[ec.NAME[d] for d in ec.TYPES])
def test_unaligned_and_w_strided_inputs_are_refused(dt):
    """a W-strided view, a channel stride that is no multiple of 8 elements and a base pointer 8 bytes off the 16-byte grid: not
    taken by effn_fwd_ok, and the raw op raises instead of launching"""
    case = ec.Case("e", 48, dt, True, (1, 9, 24))
    _, xd, rest, _ = _launch(case)
    B, D, H, W = xd.shape
    w_strided = torch.zeros(B, D, H, 2 * W, dtype=dt, device=DEV)[..., ::2]
    planes = torch.zeros(B * D * (H * W + 4), dtype=dt, device=DEV).as_strided((B, D, H, W), (D * (H * W + 4), H * W + 4, W, 1))
    off8 = _offset(xd, 4)
    assert planes.stride(1) % 8 == 4 and off8.data_ptr() % 16 == 8
    for v in (w_strided, planes, off8):
        assert not ffn_ops.effn_fwd_ok(v, case.h)
        with pytest.raises(RuntimeError):
            torch.ops.vmambair.effn_fwd(v, *rest, case.h)


# ---- f. the reference's own vectors under the new measure ----------------------------------------------------------------------
def _g9(name):
    """the reference's ``norm2`` + ``ffn`` of one G9 fixture as this repo's modules (as test_effn_gpu.py loads them), input, output"""
    z = load_golden(name)
    norm = oss_block.LayerNorm(int(z["dim"]), str(z["ln"]))
    ff = oss_block.FeedForward(int(z["dim"]), 2.66, False)
    norm.load_state_dict({k[len("sd.norm2."):]: v.float() for k, v in z.items() if k.startswith("sd.norm2.")}, strict=True)
    ff.load_state_dict({k[len("sd.ffn."):]: v.float() for k, v in z.items() if k.startswith("sd.ffn.")}, strict=True)
    return norm, ff, z["x"].float(), z["y"].float()


@pytest.mark.parametrize("name", golden_files("g9_effn_"))
def test_g9_golden_fixtures_under_the_float64_measure(name):
    """G9 (``x + ffn(norm2(x))`` of the reference's MamberBlock, fp16-exact weights and input, fp32 arithmetic): the reference's own y
    takes the place of the float64 reference, the twin is built from the fixture's weights; the module runs the one launch"""
    norm, ff, x, want = _g9(name)
    D, h, dt = x.shape[1], ff.project_out.in_channels, torch.float16
    w = ec.round_weights(ff.project_in.weight.detach().reshape(2 * h, D), ff.dwconv.weight.detach().reshape(2 * h, 9),
                         ff.project_out.weight.detach().reshape(D, h), dt)
    lw, lb = norm.body.weight.detach(), (norm.body.bias.detach() if norm.with_bias else None)
    twin64 = ec.reference(x.to(dt), lw, lb, *w, dt, "f64", True)
    xh = x.to(DEV).half()
    assert ffn_ops.effn_fwd_ok(xh, h)
    with torch.no_grad():
        got = ff.to(DEV)(xh, pre_norm=norm.to(DEV))
    rel = float((got.float().cpu() - want).norm() / want.norm())
    print(f"[effn f64] f-{name}: needs {float(ec.needed(got, want.double(), twin64, dt)[0].max()):.3f} (rel-L2 vs the reference {rel:.2e})")
    ec.compare(got, want.double(), twin64, dt, f"f-{name}")
