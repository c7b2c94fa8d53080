"""The HIP selective scan (oss_scan_fwd.hip, oss_scan_bwd.hip, oss_scan_bwd_v2.h) against the FLOAT64 oracle in the input
regimes of tests/scan_regimes.py, where the carries dominate: every output, the saved ``x`` and all seven gradients of every
case, with limits tied to the fp32 oracle's own error (scan_regimes.compare; what that limit catches is shown on the CPU in
test_scan_regimes_host.py).  One forward and one backward per case, small shapes: batch 2, dstate 16, 2 groups, 24 rows."""
import contextlib

import pytest
import torch

import scan_regimes as sr
import vmambair_amd
from vmambair_amd import _capi

pytestmark = [pytest.mark.gpu, pytest.mark.tier(0)]
DEV = "cuda:0"
BATCH, N, G = 2, 16, 2
TYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


@contextlib.contextmanager
def _launch(fv=-1, bv=-1, segs=-1, split=0):
    """the test-only knobs of the library, restored whatever happens"""
    lib = _capi.load()
    lib.oss_scan_set_variant(fv, bv)
    lib.oss_scan_set_segments(segs, segs)
    lib.oss_scan_set_carry_split(split)
    try:
        yield lib
    finally:
        lib.oss_scan_set_variant(-1, -1)
        lib.oss_scan_set_segments(-1, -1)
        lib.oss_scan_set_carry_split(0)


def _dev(ts):
    return [None if t is None else t.to(DEV) for t in ts]


def _plain_case(regime, itype, L, dim=24, fv=-1, bv=-1, segs=-1, split=0, lane_states=False, seed=0, label=""):
    """one forward and one backward of the plain form -> the library handle, for the caller's launch-shape assertions"""
    cpu = sr.make_regime(regime, BATCH, dim, N, G, L, itype, seed)
    sp = sr.SOFTPLUS[regime]
    ref64, ref32 = sr.references(cpu, sp, chunk=vmambair_amd.scan_chunk(), lane_states=lane_states)
    u, delta, A, B, C, D, bias, dout = _dev(cpu)
    shape = {}
    with _launch(fv, bv, segs, split) as lib:
        fwd = vmambair_amd.selective_scan_fwd(u, delta, A, B, C, D, bias, sp, 1, want_hs=lane_states)
        shape["fwd_segments"] = lib.oss_scan_last_segments(0)
        grads = vmambair_amd.selective_scan_bwd(u, delta, A, B, C, D, bias, dout, fwd[1], sp, 1, hs=fwd[2] if lane_states else None)
        shape["bwd_segments"], shape["lane_states"] = lib.oss_scan_last_segments(1), lib.oss_scan_last_lane_states()
        torch.cuda.synchronize()
    assert fwd[0].dtype == itype and fwd[1].dtype == torch.float32
    got = dict(zip(sr.GRADS, grads), out=fwd[0], x=fwd[1])
    if lane_states:
        got["hs"] = _lane_states(fwd[2], BATCH, dim, L)
    sr.compare(got, ref64, ref32, itype, label=label or f"{regime} L={L} dim={dim} f{fv} b{bv} segs={segs} split={split}")
    return shape


def _lane_states(hs, batch, dim, L):
    """entries 1 .. blocks - 1 of every (batch, row, state): the states after the 8-step blocks 0 .. blocks - 2; entry 0 is 0"""
    L8 = (L + 7) // 8
    hs = hs.view(batch, dim, N, hs.numel() // (batch * dim * N))
    assert float(hs[..., 0].abs().max()) == 0.0, "the state entering step 0 is 0"
    return hs[..., 1:L8]


def _omni_case(regime, itype, L, rows=12, a_log_form=False, fv=-1, bv=-1, segs=-1, split=0, lane_states=False, label=""):
    """the omni form as the blocks issue it: 4 groups = directions, groups 2 and 3 scan the mirrored sequence (they carry from the
    END of it), directions k and k + 2 share their u and dout rows.  The reference is the oracle on the materialised directions."""
    K = 4
    u4, delta, A, B, C, D, bias, dout4 = sr.make_regime(regime, BATCH, K * rows, N, K, L, itype, seed=11)
    x2, dout2 = u4[:, :2 * rows].contiguous(), dout4[:, :2 * rows].contiguous()
    sp = sr.SOFTPLUS[regime]
    A_arg = A
    if a_log_form:
        assert regime in ("arch", "stiff")
        A_arg = torch.log(-A)                                 # fp32 log(1..N)
        A = -torch.exp(A_arg.double())                        # what the kernels are given, to the last bit
    cpu = (sr.mirror(x2.repeat(1, 2, 1), rows), sr.mirror(delta, rows), A, sr.mirror(B, 1), sr.mirror(C, 1), D, bias,
           sr.mirror(dout2.repeat(1, 2, 1), rows))
    ref64, ref32 = sr.references(cpu, sp, chunk=vmambair_amd.scan_chunk(), lane_states=lane_states)
    if a_log_form:                                            # A = -exp(A_log)  =>  d/dA_log = dA * A
        ref64["dA"], ref32["dA"] = ref64["dA"] * A, ref32["dA"] * A
    dv = _dev((x2, delta, A_arg, B, C, D, bias))
    kw = dict(rev_group_start=2, u_row_mod=2 * rows, a_log_form=a_log_form)
    shape = {}
    with _launch(fv, bv, segs, split) as lib:
        fwd = vmambair_amd.selective_scan_fwd(*dv, sp, 1, want_hs=lane_states, **kw)
        shape["fwd_segments"] = lib.oss_scan_last_segments(0)
        grads = vmambair_amd.selective_scan_bwd(*dv, dout2.to(DEV), fwd[1], sp, 1, dout_row_mod=2 * rows,
                                                hs=fwd[2] if lane_states else None, **kw)
        shape["bwd_segments"], shape["lane_states"] = lib.oss_scan_last_segments(1), lib.oss_scan_last_lane_states()
        torch.cuda.synchronize()
    got = dict(zip(sr.GRADS, grads), out=fwd[0], x=fwd[1])     # x and the lane states are indexed by SCAN position
    for q, per in (("out", rows), ("du", rows), ("ddelta", rows), ("dB", 1), ("dC", 1)):
        got[q] = sr.mirror(got[q], per)
    if lane_states:
        got["hs"] = _lane_states(fwd[2], BATCH, K * rows, L)
    sr.compare(got, ref64, ref32, itype, label=label or f"omni {regime} L={L} a_log={int(a_log_form)} f{fv} b{bv} segs={segs}")
    return shape


# ---- a. every regime, every I/O type, heuristic launch --------------------------------------------------------------------
@pytest.mark.parametrize("L", [1541, 4099])
@pytest.mark.parametrize("itype", list(TYPES), ids=list(TYPES))
@pytest.mark.parametrize("regime", sr.REGIMES)
def test_every_regime_and_type_vs_float64(regime, itype, L):
    _plain_case(regime, TYPES[itype], L)


# ---- b. every kernel variant where carries matter -------------------------------------------------------------------------
@pytest.mark.parametrize("fv,bv,dim", [(0, 10, 24), (1, 11, 24), (2, 12, 24), (3, 13, 24), (4, 1, 24), (6, 13, 24),
                                       (0, 13, 26), (6, 10, 26)])          # dim 26: a ragged row tile
@pytest.mark.parametrize("regime", ["slow", "none"])
def test_every_kernel_variant_vs_float64(regime, fv, bv, dim):
    _plain_case(regime, torch.float32, 2085, dim=dim, fv=fv, bv=bv)


# ---- c. time segments and the carry split (forward 0 / backward 13: 512-step chunks both ways) ----------------------------
@pytest.mark.parametrize("segs,split", [(2, 1), (2, 3), (3, 2), (64, 4)])
@pytest.mark.parametrize("itype", ["f32", "bf16"])
@pytest.mark.parametrize("regime", ["arch", "slow", "none"])
def test_time_segments_and_carry_split_vs_float64(regime, itype, segs, split):
    L = 6 * 512 + 5
    shape = _plain_case(regime, TYPES[itype], L, fv=0, bv=13, segs=segs, split=split)
    want = min(segs, (L + 511) // 512)
    assert shape["fwd_segments"] == want and shape["bwd_segments"] == want, "the segmented kernels did not run"


def test_short_segment_with_an_empty_last_piece_vs_float64():
    """13 chunks in 2 segments of 7 and 6, 4 pieces of 2 chunks each: the short segment leaves its last piece empty"""
    shape = _plain_case("slow", torch.float32, 13 * 512, fv=0, bv=13, segs=2, split=4)
    assert shape["fwd_segments"] == 2 and shape["bwd_segments"] == 2


# ---- d. omni form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("itype", ["f32", "bf16"])
@pytest.mark.parametrize("regime", ["arch", "slow"])
def test_omni_form_vs_float64(regime, itype):
    _omni_case(regime, TYPES[itype], 2085)


def test_omni_a_log_form_vs_float64():
    """A handed over as A_log = log(1..N): dA_log against dA * A of the float64 reference"""
    _omni_case("arch", torch.float32, 2085, a_log_form=True)


# ---- e. lane states -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["slow", "none"])
def test_lane_states_vs_float64(regime):
    """the saved state entering every 8-step block against the float64 oracle's chunk = 8 states, per state slot, and the
    backward that loads them instead of recomputing"""
    assert _capi.has_feature(_capi.FEATURE_LANE_STATES)
    shape = _plain_case(regime, torch.float32, 2085, lane_states=True)
    assert shape["lane_states"] == 1, "the lane-state kernels did not run"


@pytest.mark.parametrize("regime", ["slow", "none"])
def test_lane_states_segmented_omni_vs_float64(regime):
    assert _capi.has_feature(_capi.FEATURE_LANE_STATES)
    shape = _omni_case(regime, torch.float32, 2085, fv=3, bv=11, segs=3, split=4, lane_states=True)
    assert shape["lane_states"] == 1, "the lane-state kernels did not run"
    assert shape["fwd_segments"] == 3 and shape["bwd_segments"] == 3


# ---- f. fused delta -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("itype", ["f32", "bf16"])
def test_fused_delta_vs_float64(itype):
    """``dt_weight`` form in the archs' regime: delta = W . z inside the kernels.  Reference: the float64 oracle on the float64
    projection, the gradients of z and W by the projection's adjoint in float64; E32 from the same chain in fp32."""
    assert _capi.has_feature(_capi.FEATURE_FUSED_DT)
    itype = TYPES[itype]
    K, rows, R, L = 4, 12, 6, 1539
    dim = K * rows
    g = torch.Generator().manual_seed(17)
    _, _, A, _, _, D, bias, _ = sr.make_regime("arch", BATCH, dim, N, K, 8, itype, seed=3)    # A, D and the arch bias
    x2 = torch.randn(BATCH, 2 * rows, L, generator=g).to(itype)
    xdbl = torch.randn(BATCH, K, R + 2 * N, L, generator=g)
    xdbl[:, :, :R] *= 0.3
    xdbl = xdbl.to(itype)
    W = 0.5 * torch.randn(dim, R, generator=g) / R ** 0.5
    dout2 = torch.randn(BATCH, 2 * rows, L, generator=g).to(itype)
    A_log = torch.log(-A)
    A64 = -torch.exp(A_log.double())

    z4 = sr.mirror(xdbl[:, :, :R], 1)
    B4, C4 = sr.mirror(xdbl[:, :, R:R + N], 1), sr.mirror(xdbl[:, :, R + N:], 1)
    u4, g4 = sr.mirror(x2.repeat(1, 2, 1), rows), sr.mirror(dout2.repeat(1, 2, 1), rows)
    refs = []
    for real in (torch.float64, torch.float32):
        zr, Wr = z4.to(real), W.to(real).view(K, rows, R)
        delta4 = torch.einsum("kdr,bkrl->bkdl", Wr, zr).reshape(BATCH, dim, L)
        ref = sr._oracle((u4, delta4, A64, B4, C4, D, bias, g4), True, vmambair_amd.scan_chunk(),
                         "f64" if real == torch.float64 else "f32", False)
        dd4 = ref.pop("ddelta").to(real).view(BATCH, K, rows, L)
        ref["dz"] = torch.einsum("kdr,bkdl->bkrl", Wr, dd4).double()
        ref["dW"] = torch.einsum("bkdl,bkrl->kdr", dd4, zr).reshape(dim, R).double()
        ref["dA"] = ref["dA"] * A64
        refs.append(ref)
        if real == torch.float64:
            # The one quantity-specific limit of this file.  At 16-bit I/O the fused backward keeps softplus'(delta) of a chunk as
            # packed pairs IN THE I/O TYPE from the chunk's first pass to its per-element outputs (oss_scan_bwd_v2.h: `sigp`, packed
            # at "sigp[i] = pack2<T>(...)", unpacked before "dv[i] = ddel * sg[i]"): every ddelta[d, t] that enters the three sums
            # below carries ONE round-to-nearest to the I/O type, a relative error of at most sr.UNIT (2^-8 for bfloat16, at the
            # bottom of a binade).  Measured through an identity projection (dz = ddelta / 2): largest relative error of ddelta
            # 0.0073 < 2 x 2^-8, this rounding plus the one of the store.  ddelta itself is never stored in this form; out, x, du,
            # dA, dB, dC and dD do not see the factor and keep the common limit.  The allowance is the worst case of that rounding,
            # one unit times the sum of the ABSOLUTE terms of the float64 reference:
            #   dz[r, t] = sum_d W[d, r] ddelta[d, t]    dW[d, r] = sum_t ddelta[d, t] z[r, t]    dbias[d] = sum_t ddelta[d, t]
            # At fp32 I/O the factor stays fp32, the allowance is 0 and the same three sums meet the common limit.
            unit = sr.UNIT[itype]
            extra = {"dz": unit * torch.einsum("kdr,bkdl->bkrl", Wr.abs(), dd4.abs()),
                     "dW": unit * torch.einsum("bkdl,bkrl->kdr", dd4.abs(), zr.abs()).reshape(dim, R),
                     "ddelta_bias": unit * dd4.abs().sum(dim=(0, 3)).reshape(dim)}

    dv = _dev((x2, xdbl, A_log, D, bias, W))
    Bm, Cm = dv[1][:, :, R:R + N], dv[1][:, :, R + N:]
    kw = dict(rev_group_start=2, u_row_mod=2 * rows, a_log_form=True, dt_weight=dv[5])
    out, x = vmambair_amd.selective_scan_fwd(dv[0], dv[1], dv[2], Bm, Cm, dv[3], dv[4], True, 1, **kw)
    into = torch.full_like(dv[1], float("nan"))
    gf = vmambair_amd.selective_scan_bwd(dv[0], dv[1], dv[2], Bm, Cm, dv[3], dv[4], dout2.to(DEV), x, True, 1,
                                         dout_row_mod=2 * rows, dbc_into=into, **kw)
    torch.cuda.synchronize()
    assert len(gf) == 8 and gf[1] is None
    got = {"out": sr.mirror(out, rows), "x": x, "du": sr.mirror(gf[0], rows), "dA": gf[2], "dB": sr.mirror(into[:, :, R:R + N], 1),
           "dC": sr.mirror(into[:, :, R + N:], 1), "dD": gf[5], "ddelta_bias": gf[6], "dz": sr.mirror(into[:, :, :R], 1), "dW": gf[7]}
    sr.compare(got, refs[0], refs[1], itype, label="fused delta arch L=1539", extra=extra)
