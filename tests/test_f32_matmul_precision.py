"""The opt-in "high" precision mode of the fp32 GEMM-shaped products (split bf16: csrc/oss_conv1x1_f32x3.h,
include/vmambair_oss.h ``OSS_F32_BF16X3``) -- everything that needs no GPU: the Python switch, the environment variable, the
C-ABI value and query, and the documented error bound on a torch emulation of the arithmetic contract."""
import os
import subprocess
import sys

import pytest
import torch

import vmambair_amd
from vmambair_amd import _capi, _precision

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_is_highest_and_the_switch_round_trips():
    assert os.environ.get(_precision.ENV, "highest") == "highest", "the suite runs with the default mode"
    assert vmambair_amd.get_float32_matmul_precision() == "highest"
    try:
        vmambair_amd.set_float32_matmul_precision("high")
        assert vmambair_amd.get_float32_matmul_precision() == "high"
        assert _precision.io_code(torch.float32) == _capi.OSS_F32_BF16X3
        # 16-bit tensors never see the mode
        assert _precision.io_code(torch.bfloat16) == _capi.OSS_BF16 and _precision.io_code(torch.float16) == _capi.OSS_F16
        vmambair_amd.set_float32_matmul_precision("highest")
        assert vmambair_amd.get_float32_matmul_precision() == "highest"
        assert _precision.io_code(torch.float32) == _capi.OSS_F32
    finally:
        vmambair_amd.set_float32_matmul_precision("highest")


def test_context_manager_restores_the_previous_mode_on_exceptions_too():
    assert vmambair_amd.get_float32_matmul_precision() == "highest"
    with vmambair_amd.float32_matmul_precision("high"):
        assert vmambair_amd.get_float32_matmul_precision() == "high"
        with vmambair_amd.float32_matmul_precision("highest"):
            assert vmambair_amd.get_float32_matmul_precision() == "highest"
        assert vmambair_amd.get_float32_matmul_precision() == "high"
    assert vmambair_amd.get_float32_matmul_precision() == "highest"
    with pytest.raises(RuntimeError, match="inside"):
        with vmambair_amd.float32_matmul_precision("high"):
            raise RuntimeError("inside")
    assert vmambair_amd.get_float32_matmul_precision() == "highest"


@pytest.mark.parametrize("bad", ["medium", "HIGH", "", "tf32", None, 1])
def test_a_bad_value_raises_value_error_and_changes_nothing(bad):
    with pytest.raises(ValueError):
        vmambair_amd.set_float32_matmul_precision(bad)
    with pytest.raises(ValueError):
        with vmambair_amd.float32_matmul_precision(bad):
            pass
    assert vmambair_amd.get_float32_matmul_precision() == "highest"


def _child(env_value):
    env = {k: v for k, v in os.environ.items() if k != _precision.ENV}
    if env_value is not None:
        env[_precision.ENV] = env_value
    code = "import vmambair_amd; print(vmambair_amd.get_float32_matmul_precision())"
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("value,want", [(None, "highest"), ("highest", "highest"), ("high", "high")])
def test_environment_variable_sets_the_initial_mode_of_a_fresh_process(value, want):
    r = _child(value)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == want


def test_environment_variable_with_another_value_is_a_value_error():
    r = _child("medium")
    assert r.returncode != 0 and "ValueError" in r.stderr and _precision.ENV in r.stderr


def test_capi_exposes_the_selector_and_the_library_reports_the_mode():
    assert _capi.OSS_F32_BF16X3 == 3
    assert (_capi.OSS_F32, _capi.OSS_F16, _capi.OSS_BF16) == (0, 1, 2)
    modes = _capi.load().oss_f32_matmul_modes()
    assert modes & _capi.F32_MODE_EXACT, "the exact fp32 products are always there"
    assert modes & 2, "the library was built without the split-bf16 products"


# ---- the arithmetic contract and its bound ----------------------------------------------------------------------------------------
def split_bf16(a):
    """hi = bf16_rne(a), lo = bf16_rne(a - hi) (exact subtraction); where a - hi is not finite the value travels in lo alone
    (hi = 0, lo = bf16_rne(a)): csrc/oss_conv1x1_f32x3.h.  Both returned as fp32."""
    hi = a.to(torch.bfloat16).float()
    r = a - hi
    ok = torch.isfinite(r)
    return torch.where(ok, hi, torch.zeros_like(hi)), torch.where(ok, r, hi).to(torch.bfloat16).float()


def emulate_high(w, x, terms=(True, True, True)):
    """y[m, p] = sum_k w[m, k] x[k, p] as the "high" kernels form it: hi_w lo_x, lo_w hi_x, hi_w hi_x accumulated in fp32 (a
    k-ordered chain of single fp32 additions of exact products, which is the worst rounding any fp32 accumulation order has)"""
    wh, wl = split_bf16(w)
    xh, xl = split_bf16(x)
    acc = torch.zeros(w.shape[0], x.shape[1], dtype=torch.float32)
    for k in range(w.shape[1]):
        for on, a, b in zip(terms, (wh, wl, wh), (xl, xh, xh)):
            if on:   # a product of two bf16 numbers has 16 significant bits: exact in fp32 (and in the MFMA)
                acc = acc + a[:, k:k + 1] * b[k:k + 1, :]
    return acc


def bound(w, x):
    """(3 * 2^-16 + (K + 2) * 2^-23) * sum_k |w_k||x_k|   """
    K = w.shape[1]
    return (3 * 2.0 ** -16 + (K + 2) * 2.0 ** -23) * (w.double().abs() @ x.double().abs())


@pytest.mark.parametrize("K", [3, 38, 127, 510])
def test_emulated_split_obeys_the_documented_bound_and_a_missing_term_does_not(K):
    g = torch.Generator().manual_seed(1000 + K)
    worst = 0.0
    for scale, positive in ((1e-3, False), (1.0, False), (50.0, False), (1.0, True)):
        w = torch.randn(24, K, generator=g) * scale
        x = torch.randn(K, 40, generator=g) * scale
        if positive:
            w, x = w.abs(), x.abs()
        ref = w.double() @ x.double()
        b = bound(w, x)
        err = (emulate_high(w, x).double() - ref).abs()
        worst = max(worst, float((err / b).max()))
        assert bool((err <= b).all()), f"K {K} scale {scale}: {float((err / b).max()):.3f} of the bound"
        # the bound has teeth: without one cross term the error is far outside it
        for terms in ((False, True, True), (True, False, True)):
            e1 = (emulate_high(w, x, terms).double() - ref).abs()
            assert float((e1 / b).max()) > 3.0, f"K {K}: a missing cross term stayed inside the bound"
    print(f"[f32 matmul high] K {K}: worst error {worst:.3f} of the bound")


def test_emulated_split_keeps_infinities_and_is_exact_on_bf16_operands():
    a = torch.tensor([float("inf"), float("-inf"), float("nan"), 3.4e38, 1.0, -0.3])   # (3.4e38 rounds to infinity in bf16)
    hi, lo = split_bf16(a)
    assert torch.equal(hi[:4], torch.zeros(4)), "a value whose remainder is not finite travels in lo alone"
    assert lo[0] == float("inf") and lo[1] == float("-inf") and torch.isnan(lo[2]) and lo[3] == float("inf")
    assert torch.equal(hi[4:] + lo[4:], a[4:].to(torch.bfloat16).float() + (a[4:] - a[4:].to(torch.bfloat16).float()).to(torch.bfloat16).float())
    g = torch.Generator().manual_seed(7)
    # an infinity and a NaN among the activations: infinities of the exact product's sign and NaNs, in the exact product's places
    # (with the infinity in hi_x the cross term lo_w * hi_x would turn half of them into NaN)
    w = torch.randn(16, 35, generator=g)
    x = torch.randn(35, 12, generator=g)
    x[3, 5], x[20, 7] = float("inf"), float("nan")
    exact, high = w @ x, emulate_high(w, x)
    assert torch.equal(torch.isnan(high), torch.isnan(exact)) and bool(torch.isnan(exact[:, 7]).all())
    assert torch.equal(high[:, 5], exact[:, 5]) and bool(torch.isinf(exact[:, 5]).all())
    w = torch.randint(-4, 5, (16, 35), generator=g).float()
    x = torch.randint(-4, 5, (35, 12), generator=g).float()
    assert torch.equal(emulate_high(w, x), (w.double() @ x.double()).float())
