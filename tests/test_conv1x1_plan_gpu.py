"""Every instantiation the 1x1-convolution launchers can emit (tests/conv1x1_plan_cases.py), at the smallest call that reaches it:
``oss_conv1x1_describe`` names that instantiation for the very call, and the result equals the float64 product of the inputs."""
import pytest
import torch

from conftest import assert_close
from conv1x1_plan_cases import FAMILY_NAMES, FIELDS, SMALLEST, run_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("t", sorted(SMALLEST), ids=lambda t: FAMILY_NAMES[t[0]] + "-" + "-".join(map(str, t[1:])))
def test_each_instantiation_against_float64(t):
    case = SMALLEST[t]
    io, dgrad = case[0], case[1]
    r = run_case(case, seed=1)
    assert tuple(getattr(r["describe"], f) for f in FIELDS) == t
    dt = r["dtype"]
    # weights rounded as the loaders round them: to the I/O type (16-bit), not at all (fp32)
    w = (r["w"].to(dt) if dt != torch.float32 else r["w"]).double()
    x = r["x"].double().flatten(2)                                   # (B, K, P)
    want = torch.matmul(w.t() if dgrad else w, x)                    # (B, M, P)
    mag = torch.matmul((w.t() if dgrad else w).abs(), x.abs())
    if r["bias"] is not None:
        want = want + r["bias"].double()[None, :, None]
        mag = mag + r["bias"].double().abs()[None, :, None]
    if r["res"] is not None:
        want = want + r["res"].double().flatten(2)
        mag = mag + r["res"].double().flatten(2).abs()
    got = r["got"].flatten(2)
    assert got.dtype == dt and got.shape == want.shape
    if io == "bf16":
        assert_close(got, want, 2e-2, 3e-2, "bf16")
    elif io == "f16":
        assert_close(got, want, 3e-3, 3e-2, "f16")
    elif io == "f32":     # the limits of test_conv1x1_fp32_matrix_core_kernels
        assert_close(got, want, 2e-5, 2e-5 * float(want.abs().max()), "f32")
    else:
        # split bf16 (tests/test_f32_matmul_high_gpu.py): (3 * 2^-16 + (K + 2) * 2^-23) * sum_k |w_k||x_k|, one fp32
        # rounding per epilogue addend and one for the comparison in fp32
        K = x.shape[1]
        bound = (3 * 2.0 ** -16 + (K + 2) * 2.0 ** -23) * mag + 2.0 ** -22 * (mag + want.abs())
        err = (got.double() - want).abs()
        assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
