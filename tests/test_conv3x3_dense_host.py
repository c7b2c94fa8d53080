"""Host side of the dense 3x3 MFMA kernels (oss_conv3x3_dense.hip): exported symbols, the pure host queries, the opt-in switch, and
the nets' unchanged behaviour with the switch off.  No GPU."""
import ctypes
import os

import pytest
import torch

from vmambair_amd import _build, _capi
from vmambair_amd.ops import conv3x3 as c3

BF16, F16, F32 = _capi.OSS_BF16, _capi.OSS_F16, _capi.OSS_F32
# (B, Cin, H, W) -> Cout: the shapes of tests/test_conv3x3_dense_gpu.py
SHAPES = [((2, 16, 5, 7), 24), ((1, 48, 9, 33), 40), ((2, 96, 8, 16), 192), ((1, 192, 3, 5), 96), ((3, 32, 1, 1), 8), ((1, 384, 4, 6), 33),
          ((1, 16, 17, 70), 100), ((2, 64, 2, 40), 64), ((3, 128, 41, 8), 192)]


def test_the_five_symbols_are_exported():
    lib = ctypes.CDLL(_build.LIB_PATH)
    for name in ("oss_conv3x3_dense_ok", "oss_conv3x3_dense_fwd", "oss_conv3x3_dense_dgrad", "oss_conv3x3_dense_wgrad_partial_floats",
                 "oss_conv3x3_dense_wgrad"):
        assert hasattr(lib, name) and name in _capi.SYMBOLS, name


def test_shape_rules_are_pure_host_queries():
    lib = _capi.load()
    for (B, Cin, H, W), Cout in SHAPES:
        for io in (BF16, F16):
            assert lib.oss_conv3x3_dense_ok(io, Cin, Cout, H, W) == 1
        n = lib.oss_conv3x3_dense_wgrad_partial_floats(B, Cin, Cout, H, W)
        vec = 9 * Cin * Cout
        # whole partial vectors, one per (image, row band): at least one band, never more bands than rows
        assert n % vec == 0 and B <= n // vec <= B * H
    # the headline's tail layer: 12 (co, ci) tiles x 8 images -> ceil(512 / 96) = 6 bands of 22 rows
    assert lib.oss_conv3x3_dense_wgrad_partial_floats(8, 96, 384, 128, 128) == 8 * 6 * 9 * 96 * 384
    assert lib.oss_conv3x3_dense_ok(BF16, 96, 384, 128, 128) == 1 and lib.oss_conv3x3_dense_ok(F16, 48, 24, 19, 19) == 1
    for cin in (24, 8, 15, 0, -16):
        assert lib.oss_conv3x3_dense_ok(BF16, cin, 24, 8, 8) == 0
    for cout in (4, 3, 1, 0, -5):
        assert lib.oss_conv3x3_dense_ok(BF16, 32, cout, 8, 8) == 0
    assert lib.oss_conv3x3_dense_ok(F32, 32, 24, 8, 8) == 0 and lib.oss_conv3x3_dense_ok(_capi.OSS_F32_BF16X3, 32, 24, 8, 8) == 0
    for h, w in ((0, 8), (8, 0), (-1, 8), (8, -3), (1 << 20, 8)):
        assert lib.oss_conv3x3_dense_ok(BF16, 32, 24, h, w) == 0
    for args in ((0, 32, 24, 8, 8), (-2, 32, 24, 8, 8), (70000, 32, 24, 8, 8), (2, 24, 24, 8, 8), (2, 32, 4, 8, 8), (2, 32, 24, 0, 8), (2, 32, 24, 8, 0)):
        assert lib.oss_conv3x3_dense_wgrad_partial_floats(*args) == 0
    # a refused call is an error code, not a launch: NULL pointers and refused shapes never reach the device
    assert lib.oss_conv3x3_dense_fwd(BF16, None, None, None, None, 1, 32, 24, 8, 8, 0, 0, 0, 0, None) == -1   # OSS_ERR_NULL


def test_cpu_tensors_are_rejected_not_computed():
    x = torch.zeros(1, 16, 4, 4, dtype=torch.bfloat16)
    w = torch.zeros(8, 16, 3, 3)
    assert not c3.dense_ok(x, w)
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.vmambair.conv3x3_dense_fwd(x, w, None)
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.vmambair.conv3x3_dense_bwd(x, w, torch.zeros(1, 8, 4, 4, dtype=torch.bfloat16), False, True)


def test_switch_is_off_by_default_and_round_trips():
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k != "VMAMBAIR_CONV3X3_DENSE"}
    code = "from vmambair_amd.ops import conv3x3 as c; print(c.DENSE_IMPL)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert subprocess.check_output([sys.executable, "-c", code], env=env, cwd=root).split()[-1] == b"False"
    assert subprocess.check_output([sys.executable, "-c", code], env=dict(env, VMAMBAIR_CONV3X3_DENSE="1"), cwd=root).split()[-1] == b"True"
    start = c3.DENSE_IMPL
    try:
        assert c3.set_dense(True) is start and c3.DENSE_IMPL is True
        assert c3.set_dense(False) is True and c3.DENSE_IMPL is False
        assert c3.set_dense(1) is False and c3.DENSE_IMPL is True
    finally:
        c3.set_dense(start)
    assert c3.DENSE_IMPL is start


def test_switch_off_leaves_the_nets_on_their_own_modules():
    """Downsample / Upsample / the x4 tail return exactly what their Sequential returned before, and keep their parameter names"""
    from vmambair_amd.archs import Downsample, MambaSISR6, Upsample, _x4_tail
    prev = c3.set_dense(False)
    assert prev is False or os.environ.get("VMAMBAIR_CONV3X3_DENSE") == "1"
    torch.manual_seed(0)
    x = torch.randn(1, 16, 6, 8)
    for m in (Downsample(16), Upsample(16)):
        assert [k for k, _ in m.named_parameters()] == ["body.0.weight"]
        assert torch.equal(m(x), m.body(x))
    ref_tail = _x4_tail(32, 3)
    net = MambaSISR6(dim=16, num_blocks=(1, 1, 1, 1), num_refinement_blocks=1)
    keys = list(net.state_dict().keys())
    for k in ("tail.0.0.weight", "tail.0.0.bias", "tail.0.2.weight", "tail.0.2.bias", "tail.1.weight", "tail.1.bias"):
        assert k in keys
    assert [k for k, _ in net.tail.named_parameters()] == [k for k, _ in ref_tail.named_parameters()]
    # the tail as the forward now walks it == the Sequential called as a whole
    t = torch.randn(1, 32, 4, 4)
    up, last = net.tail
    walked = last(up[3](c3.conv3x3(up[1](c3.conv3x3(t, up[0])), up[2])))
    assert torch.equal(walked, net.tail(t))
    # even with the switch on a CPU tensor ends in the module's own forward
    prev = c3.set_dense(True)
    try:
        m = Downsample(16)
        assert torch.equal(m(x), m.body(x))
    finally:
        c3.set_dense(prev)
