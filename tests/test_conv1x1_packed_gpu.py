"""Pre-packed 16-bit weight images of the MFMA 1x1 convolutions (csrc/oss_conv1x1.hip: oss_conv1x1_pack_kernel and the image
form of the weight loader of oss_conv1x1_pair_kernel / oss_conv1x1_pairk_kernel; csrc/oss_conv1x1_wg.hip: the same for
oss_conv1x1_wg_kernel, plain and LayerNorm-fused.  oss_conv1x1_dgrad_lnbwd_kernel has no image form: it measured no gain).

* the pack launch writes exactly the image of include/vmambair_oss.h (built here with torch ops from that formula);
* ``oss_conv1x1_fwd_packed`` / ``oss_conv1x1_dgrad_packed`` (and ``oss_ln_conv1x1_fwd_packed``) are
  BIT-IDENTICAL to the fp32-weight entry points: the same fragments, the same k-steps added in the same order;
* one absolute anchor per direction against a float64 product of the rounded operands, with the tolerance the fp32-weight path
  has in tests/test_glue_gpu.py (test_conv1x1_mfma).

The ``per`` = 2 / 3 forms of oss_conv1x1_pairk_kernel (several row tiles per workgroup) are chosen only when a launch has >= 4096
waves (batch x pixels / 64 x row-tile groups), i.e. >= 128 K pixels at these widths: not reachable at a test-sized shape.  They
share the image addressing with the ``per`` = 1 form that runs here (tile index clamped into the image, MFMAs of a tile outside
the matrix skipped), and the headline step does not launch them either (its largest launch has 512 x 2 waves).
"""
import pytest
import torch

from conftest import assert_close
from vmambair_amd import _capi, ops
from vmambair_amd.ops import pointwise as pw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTS = [torch.bfloat16, torch.float16]


def ref_image(W: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    """img[((t * KSTEPS + s) * 64 + l) * 8 + e] = W(32 t + (l & 31), 16 s + 8 (l >> 5) + e) rounded to dt, 0 outside (M x K)"""
    M, K = W.shape
    MT, KS = (M + 31) // 32, (K + 15) // 16
    pad = torch.zeros(MT * 32, KS * 16, dtype=torch.float32, device=W.device)
    pad[:M, :K] = W
    v = pad.to(dt).view(MT, 32, KS, 2, 8)                   # [t, l & 31, s, l >> 5, e]
    return v.permute(0, 2, 3, 1, 4).contiguous().view(torch.int16).flatten()


def bits(img: torch.Tensor) -> torch.Tensor:
    return img.view(torch.int16)


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
def test_pack_launch_writes_the_documented_image(dt):
    """all six shapes as ONE table (the descriptor walk: 2 images x 6 weights, 1 - 33 rows each), then two of them as a table of
    their own; padding must be exact zeros, so the buffers are poisoned first"""
    torch.manual_seed(0)
    shapes = [(96, 255), (48, 127), (33, 193), (254, 48), (96, 48), (5, 17)]
    ws = [torch.randn(co, ci, 1, 1, device=DEV) * ci ** -0.5 for co, ci in shapes]
    ws[0].view(-1)[:4] = torch.tensor([0.0, -0.0, 1e-30, -3.0e38], device=DEV)   # signed zero, a value that flushes, a huge one
    lib = _capi.load()
    for group in (ws, ws[1:3]):
        pk = pw.PackedConv1x1Weights(group, dt)
        pk.buffer.fill_(0x5a)
        pk.refresh()
        torch.cuda.synchronize()
        assert len(pk.images) == len(group)
        for w in group:
            co, ci, idt, fimg, dimg = pk.images[w.data_ptr()]
            assert (co, ci, idt) == (w.shape[0], w.shape[1], dt)
            assert fimg.numel() == lib.oss_conv1x1_fwd_image_bytes(co, ci) and dimg.numel() == lib.oss_conv1x1_dgrad_image_bytes(co, ci)
            w2 = w.view(co, ci)
            assert torch.equal(bits(fimg), ref_image(w2, dt)), (co, ci, "forward image")
            assert torch.equal(bits(dimg), ref_image(w2.t(), dt)), (co, ci, "input-gradient image")


def _both(fn, pk):
    """fn() with the fp32 weights, then with the images; the second call must really have found one"""
    pw.clear_packed_images()
    a = fn()
    pw.set_packed_images(pk.images)
    assert pw.packed_images_active() == len(pk.images) > 0
    try:
        b = fn()
    finally:
        pw.clear_packed_images()
    torch.cuda.synchronize()
    return a, b


@pytest.fixture(params=[0, 1], ids=["wave_level_only", "default_dispatch"])
def wg(request):
    """0: the workgroup-level kernel off, so that EVERY shape reaches the pixel-pair kernels (K % 16 == 0 with pixels % 128 == 0
    and no residual goes to oss_conv1x1_wg_kernel otherwise: its own test is further down); 1: the dispatch as shipped"""
    lib = _capi.load()
    lib.oss_conv1x1_set_wg(request.param, 0)
    yield request.param
    lib.oss_conv1x1_set_wg(1, 0)


# (K, M): pair KS 3 | KS 6 | KS 8 with odd K (pairw without an image) | KS 12 with a ragged last row tile | pairk: K > 192, odd x ragged
FWD_SHAPES = [(48, 96), (96, 48), (127, 96), (177, 33), (255, 96), (510, 96), (193, 33)]
PLANES = [(8, 8), (16, 16), (32, 32)]   # 64 = the UNet's level-4 plane, 256 = one workgroup's pixels, 1024 = several workgroups


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("K,M", FWD_SHAPES)
def test_packed_forward_is_bit_identical_to_the_fp32_weight_path(dt, K, M, wg):
    torch.manual_seed(1)
    w = torch.randn(M, K, 1, 1, device=DEV) * K ** -0.5
    b = torch.randn(M, device=DEV)
    pk = pw.PackedConv1x1Weights([w], dt)
    pk.refresh()
    for H, W in PLANES:
        x = torch.randn(2, K, H, W, device=DEV).to(dt)
        res = torch.randn(2, M, H, W, device=DEV).to(dt)
        for bias in (b, None):
            for r in (None, res):
                want, got = _both(lambda: ops.conv1x1_fwd(x, w, bias, r), pk)
                assert torch.equal(got, want), (K, M, H * W, bias is not None, r is not None)


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("Cout,Cin", [(254, 48), (510, 96), (127, 48), (96, 127), (48, 96), (177, 33)])
def test_packed_input_gradient_is_bit_identical_to_the_fp32_weight_path(dt, Cout, Cin, wg):
    """the transposed direction (K = Cout): project_in's input gradient at dim 48 / 96 (pairk), an odd K on the whole-K kernel
    (KS 8), and three more shapes for the KS 6 / 3 / 12 image forms of the pair kernel (the last with a ragged row tile)"""
    torch.manual_seed(2)
    w = torch.randn(Cout, Cin, 1, 1, device=DEV) * Cin ** -0.5
    pk = pw.PackedConv1x1Weights([w], dt)
    pk.refresh()
    for H, W in PLANES:
        x = torch.randn(2, Cin, H, W, device=DEV).to(dt)
        dy = torch.randn(2, Cout, H, W, device=DEV).to(dt)
        want, got = _both(lambda: ops.conv1x1_bwd(x, w, dy, False)[0], pk)
        assert torch.equal(got, want), (Cout, Cin, H * W)


# ---- the workgroup-level kernels of oss_conv1x1_wg.hip (K % 16 == 0, pixels % 128 == 0, no residual) ------------------------------
WG_SHAPES = [(48, 96), (96, 254)]        # (K, M): KS 3 and 6, whole and ragged row tiles
WG_PLANES = [(8, 16), (16, 16)]          # 128 and 256 pixels: one and two 128-pixel tiles (two and four of 64)


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("K,M", WG_SHAPES)
def test_packed_workgroup_level_kernels_are_bit_identical_to_the_fp32_weight_path(dt, K, M):
    """oss_conv1x1_wg_kernel with an image: plain forward, LayerNorm-fused forward (all four outputs), input gradient (the
    transposed weight: a (K, M) convolution's dx)"""
    lib = _capi.load()
    torch.manual_seed(5)
    w = torch.randn(M, K, 1, 1, device=DEV) * K ** -0.5          # forward: K -> M
    wt = torch.randn(K, M, 1, 1, device=DEV) * M ** -0.5         # input gradient of a M -> K convolution: the product's depth is K
    b = torch.randn(M, device=DEV)
    lw, lb = torch.randn(K, device=DEV) * 0.5 + 1, torch.randn(K, device=DEV)
    pk = pw.PackedConv1x1Weights([w, wt], dt)
    pk.refresh()
    for H, W in WG_PLANES:
        assert lib.oss_ln_conv1x1_ok(_capi.OSS_BF16 if dt == torch.bfloat16 else _capi.OSS_F16, M, K, H * W) == 1
        x = torch.randn(2, K, H, W, device=DEV).to(dt)
        xm = torch.randn(2, M, H, W, device=DEV).to(dt)
        for bias in (b, None):
            want, got = _both(lambda: ops.conv1x1_fwd(x, w, bias), pk)
            assert torch.equal(got, want), (K, M, H * W, "forward")
            for lnb in (lb, None):
                want, got = _both(lambda: ops.ln_conv1x1_fwd(x * 2 + 0.5, lw, lnb, w, bias), pk)
                for name, g, r in zip(("y", "n", "mean", "rstd"), got, want):
                    assert torch.equal(g, r), (K, M, H * W, "LayerNorm-fused forward", name)
        want, got = _both(lambda: ops.conv1x1_bwd(xm, wt, x, False)[0], pk)
        assert torch.equal(got, want), (K, M, H * W, "input gradient")


def test_images_follow_the_weights_only_through_a_pack_launch():
    """the image is a snapshot: a weight written in place (as the fused optimizer does, through a raw pointer) is seen by the packed
    entry point after the next pack launch and not before"""
    torch.manual_seed(3)
    dt = torch.bfloat16
    w = torch.randn(96, 127, 1, 1, device=DEV) * 127 ** -0.5
    x = torch.randn(2, 127, 8, 8, device=DEV).to(dt)
    pk = pw.PackedConv1x1Weights([w], dt)
    pk.refresh()
    pw.set_packed_images(pk.images)
    try:
        y0 = ops.conv1x1_fwd(x, w, None)
        w.mul_(2.0)
        stale = ops.conv1x1_fwd(x, w, None)
        pk.refresh()
        y1 = ops.conv1x1_fwd(x, w, None)
    finally:
        pw.clear_packed_images()
    assert torch.equal(stale, y0)
    assert torch.equal(y1.float(), 2.0 * y0.float())      # a power of two: exact in every rounding on the way
    assert torch.equal(y1, ops.conv1x1_fwd(x, w, None))   # registry cleared: the fp32 path on the doubled weights


@pytest.mark.parametrize("direction", ["forward", "input_gradient"])
def test_packed_path_against_float64_of_the_rounded_operands(direction):
    """absolute anchor: float64 product of the operands as the kernel sees them (weights rounded to bf16), tolerance of
    tests/test_glue_gpu.py::test_conv1x1_mfma for the fp32-weight path (y: 2e-2 / 3e-2, dx: 2e-2 / 6e-2)"""
    torch.manual_seed(4)
    dt = torch.bfloat16
    Cout, Cin = (96, 255) if direction == "forward" else (254, 48)
    w = torch.randn(Cout, Cin, 1, 1, device=DEV) * Cin ** -0.5
    b = torch.randn(Cout, device=DEV)
    x = torch.randn(2, Cin, 16, 16, device=DEV).to(dt)
    dy = torch.randn(2, Cout, 16, 16, device=DEV).to(dt)
    pk = pw.PackedConv1x1Weights([w], dt)
    pk.refresh()
    wr = w.view(Cout, Cin).to(dt).double()
    pw.set_packed_images(pk.images)
    try:
        assert pw._packed_image(w.view(Cout, Cin), dt, 0) != 0
        if direction == "forward":
            got = ops.conv1x1_fwd(x, w, b)
            want = torch.einsum("mk,bkhw->bmhw", wr, x.double()) + b.double().view(1, -1, 1, 1)
            rt, at = 2e-2, 3e-2
        else:
            got = ops.conv1x1_bwd(x, w, dy, False)[0]
            want = torch.einsum("mk,bmhw->bkhw", wr, dy.double())
            rt, at = 2e-2, 6e-2
    finally:
        pw.clear_packed_images()
    assert_close(got, want.float(), rt, at, direction)
