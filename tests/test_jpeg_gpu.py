"""``oss_jpeg.hip`` on the device (``torch.ops.vmambair.jpeg_roundtrip`` and its public face ``vmambair_amd.degradations.DiffJPEG``)
against the independent float64 evaluation of tests/golden/g16_jpeg.npz (numpy + scipy.fft, tests/golden/make_golden_jpeg.py).

Rounding makes the operator discontinuous, so the comparison is in stages (u = 2^-24):
  (a) coefficients   the device's quantised coefficient equals round(v) of the float64 v = F / (T factor) wherever v is at least
                     TAU = 0.01 away from a half-integer; inside that band it may differ by at most 1.  TAU is derived: an fp32
                     evaluation of F is a sum of at most 64 terms with sum|terms| <= 1/4 * 64 * 128 = 2048, plus the colour
                     conversion and the factor: its error is <= ~72 u * 2048 = 8.8e-3, and it is divided by T factor >= 1 for
                     quality <= 95.
  (b) band share     the band holds at most 3 % of the coefficients of every case: asserted on the fixture alone in
                     tests/test_jpeg_host.py::test_band_share_of_the_fixture (no device needed), repeated here per case
  (c) pixels         every pixel: |out - D| <= (64 + 16) u A / 255, where D is the float64 decompression (this file's numpy / scipy
                     code) of the DEVICE's own coefficients, and A is the per-pixel sum of the absolute values of all terms:
                       A_Y  = sum_uv |C[u][x]| |C[v][y]| |c T factor|[u][v] + 128      (likewise A_Cb, A_Cr, + 128 for the - 128)
                       A_R = A_Y + 1.402 A_Cr;  A_G = A_Y + 0.344136 A_Cb + 0.714136 A_Cr;  A_B = A_Y + 1.772 A_Cb
                     Derivation: every term of the final sum passes through at most 64 roundings on its way -- fp32(T factor)
                     against the float64 factor (3), c (T factor) (1), the rounded DCT constants (2), 8 + 8 accumulations of the
                     two passes (16), + 128, - 128, the colour constants and three accumulations (8), the clamp and the
                     multiplication by fp32(1 / 255) against the true quotient (3): 33, rounded up to 64 -- each of relative size u on a
                     partial sum bounded by A; the 16 covers second-order terms and the float64 side.  A is computed from the
                     data, as ``dot_bound`` in tests/test_degrade_host.py.
  (d) stages, (e) locality and padding, (f) scalar and tensor quality, (g) no host read (graph replay), (h) fallbacks: bit for bit.
Measured on an MI355X: profiles/jpeg_error.txt; every test prints its own figures.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from scipy import fft

from test_jpeg_host import CASES, TAU, band, case, golden, unrounded
from vmambair_amd import degradations as D
from vmambair_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24

# the float64 decompression of given coefficients: this file's own numpy / scipy code
T_Y = np.array([[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56],
                [14, 17, 22, 29, 51, 87, 80, 62], [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92],
                [49, 64, 78, 87, 103, 121, 120, 101], [72, 92, 95, 98, 112, 100, 103, 99]], np.float64).T
T_C = np.full((8, 8), 99.0)
T_C[:4, :4] = [[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]]
INV = np.array([[1.0, 0.0, 1.402], [1.0, -0.344136, -0.714136], [1.0, 1.772, 0.0]], np.float32).astype(np.float64)
ABS_C = np.abs(fft.idct(np.eye(8), type=2, axis=0, norm='ortho'))   # |C[u][x]| as [x][u]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(bits(a), bits(b))


def merge(blocks, hh, ww):
    b = blocks.shape[0]
    return blocks.reshape(b, hh // 8, ww // 8, 8, 8).transpose(0, 1, 3, 2, 4).reshape(b, hh, ww)


def decompress_f64(coef, q, h, w):
    """-> (D, A): the float64 output for these quantised coefficients, and the per-pixel sum of absolute terms"""
    hh, ww = h + -h % 16, w + -w % 16
    qq = np.asarray(q, np.float64)
    f = (np.where(qq < 50, 5000.0 / qq, 200.0 - 2.0 * qq) / 100.0)[:, None, None, None]
    planes, bounds = [], []
    for c, table, (ph, pw) in zip(coef, (T_Y, T_C, T_C), ((hh, ww), (hh // 2, ww // 2), (hh // 2, ww // 2))):
        g = np.asarray(c, np.float64) * (table * f)
        planes.append(merge(fft.idctn(g, type=2, axes=(-2, -1), norm='ortho') + 128.0, ph, pw))
        bounds.append(merge(np.einsum('xu,bnuv,yv->bnxy', ABS_C, np.abs(g), ABS_C) + 128.0, ph, pw))
    up = lambda p: np.repeat(np.repeat(p, 2, axis=1), 2, axis=2)   # noqa: E731
    ycc = np.stack([planes[0], up(planes[1]) - 128.0, up(planes[2]) - 128.0], axis=1)
    a = np.stack([bounds[0], up(bounds[1]) + 128.0, up(bounds[2]) + 128.0], axis=1)
    out = np.clip(np.einsum('ck,bkhw->bchw', INV, ycc), 0.0, 255.0) / 255.0
    return out[:, :, :h, :w], np.einsum('ck,bkhw->bchw', np.abs(INV), a)[:, :, :h, :w]


def run(x, quality, differentiable=False, **kw):
    q = quality.to(DEV) if torch.is_tensor(quality) else quality
    with torch.no_grad():
        return D.DiffJPEG(differentiable=differentiable)(x.to(DEV), q, **kw)


# ---- (a), (b), (c): against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.tier(0)
@pytest.mark.parametrize("name", CASES)
def test_coefficients_and_pixels_match_float64(name):
    x, quality, q = case(name)
    b, _, h, w = x.shape
    out, coef = run(x, quality, return_coefficients=True)
    assert out.shape == x.shape and out.dtype == torch.float32 and out.is_cuda
    coef = [c.cpu().double() for c in coef]
    want = unrounded(name)
    n_band = n_all = n_diff = 0
    worst_outside, farthest_flip = 0.0, 0.0
    for c, v in zip(coef, want):
        assert c.shape == v.shape and torch.equal(c, torch.round(c))          # integers
        inside, diff = band(v), (c - torch.round(v)).abs()
        n_band, n_all, n_diff = n_band + int(inside.sum()), n_all + v.numel(), n_diff + int((diff != 0).sum())
        worst_outside = max(worst_outside, float(diff[~inside].max()) if (~inside).any() else 0.0)
        if (diff != 0).any():
            farthest_flip = max(farthest_flip, float((((v - torch.floor(v)) - 0.5).abs())[diff != 0].max()))
        assert float(diff.max()) <= 1                                          # inside the band: at most 1
    print(f"[jpeg] {name} {tuple(x.shape)}: {n_all} coefficients, {n_band} ({100 * n_band / n_all:.2f} %) within {TAU} of a "
          f"half-integer; device != round(float64) at {n_diff}, largest difference outside the band {worst_outside:.0f}"
          + (f", farthest flipped value {farthest_flip:.2e} from its half-integer" if n_diff else ""))
    assert n_band <= 0.03 * n_all                                              # (b)
    assert worst_outside == 0                                                  # (a)
    # (c): the device's pixels against the float64 decompression of the device's own coefficients
    ref, a = decompress_f64([c.numpy() for c in coef], q.numpy(), h, w)
    err = np.abs(out.cpu().double().numpy() - ref)
    ratio = float((err / ((64 + 16) * U * a / 255.0)).max())
    print(f"[jpeg] {name}: pixels vs float64 decompression of the device's coefficients: max err {err.max():.3e}, "
          f"{ratio:.4f} of the bound (mean bound {float(((64 + 16) * U * a / 255.0).mean()):.2e})")
    assert ratio <= 1.0
    if n_diff == 0:   # then the fixture's output is that decompression
        assert float(np.abs(ref - golden()[f"{name}.out"].numpy()).max()) <= 1e-12


# ---- (d) stages ---------------------------------------------------------------------------------------------------------------
def test_clamp_and_quantise_stages_are_bit_equal_to_torch():
    x, quality, _ = case("edges")
    wide = x * 1.5 - 0.2
    assert float(wide.min()) < 0 and float(wide.max()) > 1
    assert same_bits(run(wide, quality, clamp_input=True), run(torch.clamp(wide, 0, 1), quality))
    assert not same_bits(run(wide, quality, clamp_input=True), run(wide, quality))
    plain = run(x, quality)
    quantised = run(x, quality, quantise=True)
    assert same_bits(quantised, torch.clamp((plain * 255.0).round(), 0, 255) / 255.)
    assert not same_bits(quantised, plain)
    both = run(wide, quality, clamp_input=True, quantise=True)
    assert same_bits(both, torch.clamp((run(torch.clamp(wide, 0, 1), quality) * 255.0).round(), 0, 255) / 255.)


# ---- (e) locality ---------------------------------------------------------------------------------------------------------------
def test_one_pixel_changes_only_its_macroblock_and_padding_never_leaks():
    x, quality, _ = case("odd")
    base = run(x, quality)
    for (c, y, xx) in ((0, 0, 0), (1, 37, 70), (2, 79, 143), (1, 16, 15), (0, 47, 128)):
        moved = x.clone()
        moved[0, c, y, xx] = 1.0 - moved[0, c, y, xx]
        got = run(moved, quality)
        changed = bits(got) != bits(base)
        y0, x0 = y // 16 * 16, xx // 16 * 16
        assert bool(changed[:, :, y0:y0 + 16, x0:x0 + 16].any()), (c, y, xx)
        changed[:, :, y0:y0 + 16, x0:x0 + 16] = False
        assert not bool(changed.any()), (c, y, xx)
    # per sample as well: another sample's pixels and quality are not read
    x, quality, _ = case("edges")
    base = run(x, quality)
    moved, q2 = x.clone(), quality.clone()
    moved[1] = 1.0 - moved[1]
    q2[1] = 40.0
    got = run(moved, q2)
    assert same_bits(got[0], base[0]) and same_bits(got[2], base[2]) and not same_bits(got[1], base[1])
    # padding inside the load == padding by hand
    padded = F.pad(x, (0, 48 - 33, 0, 32 - 17))
    assert tuple(padded.shape) == (3, 3, 32, 48)
    assert same_bits(base, run(padded, quality)[:, :, :17, :33].contiguous())
    # ... down to the coefficients of the padded planes
    _, coef = run(x, quality, return_coefficients=True)
    _, coef2 = run(padded, quality, return_coefficients=True)
    assert all(same_bits(a, b) for a, b in zip(coef, coef2))


# ---- (f) scalar and tensor quality ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", (30, 49.5, 50, 72.3, 95))
def test_scalar_and_tensor_quality_are_bit_identical(quality):
    x, _, _ = case("edges")
    tensor = torch.full((3,), float(quality), dtype=torch.float32, device=DEV)
    before = tensor.clone()
    a, ca = run(x, quality, return_coefficients=True)
    b, cb = run(x, tensor, return_coefficients=True)
    assert same_bits(a, b) and all(same_bits(p, q) for p, q in zip(ca, cb))
    assert same_bits(tensor, before)                                           # the caller's tensor is unchanged
    blocks = 2 * 3
    assert [tuple(c.shape) for c in ca] == [(3, 4 * blocks, 8, 8), (3, blocks, 8, 8), (3, blocks, 8, 8)]


def test_coefficient_layout_is_the_packages():
    """block n of ``y`` is rows 8 (n // (W / 8)) ..., columns 8 (n % (W / 8)) ... of the padded plane, [u][v] = [vertical][horizontal]:
    a plane that varies along one axis only has coefficients in the first column (or row) of every block"""
    h, w = 32, 48
    ramp = torch.linspace(0.1, 0.9, h).view(1, 1, h, 1).expand(1, 3, h, w).contiguous()
    _, (y, cb, cr) = run(ramp, 90, return_coefficients=True)
    assert tuple(y.shape) == (1, 24, 8, 8) and tuple(cb.shape) == tuple(cr.shape) == (1, 6, 8, 8)
    assert float(y[..., 1:].abs().max()) == 0 and float(y[..., 1:, 0].abs().max()) > 0    # vertical frequencies only
    _, (yt, _, _) = run(ramp.transpose(2, 3).contiguous(), 90, return_coefficients=True)
    assert float(yt[..., 1:, :].abs().max()) == 0 and float(yt[..., 0, 1:].abs().max()) > 0
    # the DC terms are the block means in row-major block order: brighter downwards, equal along a row of blocks
    dc = y[0, :, 0, 0].view(h // 8, w // 8).cpu()
    assert bool((dc[1:] > dc[:-1]).all()) and bool((dc == dc[:, :1]).all())
    # a grey image has no chroma
    assert float(cb.abs().max()) == 0 and float(cr.abs().max()) == 0


# ---- (g) no host read -------------------------------------------------------------------------------------------------------------
def test_graph_replay_follows_the_quality_tensor():
    x, quality, _ = case("edges")
    xd, static_q = x.to(DEV), quality.to(DEV).clone()
    jpeg = D.DiffJPEG(differentiable=False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        jpeg(xd, static_q)   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = jpeg(xd, static_q)
    results = []
    for new in ((30.0, 95.0, 49.5), (80.0, 20.0, 55.5), (49.9, 50.0, 61.0)):
        fresh = torch.tensor(new, dtype=torch.float32, device=DEV)
        static_q.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out, run(x, fresh)), new
        results.append(out.clone())
    assert not same_bits(results[0], results[1]) and not same_bits(results[1], results[2])


# ---- (h) fallbacks ----------------------------------------------------------------------------------------------------------------
def test_other_inputs_fall_back_to_the_restatement():
    x, quality, _ = case("rect")
    xd, qd = x.to(DEV), quality.to(DEV)
    jpeg = D.DiffJPEG(differentiable=False)
    with torch.no_grad():
        half = jpeg(xd.half(), qd)
        assert half.dtype == torch.float16 and torch.equal(half, D.restate_diffjpeg(xd.half(), qd, False))
        view = xd.flip(-1).transpose(2, 3)                                     # (2, 3, 40, 48), not contiguous
        assert not view.is_contiguous()
        assert same_bits(jpeg(view, qd), D.restate_diffjpeg(view, qd, False).contiguous())
    # differentiable=True with gradients enabled: the restatement, with a graph
    leaf = xd.clone().requires_grad_(True)
    soft = D.DiffJPEG()(leaf, qd)
    assert soft.requires_grad and same_bits(soft, D.restate_diffjpeg(leaf, qd, True))
    soft.sum().backward()
    assert bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad.abs().max()) > 0
    assert torch.equal(qd.cpu(), quality)


def test_differentiable_rounding_without_a_graph_is_the_kernels():
    """``DiffJPEG()`` (differentiable=True, the package's default) under ``no_grad`` stays on the device: c = r + (v - r)^3 with
    r = round(v).  Outside the band of (a) r is float64's, and d^3 has slope <= 3/4 for |d| <= 1/2, so
    |c - (r + (v - r)^3)| <= 3/4 * 8.8e-3 (the error budget of v behind TAU) + 2^-14 (one fp32 rounding of c below 1024) = 6.7e-3."""
    x, quality, _ = case("edges")
    out, coef = run(x, quality, differentiable=True, return_coefficients=True)
    assert not out.requires_grad and out.is_cuda
    worst = 0.0
    for c, v in zip(coef, unrounded("edges")):
        r = torch.round(v)
        err = (c.cpu().double() - (r + (v - r) ** 3)).abs()[~band(v)]
        worst = max(worst, float(err.max()))
    print(f"[jpeg] differentiable rounding on the device vs float64 outside the band: max err {worst:.3e} (limit 6.7e-3)")
    assert worst <= 6.7e-3
    hard = run(x, quality)
    assert not same_bits(out, hard)
