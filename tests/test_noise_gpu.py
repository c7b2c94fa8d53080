"""The noise kernels of csrc/oss_noise.hip on the MI355X against the library's host twins (the same per-element text on the CPU,
checked for its distribution and its formulas in tests/test_noise_host.py) and against float64 on the same Philox words.

Tolerances.
  normals    measured on the CPU: the host fp32 twin's maximum error against the float64 evaluation of the same transform on the same
             words, E (2^16 draws).  The device may differ from float64 by at most 4 E: device and host ``log`` / ``cos`` / ``sin``
             differ by a few units in the last place.  Both figures are printed; profiles/noise_error.txt holds them as measured:
                 normals on 65536 draws: host fp32 twin vs float64 max err 1.590e-06 (= E); device vs float64 1.566e-06, bound 4 E
  Gaussian   out against the float64 formula on float64 normals: 4 E sigma_b / 255 + 4 * 2^-24 max(1, |noise|) (the fp32 round-off of
             the final expression, as in the host suite)
  Poisson    vals exactly the twin's; counts equal to the twin's except where a comparison inside the sampler lies within fp32
             round-off (``exp`` / ``log`` / ``lgamma`` of the two sides differ in the last places): at most 1 element in 1000, and a
             differing element is still a non-negative integer count; the host suite holds the fp32 twin to the same allowance
             against the float64 sampler.  Image outputs: the twin's within 4 * 2^-24 max(1, |noise|) off those elements.
  epilogues  bit-equal to torch's expressions on the device-produced unclipped output.
  distribution on the device: the chi^2, Kolmogorov-Smirnov and moment checks of the host suite, on (1, 3, 148, 148) draws.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import noise_cases as nc
from conftest import load_golden
from vmambair_amd import degradations as D
from vmambair_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = load_golden("g17_noise.npz")
F = nc.N
U = 2.0 ** -24


def stream(seed, calls=0):
    s = D.NoiseStream(seed, DEV)
    if calls:
        s.load_state_dict({"seed": seed, "calls": calls})
    return s


def image(shape, seed=0, lo=-0.1, hi=1.1):
    return (np.random.default_rng(seed).random(shape) * (hi - lo) + lo).astype(np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_E = {}


def host_normal_error():
    """E of the docstring: the host fp32 twin against float64 on the same 2^16 words"""
    if not _E:
        n32 = nc.twin_normals(123, 0, (1, 1, 256, 256)).reshape(-1)
        _E["n64"] = nc.normal_field64(123, 0, 1 << 16)
        _E["E"] = float(np.abs(n32 - _E["n64"]).max())
    return _E["E"]


def test_device_normals_against_float64_on_the_same_words():
    E = host_normal_error()
    x = torch.zeros(1, 1, 256, 256, device=DEV)
    out, _ = ops.noise_gaussian(x, stream(123).state(x.device), None, None, 0.0, 0.0, 0.0, F["RAW"], False)
    err = float(np.abs(out.cpu().numpy().reshape(-1) - _E["n64"]).max())
    print(f"normals on 65536 draws: host fp32 twin vs float64 max err {E:.3e} (= E); device vs float64 {err:.3e}, bound 4 E")
    assert 0 < E < 1e-5 and err <= 4 * E
    grey, _ = ops.noise_gaussian(x, stream(123).state(x.device), None, None, 0.0, 0.0, 1.0, F["RAW"], False)
    assert float(np.abs(grey.cpu().numpy().reshape(-1) - nc.normal_field64(123, 0, 1 << 16, nc.TAG_GREY)).max()) <= 4 * E


# ---- Gaussian ---------------------------------------------------------------------------------------------------------------------
def _gaussian_want(x, seed, call, s, g, only):
    b, c, h, w = x.shape
    n_c = nc.normal_field64(seed, call, x.size).reshape(x.shape)
    n_g = nc.normal_field64(seed, call, h * w, nc.TAG_GREY).reshape(1, 1, h, w)
    s4, g4 = np.asarray(s, np.float64).reshape(b, 1, 1, 1), np.asarray(g, np.float64).reshape(b, 1, 1, 1)
    noise = (n_c * s4 / 255.0) * (1 - g4) + (n_g * s4 / 255.0) * g4
    return (noise if only else x.astype(np.float64) + noise), noise, s4


@pytest.mark.parametrize("shape", nc.GPU_SHAPES + nc.GAUSSIAN_ONLY_SHAPES)
def test_gaussian_device_matches_twin_and_float64(shape):
    """all four forms with sigma and gray given (vectors, numbers) and drawn; return_params equals the twin's"""
    E = host_normal_error()
    b = shape[0]
    x = image(shape, seed=b)
    xd = dev(x)
    seed, call = 2024, 7
    sigma = np.linspace(2, 30, b).astype(np.float32)
    gray = np.array([1.0, 0.0, 0.5][:b], np.float32)

    def check(out, s, g, only):
        want, noise, s4 = _gaussian_want(x, seed, call, s, g, only)
        err = np.abs(out.cpu().numpy().astype(np.float64) - want)
        tol = 4 * E * s4 / 255.0 + 4 * U * np.maximum(1.0, np.abs(noise))
        assert (err <= tol).all(), float((err / tol).max())

    kw = dict(clip=False, rounds=False)
    check(D.add_gaussian_noise_pt(xd, dev(sigma), dev(gray), stream=stream(seed, call), **kw), sigma, gray, False)
    check(D.generate_gaussian_noise_pt(xd, dev(sigma), dev(gray), stream=stream(seed, call)), sigma, gray, True)
    check(D.add_gaussian_noise_pt(xd, 12.5, 0.25, stream=stream(seed, call), **kw), np.full(b, 12.5), np.full(b, 0.25), False)
    check(D.generate_gaussian_noise_pt(xd, 12.5, 0, stream=stream(seed, call)), np.full(b, 12.5), np.zeros(b), True)
    s, g = nc.params32(seed, call, b, 1, 30, 0.4)
    out, ps, pg = D.random_add_gaussian_noise_pt(xd, (1, 30), 0.4, stream=stream(seed, call), return_params=True, **kw)
    assert np.array_equal(ps.cpu().numpy(), s) and np.array_equal(pg.cpu().numpy(), g)
    assert np.array_equal(nc.twin_gaussian(x, seed, call, lo=1, hi=30, gray_scalar=0.4, flags=F["DRAW_PARAMS"])[1], np.stack([s, g]))
    check(out, s, g, False)
    out, ps, pg = D.random_generate_gaussian_noise_pt(xd, (1, 30), 0.4, stream=stream(seed, call), return_params=True)
    assert np.array_equal(ps.cpu().numpy(), s) and np.array_equal(pg.cpu().numpy(), g)
    check(out, s, g, True)
    check(D.random_add_gaussian_noise_pt(xd, (1, 30), 0.4, stream=stream(seed, call), **kw), s, g, False)
    # against the twin directly: the two fp32 evaluations differ by the normals' last places only
    twin = nc.twin_gaussian(x, seed, call, sigma=sigma, gray=gray)[0]
    got = D.add_gaussian_noise_pt(xd, dev(sigma), dev(gray), stream=stream(seed, call), **kw).cpu().numpy()
    assert float(np.abs(got - twin).max()) <= 5 * E * 30 / 255 + 2 * U * 2


# ---- Poisson ----------------------------------------------------------------------------------------------------------------------
def _level_images():
    """the fixture's images (1, 2, 3, 128, 129, 256 levels, a different count per sample, levels in one channel only) and two
    constant ones whose extra levels occur in one corner pixel only"""
    x = G["p.x"].numpy().copy()
    corner = np.full((2, 3, 12, 12), 100 / 255, np.float32)
    corner[0, :, 0, 0] = (7 / 255, 8 / 255, 9 / 255)             # 4 levels, three of them in one pixel
    corner[1, 2, 11, 11] = 1.0                                   # 2 levels, one of them in the last pixel
    return np.concatenate([x, corner])


def test_poisson_vals_are_exactly_the_twins():
    x = _level_images()
    _, params = ops.noise_poisson(dev(x), stream(5).state(torch.device(DEV, torch.cuda.current_device())), None, None, 1.0, 1.0, 0.0, 0, True)
    twin = nc.twin_poisson(x, 5, 0, lo=1.0)[1]
    assert np.array_equal(params.cpu().numpy(), twin)
    assert twin[2].tolist() == [1, 2, 4, 128, 256, 256, 128, 4, 2]
    assert np.array_equal(twin[2, :7], G["p.vals_c"].numpy()) and np.array_equal(twin[3, :7], G["p.vals_g"].numpy())


def _differing(got, want, x):
    tol = 4 * U * np.maximum(1.0, np.maximum(np.abs(want), np.abs(want - x)))      # |noise| is one of the two
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) > tol


@pytest.mark.parametrize("shape", nc.GPU_SHAPES)
def test_poisson_device_matches_the_twin(shape):
    """raw counts and all four forms, scale and gray given and drawn: equal to the twin's up to 1 element in 1000, and a differing
    element is still a non-negative integer count"""
    b = shape[0]
    x = image(shape, seed=10 + b, lo=-0.05, hi=1.05)
    if b > 1:
        x[1] = np.round(x[1] * 5) / 5                               # few levels: another vals, small lambda
    xd = dev(x)
    seed, call = 99, 3
    allowed = x.size // 1000
    lam = (nc.levels32(x) / np.float32(255)) * nc.vals_of(nc.levels32(x)).reshape(b, 1, 1, 1)
    for grey in (0.0, 1.0):
        k_dev, _ = ops.noise_poisson(dev(lam), stream(seed, call).state(xd.device), None, None, 0.0, 0.0, grey, F["RAW"], False)
        k_dev, k_twin = k_dev.cpu().numpy(), nc.twin_counts(lam, seed, call, grey=bool(grey))
        assert (k_dev >= 0).all() and (k_dev == np.rint(k_dev)).all() and int((k_dev != k_twin).sum()) <= allowed
    scale = np.linspace(0.05, 3, b).astype(np.float32)
    gray = np.array([0.0, 1.0, 0.5][:b], np.float32)
    s, g = nc.params32(seed, call, b, 0.05, 3, 0.4)
    kw = dict(clip=False, rounds=False)
    cases = [
        (D.add_poisson_noise_pt(xd, dev(scale), gray_noise=dev(gray), stream=stream(seed, call), **kw),
         nc.twin_poisson(x, seed, call, scale=scale, gray=gray)[0]),
        (D.generate_poisson_noise_pt(xd, dev(scale), dev(gray), stream=stream(seed, call)),
         nc.twin_poisson(x, seed, call, scale=scale, gray=gray, flags=F["ONLY"])[0]),
        (D.add_poisson_noise_pt(xd, 1.5, gray_noise=0, stream=stream(seed, call), **kw), nc.twin_poisson(x, seed, call, lo=1.5)[0]),
        (D.random_generate_poisson_noise_pt(xd, (0.05, 3), 0.4, stream=stream(seed, call)),
         nc.twin_poisson(x, seed, call, lo=0.05, hi=3, gray_scalar=0.4, flags=F["ONLY"] | F["DRAW_PARAMS"])[0]),
    ]
    out, ps, pg = D.random_add_poisson_noise_pt(xd, (0.05, 3), 0.4, stream=stream(seed, call), return_params=True, **kw)
    assert np.array_equal(ps.cpu().numpy(), s) and np.array_equal(pg.cpu().numpy(), g)
    cases.append((out, nc.twin_poisson(x, seed, call, lo=0.05, hi=3, gray_scalar=0.4, flags=F["DRAW_PARAMS"])[0]))
    for got, want in cases:
        got = got.cpu().numpy()
        assert got.shape == want.shape and np.isfinite(got).all()
        assert int(_differing(got, want, x).sum()) <= allowed
    # a differing element of the plain noise is still a count: (noise + q) * vals is a non-negative integer
    noise = D.generate_poisson_noise_pt(xd, 1.0, 0, stream=stream(seed, call)).cpu().numpy().astype(np.float64)
    vals = nc.vals_of(nc.levels32(x)).astype(np.float64).reshape(b, 1, 1, 1)
    counts = (noise + (nc.levels32(x) / np.float32(255)).astype(np.float64)) * vals
    assert float(np.abs(counts - np.rint(counts)).max()) <= 256 * 4 * U and counts.min() > -1e-4


# ---- the distribution on the device -----------------------------------------------------------------------------------------------
def test_device_normals_are_standard_normal():
    x = torch.zeros(1, 3, 148, 148, device=DEV)
    out, _ = ops.noise_gaussian(x, stream(31).state(x.device), None, None, 0.0, 0.0, 0.0, F["RAW"], False)
    assert nc.normal_failures(out.cpu().numpy()) == []


@pytest.mark.parametrize("lam", nc.poisson_lambdas())
def test_device_counts_follow_the_exact_pmf(lam):
    x = torch.full((1, 3, 148, 148), lam, device=DEV)
    out, _ = ops.noise_poisson(x, stream(32).state(x.device), None, None, 0.0, 0.0, 0.0, F["RAW"], False)
    k = out.cpu().numpy()
    assert k.size >= 1 << 16 and nc.poisson_failures(k, np.float32(lam)) == []
    assert lam > 0 or not k.any()


# ---- epilogues ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gaussian", "poisson"])
def test_epilogues_are_bit_equal_to_torch_on_the_device_output(kind):
    x = dev(image((3, 3, 33, 65), seed=3, lo=-0.2, hi=1.2))
    if kind == "gaussian":
        call = lambda **kw: D.random_add_gaussian_noise_pt(x, (1, 30), 0.4, stream=stream(8, 2), **kw)
    else:
        call = lambda **kw: D.random_add_poisson_noise_pt(x, (0.05, 3), 0.4, stream=stream(8, 2), **kw)
    raw = call(clip=False, rounds=False)
    assert float(raw.min()) < 0 and float(raw.max()) > 1
    assert torch.equal(call(), torch.clamp(raw, 0, 1)) and torch.equal(call(clip=True, rounds=False), torch.clamp(raw, 0, 1))
    assert torch.equal(call(clip=False, rounds=True), (raw * 255.0).round() / 255.)
    assert torch.equal(call(clip=True, rounds=True), torch.clamp((raw * 255.0).round(), 0, 255) / 255.)
    assert torch.equal(call(quantise=True), D.restate_quantise(torch.clamp(raw, 0, 1)))
    assert torch.equal(call(clip=False, rounds=False, quantise=True), D.restate_quantise(raw))


# ---- capture ------------------------------------------------------------------------------------------------------------------------
def test_captured_calls_draw_a_new_field_at_every_replay_and_nothing_is_read_back():
    x = dev(image((2, 3, 64, 64), seed=5, lo=0, hi=1))

    def both(s):
        return (D.random_add_poisson_noise_pt(x, (0.05, 3), 0.4, stream=s), D.random_add_gaussian_noise_pt(x, (1, 30), 0.4, stream=s))

    first = stream(77, 10)
    eager_stream, warm = first.clone(), first.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both(warm)                                   # warm-up outside the capture, on a stream of its own
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = both(first)
    replays = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        replays.append([o.clone() for o in outs])
    eager = [both(eager_stream) for _ in range(3)]
    for i in range(3):
        for j in range(2):
            assert torch.equal(replays[i][j], eager[i][j]), (i, j)
            assert not torch.equal(replays[i][j], replays[(i + 1) % 3][j]), (i, j)
    assert first.state_dict() == eager_stream.state_dict() == {"seed": 77, "calls": 16}
    sigma, gray = dev(np.array([3.0, 4.0], np.float32)), dev(np.array([0.0, 1.0], np.float32))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        both(eager_stream)
        D.add_gaussian_noise_pt(x, sigma, 1.0, stream=eager_stream)
        D.generate_poisson_noise_pt(x, 1.0, gray, stream=eager_stream)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert eager_stream.state_dict()["calls"] == 20


def test_default_stream_is_seeded_from_torch_and_advances():
    x = dev(image((1, 3, 8, 8), seed=6, lo=0, hi=1))
    a, b = D.random_add_gaussian_noise_pt(x), D.random_add_gaussian_noise_pt(x)
    assert not torch.equal(a, b)
    s = D.default_noise_stream(x.device)
    assert s.state_dict()["seed"] == D.NoiseStream(torch.initial_seed()).seed and s.state_dict()["calls"] >= 2
    resumed = D.NoiseStream(0, DEV)
    resumed.load_state_dict(s.state_dict())
    assert torch.equal(D.random_add_poisson_noise_pt(x, stream=resumed), D.random_add_poisson_noise_pt(x, stream=s))


# ---- dispatch -----------------------------------------------------------------------------------------------------------------------
def test_other_inputs_take_the_restatement_and_the_ops_reject_them():
    x = image((2, 3, 12, 10), seed=7, lo=0, hi=1)
    xd = dev(x)
    view = xd.transpose(2, 3)
    assert not view.is_contiguous()
    four = dev(image((2, 4, 6, 6), seed=8, lo=0, hi=1))
    for inp in (torch.from_numpy(x), xd.double(), view, four):
        torch.manual_seed(21)
        got = D.random_add_gaussian_noise_pt(inp, (1, 30), 0.4) if inp is not four else D.random_add_poisson_noise_pt(inp, (0.05, 3), 0)
        torch.manual_seed(21)
        want = D.restate_random_add_gaussian_noise_pt(inp, (1, 30), 0.4) if inp is not four else \
            D.restate_random_add_poisson_noise_pt(inp, (0.05, 3), 0)
        assert got.dtype == inp.dtype and got.device == inp.device and torch.equal(got, want)
    for inp in (xd.double(), view):
        torch.manual_seed(22)
        got = D.add_poisson_noise_pt(inp, 1.5, gray_noise=1.0)
        torch.manual_seed(22)
        assert torch.equal(got, D.restate_add_poisson_noise_pt(inp, 1.5, gray_noise=1.0))
    state = stream(1).state(xd.device)
    args = (state, None, None, 1.0, 1.0, 0.0, 0, False)
    assert ops.noise_ok(xd, 0) and ops.noise_ok(xd, 1) and ops.noise_ok(four, 0) and not ops.noise_ok(four, 1)
    assert not ops.noise_ok(xd.double(), 0) and not ops.noise_ok(torch.from_numpy(x), 1)
    for op in (torch.ops.vmambair.noise_gaussian, torch.ops.vmambair.noise_poisson):
        with pytest.raises(RuntimeError, match="fp32 tensors"):
            op(xd.double(), *args)
        with pytest.raises(RuntimeError, match="img must be contiguous"):
            op(view, *args)
        with pytest.raises(RuntimeError, match="unknown flags"):
            op(xd, state, None, None, 1.0, 1.0, 0.0, 64, False)
        with pytest.raises(RuntimeError, match=r"fp32 \(B,\) tensor"):
            op(xd, state, dev(np.ones(3, np.float32)), None, 1.0, 1.0, 0.0, 0, False)
        with pytest.raises(RuntimeError, match="state must be"):
            op(xd, state.int(), None, None, 1.0, 1.0, 0.0, 0, False)
    with pytest.raises(RuntimeError, match="is not supported"):
        torch.ops.vmambair.noise_poisson(four, *args)


# ---- the chain ----------------------------------------------------------------------------------------------------------------------
def test_first_degradation_stage_runs_under_one_capture():
    """filter2D -> F.interpolate(bilinear, 0.5) -> random_add_gaussian_noise_pt -> DiffJPEG(clamp_input=True)"""
    x = dev(image((2, 3, 32, 32), seed=9, lo=0, hi=1))
    g = D.gaussian_kernel1d(21, 2.0)
    kernel = torch.outer(g, g).float().expand(2, 21, 21).contiguous().to(DEV)
    quality = torch.tensor([45.0, 80.0], device=DEV)
    jpeg = D.DiffJPEG(differentiable=False)
    s = stream(55)

    def stage(st):
        out = D.filter2D(x, kernel)
        out = Fn.interpolate(out, scale_factor=0.5, mode="bilinear")
        out = D.random_add_gaussian_noise_pt(out, sigma_range=(1, 30), clip=True, rounds=False, gray_prob=0.4, stream=st)
        return jpeg(out, quality, clamp_input=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        stage(s.clone())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = stage(s)
    graph.replay()
    torch.cuda.synchronize()
    a = out.clone()
    graph.replay()
    torch.cuda.synchronize()
    assert out.shape == (2, 3, 16, 16) and float(out.min()) >= 0 and float(out.max()) <= 1 and bool(torch.isfinite(out).all())
    assert not torch.equal(a, out) and s.state_dict()["calls"] == 2
    with torch.no_grad():
        assert torch.equal(stage(stream(55, 1)), out)
