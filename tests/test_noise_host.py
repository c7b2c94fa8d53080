"""Host side of the noise steps of the RealSR degradation (vmambair_amd/degradations.py on csrc/oss_noise.hip): the plain-torch
restatement of basicsr's ``*_noise_pt`` functions against the float64 fixture G17, and the library's host twins -- the text the
kernels are compiled from, run on the CPU -- for their distribution, their independence and every formula.  No GPU needed.

The fixture (tests/golden/make_golden_noise.py) evaluates the published definitions independently in numpy float64 on random fields
that torch's CPU generator draws in the package's order; no reference and no package code stands behind it (the pip ``basicsr``
package is neither in the reference tree nor installed), as for tests/test_jpeg_host.py.

Bounds.  Restatement vs fixture: 1e-12 (the same float64 operations; a handful of terms of magnitude <= 2).  Distribution: the
statistic of every check must lie below the 1 - 1e-6 quantile of its distribution, moments within 5 standard errors; NumPy's own
generators pass the same checks for three seeds, asserted here, so the bounds are not tight.  Twin image formula: with the twin's
OWN fp32 normals and counts the output equals the float64 formula within the fp32 round-off of the final expression,
4 * 2^-24 * max(1, |noise|); rounding to a level is discontinuous, so elements whose float64 value lies within 1e-4 * max(1, |noise|)
levels of a half-integer are left out there, at most 1 % of a case.
"""
import math

import numpy as np
import pytest
import torch

import noise_cases as nc
from conftest import load_golden
from vmambair_amd import _capi
from vmambair_amd import degradations as D

G = load_golden("g17_noise.npz")
F = _capi.NOISE
NDRAWS = 1 << 16
GAUSS_CASES = ("num", "grey1", "vec", "vec0", "c1", "c4", "rand")
COMBOS = (("c", True, False), ("r", False, True), ("cr", True, True))


def _close(got, want, tol=1e-12):
    got = got.numpy() if torch.is_tensor(got) else np.asarray(got)
    want = want.numpy() if torch.is_tensor(want) else np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64
    err = float(np.abs(got - want).max())
    assert err <= tol, err


# ---- the restatement against the fixture ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GAUSS_CASES)
def test_gaussian_restatement_matches_the_fixture(name):
    """all four forms, numbers and tensors, C = 1 and C = 4, the three clip / rounds combinations; float64 CPU tensors take the
    restatement through the public functions"""
    x, seed = G[f"{name}.x"], int(G[f"{name}.seed"])
    assert x.dtype == torch.float64
    if name == "rand":
        lo, hi, prob = (float(v) for v in G["rand.range"])
        torch.manual_seed(seed)
        noise, sigma, gray = D.random_generate_gaussian_noise_pt(x, (lo, hi), prob, return_params=True)
        _close(noise, G["rand.noise"]), _close(sigma, G["rand.sigma"]), _close(gray.double(), G["rand.gray"])
        torch.manual_seed(seed)
        _close(D.random_generate_gaussian_noise_pt(x, (lo, hi), prob), G["rand.noise"])
        for tag, clip, rounds in COMBOS:
            torch.manual_seed(seed)
            _close(D.random_add_gaussian_noise_pt(x, (lo, hi), prob, clip, rounds), G[f"rand.out_{tag}"])
        torch.manual_seed(seed)
        _close(D.random_add_gaussian_noise_pt(x, (lo, hi), prob), G["rand.out_c"])     # the defaults: clip, no rounds
        return
    sigma, gray = G[f"{name}.sigma"], G[f"{name}.gray"]
    if int(G[f"{name}.numbers"]):
        sigma, gray = float(sigma[0]), float(gray[0])
    torch.manual_seed(seed)
    _close(D.generate_gaussian_noise_pt(x, sigma, gray), G[f"{name}.noise"])
    for tag, clip, rounds in COMBOS:
        torch.manual_seed(seed)
        _close(D.add_gaussian_noise_pt(x, sigma, gray, clip, rounds), G[f"{name}.out_{tag}"])
    torch.manual_seed(seed)
    _close(D.add_gaussian_noise_pt(x, sigma, gray), G[f"{name}.out_c"])
    torch.manual_seed(seed)
    _close(D.add_gaussian_noise_pt(x, sigma, gray, True, False, quantise=True), G[f"{name}.out_c"].mul(255).round().clamp(0, 255) / 255.)


def test_gaussian_grey_field_is_shared_by_the_batch():
    """samples 1 and 2 of ``vec`` are all grey: the same (h, w) field scaled by sigma_b, equal in the three channels"""
    x, sigma = G["vec.x"], G["vec.sigma"]
    torch.manual_seed(int(G["vec.seed"]))
    noise = D.generate_gaussian_noise_pt(x, sigma, G["vec.gray"])
    a, b = noise[1] * 255 / sigma[1], noise[2] * 255 / sigma[2]
    assert float((a - b).abs().max()) <= 1e-12 and float(a.abs().max()) > 0.5
    assert torch.equal(noise[1, 0], noise[1, 1]) and torch.equal(noise[1, 0], noise[1, 2])
    assert not torch.equal(noise[0, 0], noise[0, 1])                                   # the colour sample is not


def test_gaussian_number_sigma_with_grey_noise_needs_batch_one_as_in_the_package():
    with pytest.raises(RuntimeError):
        D.restate_generate_gaussian_noise_pt(torch.zeros(2, 3, 4, 4, dtype=torch.float64), 10, 1)


def test_poisson_restatement_structure():
    """vals as the fixture has them on images with exactly 1, 2, 3, 128, 129, 256 levels (a different count per sample) and with
    the levels confined to one channel; (noise / scale + q) * vals is a non-negative integer; all-grey noise is equal in the
    three channels; doubling the scale doubles the noise"""
    x = G["p.x"].double()
    q, g, vals_c, vals_g = G["p.q"], G["p.g"], G["p.vals_c"], G["p.vals_g"]
    assert D._poisson_vals(D.restate_quantise(x)) == vals_c.tolist() == [1, 2, 4, 128, 256, 256, 128]
    assert D._poisson_vals(D.restate_quantise(D._rgb_to_grayscale(x))) == vals_g.tolist()
    _close(D.restate_quantise(x), q), _close(D.restate_quantise(D._rgb_to_grayscale(x)), g)
    b = x.size(0)
    scale = torch.linspace(0.5, 3.0, b, dtype=torch.float64)
    torch.manual_seed(11)
    noise = D.generate_poisson_noise_pt(x, scale, 0)
    counts = (noise / scale.view(b, 1, 1, 1) + q) * vals_c.view(b, 1, 1, 1)
    assert float((counts - counts.round()).abs().max()) <= 1e-9 and float(counts.min()) > -1e-9
    assert float(noise[0].abs().max()) > 0            # one level, vals = 1: poisson(q) - q
    torch.manual_seed(11)
    _close(D.generate_poisson_noise_pt(x, 2 * scale, 0), 2 * noise)
    torch.manual_seed(12)
    grey = D.generate_poisson_noise_pt(x, 1.0, torch.ones(b, dtype=torch.float64))
    assert torch.equal(grey[:, 0], grey[:, 1]) and torch.equal(grey[:, 0], grey[:, 2])
    counts = (grey[:, :1] + g) * vals_g.view(b, 1, 1, 1)
    assert float((counts - counts.round()).abs().max()) <= 1e-9 and float(counts.min()) > -1e-9
    torch.manual_seed(13)
    out = D.random_add_poisson_noise_pt(x, (0.05, 3), 0.4)
    assert out.dtype == torch.float64 and float(out.min()) >= 0 and float(out.max()) <= 1
    torch.manual_seed(13)
    same, s, gr = D.random_add_poisson_noise_pt(x, (0.05, 3), 0.4, return_params=True)
    assert torch.equal(same, out) and s.shape == gr.shape == (b,) and float(s.min()) >= 0.05 and float(s.max()) < 3
    for c in (1, 4):                                  # the package's behaviour off three channels
        xc = torch.rand(2, c, 4, 4, dtype=torch.float64)
        assert D.generate_poisson_noise_pt(xc, 1.0, 0).shape == xc.shape
    assert D.generate_poisson_noise_pt(torch.rand(2, 1, 4, 4, dtype=torch.float64), 1.0, 1).shape == (2, 3, 4, 4)
    with pytest.raises(TypeError):
        D.generate_poisson_noise_pt(torch.rand(2, 4, 4, 4, dtype=torch.float64), 1.0, 1)


def test_poisson_positional_order_follows_the_package():
    """add_poisson_noise_pt(img, scale, clip, rounds, gray_noise): the package puts clip and rounds before gray_noise here"""
    x = G["p.x"].double()[:2]
    torch.manual_seed(3)
    a = D.add_poisson_noise_pt(x, 1.5, False, True, 0)
    torch.manual_seed(3)
    b = D.add_poisson_noise_pt(x, 1.5, clip=False, rounds=True, gray_noise=0)
    assert torch.equal(a, b) and float(((a * 255) - (a * 255).round()).abs().max()) < 1e-9


# ---- the host twins: distribution ---------------------------------------------------------------------------------------------
def test_normals_are_standard_normal_and_finite_for_every_word():
    x = nc.twin_normals(seed=20240, call=3, shape=(1, 1, 256, 256))
    assert x.size == NDRAWS and nc.normal_failures(x) == []
    grey = nc.twin_normals(seed=20240, call=3, shape=(1, 1, 256, 256), grey=True)
    assert nc.normal_failures(grey) == [] and abs(nc.pearson_r(x, grey)) <= 5 / math.sqrt(NDRAWS)
    for s in (0, 1, 2):                               # the bounds are not tight: NumPy's generator passes them
        assert nc.normal_failures(np.random.default_rng(s).standard_normal(NDRAWS)) == []
    assert nc.normal_failures(x * 1.02) != [] and nc.normal_failures(x + 0.03) != []   # and they do catch a wrong scale or shift
    extreme = [0, 0xFFFFFFFF, 1, 0xFFFFFFFE, 0x80000000]
    words = np.array([[a, b, c, d] for a in extreme for b in extreme for c in extreme[:2] for d in extreme[:2]], np.uint32)
    out = np.full(words.shape, np.nan, np.float32)
    assert _capi.load().oss_noise_normals_host(words.ctypes.data, out.ctypes.data, len(words)) == 0
    assert np.isfinite(out).all() and np.abs(out).max() < 6.8
    w64 = words.astype(np.uint64)
    want = np.stack([*nc.normals64(w64[:, 0], w64[:, 1]), *nc.normals64(w64[:, 2], w64[:, 3])], axis=-1)
    assert float(np.abs(out - want).max()) <= 1e-5    # also where u1 is next to 0 or next to 1


@pytest.mark.parametrize("lam", nc.poisson_lambdas())
def test_poisson_counts_follow_the_exact_pmf(lam):
    """inversion below the switch-over, PTRS from it on; lambda = 0 gives only zeros"""
    k = nc.twin_counts(np.full((1, 1, 256, 256), lam, np.float32), seed=77, call=5)
    assert k.size == NDRAWS and nc.poisson_failures(k, np.float32(lam)) == []
    if lam == 0:
        assert not k.any()
    grey = nc.twin_counts(np.full((1, 1, 256, 256), lam, np.float32), seed=77, call=5, grey=True)
    assert nc.poisson_failures(grey, np.float32(lam)) == [] and (lam == 0 or not np.array_equal(k, grey))
    for s in (0, 1, 2):
        assert nc.poisson_failures(np.random.default_rng(s).poisson(lam, NDRAWS), lam) == []
    if lam >= 1:                                      # the checks do catch a wrong rate
        assert nc.poisson_failures(k, lam * 1.03) != []


def test_draws_are_independent():
    """|Pearson r| <= 5 / sqrt(N) between horizontal neighbours, channels, samples and two consecutive calls of a stream"""
    shape = (2, 3, 128, 256)
    sigma = np.full(2, 255.0, np.float32)
    a = nc.twin_gaussian(None, 5, 10, sigma=sigma, flags=F["ONLY"], shape=shape)[0]
    b = nc.twin_gaussian(None, 5, 11, sigma=sigma, flags=F["ONLY"], shape=shape)[0]
    assert nc.normal_failures(a) == []
    for what, (u, v) in {"neighbours": (a[..., :-1], a[..., 1:]), "rows": (a[..., :-1, :], a[..., 1:, :]), "channels": (a[:, 0], a[:, 1]),
                         "samples": (a[0], a[1]), "calls": (a, b)}.items():
        assert abs(nc.pearson_r(u, v)) <= 5 / math.sqrt(u.size), what
    lam = np.full((2, 3, 64, 128), 40.0, np.float32)
    ka, kb = nc.twin_counts(lam, 5, 10), nc.twin_counts(lam, 5, 11)
    for what, (u, v) in {"neighbours": (ka[..., :-1], ka[..., 1:]), "channels": (ka[:, 0], ka[:, 2]), "samples": (ka[0], ka[1]),
                         "calls": (ka, kb)}.items():
        assert abs(nc.pearson_r(u, v)) <= 5 / math.sqrt(u.size), what


def test_twin_samplers_against_float64_on_the_same_words():
    """the twin consumes the draws the header numbers: fp32 normals within 1e-5 of the float64 transform of the same words (the
    figure itself is what tests/test_noise_gpu.py scales its tolerance from), counts equal to the float64 sampler's except where a
    comparison inside the sampler lies within fp32 round-off: at most 1 in 1000"""
    shape = (2, 3, 33, 65)
    count = int(np.prod(shape))
    big = nc.twin_normals(123, 0, (1, 1, 512, 512)).reshape(-1)
    err = float(np.abs(big - nc.normal_field64(123, 0, big.size)).max())
    print(f"normals, host fp32 twin vs float64 on the same words, {big.size} draws: max err {err:.3e}")
    assert err <= 1e-5                                # theta = 2 pi u2 carries u2's fp32 rounding: 6.77 * 2 pi * 2^-24 = 2.5e-6
    n32 = nc.twin_normals(9, 2, shape).reshape(-1)
    assert float(np.abs(n32 - nc.normal_field64(9, 2, count)).max()) <= 1e-5
    g32 = nc.twin_normals(9, 2, (1, 1, 33, 65), grey=True).reshape(-1)
    assert float(np.abs(g32 - nc.normal_field64(9, 2, 33 * 65, nc.TAG_GREY)).max()) <= 1e-5
    rng = np.random.default_rng(4)
    lam = (rng.integers(0, 256, shape).astype(np.float32) / np.float32(255)) * np.float32(256)     # level / 255 * vals
    lam[0, 0, 0, :8] = [0, 256, 10, np.nextafter(np.float32(10), np.float32(0)), 0.05, 1, 40, 255.5]
    k32 = nc.twin_counts(lam, 9, 2).reshape(-1)
    k64 = nc.poisson64(lam.astype(np.float64), 9, 2, np.arange(count))
    differ = int((k32 != k64).sum())
    print(f"counts, host fp32 twin vs float64 sampler on the same draws: {differ} of {count} differ")
    assert differ <= count // 1000 and (k32 >= 0).all() and (k32 == np.rint(k32)).all()


# ---- the host twins: every formula ----------------------------------------------------------------------------------------------
def _check_formula(out32, want64, noise64, rounded):
    tol = 4 * 2.0 ** -24 * np.maximum(1.0, np.abs(noise64))
    keep = np.ones(want64.shape, bool)
    if rounded is not None:                           # rounded: the float64 value before the rounding
        keep = ~nc.near_level_boundary(rounded, 1e-4 * np.maximum(1.0, np.abs(noise64)))
        assert (~keep).mean() <= 0.01, (~keep).mean()
    err = np.abs(out32.astype(np.float64) - want64)
    assert (err[keep] <= tol[keep]).all(), float((err[keep] / tol[keep]).max())


_GAUSS_FORMS = [(0, "add"), (F["CLIP"], "clip"), (F["ROUNDS"], "rounds"), (F["CLIP"] | F["ROUNDS"], "clip+rounds"),
                (F["CLIP"] | F["QUANTISE"], "clip+quantise"), (F["ONLY"], "generate")]


@pytest.mark.parametrize("shape", [(3, 3, 9, 11), (2, 1, 5, 5), (2, 4, 3, 7)])
@pytest.mark.parametrize("flags, what", _GAUSS_FORMS)
def test_gaussian_twin_image_formula(shape, flags, what):
    """out = epilogue(img + (n_c sigma / 255) (1 - g) + (n_g sigma / 255) g) with the twin's own normals, for given and drawn
    sigma / gray; the grey field carries no sample index"""
    b, c, h, w = shape
    rng = np.random.default_rng(b * 100 + c)
    x = (rng.random(shape) * 1.2 - 0.1).astype(np.float32)
    seed, call = 31337, 6
    n_c = nc.twin_normals(seed, call, shape).astype(np.float64)
    n_g = nc.twin_normals(seed, call, (1, 1, h, w), grey=True).astype(np.float64)
    sigma = np.linspace(1, 30, b).astype(np.float32)
    gray = np.array([0.0, 1.0, 0.25][:b], np.float32)
    for drawn in (False, True):
        if drawn:
            out, params = nc.twin_gaussian(x, seed, call, lo=1, hi=30, gray_scalar=0.4, flags=flags | F["DRAW_PARAMS"])
            s, g = nc.params32(seed, call, b, 1, 30, 0.4)
            assert np.array_equal(params[0], s) and np.array_equal(params[1], g)
        else:
            out, params = nc.twin_gaussian(x, seed, call, sigma=sigma, gray=gray, flags=flags)
            s, g = sigma, gray
            assert np.array_equal(params[0], s) and np.array_equal(params[1], g)
        s4, g4 = s.astype(np.float64).reshape(b, 1, 1, 1), g.astype(np.float64).reshape(b, 1, 1, 1)
        noise = (n_c * s4 / 255.0) * (1 - g4) + (n_g * s4 / 255.0) * g4
        pre = noise if flags & F["ONLY"] else x.astype(np.float64) + noise
        clip, rounds, quant = bool(flags & F["CLIP"]), bool(flags & F["ROUNDS"]), bool(flags & F["QUANTISE"])
        want = nc.epilogue64(pre, clip, rounds, quant)
        _check_formula(out, want, noise, np.clip(pre, 0, 1) if quant and not rounds else pre if rounds else None)
    # scalars stand for vectors of equal entries
    a = nc.twin_gaussian(x, seed, call, lo=7.5, gray_scalar=0.5, flags=flags)[0]
    v = nc.twin_gaussian(x, seed, call, sigma=np.full(b, 7.5), gray=np.full(b, 0.5), flags=flags)[0]
    assert np.array_equal(a, v)


@pytest.mark.parametrize("flags, what", _GAUSS_FORMS)
def test_poisson_twin_image_formula(flags, what):
    """out = epilogue(img + ((k_c / vals_c - q) (1 - g) + (k_g / vals_g - q_g) g) scale) with the twin's own counts for lambda =
    q vals, the levels, grey levels and vals formed as the kernel forms them"""
    shape = (3, 3, 16, 24)
    b = shape[0]
    rng = np.random.default_rng(8)
    x = (rng.random(shape) * 1.1 - 0.05).astype(np.float32)
    x[1] = np.round(x[1] * 6) / 6                      # a sample with few levels: another vals
    seed, call = 4242, 1
    q = nc.levels32(x) / np.float32(255)
    qg = nc.grey_levels32(x) / np.float32(255)
    vals_c, vals_g = nc.vals_of(q), nc.vals_of(qg)
    assert len(set(vals_c.tolist())) > 1
    k_c = nc.twin_counts(q * vals_c.reshape(b, 1, 1, 1), seed, call).astype(np.float64)
    k_g = nc.twin_counts(qg * vals_g.reshape(b, 1, 1, 1), seed, call, grey=True).astype(np.float64)
    scale = np.array([0.05, 1.0, 3.0], np.float32)
    gray = np.array([0.0, 1.0, 0.5], np.float32)
    for drawn in (False, True):
        if drawn:
            out, params = nc.twin_poisson(x, seed, call, lo=0.05, hi=3, gray_scalar=0.4, flags=flags | F["DRAW_PARAMS"])
            s, g = nc.params32(seed, call, b, 0.05, 3, 0.4)
        else:
            out, params = nc.twin_poisson(x, seed, call, scale=scale, gray=gray, flags=flags)
            s, g = scale, gray
        assert np.array_equal(params, np.stack([s, g, vals_c, vals_g]))
        s4, g4 = s.astype(np.float64).reshape(b, 1, 1, 1), g.astype(np.float64).reshape(b, 1, 1, 1)
        vc, vg = vals_c.astype(np.float64).reshape(b, 1, 1, 1), vals_g.astype(np.float64).reshape(b, 1, 1, 1)
        noise = ((k_c / vc - q.astype(np.float64)) * (1 - g4) + (k_g / vg - qg.astype(np.float64)) * g4) * s4
        pre = noise if flags & F["ONLY"] else x.astype(np.float64) + noise
        clip, rounds, quant = bool(flags & F["CLIP"]), bool(flags & F["ROUNDS"]), bool(flags & F["QUANTISE"])
        want = nc.epilogue64(pre, clip, rounds, quant)
        _check_formula(out, want, noise, np.clip(pre, 0, 1) if quant and not rounds else pre if rounds else None)


def test_poisson_twin_vals_on_the_fixture_images():
    """the census of the twin gives the fixture's vals: 1, 2, 3, 128, 129, 256 levels, a different count per sample, levels in one
    channel only"""
    x = G["p.x"].numpy()
    params = nc.twin_poisson(x, 1, 0, lo=1.0)[1]
    assert np.array_equal(params[2], G["p.vals_c"].numpy()) and np.array_equal(params[3], G["p.vals_g"].numpy())


# ---- support query and error codes ----------------------------------------------------------------------------------------------
def test_support_query_and_error_codes():
    lib = _capi.load()
    assert F == {"DRAW_PARAMS": 1, "CLIP": 2, "ROUNDS": 4, "QUANTISE": 8, "RAW": 16, "ONLY": 32, "POISSON_SWITCH": 10,
                 "INVERSION_MAX": 64, "PTRS_MAX_ROUNDS": 16} and _capi.ABI_VERSION >= 13
    wg = lib.oss_noise_workgroups
    assert wg(0, 9, 3, 400, 400, 0) == (9 * 3 * 400 * 400 // 4 + 255) // 256 and wg(0, 1, 1, 1, 1, 0) == 1
    assert wg(1, 9, 3, 400, 400, 0) == 9 * 625 and wg(1, 2, 3, 7, 5, F["CLIP"]) == 2
    assert wg(0, 2, 4, 9, 9, 0) > 0 and wg(1, 2, 4, 9, 9, 0) == 0 and wg(1, 2, 1, 9, 9, 0) == 0       # Poisson: three channels
    assert wg(1, 2, 4, 9, 9, F["RAW"]) > 0
    for bad in ((0, 3, 8, 8), (-1, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, -2), (1 << 25, 3, 8, 8), (1 << 20, 3, 1 << 12, 1 << 12)):
        assert wg(0, *bad, 0) == 0 and wg(1, *bad, 0) == 0, bad
    assert wg(2, 1, 3, 8, 8, 0) == 0 and wg(-1, 1, 3, 8, 8, 0) == 0 and wg(0, 1, 3, 8, 8, 64) == 0 and wg(1, 1, 3, 8, 8, -1) == 0
    assert lib.oss_noise_scratch_words(9) == 144 and lib.oss_noise_scratch_words(0) == 0 and lib.oss_noise_scratch_words(-3) == 0
    SHAPE, NULL = _capi._K["OSS_ERR_SHAPE"], _capi._K["OSS_ERR_NULL"]
    x = np.zeros((1, 3, 4, 4), np.float32)
    out, scr = np.zeros_like(x), np.zeros(16, np.uint32)
    p = lambda a: a.ctypes.data
    g = lambda img, o, shape, flags: lib.oss_noise_gaussian_host(img, o, 1, 0, None, None, 1.0, 1.0, 0.0, None, *shape, flags)
    po = lambda img, o, s, shape, flags: lib.oss_noise_poisson_host(img, o, 1, 0, None, None, 1.0, 1.0, 0.0, None, s, *shape, flags)
    assert g(p(x), p(out), x.shape, 0) == 0 and po(p(x), p(out), p(scr), x.shape, 0) == 0
    assert g(None, p(out), x.shape, 0) == NULL and g(p(x), None, x.shape, 0) == NULL and g(None, p(out), x.shape, F["ONLY"]) == 0
    assert po(None, p(out), p(scr), x.shape, F["ONLY"]) == NULL and po(p(x), p(out), None, x.shape, 0) == NULL
    assert po(p(x), None, p(scr), x.shape, 0) == NULL and po(p(x), p(out), None, x.shape, F["RAW"]) == 0
    for shape in ((0, 3, 4, 4), (1, 3, -4, 4), (1, 3, 4, 0)):
        assert g(p(x), p(out), shape, 0) == SHAPE and po(p(x), p(out), p(scr), shape, 0) == SHAPE
    assert po(p(x), p(out), p(scr), (1, 4, 2, 2), 0) == SHAPE and po(p(x), p(out), p(scr), (3, 1, 4, 4), 0) == SHAPE
    assert g(p(x), p(out), x.shape, 64) == SHAPE and po(p(x), p(out), p(scr), x.shape, 128) == SHAPE
    assert g(p(x), p(x), x.shape, 0) == SHAPE                                            # out must not be img
    # the device entry points refuse the same before any launch (no GPU is touched)
    dev = lambda img, o, st, shape, flags: lib.oss_noise_gaussian(img, o, st, None, None, 1.0, 1.0, 0.0, None, *shape, flags, None)
    assert dev(p(x), p(out), None, x.shape, 0) == NULL and dev(None, p(out), p(scr), x.shape, 0) == NULL
    assert dev(p(x), p(out), p(scr), (1, 3, 0, 4), 0) == SHAPE and dev(p(x), p(out), p(scr), x.shape, 64) == SHAPE
    devp = lambda img, o, st, s, shape, flags: lib.oss_noise_poisson(img, o, st, None, None, 1.0, 1.0, 0.0, None, s, *shape, flags, None)
    assert devp(p(x), p(out), None, p(scr), x.shape, 0) == NULL and devp(p(x), p(out), p(scr), None, x.shape, 0) == NULL
    assert devp(p(x), p(out), p(scr), p(scr), (1, 4, 2, 2), 0) == SHAPE and devp(p(x), p(out), p(scr), p(scr), x.shape, 256) == SHAPE
    assert lib.oss_noise_normals_host(None, p(out), 1) == NULL and lib.oss_noise_normals_host(p(scr), p(out), -1) == SHAPE


def test_cpu_and_float64_inputs_are_rejected_by_the_ops_not_silently_computed():
    x = torch.rand(1, 3, 4, 4)
    state = torch.zeros(2, dtype=torch.int64)
    for op in (torch.ops.vmambair.noise_gaussian, torch.ops.vmambair.noise_poisson):
        with pytest.raises((RuntimeError, NotImplementedError)):
            op(x, state, None, None, 1.0, 1.0, 0.0, 0, False)


def test_noise_stream_state_round_trip_without_a_device():
    s = D.NoiseStream(2 ** 64 - 5)
    assert s.state_dict() == {"seed": -5, "calls": 0}
    t = D.NoiseStream(0)
    t.load_state_dict(s.state_dict())
    assert t.state_dict() == s.state_dict() and s.clone().state_dict() == s.state_dict()
    with pytest.raises(RuntimeError, match="bind the stream"):
        t.load_state_dict({"seed": 1, "calls": 3})
