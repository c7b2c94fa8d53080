"""Shared by tests/test_noise_host.py and tests/test_noise_gpu.py: the random stream of csrc/oss_noise.hip restated on NumPy integers
(Philox4x32-10 and the counter layout of include/vmambair_oss.h), float64 evaluations of the two samplers on the same words, callers
of the library's host twins, and the distribution checks both suites apply.  No GPU needed."""
import math

import numpy as np
from scipy import special, stats

from vmambair_amd import _capi

M32 = np.uint64(0xFFFFFFFF)
TAG_COLOUR, TAG_GREY, TAG_PARAM = 0x63 << 24, 0x67 << 24, 0x70 << 24
N = _capi.NOISE
SWITCH, INVERSION_MAX, PTRS_ROUNDS = N["POISSON_SWITCH"], N["INVERSION_MAX"], N["PTRS_MAX_ROUNDS"]
GPU_SHAPES = ((1, 3, 1, 1), (2, 3, 7, 5), (3, 3, 33, 65), (2, 3, 64, 64))
GAUSSIAN_ONLY_SHAPES = ((2, 1, 16, 16), (1, 4, 9, 9))


# ---- the stream ---------------------------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Salmon et al. (SC'11), Philox4x32 with 10 rounds, on uint64 arrays that hold 32-bit words"""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0), int(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def noise_words(seed, call, element, tag, draw=0):
    """the four words of block (element, tag, draw) of call ``call`` of the stream with seed ``seed``"""
    seed, call = int(seed) & 0xFFFFFFFFFFFFFFFF, int(call) & 0xFFFFFFFFFFFFFFFF
    element = np.asarray(element, np.uint64)
    c1 = ((element >> np.uint64(32)) & np.uint64(0xFF)) | np.uint64(((call >> 32) & 0xFFFFFF) << 8)
    return philox4x32_10(element & M32, c1, np.uint64(tag | draw), np.uint64(call & 0xFFFFFFFF), seed & 0xFFFFFFFF, seed >> 32)


def normals64(wa, wb):
    """the kernel's Box-Muller transform in float64 on the same word pair"""
    u1 = wa.astype(np.float64) * 2.0 ** -32 + 2.0 ** -33
    r = np.sqrt(-2.0 * np.log(u1))
    theta = 2.0 * math.pi * (wb.astype(np.float64) * 2.0 ** -32)
    return r * np.cos(theta), r * np.sin(theta)


def normal_field64(seed, call, count, tag=TAG_COLOUR):
    """float64 normals of elements 0 .. count - 1 (colour: of the flat tensor; grey: of the (h, w) field)"""
    w = noise_words(seed, call, np.arange((count + 3) // 4), tag)
    return np.stack([*normals64(w[0], w[1]), *normals64(w[2], w[3])], axis=-1).reshape(-1)[:count]


def uniform24(w):
    return (w >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def params32(seed, call, batch, lo, hi, prob):
    """sigma_b / scale_b and g_b of the random_* forms, in the kernel's fp32 operations"""
    w = noise_words(seed, call, np.arange(batch), TAG_PARAM)
    amount = uniform24(w[0]) * (np.float32(hi) - np.float32(lo)) + np.float32(lo)
    return amount.astype(np.float32), (uniform24(w[1]) < np.float32(prob)).astype(np.float32)


def poisson64(lam, seed, call, element, tag=TAG_COLOUR):
    """the kernel's Poisson sampler in float64 throughout, on the draws the kernel numbers: inversion below the switch-over, PTRS
    from it on"""
    lam = np.asarray(lam, np.float64).reshape(-1)
    element = np.asarray(element, np.uint64).reshape(-1)
    out = np.zeros_like(lam)
    low = (lam > 0) & (lam < SWITCH)
    if low.any():
        l = lam[low]
        u = (noise_words(seed, call, element[low], tag, 0)[0].astype(np.float64) + 0.5) * 2.0 ** -32
        p = np.exp(-l)
        s, k = p.copy(), np.zeros_like(l)
        for _ in range(INVERSION_MAX):
            m = u > s
            if not m.any():
                break
            k[m] += 1
            p[m] *= l[m] / k[m]
            s[m] += p[m]
        out[low] = k
    high = lam >= SWITCH
    if high.any():
        l, el = lam[high], element[high]
        b = 0.931 + 2.53 * np.sqrt(l)
        a = -0.059 + 0.02483 * b
        inv_alpha, vr = 1.1239 + 1.1328 / (b - 3.4), 0.9277 - 3.6224 / (b - 2.0)
        res, active = np.floor(l), np.ones(l.shape, bool)
        for i in range(PTRS_ROUNDS):
            if i % 2 == 0:
                w = noise_words(seed, call, el, tag, i // 2)
            U = ((w[2 * (i & 1)] >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23 - 0.5
            V = ((w[2 * (i & 1) + 1] >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
            us = 0.5 - np.abs(U)
            kf = np.floor((2.0 * a / us + b) * U + l + 0.43)
            quick = (us >= 0.07) & (V <= vr)
            reject = (kf < 0) | ((us < 0.013) & (V > us))
            with np.errstate(invalid="ignore", divide="ignore"):
                full = np.log(V * inv_alpha / (a / (us * us) + b)) <= -l + kf * np.log(l) - special.gammaln(np.maximum(kf, 0) + 1.0)
            accept = active & (quick | (~reject & full))
            res[accept] = kf[accept]
            active &= ~accept
            if not active.any():
                break
        out[high] = res
    return out


# ---- the library's host twins ---------------------------------------------------------------------------------------------------
def _ptr(a):
    return None if a is None else a.ctypes.data


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def twin_gaussian(img, seed, call, sigma=None, gray=None, lo=0.0, hi=0.0, gray_scalar=0.0, flags=0, shape=None, rc=False):
    """oss_noise_gaussian_host on NumPy arrays -> (out, params (2, B)); ``shape`` stands in for a missing ``img``"""
    img, sigma, gray = _f32(img), _f32(sigma), _f32(gray)
    shape = img.shape if img is not None else tuple(shape)
    out, params = np.zeros(shape, np.float32), np.zeros((2, shape[0]), np.float32)
    code = _capi.load().oss_noise_gaussian_host(_ptr(img), _ptr(out), int(seed), int(call), _ptr(sigma), _ptr(gray), float(lo), float(hi),
                                                float(gray_scalar), _ptr(params), *shape, int(flags))
    if rc:
        return code
    assert code == 0, code
    return out, params


def twin_poisson(img, seed, call, scale=None, gray=None, lo=0.0, hi=0.0, gray_scalar=0.0, flags=0):
    """oss_noise_poisson_host on NumPy arrays -> (out, params (4, B): scale_b, g_b, vals colour, vals grey)"""
    img, scale, gray = _f32(img), _f32(scale), _f32(gray)
    out, params = np.zeros(img.shape, np.float32), np.zeros((4, img.shape[0]), np.float32)
    raw = bool(flags & N["RAW"])
    scratch = None if raw else np.zeros(16 * img.shape[0], np.uint32)
    code = _capi.load().oss_noise_poisson_host(_ptr(img), _ptr(out), int(seed), int(call), _ptr(scale), _ptr(gray), float(lo), float(hi),
                                               float(gray_scalar), None if raw else _ptr(params), _ptr(scratch), *img.shape, int(flags))
    assert code == 0, code
    return out, params


def twin_normals(seed, call, shape, grey=False):
    return twin_gaussian(None, seed, call, gray_scalar=1.0 if grey else 0.0, flags=N["RAW"], shape=shape)[0]


def twin_counts(lam, seed, call, grey=False):
    return twin_poisson(lam, seed, call, gray_scalar=1.0 if grey else 0.0, flags=N["RAW"])[0]


# ---- what the kernel computes before it draws, in its own fp32 operations -------------------------------------------------------
def levels32(x):
    """clamp(rint(255 x), 0, 255) as the kernel forms it"""
    return np.clip(np.rint(np.asarray(x, np.float32) * np.float32(255)), 0, 255).astype(np.float32)


def grey_levels32(x):
    """the grey level of a (B, 3, h, w) image: torchvision's weights in fp32, left to right"""
    x = np.asarray(x, np.float32)
    g = (np.float32(0.2989) * x[:, 0] + np.float32(0.587) * x[:, 1]) + np.float32(0.114) * x[:, 2]
    return levels32(g)[:, None]


def vals_of(levels):
    """per sample: 2 ** ceil(log2(number of distinct levels))"""
    return np.array([2.0 ** math.ceil(math.log2(len(np.unique(s)))) for s in levels], np.float32)


def epilogue64(v, clip, rounds, quantise=False):
    v = np.asarray(v, np.float64)
    if clip and rounds:
        v = np.clip(np.rint(v * 255.0), 0, 255) / 255.0
    elif clip:
        v = np.clip(v, 0, 1)
    elif rounds:
        v = np.rint(v * 255.0) / 255.0
    return np.clip(np.rint(v * 255.0), 0, 255) / 255.0 if quantise else v


def near_level_boundary(v, width):
    """where 255 v lies within ``width`` of a half-integer, the points at which rounding to a level is discontinuous"""
    t = np.asarray(v, np.float64) * 255.0
    return np.abs(t - np.floor(t) - 0.5) < width


# ---- distribution checks --------------------------------------------------------------------------------------------------------
P_TAIL = 1e-6   # every statistic must lie below the 1 - 1e-6 quantile of its distribution


def normal_failures(x):
    """-> the list of failed checks of a standard normal sample (empty: passed)"""
    x = np.asarray(x, np.float64).reshape(-1)
    n, bad = x.size, []
    if not np.isfinite(x).all():
        return ["not finite"]
    if abs(x.mean()) > 5 / math.sqrt(n):
        bad.append(f"mean {x.mean():.3e} > {5 / math.sqrt(n):.3e}")
    if abs(x.var() - 1) > 5 * math.sqrt(2 / n):
        bad.append(f"var - 1 {x.var() - 1:.3e} > {5 * math.sqrt(2 / n):.3e}")
    ks = stats.kstest(x, "norm").statistic
    if ks >= stats.kstwo.ppf(1 - P_TAIL, n):
        bad.append(f"KS {ks:.3e} >= {stats.kstwo.ppf(1 - P_TAIL, n):.3e}")
    return bad


def poisson_failures(k, lam):
    """-> the list of failed checks of a Poisson(lam) sample: non-negative integers, mean, variance, Pearson chi^2 against the exact
    pmf with bins merged to an expected count >= 5"""
    k = np.asarray(k, np.float64).reshape(-1)
    n, lam, bad = k.size, float(lam), []
    if not (np.isfinite(k).all() and (k >= 0).all() and (k == np.rint(k)).all()):
        return ["not a non-negative integer"]
    if lam == 0:
        return [] if (k == 0).all() else ["lambda = 0 gave a non-zero count"]
    if abs(k.mean() - lam) > 5 * math.sqrt(lam / n):
        bad.append(f"mean - lam {k.mean() - lam:.3e} > {5 * math.sqrt(lam / n):.3e}")
    if abs(k.var() - lam) > 5 * math.sqrt((lam + 2 * lam * lam) / n):
        bad.append(f"var - lam {k.var() - lam:.3e} > {5 * math.sqrt((lam + 2 * lam * lam) / n):.3e}")
    top = int(max(k.max(), stats.poisson.ppf(1 - 1e-12, lam))) + 2
    expected = n * np.append(stats.poisson.pmf(np.arange(top), lam), stats.poisson.sf(top - 1, lam))
    observed = np.bincount(np.minimum(k, top).astype(np.int64), minlength=top + 1).astype(np.float64)
    groups_e, groups_o, e_acc, o_acc = [], [], 0.0, 0.0
    for e, o in zip(expected, observed):
        e_acc, o_acc = e_acc + e, o_acc + o
        if e_acc >= 5:
            groups_e.append(e_acc), groups_o.append(o_acc)
            e_acc = o_acc = 0.0
    if groups_e:
        groups_e[-1] += e_acc
        groups_o[-1] += o_acc
    ge, go = np.array(groups_e), np.array(groups_o)
    if len(ge) > 1:
        chi2, bound = float(((go - ge) ** 2 / ge).sum()), stats.chi2.ppf(1 - P_TAIL, len(ge) - 1)
        if chi2 >= bound:
            bad.append(f"chi2 {chi2:.1f} >= {bound:.1f} ({len(ge) - 1} dof)")
    return bad


def pearson_r(a, b):
    return float(np.corrcoef(np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1))[0, 1])


def poisson_lambdas():
    """the issue's lambdas plus the values just below and just above the sampler's switch-over (fp32 neighbours)"""
    sw = np.float32(SWITCH)
    return [0.0, 0.05, 1.0, float(np.nextafter(sw, np.float32(0))), float(sw), 40.0, 256.0]
