// oss_noise.hip -- the two noise steps of the RealSR degradation (MambaRealSR.feed_data, RealSR/VmambaIR/models/MambaRealSR_model.py
// :177-187, :209-219): random_add_gaussian_noise_pt and random_add_poisson_noise_pt of basicsr.data.degradations with their six
// siblings, without a host read, drawn from a counter-based stream that lives in device memory.  Semantics: include/vmambair_oss.h.
//
// The random stream.  Every random word is a word of Philox4x32-10 (oss_philox.h) with
//   key      (seed lo, seed hi)
//   counter  (element lo,  element hi [bits 0-7] | call hi [bits 8-31],  tag << 24 | draw,  call lo)
// `call` counts the entry-point calls of the stream (state[1]; 56 bits), `element` names what the block is for (< 2^40) and `draw`
// numbers the blocks one element consumes.  Tags and elements:
//   'c' 0x63  colour noise.  Gaussian: element = index / 4 of the flat (B, C, H, W) tensor, draw 0, the block's four words give the
//             normals of elements 4 e .. 4 e + 3.  Poisson: element = the flat index (b C + c) H W + p, draws 0 .. 7.
//   'g' 0x67  grey noise.  Gaussian: element = (y W + x) / 4 -- NO sample index: the package draws one (H, W) field and shares it
//             among the samples.  Poisson: element = b H W + p (one field per sample), draws 0 .. 7.
//   'p' 0x70  per-sample parameters of the random_* forms: element = b, draw 0; word 0 -> sigma or scale, word 1 -> the grey coin.
// A Poisson element consumes draw 0, word 0 below the switch-over (inversion) and the word pair 2 (i & 1), 2 (i & 1) + 1 of draw
// i / 2 in round i of the rejection loop above it: the host twin and the tests consume the same ones.
//
// Normals: Box-Muller on both word pairs of a block: u1 = (w + 1/2) 2^-32 in (0, 1), r = sqrt(-2 ln u1) in [1.5e-5, 6.77], theta =
// 2 pi * (w' * 2^-32): finite and non-zero radius for every word pair.  ln u1 is logf(u1) for w < 2^31 and log1pf(-(1 - u1)) above,
// with 1 - u1 = (~w + 1/2) 2^-32 from the complement word: fp32 cannot hold u1 near 1, and r near 0 would be off by 1e-4.
//
// Poisson counts for lambda in [0, 256] (lambda = level / 255 * vals), exact up to the arithmetic and bounded:
//   lambda < 10   inversion by sequential search in fp64 from ONE 32-bit uniform u = (w + 1/2) 2^-32: k = 0, p = s = exp(-lambda);
//                 while u > s: k += 1, p *= lambda / k, s += p.  fp64 so that s reaches 1 - 1e-15 > max u; at most 64 steps (the
//                 1 - 2^-33 quantile of Poisson(10) is 36).
//   lambda >= 10  PTRS (Hoermann 1993, "The transformed rejection method for generating Poisson random variables"; what torch's
//                 poisson uses from the same lambda on): two 23-bit uniforms per round, strictly inside (0, 1) so that us > 0 and
//                 ln V is finite; the squeeze accepts ~ 86 % at once in fp32, the full test is fp64 (k ln lambda and ln k! are
//                 ~ 1400 at lambda = 256 and cancel: fp32 would bias the acceptance by 1e-4).  At most 16 rounds: a round rejects
//                 with probability < 0.15, so all 16 fail with probability < 1e-13, and then floor(lambda) is returned.
// Divergence: the lanes of a wave hold different lambda.  A wave that has lanes on both sides of the switch-over runs both loops
// one after the other (each masked to its lanes), so the bound per wave is 64 cheap fp64 steps + 16 rounds; in expectation it is
// max over 64 lanes of (lambda + 1) steps and of a geometric(0.86) number of rounds, about 3.  Nothing in either loop is shared
// between lanes (no LDS, no cross-lane step), so an inactive lane costs nothing but its slot.
//
// Launches.  Gaussian: ONE sampling launch, 256 threads, 4 consecutive elements per thread (16-byte loads and stores when the
// pointers allow), then a one-thread launch that advances state[1].  Poisson: hipMemsetAsync of the B x 2 x 8 word census,
// the census launch, the sampling launch (one pixel = 3 colour counts + 1 grey count per thread), the advance.  Every kernel reads
// (seed, call) from `state` in device memory, so a captured call replayed N times draws N different fields.
// Census: a workgroup covers 2048 pixels of one sample, keeps 2 x 256 bits in LDS and sets a bit with atomicOr only when it
// reads it as clear (a constant image would otherwise serialise 256 atomics on one LDS word; the plain read is a broadcast),
// then 16 lanes atomicOr the non-zero words into the workspace.  Bits are only ever set: the races are benign.
//
// The per-element functions are __host__ __device__: oss_noise_gaussian_host / oss_noise_poisson_host run the same text on the
// CPU, which is how the CPU suite checks the distribution and every formula (tests/test_noise_host.py).
// Timings: profiles/noise_kernel_timing.txt.
#include <cmath>
#include <cstring>
#include "oss_host.h"
#include "oss_philox.h"
#include "oss_pixel_stage.h"

namespace oss {

constexpr uint32_t kTagColour = 0x63u << 24, kTagGrey = 0x67u << 24, kTagParam = 0x70u << 24;
constexpr int kNoiseThreads = 256, kCensusPixels = 8 * kNoiseThreads;
constexpr int kNoiseKnownFlags = OSS_NOISE_DRAW_PARAMS | OSS_NOISE_CLIP | OSS_NOISE_ROUNDS | OSS_NOISE_QUANTISE | OSS_NOISE_RAW |
                                 OSS_NOISE_ONLY;

struct NoiseKey { uint32_t k0, k1, call_lo, call_hi8; };   // call_hi8: bits 32-55 of the call counter, already shifted left by 8

__host__ __device__ inline NoiseKey noise_key(int64_t seed, int64_t calls) {
    const uint64_t s = (uint64_t)seed, c = (uint64_t)calls;
    return NoiseKey{(uint32_t)s, (uint32_t)(s >> 32), (uint32_t)c, (uint32_t)(c >> 32) << 8};
}

__host__ __device__ inline Philox4 noise_block(const NoiseKey &k, uint64_t element, uint32_t tag, uint32_t draw) {
    return philox4x32_10((uint32_t)element, ((uint32_t)(element >> 32) & 0xffu) | k.call_hi8, tag | draw, k.call_lo, k.k0, k.k1);
}

// torch.rand's fp32 uniform in [0, 1)
__host__ __device__ inline float uniform24(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-8f; }
// a uniform strictly inside (0, 1), exact in fp32
__host__ __device__ inline float uniform23_open(uint32_t w) { return ((float)(w >> 9) + 0.5f) * 1.1920928955078125e-7f; }

__host__ __device__ inline void normal_pair(uint32_t wa, uint32_t wb, float *n0, float *n1) {
#pragma clang fp contract(off)
    // u1 = (wa + 1/2) 2^-32 in (0, 1).  ln u1 is ill-conditioned at u1 -> 1, where fp32 cannot hold u1: the upper half takes
    // ln u1 = log1p(-(1 - u1)) with 1 - u1 = (~wa + 1/2) 2^-32 formed from the complement word, small and so relatively exact
    const float u = (float)(wa < 0x80000000u ? wa : ~wa) * 2.3283064365386963e-10f + 1.1641532182693481e-10f;   // (0, 1/2]
    const float r = sqrtf(-2.0f * (wa < 0x80000000u ? logf(u) : log1pf(-u)));
    const float theta = 6.2831853071795865f * ((float)wb * 2.3283064365386963e-10f);
    *n0 = r * cosf(theta), *n1 = r * sinf(theta);
}

__host__ __device__ inline void normal_block(const Philox4 &w, float n[4]) {
    normal_pair(w.v[0], w.v[1], &n[0], &n[1]);
    normal_pair(w.v[2], w.v[3], &n[2], &n[3]);
}

__host__ __device__ inline float poisson_count(float lam, const NoiseKey &key, uint64_t element, uint32_t tag) {
#pragma clang fp contract(off)
    if (!(lam > 0.0f)) return 0.0f;
    if (lam < (float)OSS_NOISE_POISSON_SWITCH) {
        const double u = ((double)noise_block(key, element, tag, 0).v[0] + 0.5) * 2.3283064365386963e-10;
        const double l = (double)lam;
        double p = exp(-l), s = p;
        int k = 0;
        while (u > s && k < OSS_NOISE_INVERSION_MAX) {
            ++k;
            p *= l / (double)k;
            s += p;
        }
        return (float)k;
    }
    const float slam = sqrtf(lam);
    const float b = 0.931f + 2.53f * slam, a = -0.059f + 0.02483f * b;
    const float inv_alpha = 1.1239f + 1.1328f / (b - 3.4f), vr = 0.9277f - 3.6224f / (b - 2.0f);
    const double loglam = log((double)lam);
    Philox4 w = {};
    for (int i = 0; i < OSS_NOISE_PTRS_MAX_ROUNDS; ++i) {
        if ((i & 1) == 0) w = noise_block(key, element, tag, (uint32_t)(i >> 1));
        const float U = uniform23_open(w.v[2 * (i & 1)]) - 0.5f, V = uniform23_open(w.v[2 * (i & 1) + 1]);
        const float us = 0.5f - fabsf(U);
        const float kf = floorf((2.0f * a / us + b) * U + lam + 0.43f);
        if (us >= 0.07f && V <= vr) return kf;
        if (kf < 0.0f || (us < 0.013f && V > us)) continue;
        const double lhs = log((double)V * (double)inv_alpha / ((double)a / ((double)us * (double)us) + (double)b));
        if (lhs <= -(double)lam + (double)kf * loglam - lgamma((double)kf + 1.0)) return kf;
    }
    return floorf(lam);
}

__host__ __device__ inline float noise_epilogue(float v, int flags) {
#pragma clang fp contract(off)
    if ((flags & OSS_NOISE_CLIP) && (flags & OSS_NOISE_ROUNDS)) v = quantise_255(v);
    else if (flags & OSS_NOISE_CLIP) v = clamp_unit(v);
    else if (flags & OSS_NOISE_ROUNDS) v = rintf(v * 255.0f) * kInv255;
    return (flags & OSS_NOISE_QUANTISE) ? quantise_255(v) : v;
}

struct NoiseArgs {
    const float *img;
    float *out;
    const float *amount, *gray;       // (B,) sigma or scale, and the grey weights; nullptr: the scalars
    float *params;                    // optional
    const uint32_t *census;           // Poisson: (B, 2, 8) words
    float lo, hi, gray_scalar;        // amount = lo, or U[lo, hi) with OSS_NOISE_DRAW_PARAMS; grey weight or grey probability
    int64_t B, N, chw, hw;            // N = B * chw elements
    int flags, vec;
};

// sigma_b / scale_b and g_b
__host__ __device__ inline void noise_sample_params(const NoiseArgs &p, const NoiseKey &key, int64_t b, float *amount, float *g) {
#pragma clang fp contract(off)
    if (p.flags & OSS_NOISE_DRAW_PARAMS) {
        const Philox4 w = noise_block(key, (uint64_t)b, kTagParam, 0);
        *amount = uniform24(w.v[0]) * (p.hi - p.lo) + p.lo;
        *g = uniform24(w.v[1]) < p.gray_scalar ? 1.0f : 0.0f;
    } else {
        *amount = p.amount ? p.amount[b] : p.lo;
        *g = p.gray ? p.gray[b] : p.gray_scalar;
    }
}

// v[i] for a lane-dependent i without an indexed (scratch) array
__host__ __device__ inline float pick4(const float v[4], int i) { return i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : v[3]; }

// ---- Gaussian: elements 4 group .. 4 group + 3 ------------------------------------------------------------------------------------
__host__ __device__ inline void gaussian_group(const NoiseArgs &p, const NoiseKey &key, int64_t group) {
#pragma clang fp contract(off)
    const int64_t e0 = 4 * group;
    if (e0 >= p.N) return;
    alignas(16) float x[4] = {0.0f, 0.0f, 0.0f, 0.0f}, o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float n[4];
    normal_block(noise_block(key, (uint64_t)group, kTagColour, 0), n);
    const int cnt = p.N - e0 < 4 ? (int)(p.N - e0) : 4;
    const bool whole = p.vec && cnt == 4;
    if (p.img) {
        if (whole) *reinterpret_cast<float4 *>(x) = *reinterpret_cast<const float4 *>(p.img + e0);
        else {
#pragma unroll
            for (int i = 0; i < 4; ++i) if (i < cnt) x[i] = p.img[e0 + i];
        }
    }
    if (p.flags & OSS_NOISE_RAW) {                              // the normals alone: colour, or with gray_scalar > 0 the grey field
        int64_t px = e0 % p.hw, have_g = -1;
        float ng[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i >= cnt) break;
            if (p.gray_scalar > 0.0f && (px >> 2) != have_g) {
                have_g = px >> 2;
                normal_block(noise_block(key, (uint64_t)have_g, kTagGrey, 0), ng);
            }
            o[i] = p.gray_scalar > 0.0f ? pick4(ng, (int)(px & 3)) : n[i];
            if (++px == p.hw) px = 0;
        }
    } else {
        int64_t b = e0 / p.chw, r = e0 - b * p.chw, px = r % p.hw;
        int64_t have_b = -1, have_g = -1;
        float sigma = 0.0f, g = 0.0f, ng[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i >= cnt) break;
            if (b != have_b) {
                noise_sample_params(p, key, b, &sigma, &g);
                have_b = b;
                if (p.params && r == 0) p.params[b] = sigma, p.params[p.B + b] = g;
            }
            if ((px >> 2) != have_g) {
                have_g = px >> 2;
                normal_block(noise_block(key, (uint64_t)have_g, kTagGrey, 0), ng);
            }
            // the package: noise = randn * sigma / 255; noise = noise * (1 - gray) + noise_gray * gray; out = img + noise
            const float colour = n[i] * sigma / 255.0f, grey = pick4(ng, (int)(px & 3)) * sigma / 255.0f;
            const float noise = colour * (1.0f - g) + grey * g;
            o[i] = noise_epilogue((p.flags & OSS_NOISE_ONLY) ? noise : x[i] + noise, p.flags);
            if (++px == p.hw) px = 0;
            if (++r == p.chw) r = 0, ++b;
        }
    }
    if (whole) *reinterpret_cast<float4 *>(p.out + e0) = *reinterpret_cast<const float4 *>(o);
    else {
#pragma unroll
        for (int i = 0; i < 4; ++i) if (i < cnt) p.out[e0 + i] = o[i];
    }
}

// ---- Poisson ----------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int noise_level(float v) {           // clamp(rint(255 v), 0, 255); a NaN counts as level 0
#pragma clang fp contract(off)
    const float r = rintf(v * 255.0f);
    return r >= 255.0f ? 255 : r > 0.0f ? (int)r : 0;
}

__host__ __device__ inline int noise_grey_level(float r, float g, float b) {   // torchvision's rgb_to_grayscale, then the level
#pragma clang fp contract(off)
    return noise_level(0.2989f * r + 0.587f * g + 0.114f * b);
}

// 2 ** ceil(log2(number of set bits)) of a 256-bit set; an empty set (never written by the census of a real sample) counts as 1
__host__ __device__ inline float noise_vals(const uint32_t *set) {
    int n = 0;
    for (int i = 0; i < 8; ++i) n += __builtin_popcount(set[i]);
    return n <= 1 ? 1.0f : (float)(1u << (32 - __builtin_clz((unsigned)(n - 1))));
}

// one pixel of sample b: three colour counts and the sample's grey count
__host__ __device__ inline void poisson_pixel(const NoiseArgs &p, const NoiseKey &key, int64_t b, int64_t px) {
#pragma clang fp contract(off)
    const float *src = p.img + b * p.chw + px;
    float *dst = p.out + b * p.chw + px;
    const float x[3] = {src[0], src[p.hw], src[2 * p.hw]};
    float scale, g;
    noise_sample_params(p, key, b, &scale, &g);
    const float vals_c = noise_vals(p.census + 16 * b), vals_g = noise_vals(p.census + 16 * b + 8);
    if (p.params && px == 0)
        p.params[b] = scale, p.params[p.B + b] = g, p.params[2 * p.B + b] = vals_c, p.params[3 * p.B + b] = vals_g;
    const float gq = (float)noise_grey_level(x[0], x[1], x[2]) / 255.0f;
    const float noise_gray = poisson_count(gq * vals_g, key, (uint64_t)(b * p.hw + px), kTagGrey) / vals_g - gq;
    for (int c = 0; c < 3; ++c) {
        const float q = (float)noise_level(x[c]) / 255.0f;
        float noise = poisson_count(q * vals_c, key, (uint64_t)(b * p.chw + c * p.hw + px), kTagColour) / vals_c - q;
        noise = (noise * (1.0f - g) + noise_gray * g) * scale;
        dst[c * p.hw] = noise_epilogue((p.flags & OSS_NOISE_ONLY) ? noise : x[c] + noise, p.flags);
    }
}

// OSS_NOISE_RAW: img holds lambda, out receives the count of the element's colour draws (gray_scalar > 0: of its grey draws)
__host__ __device__ inline void poisson_raw(const NoiseArgs &p, const NoiseKey &key, int64_t e) {
    const float lam = p.img[e];
    p.out[e] = poisson_count(lam < 256.0f ? lam : 256.0f, key, (uint64_t)e, p.gray_scalar > 0.0f ? kTagGrey : kTagColour);
}

__global__ void __launch_bounds__(kNoiseThreads) oss_noise_gaussian_kernel(const NoiseArgs p, const int64_t *__restrict__ state) {
    gaussian_group(p, noise_key(state[0], state[1]), (int64_t)blockIdx.x * kNoiseThreads + threadIdx.x);
}

__global__ void __launch_bounds__(kNoiseThreads) oss_noise_census_kernel(const float *__restrict__ img, uint32_t *census, int64_t chw,
                                                                        int64_t hw) {
    __shared__ uint32_t set[16];
    const int t = threadIdx.x;
    const int64_t b = blockIdx.y;
    if (t < 16) set[t] = 0u;
    __syncthreads();
    const float *src = img + b * chw;
    const int64_t first = (int64_t)blockIdx.x * kCensusPixels;
    for (int j = 0; j < kCensusPixels / kNoiseThreads; ++j) {
        const int64_t px = first + (int64_t)j * kNoiseThreads + t;
        if (px >= hw) break;
        const float r = src[px], g = src[hw + px], bl = src[2 * hw + px];
        const int lv[4] = {noise_level(r), noise_level(g), noise_level(bl), 256 + noise_grey_level(r, g, bl)};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t bit = 1u << (lv[i] & 31);
            uint32_t *word = &set[lv[i] >> 5];
            if (!(*(volatile uint32_t *)word & bit)) atomicOr(word, bit);
        }
    }
    __syncthreads();
    if (t < 16 && set[t]) atomicOr(&census[16 * b + t], set[t]);
}

__global__ void __launch_bounds__(kNoiseThreads) oss_noise_poisson_kernel(const NoiseArgs p, const int64_t *__restrict__ state) {
    const int64_t px = (int64_t)blockIdx.x * kNoiseThreads + threadIdx.x;
    if (px < p.hw) poisson_pixel(p, noise_key(state[0], state[1]), (int64_t)blockIdx.y, px);
}

__global__ void __launch_bounds__(kNoiseThreads) oss_noise_poisson_raw_kernel(const NoiseArgs p, const int64_t *__restrict__ state) {
    const int64_t e = (int64_t)blockIdx.x * kNoiseThreads + threadIdx.x;
    if (e < p.N) poisson_raw(p, noise_key(state[0], state[1]), e);
}

// after the sampling launch on the same stream: the next call, or the next replay of a captured one, draws another field
__global__ void oss_noise_advance_kernel(int64_t *state) { state[1] += 1; }

// ---- host side ----------------------------------------------------------------------------------------------------------------------
static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the launch geometry of kind 0 (Gaussian) / 1 (Poisson); false: refused
static bool noise_dims(int kind, int64_t B, int64_t C, int64_t h, int64_t w, int flags, int64_t *gx, int64_t *gy) {
    const int64_t lim = 1 << 24;
    if ((kind != 0 && kind != 1) || (flags & ~kNoiseKnownFlags)) return false;
    if (B < 1 || C < 1 || h < 1 || w < 1 || B > lim || C > lim || h > lim || w > lim) return false;
    const int64_t hw = h * w;                              // <= 2^48
    if (hw > ((int64_t)1 << 40) / C || C * hw > ((int64_t)1 << 40) / B) return false;   // element indices stay below 2^40
    const int64_t N = B * C * hw;
    if (kind == 0) *gx = ceil_div(ceil_div(N, 4), kNoiseThreads), *gy = 1;
    else if (flags & OSS_NOISE_RAW) *gx = ceil_div(N, kNoiseThreads), *gy = 1;
    else {
        if (C != 3 || B > 65535) return false;
        *gx = ceil_div(hw, kNoiseThreads), *gy = B;
    }
    return *gx <= 0x7fffffff;
}

static NoiseArgs noise_args(const float *img, float *out, const float *amount, const float *gray, float lo, float hi, float gray_scalar,
                            float *params, const uint32_t *census, int64_t B, int64_t C, int64_t h, int64_t w, int flags) {
    NoiseArgs p = {};
    p.img = img, p.out = out, p.amount = amount, p.gray = gray, p.params = params, p.census = census;
    p.lo = lo, p.hi = hi, p.gray_scalar = gray_scalar;
    p.B = B, p.hw = h * w, p.chw = C * p.hw, p.N = B * p.chw, p.flags = flags;
    p.vec = ((reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    return p;
}

static int noise_check(int kind, const float *img, const float *out, const void *state_or_null, bool need_state, const void *scratch,
                       int64_t B, int64_t C, int64_t h, int64_t w, int flags, int64_t *gx, int64_t *gy) {
    const bool img_optional = kind == 0 && (flags & (OSS_NOISE_ONLY | OSS_NOISE_RAW));
    if (!out || (!img && !img_optional) || (need_state && !state_or_null)) return OSS_ERR_NULL;
    if (kind == 1 && !(flags & OSS_NOISE_RAW) && !scratch) return OSS_ERR_NULL;
    if (!noise_dims(kind, B, C, h, w, flags, gx, gy)) return OSS_ERR_SHAPE;
    if (img == out) return OSS_ERR_SHAPE;
    return OSS_OK;
}

}  // namespace oss

using namespace oss;

extern "C" {

size_t oss_noise_workgroups(int kind, int64_t batch, int64_t channels, int64_t h, int64_t w, int flags) {
    int64_t gx, gy;
    return noise_dims(kind, batch, channels, h, w, flags, &gx, &gy) ? (size_t)(gx * gy) : 0;
}

size_t oss_noise_scratch_words(int64_t batch) { return batch < 1 || batch > 65535 ? 0 : (size_t)(16 * batch); }

int oss_noise_gaussian(const float *img, float *out, int64_t *state, const float *sigma, const float *gray, float sigma_lo,
                       float sigma_hi, float gray_scalar, float *params, int64_t batch, int64_t channels, int64_t h, int64_t w,
                       int flags, oss_stream_t stream) {
    int64_t gx, gy;
    const int rc = noise_check(0, img, out, state, true, nullptr, batch, channels, h, w, flags, &gx, &gy);
    if (rc != OSS_OK) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const NoiseArgs p = noise_args(img, out, sigma, gray, sigma_lo, sigma_hi, gray_scalar, params, nullptr, batch, channels, h, w, flags);
    hipLaunchKernelGGL(oss_noise_gaussian_kernel, dim3((unsigned)gx), dim3(kNoiseThreads), 0, s, p, state);
    hipLaunchKernelGGL(oss_noise_advance_kernel, dim3(1), dim3(1), 0, s, state);
    return (int)hipGetLastError();
}

int oss_noise_poisson(const float *img, float *out, int64_t *state, const float *scale, const float *gray, float scale_lo,
                      float scale_hi, float gray_scalar, float *params, uint32_t *scratch, int64_t batch, int64_t channels, int64_t h,
                      int64_t w, int flags, oss_stream_t stream) {
    int64_t gx, gy;
    const int rc = noise_check(1, img, out, state, true, scratch, batch, channels, h, w, flags, &gx, &gy);
    if (rc != OSS_OK) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const NoiseArgs p = noise_args(img, out, scale, gray, scale_lo, scale_hi, gray_scalar, params, scratch, batch, channels, h, w, flags);
    if (flags & OSS_NOISE_RAW) {
        hipLaunchKernelGGL(oss_noise_poisson_raw_kernel, dim3((unsigned)gx), dim3(kNoiseThreads), 0, s, p, state);
    } else {
        const hipError_t e = hipMemsetAsync(scratch, 0, sizeof(uint32_t) * 16 * (size_t)batch, s);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(oss_noise_census_kernel, dim3((unsigned)ceil_div(p.hw, kCensusPixels), (unsigned)batch), dim3(kNoiseThreads),
                           0, s, img, scratch, p.chw, p.hw);
        hipLaunchKernelGGL(oss_noise_poisson_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(kNoiseThreads), 0, s, p, state);
    }
    hipLaunchKernelGGL(oss_noise_advance_kernel, dim3(1), dim3(1), 0, s, state);
    return (int)hipGetLastError();
}

int oss_noise_normals_host(const uint32_t *words, float *out, int64_t blocks) {
    if (!words || !out) return OSS_ERR_NULL;
    if (blocks < 0) return OSS_ERR_SHAPE;
    for (int64_t i = 0; i < blocks; ++i)
        normal_block(Philox4{{words[4 * i], words[4 * i + 1], words[4 * i + 2], words[4 * i + 3]}}, out + 4 * i);
    return OSS_OK;
}

int oss_noise_gaussian_host(const float *img, float *out, int64_t key, int64_t counter, const float *sigma, const float *gray,
                            float sigma_lo, float sigma_hi, float gray_scalar, float *params, int64_t batch, int64_t channels,
                            int64_t h, int64_t w, int flags) {
    int64_t gx, gy;
    const int rc = noise_check(0, img, out, nullptr, false, nullptr, batch, channels, h, w, flags, &gx, &gy);
    if (rc != OSS_OK) return rc;
    const NoiseArgs p = noise_args(img, out, sigma, gray, sigma_lo, sigma_hi, gray_scalar, params, nullptr, batch, channels, h, w, flags);
    const NoiseKey k = noise_key(key, counter);
    for (int64_t group = 0; 4 * group < p.N; ++group) gaussian_group(p, k, group);
    return OSS_OK;
}

int oss_noise_poisson_host(const float *img, float *out, int64_t key, int64_t counter, const float *scale, const float *gray,
                           float scale_lo, float scale_hi, float gray_scalar, float *params, uint32_t *scratch, int64_t batch,
                           int64_t channels, int64_t h, int64_t w, int flags) {
    int64_t gx, gy;
    const int rc = noise_check(1, img, out, nullptr, false, scratch, batch, channels, h, w, flags, &gx, &gy);
    if (rc != OSS_OK) return rc;
    const NoiseArgs p = noise_args(img, out, scale, gray, scale_lo, scale_hi, gray_scalar, params, scratch, batch, channels, h, w, flags);
    const NoiseKey k = noise_key(key, counter);
    if (flags & OSS_NOISE_RAW) {
        for (int64_t e = 0; e < p.N; ++e) poisson_raw(p, k, e);
        return OSS_OK;
    }
    memset(scratch, 0, sizeof(uint32_t) * 16 * (size_t)batch);
    for (int64_t b = 0; b < batch; ++b)
        for (int64_t px = 0; px < p.hw; ++px) {
            const float *src = img + b * p.chw + px;
            const int lv[4] = {noise_level(src[0]), noise_level(src[p.hw]), noise_level(src[2 * p.hw]),
                               256 + noise_grey_level(src[0], src[p.hw], src[2 * p.hw])};
            for (int i = 0; i < 4; ++i) scratch[16 * b + (lv[i] >> 5)] |= 1u << (lv[i] & 31);
        }
    for (int64_t b = 0; b < batch; ++b)
        for (int64_t px = 0; px < p.hw; ++px) poisson_pixel(p, k, b, px);
    return OSS_OK;
}

}  // extern "C"
