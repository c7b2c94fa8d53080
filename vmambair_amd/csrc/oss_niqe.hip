// oss_niqe.hip -- the (blocks, 36) features of the reference's NIQE, the no-reference image quality metric, of a batch of images
// in ONE launch on the device.
//
// What the reference computes on the host (Deraining/basicsr/metrics/niqe.py), one image at a time:
//   calculate_niqe  :158-205   astype(float32), to_y_channel, crop_border -- the load of oss_metrics.hip (oss_metric_load.h)
//   niqe            :67-155    crop to whole 96 x 96 blocks from the top-left; at scale 1 and 2 the MSCN map
//                              n = (img - mu) / (sigma + 1), mu = convolve(img, window, 'nearest'),
//                              sigma = sqrt(|convolve(img^2, window) - mu^2|) with the 7 x 7 window, float32 arrays; between the
//                              scales cv2.resize(img / 255., half, INTER_LINEAR) * 255.: the mean of every 2 x 2 cell
//   compute_feature :40-64     per block (96 x 96, at scale 2 48 x 48) an AGGD fit of the block and of its product with the block
//                              rolled by [0, 1], [1, 0], [1, 1], [1, -1] (np.roll: the roll WRAPS INSIDE the block): 18 features
//   estimate_aggd_param :10-37 mean of squares over the negative and over the positive values, mean |x|, mean x^2;
//                              alpha = gam[argmin((r_gam - rhatnorm)^2)] on gam = arange(0.2, 10.001, 0.001)
// The covariance / pseudo-inverse of :142-155 stay on the host (vmambair_amd/metrics.py): 36 x 36, once per image.
//
// Dtypes follow the reference step by step (a float64 evaluation misses it by 2e-4 on a smooth image and by 2.5e-2 on one with a
// constant region, where img - mu is exactly 0 in float32): every window sum is 49 products and 49 additions in fp64, in the order
// scipy adds them (rows of the flipped kernel), rounded ONCE to fp32; img^2, mu^2, the difference, |.|, sqrt, img - mu, sigma + 1,
// the quotient, the four products of neighbours and every square are single fp32 operations (contraction off; the fp32 quotients
// and the square root are the fp64 operation rounded once, which is the correctly rounded fp32 result: 53 >= 2 * 24 + 2).  The
// moments are fp64 sums of those fp32 values and the fit runs in fp64 (the reference sums in fp32: 1e-7 from it).
//
// One workgroup (512 threads) per (block, scale, image); grid (blocks, 2, batch):
//   1. the block plus a 3-pixel halo goes into LDS as fp32, 102 x 102 (54 x 54 at scale 2), coordinates clamped to the
//      block-cropped plane (at scale 2: to the half-size plane) -- that IS mode 'nearest'.  Every element is converted on load as
//      oss_metrics.hip does; at scale 2 a tile pixel is built from its 2 x 2 source cell, ((a / 255 * .5 + b / 255 * .5) * .5 +
//      (c / 255 * .5 + d / 255 * .5) * .5) * 255 in fp32 with a, b the upper pair: nothing intermediate goes to memory;
//   2. MSCN: a thread owns 4 adjacent pixels of a row and walks the 7 window rows, 10 staged values per row; the block's MSCN
//      values go into a second LDS array (96 x 96 fp32);
//   3. moments: a thread takes pixels t, t + 512, ... in that order, forms the 5 maps (wrapped neighbours from LDS) and adds up
//      6 numbers per map (squares and counts below / above 0, |x|, x^2) in fp64; wave shuffles, then the 8 waves through LDS in a
//      fixed order.  No atomics: reruns are bit-identical, and a block's result does not depend on the batch it sits in;
//   4. lanes 0-4 of wave 0 finish one fit each: binary search in the increasing r_gam table, then the squared distances of the two
//      neighbours (the lower index on a tie, as argmin; a NaN -- an all-zero block has no negative and no positive value -- gives
//      index 0, so alpha = 0.2 next to NaN betas, as in the reference).  gam, r_gam, sqrt(G(1/a) / G(3/a)) and G(2/a) / G(1/a) come
//      from the caller's (4, 9801) table, computed once on the host: no gamma function is evaluated here.
// LDS: 42,432 (tile, row pitch 104) + 36,864 (MSCN block) + 1,920 (reduction) = 81,216 bytes, dynamic (above the 64 KiB static
// limit, enabled through LdsGate as the scan backward does) -> two workgroups = 16 waves per CU.  The kernel's time is fp64
// arithmetic: per pixel 196 products and additions of the two window sums, a square root and a division in fp64, and on load
// the divisions of the luma conversion (at scale 2 for four source pixels per tile pixel); a launch takes about as long as its
// slowest workgroup times the rounds of workgroups per CU, which is why 512 threads beat 256 (2048 x 2048: 141 against 155 us).
#include <cmath>
#include "oss_device.h"
#include "oss_host.h"
#include "oss_metric_load.h"

#pragma clang fp contract(off)

namespace oss {

constexpr int kNqB = OSS_NIQE_BLOCK, kNqR = 3;          // block side, window radius
constexpr int kNqT = kNqB + 2 * kNqR, kNqTP = 104;      // staged tile 102 x 102, row pitch (floats)
constexpr int kNqN = OSS_NIQE_GRID;                     // points of the alpha grid
constexpr int kNqThreads = 512, kNqWaves = kNqThreads / 64;
static_assert(kNqWaves == 8, "the last step adds the waves' sums as a fixed tree of eight");
constexpr int kNqMaps = 5, kNqMom = 6;                  // block + 4 products; sum sq < 0, sum sq > 0, sum |x|, sum sq, count < 0, count > 0
constexpr size_t kNqTileBytes = sizeof(float) * kNqT * kNqTP, kNqBlockBytes = sizeof(float) * kNqB * kNqB;
constexpr size_t kNqLdsBytes = kNqTileBytes + kNqBlockBytes + sizeof(double) * kNqWaves * kNqMaps * kNqMom;
static_assert(kNqTileBytes % 16 == 0 && kNqBlockBytes % 16 == 0, "every carve offset of the dynamic LDS is a multiple of 16");

struct NiqeArgs {
    const void *a;
    const double *tab;       // (4, kNqN): gam, r_gam, sqrt(G(1/a) / G(3/a)), G(2/a) / G(1/a)
    double *out;             // (batch, blocks, 36)
    int Hb, Wb, nbh, nbw;    // block-cropped plane, blocks along y and x
    int64_t sb, sc, rs, a0;  // batch / channel / row stride, offset of the cropped origin inside a plane (elements)
    double w[49];            // the window as convolve applies it: flipped, row-major
};

__device__ __forceinline__ float niqe_unit(float v) { return (float)((double)v / 255.0); }   // fl32(v / 255)

template <typename T, bool QUANT, bool LUMA>
__global__ void __launch_bounds__(kNqThreads)
oss_niqe_features_kernel(const NiqeArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nq_smem[];
    float *sT = reinterpret_cast<float *>(nq_smem);
    float *sN = reinterpret_cast<float *>(nq_smem + kNqTileBytes);
    double *sRed = reinterpret_cast<double *>(nq_smem + kNqTileBytes + kNqBlockBytes);   // [wave][map][moment]
    const int t = threadIdx.x;
    const int blk = blockIdx.x, half = blockIdx.y, img = blockIdx.z;
    const int bx = blk / p.nbh, by = blk - bx * p.nbh;     // the reference's order: idx_w outer, idx_h inner
    const int S = half ? kNqB / 2 : kNqB, TS = S + 2 * kNqR;
    const int Hp = half ? p.Hb / 2 : p.Hb, Wp = half ? p.Wb / 2 : p.Wb;
    const T *pa = reinterpret_cast<const T *>(p.a) + img * p.sb + p.a0;

    for (int idx = t; idx < TS * TS; idx += kNqThreads) {
        const int i = idx / TS, j = idx - i * TS;
        const int y = min(max(by * S + i - kNqR, 0), Hp - 1), x = min(max(bx * S + j - kNqR, 0), Wp - 1);
        float v;
        if (!half) {
            v = metric_pixel<T, QUANT, LUMA>(pa + y * p.rs + x, p.sc);
        } else {
            const T *q = pa + (2 * y) * p.rs + 2 * x;
            const float a = niqe_unit(metric_pixel<T, QUANT, LUMA>(q, p.sc)), b = niqe_unit(metric_pixel<T, QUANT, LUMA>(q + 1, p.sc));
            const float c = niqe_unit(metric_pixel<T, QUANT, LUMA>(q + p.rs, p.sc)), d = niqe_unit(metric_pixel<T, QUANT, LUMA>(q + p.rs + 1, p.sc));
            const float top = a * 0.5f + b * 0.5f, bottom = c * 0.5f + d * 0.5f;
            v = (top * 0.5f + bottom * 0.5f) * 255.0f;
        }
        sT[i * kNqTP + j] = v;
    }
    __syncthreads();

    const int quads = S / 4;
    for (int q = t; q < S * quads; q += kNqThreads) {
        const int y = q / quads, x0 = (q - y * quads) * 4;
        double m[4] = {0.0, 0.0, 0.0, 0.0}, e[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            double r[10], r2[10];
#pragma unroll
            for (int j = 0; j < 10; ++j) {
                const float v = sT[(y + i) * kNqTP + x0 + j];
                const float v2 = v * v;
                r[j] = (double)v;
                r2[j] = (double)v2;
            }
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                const double w = p.w[i * 7 + j];
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    m[o] = m[o] + w * r[o + j];
                    e[o] = e[o] + w * r2[o + j];
                }
            }
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const float mu = (float)m[o], ex = (float)e[o];
            const float mu2 = mu * mu;
            const float var = fabsf(ex - mu2);
            const float sigma = (float)sqrt((double)var);
            const float num = sT[(y + kNqR) * kNqTP + x0 + o + kNqR] - mu, den = sigma + 1.0f;
            sN[y * S + x0 + o] = (float)((double)num / (double)den);
        }
    }
    __syncthreads();

    double acc[kNqMaps][kNqMom];
#pragma unroll
    for (int k = 0; k < kNqMaps; ++k)
#pragma unroll
        for (int m = 0; m < kNqMom; ++m) acc[k][m] = 0.0;
    for (int idx = t; idx < S * S; idx += kNqThreads) {
        const int y = idx / S, x = idx - y * S;
        const int ym = y == 0 ? S - 1 : y - 1, xm = x == 0 ? S - 1 : x - 1, xp = x == S - 1 ? 0 : x + 1;
        const float c = sN[y * S + x];
        // np.roll(block, s, axis=(0, 1))[y, x] = block[y - s0, x - s1] (indices modulo the block), s = [0, 1], [1, 0], [1, 1], [1, -1]
        const float v[kNqMaps] = {c, c * sN[y * S + xm], c * sN[ym * S + x], c * sN[ym * S + xm], c * sN[ym * S + xp]};
#pragma unroll
        for (int k = 0; k < kNqMaps; ++k) {
            const float sq = v[k] * v[k];
            if (v[k] < 0.f) {
                acc[k][0] += (double)sq;
                acc[k][4] += 1.0;
            } else if (v[k] > 0.f) {
                acc[k][1] += (double)sq;
                acc[k][5] += 1.0;
            }
            acc[k][2] += (double)fabsf(v[k]);
            acc[k][3] += (double)sq;
        }
    }
#pragma unroll
    for (int k = 0; k < kNqMaps; ++k)
#pragma unroll
        for (int m = 0; m < kNqMom; ++m) {
            double s = acc[k][m];
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d);
            if ((t & 63) == 0) sRed[((t >> 6) * kNqMaps + k) * kNqMom + m] = s;
        }
    __syncthreads();

    if (t < kNqMaps) {
        double s[kNqMom];
#pragma unroll
        for (int m = 0; m < kNqMom; ++m) {
            double w[kNqWaves];
#pragma unroll
            for (int v = 0; v < kNqWaves; ++v) w[v] = sRed[(v * kNqMaps + t) * kNqMom + m];
            s[m] = ((w[0] + w[1]) + (w[2] + w[3])) + ((w[4] + w[5]) + (w[6] + w[7]));
        }
        // estimate_aggd_param; an empty side is 0 / 0 = NaN, as the mean of an empty slice
        const double count = (double)(S * S);
        const double left = sqrt(s[0] / s[4]), right = sqrt(s[1] / s[5]);
        const double mean_abs = s[2] / count, mean_sq = s[3] / count;
        const double gh = left / right;
        const double rhat = (mean_abs * mean_abs) / mean_sq;
        const double gh2 = gh * gh + 1.0;
        const double r = (rhat * (gh * gh * gh + 1.0) * (gh + 1.0)) / (gh2 * gh2);
        const double *rg = p.tab + kNqN;
        int idx = 0;
        if (r == r) {
            int lo = 0, hi = kNqN - 2;   // the last entry of [0, N - 2] that is not above r (0 when there is none)
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (rg[mid] <= r) lo = mid; else hi = mid - 1;
            }
            const double d0 = (rg[lo] - r) * (rg[lo] - r), d1 = (rg[lo + 1] - r) * (rg[lo + 1] - r);
            idx = d1 < d0 ? lo + 1 : lo;
        }
        const double alpha = p.tab[idx], scale = p.tab[2 * kNqN + idx], ratio = p.tab[3 * kNqN + idx];
        const double bl = left * scale, br = right * scale;
        double *o = p.out + ((size_t)img * gridDim.x + blk) * OSS_NIQE_FEATURES + half * (OSS_NIQE_FEATURES / 2);
        if (t == 0) {
            o[0] = alpha;
            o[1] = (bl + br) / 2.0;
        } else {
            o[4 * t - 2] = alpha;
            o[4 * t - 1] = (br - bl) * ratio;
            o[4 * t] = bl;
            o[4 * t + 1] = br;
        }
    }
}

int niqe_features_ok(int C, int H, int W, int crop, int flags, oss_dtype io) {
    if (!io_ok(io)) return 0;
    if ((C != 1 && C != 3) || (flags & ~(OSS_METRIC_QUANTISE | OSS_METRIC_Y))) return 0;
    if (((flags & OSS_METRIC_Y) != 0) != (C == 3)) return 0;   // one plane: the luma of three channels, or the single channel
    if (H <= 0 || W <= 0 || crop < 0) return 0;
    const int64_t Hc = (int64_t)H - 2 * (int64_t)crop, Wc = (int64_t)W - 2 * (int64_t)crop;
    if (Hc < kNqB || Wc < kNqB) return 0;
    return (Hc / kNqB) * (Wc / kNqB) <= 2147483647 ? 1 : 0;   // grid.x
}

template <typename T, bool QUANT, bool LUMA>
static int niqe_launch(const NiqeArgs &p, dim3 grid, hipStream_t s) {
    static LdsGate gate;
    auto kern = oss_niqe_features_kernel<T, QUANT, LUMA>;
    if (const int e = gate.ensure(reinterpret_cast<const void *>(kern), kNqLdsBytes)) return e;
    hipLaunchKernelGGL(kern, grid, dim3(kNqThreads), kNqLdsBytes, s, p);
    return (int)hipGetLastError();
}

int niqe_features(oss_dtype io, const void *a, const double *tables, const double *window, double *out, int B, int C, int H, int W,
                  int64_t asb, int64_t asc, int64_t ars, int crop, int flags, hipStream_t s) {
    if (!niqe_features_ok(C, H, W, crop, flags, io)) return OSS_ERR_SHAPE;
    if (B <= 0 || B > 65535) return OSS_ERR_SHAPE;   // grid.z
    NiqeArgs p;
    p.a = a, p.tab = tables, p.out = out;
    p.nbh = (H - 2 * crop) / kNqB, p.nbw = (W - 2 * crop) / kNqB;
    p.Hb = p.nbh * kNqB, p.Wb = p.nbw * kNqB;
    p.sb = asb, p.sc = asc, p.rs = ars;
    p.a0 = crop * ars + crop;
    for (int k = 0; k < 49; ++k) p.w[k] = window[48 - k];
    const dim3 grid(p.nbh * p.nbw, 2, B);
    return io_dispatch(io, [&](auto tag) {
        using T = typename decltype(tag)::type;
        if (flags & OSS_METRIC_QUANTISE)
            return (flags & OSS_METRIC_Y) ? niqe_launch<T, true, true>(p, grid, s) : niqe_launch<T, true, false>(p, grid, s);
        return (flags & OSS_METRIC_Y) ? niqe_launch<T, false, true>(p, grid, s) : niqe_launch<T, false, false>(p, grid, s);
    });
}

}  // namespace oss
