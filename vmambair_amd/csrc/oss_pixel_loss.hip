// oss_pixel_loss.hip -- the reference's pixel losses with their gradients on the device: L1Loss, MSELoss, PSNRLoss (with toY) and
// CharbonnierLoss of Deraining/basicsr/models/losses/losses.py:26-122 with the weighting and reduction of loss_util.py:25-95.
//
// pred (N, C, H, W) dense in fp32 / fp16 / bf16, target of the same shape in fp32 or pred's type, an optional fp32 weight of
// (N, C, H, W) or (N, 1, H, W).  Every element is widened to fp32; d = p - t and the per-element term (|d|, d^2, sqrt(d^2 + eps^2),
// term * w) are fp32; every sum is fp64.
//
// Forward, two launches:
//   1. oss_pixel_loss_partial_kernel: the tensor is cut into ROWS of `len` elements -- one row for L1 / MSE / Charbonnier (the
//      whole tensor), one row per image for PSNR (its C H W elements, or with toY its H W pixels: a lane then reads the three
//      channel planes of a pixel and forms dy = (k0 d0 + k1 d1 + k2 d2) / 255, k = the fp32 values of 65.481, 128.553, 24.966; the
//      + 16 cancels).  A workgroup (256 threads) owns 2048 consecutive elements of ONE row, a lane 8 consecutive ones: 16-byte
//      loads where a lane's run is whole and its address aligned (an image need not start on 16 bytes), element-wise loads with a
//      mask otherwise.  Lane sums in fp64, then the metrics kernel's fixed reduction (wave shuffles, then the four waves): one
//      double per workgroup, or two with a weight (sum of term * w, sum of w).
//   2. oss_pixel_loss_finish_kernel (one workgroup of 1024 threads): adds the partials in a fixed order -- thread t takes t,
//      t + 1024, ..., then a fixed tree; for PSNR wave v takes images v, v + 16, ... (lane l the image's partials l, l + 64, ...,
//      then shuffles), writes mse_b and adds ln(mse_b + 1e-8), the sixteen wave sums are added in order -- and writes the loss,
//      rounded ONCE from the fp64 result, and the fp64 `stats` the backward needs (the denominator, or mse_b per image).
// No atomics, no host read-back: reruns are bit-identical and every launch can be captured into a hipGraph.
//
// Backward, one launch (oss_pixel_loss_bwd_kernel, the forward's geometry without the reduction): a lane forms its row's factor
// s = grad_output * loss_weight / den  (PSNR: grad_output * loss_weight * (10 / ln 10) / (N len (mse_b + 1e-8))) in fp64 once,
// rounds it to fp32 and writes sign(d) s / 2 d s / d s / sqrt(d^2 + eps^2) [* w] in fp32, rounded once to pred's type.
//
// hipcc -Rpass-analysis=kernel-resource-usage, gfx950: no instantiation uses scratch or spills (figures in DESIGN.md 4.4).
#include <cmath>
#include <type_traits>
#include "oss_device.h"
#include "oss_host.h"

namespace oss {

constexpr int kLossThreads = 256, kLossItems = 8;
constexpr int64_t kLossChunk = (int64_t)kLossThreads * kLossItems;   // elements of one row per workgroup
constexpr int kLossFinish = 1024;
constexpr double kPsnrScale = 4.342944819032518;   // 10 / ln 10 (losses.py:90)
constexpr double kPsnrEps = 1e-8;                  // losses.py:109

// what a lane reads next to pred and target
enum LossForm { LOSS_PLAIN = 0, LOSS_WEIGHT = 1, LOSS_WEIGHT_1CH = 2, LOSS_TOY = 3 };
// what the finishing launch divides by
enum LossMode { LOSS_MODE_SUM = 0, LOSS_MODE_MEAN = 1, LOSS_MODE_WMEAN = 2, LOSS_MODE_PSNR = 3 };

struct LossArgs {
    const void *pred, *target;
    const float *weight;
    double *part;               // forward: out
    const double *stats;        // backward: in
    const float *grad_output;   // backward: in
    void *dpred;                // backward: out
    int64_t len;                // elements per row (toY: pixels)
    int64_t plane, cp;          // H W, C H W
    unsigned chunks;            // workgroups per row
    int kind, mode;
    float eps2;                 // Charbonnier: eps * eps
    double coef;                // backward: loss_weight (PSNR: loss_weight * (10 / ln 10) / (N len))
};

__device__ __forceinline__ float loss_luma(float r, float g, float b) {
#pragma clang fp contract(off)
    return (65.481f * r + 128.553f * g + 24.966f * b) / 255.0f;
}

// the 8 differences of a lane (toY: of the luma) and, with a weight, the 8 weights; elements past `valid` read as 0
template <typename TP, typename TT, int FORM>
__device__ __forceinline__ void loss_load(const LossArgs &p, unsigned row, int64_t e0, int valid, float (&d)[kLossItems],
                                          float (&w)[kLossItems], float (&dc)[3][kLossItems]) {
    const TP *pp = reinterpret_cast<const TP *>(p.pred);
    const TT *pt = reinterpret_cast<const TT *>(p.target);
    if constexpr (FORM == LOSS_TOY) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int64_t base = ((int64_t)row * 3 + c) * p.plane + e0;
            float a[kLossItems], b[kLossItems];
            load_items<kLossItems>(pp + base, valid, valid == kLossItems && aligned16(pp + base), a);
            load_items<kLossItems>(pt + base, valid, valid == kLossItems && aligned16(pt + base), b);
#pragma unroll
            for (int i = 0; i < kLossItems; ++i) dc[c][i] = a[i] - b[i];
        }
#pragma unroll
        for (int i = 0; i < kLossItems; ++i) d[i] = loss_luma(dc[0][i], dc[1][i], dc[2][i]);
    } else {
        const int64_t base = (int64_t)row * p.len + e0;
        float a[kLossItems], b[kLossItems];
        load_items<kLossItems>(pp + base, valid, valid == kLossItems && aligned16(pp + base), a);
        load_items<kLossItems>(pt + base, valid, valid == kLossItems && aligned16(pt + base), b);
#pragma unroll
        for (int i = 0; i < kLossItems; ++i) d[i] = a[i] - b[i];
        if constexpr (FORM == LOSS_WEIGHT) {
            load_items<kLossItems>(p.weight + base, valid, valid == kLossItems && aligned16(p.weight + base), w);
        } else if constexpr (FORM == LOSS_WEIGHT_1CH) {
            // (N, 1, H, W) broadcast over the channels: element (b, c, q) reads weight (b, q)
            const int64_t img = base / p.cp, q0 = (base - img * p.cp) % p.plane;
            if (q0 + valid <= p.plane) {   // the lane's run stays inside one plane
                const float *pw = p.weight + img * p.plane + q0;
                load_items<kLossItems>(pw, valid, valid == kLossItems && aligned16(pw), w);
            } else {
#pragma unroll
                for (int i = 0; i < kLossItems; ++i) {
                    const int64_t e = base + i, b2 = e / p.cp;
                    w[i] = i < valid ? p.weight[b2 * p.plane + (e - b2 * p.cp) % p.plane] : 0.f;
                }
            }
        }
    }
}

__device__ __forceinline__ float loss_term(int kind, float d, float eps2) {
#pragma clang fp contract(off)
    if (kind == OSS_LOSS_L1) return __builtin_fabsf(d);
    if (kind == OSS_LOSS_CHARBONNIER) return __builtin_sqrtf(d * d + eps2);
    return d * d;
}

// d term / d d up to the row's factor
__device__ __forceinline__ float loss_slope(int kind, float d, float eps2) {
#pragma clang fp contract(off)
    if (kind == OSS_LOSS_L1) return (float)(d > 0.f) - (float)(d < 0.f);   // sign(0) = 0, as torch
    if (kind == OSS_LOSS_CHARBONNIER) return d / __builtin_sqrtf(d * d + eps2);
    return 2.0f * d;
}

// grid (rows * chunks)
template <typename TP, typename TT, int FORM>
__global__ void __launch_bounds__(kLossThreads)
oss_pixel_loss_partial_kernel(const LossArgs p) {
    constexpr bool WEIGHTED = FORM == LOSS_WEIGHT || FORM == LOSS_WEIGHT_1CH;
    __shared__ double sRed[2][4];
    const int t = threadIdx.x;
    const unsigned row = blockIdx.x / p.chunks, c = blockIdx.x - row * p.chunks;
    const int64_t e0 = (int64_t)c * kLossChunk + (int64_t)t * kLossItems;
    const int64_t left = p.len - e0;
    const int valid = left >= kLossItems ? kLossItems : (left > 0 ? (int)left : 0);

    double sum = 0.0, wsum = 0.0;
    if (valid > 0) {
        float d[kLossItems], w[kLossItems], dc[3][kLossItems];
        loss_load<TP, TT, FORM>(p, row, e0, valid, d, w, dc);
#pragma unroll
        for (int i = 0; i < kLossItems; ++i) {
            if (i < valid) {
                float term = loss_term(p.kind, d[i], p.eps2);
                if constexpr (WEIGHTED) {
                    term = term * w[i];
                    wsum += (double)w[i];
                }
                sum += (double)term;
            }
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        sum += __shfl_down(sum, s);
        if constexpr (WEIGHTED) wsum += __shfl_down(wsum, s);
    }
    if ((t & 63) == 0) {
        sRed[0][t >> 6] = sum;
        sRed[1][t >> 6] = wsum;
    }
    __syncthreads();
    if (t == 0) {
        const double a = (sRed[0][0] + sRed[0][1]) + (sRed[0][2] + sRed[0][3]);
        if constexpr (WEIGHTED) {
            p.part[2 * (size_t)blockIdx.x] = a;
            p.part[2 * (size_t)blockIdx.x + 1] = (sRed[1][0] + sRed[1][1]) + (sRed[1][2] + sRed[1][3]);
        } else {
            p.part[blockIdx.x] = a;
        }
    }
}

// one workgroup.  n = partials per row (pairs with a weight), den = elements of the mean (WMEAN: the factor of sum w)
__global__ void __launch_bounds__(kLossFinish)
oss_pixel_loss_finish_kernel(const double *__restrict__ part, float *__restrict__ loss, double *__restrict__ stats, int mode, int pairs,
                             size_t rows, size_t n, double den, double loss_weight) {
    __shared__ double s[2][kLossFinish];
    const int t = threadIdx.x;
    if (mode == LOSS_MODE_PSNR) {
        const int lane = t & 63, wave = t >> 6;
        double logs = 0.0;
        for (size_t b = wave; b < rows; b += kLossFinish / 64) {
            const double *p = part + b * n;
            double a = 0.0;
            for (size_t i = lane; i < n; i += 64) a += p[i];
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) a += __shfl_down(a, d);
            if (lane == 0) {
                const double mse = a / den;
                stats[b] = mse;
                logs += log(mse + kPsnrEps);
            }
        }
        if (lane == 0) s[0][wave] = logs;
        __syncthreads();
        if (t == 0) {
            double a = 0.0;
            for (int v = 0; v < kLossFinish / 64; ++v) a += s[0][v];
            *loss = (float)(loss_weight * kPsnrScale * (a / (double)rows));
        }
        return;
    }
    double a0 = 0.0, a1 = 0.0;
    if (pairs) {
        for (size_t i = t; i < n; i += kLossFinish) {
            a0 += part[2 * i];
            a1 += part[2 * i + 1];
        }
    } else {
        for (size_t i = t; i < n; i += kLossFinish) a0 += part[i];
    }
    s[0][t] = a0;
    s[1][t] = a1;
    __syncthreads();
    for (int w = kLossFinish / 2; w > 0; w >>= 1) {
        if (t < w) {
            s[0][t] += s[0][t + w];
            s[1][t] += s[1][t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        const double d = mode == LOSS_MODE_SUM ? 1.0 : (mode == LOSS_MODE_WMEAN ? s[1][0] * den : den);
        stats[0] = d;
        *loss = (float)(loss_weight * s[0][0] / d);
    }
}

// grid (rows * chunks)
template <typename TP, typename TT, int FORM>
__global__ void __launch_bounds__(kLossThreads)
oss_pixel_loss_bwd_kernel(const LossArgs p) {
    constexpr bool WEIGHTED = FORM == LOSS_WEIGHT || FORM == LOSS_WEIGHT_1CH;
    const int t = threadIdx.x;
    const unsigned row = blockIdx.x / p.chunks, c = blockIdx.x - row * p.chunks;
    const int64_t e0 = (int64_t)c * kLossChunk + (int64_t)t * kLossItems;
    const int64_t left = p.len - e0;
    const int valid = left >= kLossItems ? kLossItems : (left > 0 ? (int)left : 0);
    if (valid <= 0) return;
    const double g = (double)*p.grad_output * p.coef;
    const float s = (float)(p.mode == LOSS_MODE_PSNR ? g / (p.stats[row] + kPsnrEps) : g / p.stats[0]);

    float d[kLossItems], w[kLossItems], dc[3][kLossItems];
    loss_load<TP, TT, FORM>(p, row, e0, valid, d, w, dc);
    TP *out = reinterpret_cast<TP *>(p.dpred);
    float o[kLossItems];
    if constexpr (FORM == LOSS_TOY) {
        const float k[3] = {65.481f / 255.0f, 128.553f / 255.0f, 24.966f / 255.0f};
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
            for (int i = 0; i < kLossItems; ++i) o[i] = (2.0f * d[i]) * (s * k[ch]);
            TP *q = out + ((int64_t)row * 3 + ch) * p.plane + e0;
            store_items<kLossItems>(q, valid, valid == kLossItems && aligned16(q), o);
        }
    } else {
#pragma unroll
        for (int i = 0; i < kLossItems; ++i) {
            float v = loss_slope(p.kind, d[i], p.eps2) * s;
            if constexpr (WEIGHTED) v = v * w[i];
            o[i] = v;
        }
        TP *q = out + (int64_t)row * p.len + e0;
        store_items<kLossItems>(q, valid, valid == kLossItems && aligned16(q), o);
    }
}

// the launch geometry of a (kind, flags, shape) the kernels take; false: not taken
struct LossPlan {
    int form, mode;
    int64_t rows, len;
    unsigned chunks;
    double den;
};

static bool loss_plan(int kind, int flags, int64_t N, int64_t C, int64_t plane, LossPlan &pl) {
    if (kind < OSS_LOSS_L1 || kind > OSS_LOSS_PSNR) return false;
    if (flags & ~(OSS_LOSS_SUM | OSS_LOSS_TOY | OSS_LOSS_WEIGHT | OSS_LOSS_WEIGHT_1CH)) return false;
    if (N <= 0 || C <= 0 || plane <= 0) return false;
    const int64_t lim = (int64_t)1 << 40;   // elements: far past any device memory, and every product below stays in 64 bits
    if (N > lim || C > lim || plane > lim || C * plane > lim || N > lim / (C * plane)) return false;
    const bool elementwise = kind == OSS_LOSS_L1 || kind == OSS_LOSS_MSE;
    const int wbits = flags & (OSS_LOSS_WEIGHT | OSS_LOSS_WEIGHT_1CH);
    if (wbits == (OSS_LOSS_WEIGHT | OSS_LOSS_WEIGHT_1CH)) return false;
    if (!elementwise && (wbits || (flags & OSS_LOSS_SUM))) return false;   // losses.py:95, :118: no weight, one reduction
    if ((flags & OSS_LOSS_TOY) && (kind != OSS_LOSS_PSNR || C != 3)) return false;
    const int64_t n = N * C * plane;
    if (kind == OSS_LOSS_PSNR) {
        pl.form = (flags & OSS_LOSS_TOY) ? LOSS_TOY : LOSS_PLAIN;
        pl.mode = LOSS_MODE_PSNR;
        pl.rows = N;
        pl.len = (flags & OSS_LOSS_TOY) ? plane : C * plane;
        pl.den = (double)pl.len;
    } else {
        pl.form = wbits == OSS_LOSS_WEIGHT ? LOSS_WEIGHT : (wbits ? LOSS_WEIGHT_1CH : LOSS_PLAIN);
        pl.mode = (flags & OSS_LOSS_SUM) ? LOSS_MODE_SUM : (wbits ? LOSS_MODE_WMEAN : LOSS_MODE_MEAN);
        pl.rows = 1;
        pl.len = n;
        // loss_util.py:48-51: sum w, or C sum w for a one-channel weight -- which is what the per-ELEMENT sum of the broadcast weight is
        pl.den = pl.mode == LOSS_MODE_WMEAN ? 1.0 : (double)n;
    }
    const int64_t chunks = (pl.len + kLossChunk - 1) / kLossChunk;
    if (chunks * pl.rows > 0x7fffffff) return false;   // grid.x
    pl.chunks = (unsigned)chunks;
    return true;
}

static bool loss_types_ok(oss_dtype pred_io, oss_dtype target_io) {
    return io_ok(pred_io) && io_ok(target_io) && (target_io == pred_io || target_io == OSS_F32);
}

size_t pixel_loss_partial_doubles(int kind, int flags, oss_dtype pred_io, oss_dtype target_io, int64_t N, int64_t C, int64_t plane) {
    LossPlan pl;
    if (!loss_types_ok(pred_io, target_io) || !loss_plan(kind, flags, N, C, plane, pl)) return 0;
    return (size_t)pl.rows * pl.chunks * (pl.form == LOSS_WEIGHT || pl.form == LOSS_WEIGHT_1CH ? 2 : 1);
}

size_t pixel_loss_stat_doubles(int kind, int flags, int64_t N, int64_t C, int64_t plane) {
    LossPlan pl;
    if (!loss_plan(kind, flags, N, C, plane, pl)) return 0;
    return kind == OSS_LOSS_PSNR ? (size_t)N : 1;
}

template <bool BWD, typename TP, typename TT>
static int loss_launch(const LossArgs &p, int form, unsigned grid, hipStream_t s) {
#define OSS_LOSS_GO(F_)                                                                                                        \
    do {                                                                                                                       \
        if constexpr (BWD) hipLaunchKernelGGL((oss_pixel_loss_bwd_kernel<TP, TT, F_>), dim3(grid), dim3(kLossThreads), 0, s, p); \
        else hipLaunchKernelGGL((oss_pixel_loss_partial_kernel<TP, TT, F_>), dim3(grid), dim3(kLossThreads), 0, s, p);          \
    } while (0)
    switch (form) {
        case LOSS_PLAIN: OSS_LOSS_GO(LOSS_PLAIN); break;
        case LOSS_WEIGHT: OSS_LOSS_GO(LOSS_WEIGHT); break;
        case LOSS_WEIGHT_1CH: OSS_LOSS_GO(LOSS_WEIGHT_1CH); break;
        default: OSS_LOSS_GO(LOSS_TOY); break;
    }
#undef OSS_LOSS_GO
    return (int)hipGetLastError();
}

// both element types through the one decoder; target: pred's type or fp32
template <bool BWD>
static int loss_dispatch(oss_dtype pred_io, oss_dtype target_io, const LossArgs &p, int form, unsigned grid, hipStream_t s) {
    return io_dispatch(pred_io, [&](auto ptag) {
        using TP = typename decltype(ptag)::type;
        return io_dispatch(target_io, [&](auto ttag) {
            using TT = typename decltype(ttag)::type;
            if constexpr (std::is_same<TT, TP>::value || std::is_same<TT, float>::value) return loss_launch<BWD, TP, TT>(p, form, grid, s);
            else return (int)OSS_ERR_SHAPE;
        });
    });
}

static void loss_fill(LossArgs &p, const LossPlan &pl, int kind, int64_t C, int64_t plane, float eps) {
    p.len = pl.len;
    p.plane = plane;
    p.cp = C * plane;
    p.chunks = pl.chunks;
    p.kind = kind == OSS_LOSS_PSNR ? OSS_LOSS_MSE : kind;
    p.mode = pl.mode;
    p.eps2 = eps * eps;
}

int pixel_loss_fwd(int kind, int flags, oss_dtype pred_io, oss_dtype target_io, const void *pred, const void *target, const float *weight,
                   float *loss, double *stats, double *part, int64_t N, int64_t C, int64_t plane, float loss_weight, float eps,
                   hipStream_t s) {
    LossPlan pl;
    if (!loss_types_ok(pred_io, target_io) || !loss_plan(kind, flags, N, C, plane, pl)) return OSS_ERR_SHAPE;
    LossArgs p = {};
    p.pred = pred, p.target = target, p.weight = weight, p.part = part;
    loss_fill(p, pl, kind, C, plane, eps);
    const int e = loss_dispatch<false>(pred_io, target_io, p, pl.form, (unsigned)(pl.rows * pl.chunks), s);
    if (e != 0) return e;
    const bool pairs = pl.form == LOSS_WEIGHT || pl.form == LOSS_WEIGHT_1CH;
    const size_t n = pl.mode == LOSS_MODE_PSNR ? (size_t)pl.chunks : (size_t)pl.rows * pl.chunks;
    // the reference's CharbonnierLoss takes loss_weight and uses none (losses.py:114-122)
    const double lw = kind == OSS_LOSS_CHARBONNIER ? 1.0 : (double)loss_weight;
    hipLaunchKernelGGL(oss_pixel_loss_finish_kernel, dim3(1), dim3(kLossFinish), 0, s, part, loss, stats, pl.mode, pairs ? 1 : 0,
                       (size_t)pl.rows, n, pl.den, lw);
    return (int)hipGetLastError();
}

int pixel_loss_bwd(int kind, int flags, oss_dtype pred_io, oss_dtype target_io, const void *pred, const void *target, const float *weight,
                   const double *stats, const float *grad_output, void *dpred, int64_t N, int64_t C, int64_t plane, float loss_weight,
                   float eps, hipStream_t s) {
    LossPlan pl;
    if (!loss_types_ok(pred_io, target_io) || !loss_plan(kind, flags, N, C, plane, pl)) return OSS_ERR_SHAPE;
    LossArgs p = {};
    p.pred = pred, p.target = target, p.weight = weight, p.stats = stats, p.grad_output = grad_output, p.dpred = dpred;
    loss_fill(p, pl, kind, C, plane, eps);
    const double lw = kind == OSS_LOSS_CHARBONNIER ? 1.0 : (double)loss_weight;
    p.coef = pl.mode == LOSS_MODE_PSNR ? lw * kPsnrScale / ((double)N * pl.den) : lw;
    return loss_dispatch<true>(pred_io, target_io, p, pl.form, (unsigned)(pl.rows * pl.chunks), s);
}

}  // namespace oss
