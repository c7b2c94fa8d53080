// oss_metrics.hip -- the reference's validation metrics, PSNR and SSIM, of a batch of image pairs in ONE call on the device.
//
// What the reference computes on the host, one image at a time, after tensor2img (SRGAN/VmambaIR/utils/img_util.py:68-92):
//   calculate_psnr  Deraining/basicsr/metrics/psnr_ssim.py:9-63      mean squared error of the cropped (Y or BGR) planes
//   _ssim           psnr_ssim.py:66-99, Deraining/Deraining/utils.py:58-78   11 x 11 Gaussian window (sigma 1.5), float64, only
//                   windows that lie inside the cropped plane ("valid")
//   _ssim_cly       psnr_ssim.py:184-222                             the same with cv2.BORDER_REPLICATE: every pixel is a centre
//   to_y_channel    metrics/metric_util.py:34-47 + utils/matlab_functions.py:207-238     BT.601 luma, float32 result
// Here a, b are the network's own (batch, 1 | 3, H, W) RGB tensors (fp32 / fp16 / bf16, any batch / channel / row stride, column
// stride 1) and every pixel is converted on load: [clamp to [0, 1], * 255, round half to even -- tensor2img's arithmetic in
// fp32], [luma: / 255 in fp32, the three products and sums in fp64 with contraction off, + 16, / 255, cast to fp32, * 255 in
// fp32].  Integers <= 255 and fp32 luma values are exact in the fp32 LDS tiles.
//
// A workgroup (256 threads) owns a 16 x 32 tile of window centres of one plane:
//   1. the 26 x 42 halo tile of both images goes into LDS as fp32 (coordinates clamped to the cropped plane: that IS the replicate
//      border, and in valid mode it only keeps the loads of masked-out centres in bounds).  The same pass adds up the squared
//      difference of the pixels the tile OWNS (its centres; the edge tiles of valid mode also own the 5-pixel frame), so that
//      every cropped pixel is counted once: without luma an fp64 sum of exact squares, with luma the difference and the square
//      in fp32 and the sum in fp64, as metrics.calculate_psnr has it;
//   2. row pass: 208 threads filter 4 adjacent columns of one halo row each -- 14 pixels of a and b, the five moments a, b, a^2,
//      b^2, ab formed in fp64 (exact), 11 taps each by fp64 FMA -- into a 5 x 26 x 32 fp64 LDS image;
//   3. column pass: a thread owns 2 vertically adjacent centres of one column: 12 fp64 reads and 22 FMAs per moment, then the SSIM
//      quotient exactly as the reference writes it (contraction off);
//   4. (sse, ssim sum) are reduced in a fixed order (wave shuffles, then the four waves) and written as one pair of doubles per
//      workgroup.  oss_image_metrics_finish_kernel adds an image's pairs in a fixed order -- thread t takes partials t, t + 1024,
//      ..., then a fixed tree -- and writes mse and mean SSIM.  No atomics: reruns are bit-identical.
// The separable fp64 form agrees with the reference's 2-D window to 2e-14; an fp32 form does not survive E[x^2] - mu^2 on a smooth
// image (8.7e-7).  The kernel's time is fp64 arithmetic -- 55 (1 + 26 / 16) = 144 FMAs per centre and plane, the correctly rounded
// divisions of the luma conversion and of the quotient -- against 2 x 2.1 element loads: it reads at 3-6 % of the HBM peak (scalar
// loads on purpose: the cropped origin of a sliced view has no alignment to build 16-byte loads on, and the halo re-reads hit L2).
//
// hipcc -Rpass-analysis=kernel-resource-usage, gfx950, all twelve instantiations of oss_image_metrics_kernel alike: 132 VGPRs,
// 48 SGPRs (71-73 with luma), no scratch, 42,496 bytes of LDS (halo tiles 2 x 4,576, row-pass image 33,280, reduction 64) -> three
// workgroups = 12 waves per CU, 3 per SIMD, which is also what 132 VGPRs admit; oss_image_metrics_finish_kernel (1024 threads): 14 VGPRs,
// 24 SGPRs, 16 KiB of LDS, no scratch.  Timings: profiles/metrics_kernel_timing.txt.
#include <cmath>
#include "oss_device.h"
#include "oss_host.h"
#include "oss_metric_load.h"

namespace oss {

constexpr int kMetTH = 16, kMetTW = 32, kMetR = 5;                    // centre tile, window radius
constexpr int kMetHH = kMetTH + 2 * kMetR, kMetHW = kMetTW + 2 * kMetR;   // halo tile 26 x 42
constexpr int kMetHP = 44;                                            // halo row pitch (floats): 16-byte rows

struct MetricArgs {
    const void *a, *b;
    double *part;
    int Hc, Wc, Ho, Wo;      // cropped plane, centre domain (valid: Hc - 10, Wc - 10; replicate: Hc, Wc)
    int off, K;              // first centre (5 | 0), planes per image (3 channels, or 1: grey or luma)
    int64_t asb, asc, ars, bsb, bsc, brs;
    int64_t a0, b0;          // element offset of the cropped origin inside a plane
    double g[11], c1, c2;
};

// psnr_ssim.py:89-98 term by term
__device__ __forceinline__ double metric_ssim(double mu1, double mu2, double e11, double e22, double e12, double c1, double c2) {
#pragma clang fp contract(off)
    const double m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
    const double s1 = e11 - m11, s2 = e22 - m22, s12 = e12 - m12;
    return ((2.0 * m12 + c1) * (2.0 * s12 + c2)) / ((m11 + m22 + c1) * (s1 + s2 + c2));
}

// grid (centre tiles along x, along y, batch * K)
template <typename T, bool QUANT, bool LUMA>
__global__ void __launch_bounds__(256)
oss_image_metrics_kernel(const MetricArgs p) {
    __shared__ __attribute__((aligned(16))) float sA[kMetHH][kMetHP];
    __shared__ __attribute__((aligned(16))) float sB[kMetHH][kMetHP];
    __shared__ __attribute__((aligned(16))) double sR[5][kMetHH][kMetTW];
    __shared__ double sRed[2][4];
    const int t = threadIdx.x;
    const int img = blockIdx.z / p.K, k = blockIdx.z - img * p.K;
    const int ty0 = blockIdx.y * kMetTH, tx0 = blockIdx.x * kMetTW;
    const T *pa = reinterpret_cast<const T *>(p.a) + img * p.asb + k * p.asc + p.a0;
    const T *pb = reinterpret_cast<const T *>(p.b) + img * p.bsb + k * p.bsc + p.b0;
    // the pixels whose squared difference this tile adds up, in cropped coordinates
    const int oy0 = blockIdx.y == 0 ? 0 : ty0 + p.off, oy1 = blockIdx.y == gridDim.y - 1 ? p.Hc : ty0 + p.off + kMetTH;
    const int ox0 = blockIdx.x == 0 ? 0 : tx0 + p.off, ox1 = blockIdx.x == gridDim.x - 1 ? p.Wc : tx0 + p.off + kMetTW;

    double sse = 0.0;
    for (int idx = t; idx < kMetHH * kMetHW; idx += 256) {
        const int i = idx / kMetHW, j = idx - i * kMetHW;
        const int uy = ty0 + p.off + i - kMetR, ux = tx0 + p.off + j - kMetR;
        const int cy = min(max(uy, 0), p.Hc - 1), cx = min(max(ux, 0), p.Wc - 1);
        const float va = metric_pixel<T, QUANT, LUMA>(pa + cy * p.ars + cx, p.asc);
        const float vb = metric_pixel<T, QUANT, LUMA>(pb + cy * p.brs + cx, p.bsc);
        sA[i][j] = va;
        sB[i][j] = vb;
        if (uy >= oy0 && uy < oy1 && ux >= ox0 && ux < ox1) {
            if (LUMA) {
                const float d = va - vb;
                const float sq = d * d;
                sse += (double)sq;
            } else {
                const double d = (double)va - (double)vb;
                sse += d * d;
            }
        }
    }
    __syncthreads();

    if (t < kMetHH * (kMetTW / 4)) {
        const int r = t >> 3, q = (t & 7) << 2;
        double acc[5][4];
#pragma unroll
        for (int m = 0; m < 5; ++m)
#pragma unroll
            for (int o = 0; o < 4; ++o) acc[m][o] = 0.0;
#pragma unroll
        for (int j = 0; j < 14; ++j) {
            const double da = (double)sA[r][q + j], db = (double)sB[r][q + j];
            const double v[5] = {da, db, da * da, db * db, da * db};
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const int tap = j - o;
                if (tap >= 0 && tap <= 2 * kMetR) {
#pragma unroll
                    for (int m = 0; m < 5; ++m) acc[m][o] = __builtin_fma(p.g[tap], v[m], acc[m][o]);
                }
            }
        }
#pragma unroll
        for (int m = 0; m < 5; ++m)
#pragma unroll
            for (int o = 0; o < 4; ++o) sR[m][r][q + o] = acc[m][o];
    }
    __syncthreads();

    const int x = t & 31, y2 = (t >> 5) << 1;
    double e[5][2];
#pragma unroll
    for (int m = 0; m < 5; ++m) {
        double e0 = 0.0, e1 = 0.0;
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            const double v = sR[m][y2 + j][x];
            if (j <= 10) e0 = __builtin_fma(p.g[j], v, e0);
            if (j >= 1) e1 = __builtin_fma(p.g[j - 1], v, e1);
        }
        e[m][0] = e0;
        e[m][1] = e1;
    }
    double ssim = 0.0;
    if (tx0 + x < p.Wo) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (ty0 + y2 + i < p.Ho) ssim += metric_ssim(e[0][i], e[1][i], e[2][i], e[3][i], e[4][i], p.c1, p.c2);
    }

#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        sse += __shfl_down(sse, d);
        ssim += __shfl_down(ssim, d);
    }
    if ((t & 63) == 0) {
        sRed[0][t >> 6] = sse;
        sRed[1][t >> 6] = ssim;
    }
    __syncthreads();
    if (t == 0) {
        const size_t wg = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        p.part[2 * wg] = (sRed[0][0] + sRed[0][1]) + (sRed[0][2] + sRed[0][3]);
        p.part[2 * wg + 1] = (sRed[1][0] + sRed[1][1]) + (sRed[1][2] + sRed[1][3]);
    }
}

// grid (batch), 1024 threads (a 2048 x 2048 RGB pair has 24,576 pairs: 24 dependent steps per thread instead of 96):
// out[b] = (sum sse / pixels, sum ssim / windows) over the n workgroup pairs of image b
constexpr int kMetFinish = 1024;
__global__ void __launch_bounds__(kMetFinish)
oss_image_metrics_finish_kernel(const double *__restrict__ part, double *__restrict__ out, size_t n, double pixels, double windows) {
    __shared__ double s[2][kMetFinish];
    const int t = threadIdx.x;
    const double *p = part + 2 * n * blockIdx.x;
    double a0 = 0.0, a1 = 0.0;
    for (size_t i = t; i < n; i += kMetFinish) {
        a0 += p[2 * i];
        a1 += p[2 * i + 1];
    }
    s[0][t] = a0;
    s[1][t] = a1;
    __syncthreads();
    for (int w = kMetFinish / 2; w > 0; w >>= 1) {
        if (t < w) {
            s[0][t] += s[0][t + w];
            s[1][t] += s[1][t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        out[2 * blockIdx.x] = s[0][0] / pixels;
        out[2 * blockIdx.x + 1] = s[1][0] / windows;
    }
}

static inline int met_tiles(int n, int tile) { return (n + tile - 1) / tile; }

int image_metrics_ok(oss_dtype io, int C, int H, int W, int crop, int flags) {
    if (!io_ok(io)) return 0;
    if ((C != 1 && C != 3) || (flags & ~(OSS_METRIC_QUANTISE | OSS_METRIC_Y | OSS_METRIC_REPLICATE))) return 0;
    if ((flags & OSS_METRIC_Y) && C != 3) return 0;
    if (H <= 0 || W <= 0 || crop < 0 || 2 * (int64_t)crop >= H || 2 * (int64_t)crop >= W) return 0;
    const int Hc = H - 2 * crop, Wc = W - 2 * crop;
    if (!(flags & OSS_METRIC_REPLICATE) && (Hc < 2 * kMetR + 1 || Wc < 2 * kMetR + 1)) return 0;
    return met_tiles(Hc, kMetTH) <= 65535;   // grid.y; grid.x is below 2^31 for every int width
}

// sized for the larger grid of the two border modes and for 3 planes: the query does not know the flags
size_t image_metrics_partial_doubles(int B, int C, int H, int W, int crop) {
    if (B <= 0 || !image_metrics_ok(OSS_F32, C, H, W, crop, OSS_METRIC_REPLICATE)) return 0;
    return (size_t)2 * B * C * met_tiles(H - 2 * crop, kMetTH) * met_tiles(W - 2 * crop, kMetTW);
}

template <typename T>
static void met_launch(const MetricArgs &p, int flags, dim3 grid, hipStream_t s) {
#define OSS_MET(Q_, L_) hipLaunchKernelGGL((oss_image_metrics_kernel<T, Q_, L_>), grid, dim3(256), 0, s, p)
    if (flags & OSS_METRIC_QUANTISE) { if (flags & OSS_METRIC_Y) OSS_MET(true, true); else OSS_MET(true, false); }
    else { if (flags & OSS_METRIC_Y) OSS_MET(false, true); else OSS_MET(false, false); }
#undef OSS_MET
}

int image_metrics(oss_dtype io, const void *a, const void *b, double *out, double *part, int B, int C, int H, int W, int64_t asb,
                  int64_t asc, int64_t ars, int64_t bsb, int64_t bsc, int64_t brs, int crop, int flags, hipStream_t s) {
    if (!image_metrics_ok(io, C, H, W, crop, flags)) return OSS_ERR_SHAPE;
    const int K = (flags & OSS_METRIC_Y) ? 1 : C;
    if (B <= 0 || (int64_t)B * K > 65535) return OSS_ERR_SHAPE;   // grid.z
    MetricArgs p;
    p.a = a, p.b = b, p.part = part;
    p.Hc = H - 2 * crop, p.Wc = W - 2 * crop;
    p.off = (flags & OSS_METRIC_REPLICATE) ? 0 : kMetR;
    p.Ho = p.Hc - 2 * p.off, p.Wo = p.Wc - 2 * p.off;
    p.K = K;
    p.asb = asb, p.asc = asc, p.ars = ars, p.bsb = bsb, p.bsc = bsc, p.brs = brs;
    p.a0 = crop * ars + crop, p.b0 = crop * brs + crop;
    // cv2.getGaussianKernel(11, 1.5)
    double sum = 0.0;
    for (int i = 0; i <= 2 * kMetR; ++i) {
        p.g[i] = std::exp(-(double)((i - kMetR) * (i - kMetR)) / (2.0 * 1.5 * 1.5));
        sum += p.g[i];
    }
    for (int i = 0; i <= 2 * kMetR; ++i) p.g[i] /= sum;
    p.c1 = (0.01 * 255) * (0.01 * 255), p.c2 = (0.03 * 255) * (0.03 * 255);
    const dim3 grid(met_tiles(p.Wo, kMetTW), met_tiles(p.Ho, kMetTH), B * K);
    const int e = io_dispatch(io, [&](auto tag) {
        met_launch<typename decltype(tag)::type>(p, flags, grid, s);
        return (int)hipGetLastError();
    });
    if (e != 0) return e;
    const double pixels = (double)K * p.Hc * p.Wc, windows = (double)K * p.Ho * p.Wo;
    hipLaunchKernelGGL(oss_image_metrics_finish_kernel, dim3(B), dim3(kMetFinish), 0, s, part, out, (size_t)K * grid.x * grid.y, pixels, windows);
    return (int)hipGetLastError();
}

}  // namespace oss
