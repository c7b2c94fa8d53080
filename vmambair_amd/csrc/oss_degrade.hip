// oss_degrade.hip -- the two custom operators of the RealSR degradation pipeline (MambaRealSR.feed_data,
// RealSR/VmambaIR/models/MambaRealSR_model.py:146-263) on the device: filter2D (a different blur or sinc kernel per sample after
// reflect padding, :165, :196, :232/245) and USMSharp (:154-155, :262).  fp32 in and out, fp32 accumulation, no allocation, no
// host read-back: every call is a fixed sequence of launches on the caller's stream and can be captured into a hipGraph.
//
// Reflect addressing happens in the load (no padded copy): index v of an axis of n elements reads -v below 0 and 2n - 2 - v from
// n on, and the result is clamped to [0, n - 1].  The host entries refuse n <= k / 2, where one reflection is not enough; the
// clamp keeps every address inside the plane whatever reaches the kernel (ragged tiles read past the plane's end by design and
// discard those outputs).
//
// oss_filter2d_kernel: dense k x k correlation (no flip), k odd <= 21.  A workgroup (256 threads) owns a 32 x 64 output tile of
// one plane.  It first finds the non-zero bounding box of its sample's kernel in LDS (the dataset zero-pads 7...19-tap kernels to
// 21: a zero tap adds +0 to a sum that starts at +0, so leaving it out changes nothing for finite input) and stores the box's
// weights in rows of 24 floats, zero filled.  The input tile plus the box's halo goes to LDS with a row stride of 87 floats (odd: the
// 32 rows a lane group reads fall on 32 banks).  A lane owns 8 consecutive outputs of one row: per kernel row it reads a window of
// JT + 7 floats into registers once and runs JT x 8 fmaf on it, JT = 8 / 16 / 24 chosen per workgroup from the box's width.  The
// results pass through LDS so that the stores are row-contiguous.  Epilogue: none, clamp to [0, 1], or the final quantisation
// clamp(rint(x * 255), 0, 255) / 255 (:248) with round-half-even and the operations of torch's expression on the device.
//
// oss_filter_sep_kernel<COL, MODE>: one pass of a separable correlation with an odd vector g (k <= 63) along the rows (COL = false)
// or the columns of a 64 x 64 tile; a lane owns 2 x 8 consecutive outputs along the filtered axis and walks g in chunks of 8 taps
// (15 window reads per 64 fmaf).  The lanes of a wave lie across the filtered axis, so LDS reads are conflict-free in both
// directions; the row pass stores through LDS.  The column pass carries the two fused stages of USM:
//   SEP_MASK   blur = the sum; residual = img - blur -> out; mask = (|residual| * 255 > threshold) as 0 / 1 -> mask
//   SEP_BLEND  soft = the sum (the blurred mask); sharp = clip(img + weight * residual, 0, 1) with the residual read from out;
//              out = img + soft * (sharp - img), the reference's soft * sharp + (1 - soft) * img in the form that returns img
//              itself where sharp == img (weight 0) or soft == 0 (an empty mask)
// oss_usm_sharp = row pass, column pass SEP_MASK, row pass of the mask, column pass SEP_BLEND: four memory-bound launches,
// 4 k taps per pixel where the dense form has 2 k^2.
#include <cmath>
#include "oss_host.h"
#include "oss_pixel_stage.h"

namespace oss {

__device__ __forceinline__ int reflect_clamp(int v, int n) {
    v = v < 0 ? -v : v;
    v = v >= n ? 2 * n - 2 - v : v;
    return v < 0 ? 0 : (v >= n ? n - 1 : v);
}

// ---- filter2D -------------------------------------------------------------------------------------------------------------------
constexpr int kF2Threads = 256, kF2TileH = 32, kF2TileW = 64, kF2MaxK = 21;
constexpr int kF2WRow = 24;                           // floats per stored kernel row (a multiple of every JT)
constexpr int kF2Stride = kF2TileW + kF2WRow - 1;     // 87: the widest window ends at 56 + 24 + 6
constexpr int kF2Rows = kF2TileH + kF2MaxK - 1;       // 52
constexpr int kOutStride = 65;                        // row stride of a 64-wide output tile in LDS
static_assert(kF2Stride % 2 == 1 && kF2TileH * kOutStride <= kF2Rows * kF2Stride, "LDS tile of oss_filter2d_kernel");

struct F2Args {
    const float *img, *ker;
    float *out;
    int C, H, W, k, tilesX, tilesY, per_sample, epilogue;
};

__device__ __forceinline__ float f2_epilogue(float v, int epilogue) {
    if (epilogue == OSS_FILTER_CLAMP) return clamp_unit(v);
    if (epilogue == OSS_FILTER_QUANTISE) return quantise_255(v);
    return v;
}

template <int JT>
__device__ __forceinline__ void f2_accumulate(const float *sT, const float *sW, int rows, float (&acc)[8]) {
    for (int i = 0; i < rows; ++i) {
        const float *tr = sT + i * kF2Stride, *wr = sW + i * kF2WRow;
        float a[JT + 7];
#pragma unroll
        for (int m = 0; m < JT + 7; ++m) a[m] = tr[m];
#pragma unroll
        for (int j = 0; j < JT; ++j) {
            const float w = wr[j];
#pragma unroll
            for (int o = 0; o < 8; ++o) acc[o] = fmaf(w, a[j + o], acc[o]);
        }
    }
}

// grid (planes * tilesY * tilesX)
__global__ void __launch_bounds__(kF2Threads) oss_filter2d_kernel(const F2Args p) {
    __shared__ float sT[kF2Rows * kF2Stride];
    __shared__ float sW[kF2MaxK * kF2WRow];
    __shared__ int sBox[4];
    const int t = threadIdx.x, k = p.k, pad = k / 2;
    const int bx = blockIdx.x % p.tilesX, by = (blockIdx.x / p.tilesX) % p.tilesY;
    const int64_t plane = blockIdx.x / (p.tilesX * p.tilesY);
    const float *ker = p.ker + (p.per_sample ? (plane / p.C) * k * k : 0);
    const float *img = p.img + plane * p.H * p.W;

    for (int e = t; e < kF2MaxK * kF2WRow; e += kF2Threads) sW[e] = 0.0f;
    if (t < 4) sBox[t] = t < 2 ? k : -1;
    __syncthreads();
    for (int e = t; e < k * k; e += kF2Threads)
        if (ker[e] != 0.0f) {   // a NaN tap counts
            const int i = e / k, j = e - i * k;
            atomicMin(&sBox[0], i), atomicMin(&sBox[1], j), atomicMax(&sBox[2], i), atomicMax(&sBox[3], j);
        }
    __syncthreads();
    int i0 = sBox[0], j0 = sBox[1], rows = sBox[2] - i0 + 1, cols = sBox[3] - j0 + 1;
    if (rows <= 0) i0 = j0 = rows = cols = 0;   // a kernel of zeros: the output is 0

    for (int e = t; e < rows * cols; e += kF2Threads) {
        const int i = e / cols, j = e - i * cols;
        sW[i * kF2WRow + j] = ker[(i0 + i) * k + j0 + j];
    }
    // the tile: rows by*32 - pad + i0 ..., columns bx*64 - pad + j0 ...; columns past the box's halo are zeros under zero weights
    const int gy0 = by * kF2TileH - pad + i0, gx0 = bx * kF2TileW - pad + j0;
    const int nr = rows ? kF2TileH + rows - 1 : 0, nc = kF2TileW + cols - 1;
    for (int e = t; e < nr * kF2Stride; e += kF2Threads) {
        const int r = e / kF2Stride, c = e - r * kF2Stride;
        sT[e] = c < nc ? img[(int64_t)reflect_clamp(gy0 + r, p.H) * p.W + reflect_clamp(gx0 + c, p.W)] : 0.0f;
    }
    __syncthreads();

    const int row = t & 31, xl = (t >> 5) * 8;
    float acc[8] = {};
    const float *tile = sT + row * kF2Stride + xl;
    if (cols <= 8) f2_accumulate<8>(tile, sW, rows, acc);
    else if (cols <= 16) f2_accumulate<16>(tile, sW, rows, acc);
    else f2_accumulate<24>(tile, sW, rows, acc);

    __syncthreads();
#pragma unroll
    for (int o = 0; o < 8; ++o) sT[row * kOutStride + xl + o] = f2_epilogue(acc[o], p.epilogue);
    __syncthreads();
    float *out = p.out + plane * p.H * p.W;
    for (int e = t; e < kF2TileH * kF2TileW; e += kF2Threads) {
        const int r = e >> 6, c = e & 63, y = by * kF2TileH + r, x = bx * kF2TileW + c;
        if (y < p.H && x < p.W) out[(int64_t)y * p.W + x] = sT[r * kOutStride + c];
    }
}

static bool plane_dims_ok(int64_t B, int64_t C, int64_t H, int64_t W) {
    return B >= 1 && C >= 1 && H >= 1 && W >= 1 && H <= (1 << 24) && W <= (1 << 24) && B <= (1 << 24) && C <= (1 << 24);
}

size_t filter2d_workgroups(int64_t B, int64_t C, int64_t H, int64_t W, int k, int64_t kernels) {
    if (!plane_dims_ok(B, C, H, W) || k < 1 || k > kF2MaxK || k % 2 == 0 || H <= k / 2 || W <= k / 2) return 0;
    if (kernels != 1 && kernels != B) return 0;
    const int64_t tiles = ((H + kF2TileH - 1) / kF2TileH) * ((W + kF2TileW - 1) / kF2TileW);
    if (tiles > 0x7fffffff || B * C > 0x7fffffff / tiles) return 0;   // grid.x
    return (size_t)(B * C * tiles);
}

int filter2d(const float *img, const float *kernel, float *out, int64_t B, int64_t C, int64_t H, int64_t W, int k, int64_t kernels,
             int epilogue, hipStream_t s) {
    const size_t wgs = filter2d_workgroups(B, C, H, W, k, kernels);
    if (!wgs || epilogue < OSS_FILTER_NONE || epilogue > OSS_FILTER_QUANTISE) return OSS_ERR_SHAPE;
    F2Args p = {};
    p.img = img, p.ker = kernel, p.out = out;
    p.C = (int)C, p.H = (int)H, p.W = (int)W, p.k = k;
    p.tilesX = (int)((W + kF2TileW - 1) / kF2TileW), p.tilesY = (int)((H + kF2TileH - 1) / kF2TileH);
    p.per_sample = kernels != 1, p.epilogue = epilogue;
    hipLaunchKernelGGL(oss_filter2d_kernel, dim3((unsigned)wgs), dim3(kF2Threads), 0, s, p);
    return (int)hipGetLastError();
}

// ---- separable passes and USM ---------------------------------------------------------------------------------------------------
constexpr int kSepThreads = 256, kSepTile = 64, kSepMaxK = 63, kSepChunk = 8;
constexpr int kSepWin = kSepTile + ((kSepMaxK + kSepChunk - 1) / kSepChunk) * kSepChunk - 1;   // 127: the longest staged line
static_assert(kSepWin % 2 == 1 && kSepTile * kOutStride <= kSepWin * kSepTile, "LDS tile of oss_filter_sep_kernel");
enum SepMode { SEP_PLAIN = 0, SEP_MASK = 1, SEP_BLEND = 2 };

struct SepArgs {
    const float *in, *img, *g;
    float *out, *mask;
    int H, W, k, tilesX, tilesY;
    float weight, threshold;
};

// grid (planes * tilesY * tilesX)
template <bool COL, int MODE>
__global__ void __launch_bounds__(kSepThreads) oss_filter_sep_kernel(const SepArgs p) {
    static_assert(COL || MODE == SEP_PLAIN, "the fused stages ride on the column pass");
    __shared__ float sT[kSepWin * kSepTile];
    __shared__ float sG[kSepMaxK + 1];
    const int t = threadIdx.x, k = p.k, pad = k / 2;
    const int nch = (k + kSepChunk - 1) / kSepChunk, len = kSepTile + nch * kSepChunk - 1, data = kSepTile + k - 1;
    const int bx = blockIdx.x % p.tilesX, by = (blockIdx.x / p.tilesX) % p.tilesY;
    const int64_t base = (int64_t)(blockIdx.x / (p.tilesX * p.tilesY)) * p.H * p.W;
    const int y0 = by * kSepTile, x0 = bx * kSepTile;
    const float *in = p.in + base;

    if (t <= kSepMaxK) sG[t] = t < k ? p.g[t] : 0.0f;
    // the staged line is `len` long: `data` elements of the plane, then zeros under the zero taps of the last chunk
    if constexpr (COL) {
        for (int e = t; e < len * kSepTile; e += kSepThreads) {
            const int r = e >> 6, x = x0 + (e & 63);
            sT[e] = r < data && x < p.W ? in[(int64_t)reflect_clamp(y0 - pad + r, p.H) * p.W + x] : 0.0f;
        }
    } else {
        const int c = t & 127;
        const int x = reflect_clamp(x0 - pad + c, p.W);
        for (int r = t >> 7; r < kSepTile; r += 2)
            if (c < len) sT[r * kSepWin + c] = c < data && y0 + r < p.H ? in[(int64_t)(y0 + r) * p.W + x] : 0.0f;
    }
    __syncthreads();

    const int line = t & 63, strip = t >> 6;   // a wave lies across the filtered axis
    float acc[2][8] = {};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int s0 = (strip + 4 * u) * 8;
        for (int c = 0; c < nch; ++c) {
            float w[kSepChunk], a[kSepChunk + 7];
#pragma unroll
            for (int j = 0; j < kSepChunk; ++j) w[j] = sG[c * kSepChunk + j];
#pragma unroll
            for (int m = 0; m < kSepChunk + 7; ++m) {
                const int q = s0 + c * kSepChunk + m;
                a[m] = COL ? sT[q * kSepTile + line] : sT[line * kSepWin + q];
            }
#pragma unroll
            for (int j = 0; j < kSepChunk; ++j)
#pragma unroll
                for (int o = 0; o < 8; ++o) acc[u][o] = fmaf(w[j], a[j + o], acc[u][o]);
        }
    }

    if constexpr (!COL) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int o = 0; o < 8; ++o) sT[line * kOutStride + (strip + 4 * u) * 8 + o] = acc[u][o];
        __syncthreads();
        for (int e = t; e < kSepTile * kSepTile; e += kSepThreads) {
            const int r = e >> 6, c = e & 63;
            if (y0 + r < p.H && x0 + c < p.W) p.out[base + (int64_t)(y0 + r) * p.W + x0 + c] = sT[r * kOutStride + c];
        }
    } else {
        const int x = x0 + line;
        if (x >= p.W) return;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                const int y = y0 + (strip + 4 * u) * 8 + o;
                if (y >= p.H) continue;
                const int64_t at = base + (int64_t)y * p.W + x;
                const float v = acc[u][o];
                if constexpr (MODE == SEP_PLAIN) {
                    p.out[at] = v;
                } else if constexpr (MODE == SEP_MASK) {
                    const float residual = p.img[at] - v;
                    p.out[at] = residual;
                    p.mask[at] = fabsf(residual) * 255.0f > p.threshold ? 1.0f : 0.0f;
                } else {
                    const float x_in = p.img[at], sharp = fminf(fmaxf(x_in + p.weight * p.out[at], 0.0f), 1.0f);
                    p.out[at] = x_in + v * (sharp - x_in);
                }
            }
    }
}

static size_t sep_workgroups(int64_t B, int64_t C, int64_t H, int64_t W, int k) {
    if (!plane_dims_ok(B, C, H, W) || k < 1 || k > kSepMaxK || k % 2 == 0 || H <= k / 2 || W <= k / 2) return 0;
    const int64_t tiles = ((H + kSepTile - 1) / kSepTile) * ((W + kSepTile - 1) / kSepTile);
    if (tiles > 0x7fffffff || B * C > 0x7fffffff / tiles) return 0;   // grid.x
    return (size_t)(B * C * tiles);
}

size_t filter_sep_scratch_floats(int64_t B, int64_t C, int64_t H, int64_t W, int k) {
    return sep_workgroups(B, C, H, W, k) ? (size_t)(B * C * H * W) : 0;
}

size_t usm_scratch_floats(int64_t B, int64_t C, int64_t H, int64_t W, int k) { return 2 * filter_sep_scratch_floats(B, C, H, W, k); }

template <bool COL, int MODE> static int sep_launch(SepArgs p, size_t wgs, hipStream_t s) {
    hipLaunchKernelGGL((oss_filter_sep_kernel<COL, MODE>), dim3((unsigned)wgs), dim3(kSepThreads), 0, s, p);
    return (int)hipGetLastError();
}

static SepArgs sep_args(const float *g, int64_t H, int64_t W, int k) {
    SepArgs p = {};
    p.g = g, p.H = (int)H, p.W = (int)W, p.k = k;
    p.tilesX = (int)((W + kSepTile - 1) / kSepTile), p.tilesY = (int)((H + kSepTile - 1) / kSepTile);
    return p;
}

int filter_sep(const float *img, const float *g, float *out, float *scratch, int64_t B, int64_t C, int64_t H, int64_t W, int k,
               hipStream_t s) {
    const size_t wgs = sep_workgroups(B, C, H, W, k);
    if (!wgs) return OSS_ERR_SHAPE;
    SepArgs p = sep_args(g, H, W, k);
    p.in = img, p.out = scratch;
    if (const int e = sep_launch<false, SEP_PLAIN>(p, wgs, s)) return e;
    p.in = scratch, p.out = out;
    return sep_launch<true, SEP_PLAIN>(p, wgs, s);
}

int usm_sharp(const float *img, const float *g, float *out, float *mask, float *scratch, int64_t B, int64_t C, int64_t H, int64_t W,
              int k, float weight, float threshold, hipStream_t s) {
    const size_t wgs = sep_workgroups(B, C, H, W, k);
    if (!wgs) return OSS_ERR_SHAPE;
    float *tmp = scratch, *m = mask ? mask : scratch + B * C * H * W;
    SepArgs p = sep_args(g, H, W, k);
    p.img = img, p.weight = weight, p.threshold = threshold;
    p.in = img, p.out = tmp;
    if (const int e = sep_launch<false, SEP_PLAIN>(p, wgs, s)) return e;
    p.in = tmp, p.out = out, p.mask = m;                         // out holds the residual until the last pass
    if (const int e = sep_launch<true, SEP_MASK>(p, wgs, s)) return e;
    p.in = m, p.out = tmp;
    if (const int e = sep_launch<false, SEP_PLAIN>(p, wgs, s)) return e;
    p.in = tmp, p.out = out;
    return sep_launch<true, SEP_BLEND>(p, wgs, s);
}

}  // namespace oss
