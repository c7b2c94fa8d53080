// oss_jpeg.hip -- DiffJPEG, the JPEG step of the RealSR degradation pipeline (MambaRealSR.feed_data,
// RealSR/VmambaIR/models/MambaRealSR_model.py:189-191 and :234-241), as ONE launch: compression to quantised DCT coefficients and
// decompression back to RGB, as the pip basicsr package defines them (basicsr.utils.diffjpeg; restated from its published source in
// vmambair_amd/degradations.py).  fp32 in and out, no allocation, no host read-back: the per-sample quality is read from device
// memory by the kernel, so a call can be captured into a hipGraph and replayed with other qualities.
//
// The work unit is a 16 x 16 macroblock of one sample: 768 floats in, 768 floats out, six 8 x 8 blocks (four of Y, one each of the
// 2 x 2 averaged Cb and Cr) in between.  A wave owns a macroblock, a workgroup of four waves four consecutive ones (a wave past the
// last macroblock recomputes the last one and stores nothing, so that every wave reaches every barrier).  Per wave, in LDS:
//   blk  6 x 64 floats  the six blocks, 8 x 8 row-major each
//   tmp  8 x 64 floats  full-resolution Cb and Cr before the averaging, then the half-transformed blocks
//   load      lane l reads pixels (l / 16 + 4 k, l % 16), k = 0...3, of R, G and B: every load instruction of the wave covers four
//             whole 64-byte rows of the macroblock.  Rows of an arbitrary w are only 4-byte aligned, so all global accesses are
//             dwords.  Pixels at or past h, w read as 0 (the zero padding to multiples of 16; no padded copy exists).
//   colour    p = 255 x; Y, Cb, Cr with the fp32 matrix of rgb2ycbcr_jpeg; Y - 128 -> blk, Cb and Cr -> tmp
//   average   lane (i, j) = (l / 8, l % 8): the mean of its 2 x 2 of Cb and of Cr, minus 128 -> blk 4 and 5
//   DCT       separable, with the orthonormal 8-point matrix C[u][x] = 1/2 alpha(u) cos((2 x + 1) u pi / 16) held in registers:
//             rows  t[i][j] = sum_k blk[i][k] C[j][k] -> tmp;   columns  F[i][j] = sum_k C[i][k] tmp[k][j]: 8 multiply-adds each,
//             the transposition is the pass through LDS.  Reads are broadcasts of 8 (rows) or 8 consecutive words (columns):
//             free of bank conflicts.
//   quantise  tq = T[i][j] * factor; v = F / tq; c = rint(v) (round-half-even, torch.round), or c + (v - c)^3 with
//             OSS_JPEG_DIFF_ROUND; c -> the optional coefficient outputs; c * tq -> blk
//   IDCT      rows  s[i][j] = sum_k blk[i][k] C[k][j] -> tmp;   columns  f[i][j] = sum_k C[k][i] tmp[k][j] + 128 -> blk
//   store     the load's pixel mapping: Y from its block, Cb and Cr of pixel (r, c) from (r / 2, c / 2) (the 2 x 2 replication),
//             the fp32 matrix of ycbcr2rgb_jpeg, clamp to [0, 255], * fp32(1 / 255) (torch's division of a device tensor by 255),
//             optionally the final quantisation (:248); stores are guarded at the right and bottom edge.
#include <cmath>
#include "oss_host.h"
#include "oss_pixel_stage.h"

namespace oss {

constexpr int kJpegWaves = 4, kJpegThreads = 64 * kJpegWaves;
constexpr int kJpegBlk = 6 * 64, kJpegTmp = 8 * 64;
constexpr int kJpegKnownFlags = OSS_JPEG_CLAMP_INPUT | OSS_JPEG_QUANTISE | OSS_JPEG_DIFF_ROUND;

// 1/2 alpha(u) cos(m pi / 16): d0 is the row u = 0 (and cos(4 pi / 16) / 2), dm = cos(m pi / 16) / 2
#define D0 0.35355339059327373f
#define D1 0.4903926402016152f
#define D2 0.46193976625564337f
#define D3 0.4157348061512726f
#define D5 0.2777851165098011f
#define D6 0.1913417161825449f
#define D7 0.09754516100806412f
__constant__ float kJpegDct[64] = {
    D0,  D0,  D0,  D0,  D0,  D0,  D0,  D0,
    D1,  D3,  D5,  D7, -D7, -D5, -D3, -D1,
    D2,  D6, -D6, -D2, -D2, -D6,  D6,  D2,
    D3, -D7, -D1, -D5,  D5,  D1,  D7, -D3,
    D0, -D0, -D0,  D0,  D0, -D0, -D0,  D0,
    D5, -D1,  D7,  D3, -D3, -D7,  D1, -D5,
    D6, -D2,  D2, -D6, -D6,  D2, -D2,  D6,
    D7, -D5,  D3, -D1,  D1, -D3,  D5, -D7,
};
#undef D0
#undef D1
#undef D2
#undef D3
#undef D5
#undef D6
#undef D7

// [0]: the luminance table as basicsr holds it (the standard table transposed); [1]: the chrominance table (symmetric)
__constant__ float kJpegQ[2][64] = {
    {16, 12, 14, 14, 18, 24, 49, 72,
     11, 12, 13, 17, 22, 35, 64, 92,
     10, 14, 16, 22, 37, 55, 78, 95,
     16, 19, 24, 29, 56, 64, 87, 98,
     24, 26, 40, 51, 68, 81, 103, 112,
     40, 58, 57, 87, 109, 104, 121, 100,
     51, 60, 69, 80, 103, 113, 120, 103,
     61, 55, 56, 62, 77, 92, 101, 99},
    {17, 18, 24, 47, 99, 99, 99, 99,
     18, 21, 26, 66, 99, 99, 99, 99,
     24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99},
};

// basicsr's quality_to_factor in fp32; the same expression on the host (a scalar quality) and in the kernel (quality[b]): both
// divisions are correctly rounded on either side and 2 q is exact, so the two give the same bits
__host__ __device__ inline float jpeg_factor(float q) {
    return (q < 50.0f ? 5000.0f / q : 200.0f - q * 2.0f) / 100.0f;
}

struct JpegArgs {
    const float *img, *quality;
    float *out, *coef_y, *coef_cb, *coef_cr;
    float factor;
    int h, w, mbX, mbY, flags;
    int64_t total;   // macroblocks of the whole batch
};

// where pixel (r, c) of the macroblock lies among the four Y blocks
__device__ __forceinline__ int jpeg_y_slot(int r, int c) {
    return ((r >> 3) * 2 + (c >> 3)) * 64 + (r & 7) * 8 + (c & 7);
}

// grid (ceil(total / 4))
__global__ void __launch_bounds__(kJpegThreads) oss_jpeg_kernel(const JpegArgs p) {
    __shared__ float sBlk[kJpegWaves][kJpegBlk];
    __shared__ float sTmp[kJpegWaves][kJpegTmp];
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, i = l >> 3, j = l & 7;
    float *blk = sBlk[wave], *tmp = sTmp[wave];
    int64_t m = (int64_t)blockIdx.x * kJpegWaves + wave;
    const bool active = m < p.total;
    m = active ? m : p.total - 1;
    const int mx = (int)(m % p.mbX), my = (int)((m / p.mbX) % p.mbY);
    const int64_t b = m / ((int64_t)p.mbX * p.mbY);
    const int64_t plane = (int64_t)p.h * p.w;
    const float factor = p.quality ? jpeg_factor(p.quality[b]) : p.factor;

    float cri[8], crj[8], cci[8], ccj[8];   // rows i, j and columns i, j of C
#pragma unroll
    for (int k = 0; k < 8; ++k)
        cri[k] = kJpegDct[i * 8 + k], crj[k] = kJpegDct[j * 8 + k], cci[k] = kJpegDct[k * 8 + i], ccj[k] = kJpegDct[k * 8 + j];

    // ---- load, colour conversion ---------------------------------------------------------------------------------------------
    const float *img = p.img + b * 3 * plane;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = (l >> 4) + 4 * k, c = l & 15, gy = my * 16 + r, gx = mx * 16 + c;
        float R = 0.0f, G = 0.0f, B = 0.0f;
        if (gy < p.h && gx < p.w) {
            const float *px = img + (int64_t)gy * p.w + gx;
            R = px[0], G = px[plane], B = px[2 * plane];
            if (p.flags & OSS_JPEG_CLAMP_INPUT) R = clamp_unit(R), G = clamp_unit(G), B = clamp_unit(B);
        }
        R *= 255.0f, G *= 255.0f, B *= 255.0f;
        blk[jpeg_y_slot(r, c)] = fmaf(0.114f, B, fmaf(0.587f, G, 0.299f * R)) - 128.0f;
        tmp[r * 16 + c] = fmaf(0.5f, B, fmaf(-0.331264f, G, -0.168736f * R)) + 128.0f;
        tmp[256 + r * 16 + c] = fmaf(-0.081312f, B, fmaf(-0.418688f, G, 0.5f * R)) + 128.0f;
    }
    __syncthreads();
    // ---- 2 x 2 average of Cb and Cr ----------------------------------------------------------------------------------------
    {
        const float *q = tmp + i * 32 + j * 2;
        blk[256 + l] = (q[0] + q[1] + q[16] + q[17]) * 0.25f - 128.0f;
        blk[320 + l] = (q[256] + q[257] + q[272] + q[273]) * 0.25f - 128.0f;
    }
    __syncthreads();
    // ---- forward DCT: rows, then columns ----------------------------------------------------------------------------------
    float v[6];
#pragma unroll
    for (int n = 0; n < 6; ++n) {
        const float *row = blk + n * 64 + i * 8;
        float a = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) a = fmaf(row[k], crj[k], a);
        v[n] = a;
    }
#pragma unroll
    for (int n = 0; n < 6; ++n) tmp[n * 64 + l] = v[n];
    __syncthreads();
#pragma unroll
    for (int n = 0; n < 6; ++n) {
        const float *col = tmp + n * 64 + j;
        float a = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) a = fmaf(cri[k], col[k * 8], a);
        v[n] = a;
    }
    // ---- quantise, hand the coefficients out, dequantise ------------------------------------------------------------------
    const float tq[2] = {kJpegQ[0][l] * factor, kJpegQ[1][l] * factor};
    const int64_t yblocks = (int64_t)p.mbX * p.mbY * 4;   // 8 x 8 blocks of one padded Y plane
#pragma unroll
    for (int n = 0; n < 6; ++n) {
        const float t = tq[n >> 2], s = v[n] / t;
        float c = rintf(s);
        if (p.flags & OSS_JPEG_DIFF_ROUND) {
            const float d = s - c;
            c += d * d * d;
        }
        if (active) {
            if (n < 4) {
                if (p.coef_y) p.coef_y[(b * yblocks + (int64_t)(2 * my + (n >> 1)) * (2 * p.mbX) + 2 * mx + (n & 1)) * 64 + l] = c;
            } else {
                float *dst = n == 4 ? p.coef_cb : p.coef_cr;
                if (dst) dst[(b * (yblocks / 4) + (int64_t)my * p.mbX + mx) * 64 + l] = c;
            }
        }
        blk[n * 64 + l] = c * t;
    }
    __syncthreads();
    // ---- inverse DCT: rows, then columns ----------------------------------------------------------------------------------
#pragma unroll
    for (int n = 0; n < 6; ++n) {
        const float *row = blk + n * 64 + i * 8;
        float a = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) a = fmaf(row[k], ccj[k], a);
        v[n] = a;
    }
#pragma unroll
    for (int n = 0; n < 6; ++n) tmp[n * 64 + l] = v[n];
    __syncthreads();
#pragma unroll
    for (int n = 0; n < 6; ++n) {
        const float *col = tmp + n * 64 + j;
        float a = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) a = fmaf(cci[k], col[k * 8], a);
        v[n] = a + 128.0f;
    }
#pragma unroll
    for (int n = 0; n < 6; ++n) blk[n * 64 + l] = v[n];
    __syncthreads();
    // ---- chroma replication, inverse colour conversion, store ---------------------------------------------------------------
    float *out = p.out + b * 3 * plane;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = (l >> 4) + 4 * k, c = l & 15, gy = my * 16 + r, gx = mx * 16 + c;
        const float Y = blk[jpeg_y_slot(r, c)];
        const float cb = blk[256 + (r >> 1) * 8 + (c >> 1)] - 128.0f, cr = blk[320 + (r >> 1) * 8 + (c >> 1)] - 128.0f;
        float rgb[3] = {fmaf(1.402f, cr, Y), fmaf(-0.714136f, cr, fmaf(-0.344136f, cb, Y)), fmaf(1.772f, cb, Y)};
        if (active && gy < p.h && gx < p.w) {
            float *px = out + (int64_t)gy * p.w + gx;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float o = rgb[ch];
                o = (o != o ? o : fminf(fmaxf(o, 0.0f), 255.0f) + 0.0f) * kInv255;
                px[ch * plane] = (p.flags & OSS_JPEG_QUANTISE) ? quantise_255(o) : o;
            }
        }
    }
}

static bool jpeg_dims(int64_t B, int64_t h, int64_t w, int64_t *mbX, int64_t *mbY, int64_t *total) {
    if (B < 1 || h < 1 || w < 1 || B > (1 << 24) || h > (1 << 24) || w > (1 << 24)) return false;
    *mbX = (w + 15) / 16, *mbY = (h + 15) / 16;
    const int64_t per = *mbX * *mbY;           // <= 2^40
    if (per > 0x7fffffff || B > 0x7fffffff / per) return false;
    *total = B * per;
    return true;
}

size_t jpeg_workgroups(int64_t B, int64_t h, int64_t w) {
    int64_t mbX, mbY, total;
    if (!jpeg_dims(B, h, w, &mbX, &mbY, &total)) return 0;
    return (size_t)((total + kJpegWaves - 1) / kJpegWaves);
}

int jpeg_roundtrip(const float *img, const float *quality, float quality_scalar, float *out, float *coef_y, float *coef_cb,
                   float *coef_cr, int64_t B, int64_t h, int64_t w, int flags, hipStream_t s) {
    int64_t mbX, mbY, total;
    if (!jpeg_dims(B, h, w, &mbX, &mbY, &total) || (flags & ~kJpegKnownFlags)) return OSS_ERR_SHAPE;
    JpegArgs p = {};
    p.img = img, p.quality = quality, p.out = out, p.coef_y = coef_y, p.coef_cb = coef_cb, p.coef_cr = coef_cr;
    p.factor = quality ? 0.0f : jpeg_factor(quality_scalar);
    p.h = (int)h, p.w = (int)w, p.mbX = (int)mbX, p.mbY = (int)mbY, p.flags = flags, p.total = total;
    hipLaunchKernelGGL(oss_jpeg_kernel, dim3((unsigned)((total + kJpegWaves - 1) / kJpegWaves)), dim3(kJpegThreads), 0, s, p);
    return (int)hipGetLastError();
}

}  // namespace oss
