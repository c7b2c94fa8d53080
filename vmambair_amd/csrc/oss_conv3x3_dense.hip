// oss_conv3x3_dense.hip -- the GEMM-shaped 3x3 convolutions (stride 1, zero padding 1, NCHW) of the UNet skeleton on the matrix
// cores: Downsample conv(n -> n/2), Upsample conv(n -> 2n) and the two conv(n -> 4n) of the x4 tail (vmambair_amd/archs.py).
// 16-bit I/O (bf16 / fp16), fp32 master weights (Cout, Cin, 3, 3) + optional fp32 bias narrowed to the I/O type where they are
// loaded, fp32 accumulation on v_mfma_f32_32x32x16_{bf16,f16} (oss_mfma.h), one rounding after the bias.
//
//   fwd    y[m][p] = bias[m] + sum_{t, k} Wt[m][k] x[k][p + off(t)]      implicit GEMM, M = Cout, N = pixels, K = (tap, Cin)
//          A = weights: lane (r, h) holds W[m0 + r][k0 + 8 h .. + 8][t] for the nine taps -- for the forward weight layout these
//          are 72 CONSECUTIVE floats of the master, read straight from global memory (18 x 16 bytes) and narrowed in registers;
//          every wave of a workgroup owns its own 32 output channels or shares them with the waves of other image rows, so the
//          weights need no LDS and no second barrier.
//          B = activations: a (4 WN + 2) x 34 pixel tile (one-pixel halo, zeros outside the image) of 16 input channels is
//          staged in LDS as [pixel][16 channels] -- 32 bytes per pixel.  Lane (r, h) reads pixel (row, r + kw), channels
//          8 h .. 8 h + 7: ONE aligned ds_read_b128 whatever the tap, because a tap shifts the address by whole pixels = 32 bytes
//          (a [channel][pixel] image would need ds_read_b64_tr_b16, whose 8-byte alignment a one-pixel shift breaks).  The 64
//          lanes of a read cover 2048 consecutive bytes: conflict-free.  A staged chunk is read for all nine taps and by all
//          waves: 18 LDS reads feed 36 MFMAs per wave and chunk.
//          Workgroup = 4 waves as WM (Cout, 32 each) x WN = 4 / WM (4 image rows each) over 32 image columns; WM is 1, 2 or 4,
//          whichever pads Cout least.  D has the output channel in the register index and the pixel on the lane; on the fast
//          path the epilogue turns it through LDS so that a lane stores 8 pixels of one channel (16 bytes).
//   dgrad  the same kernel body on dy with M = Cin, K = Cout and the weight loader's WT flag: element (m, k, t) is read as
//          W[k][m][8 - t].  K = Cout need not be a multiple of 16: the last chunk is zero-filled on both operands.
//   wgrad  dW[co][ci][t] = sum_{b, p} dy[co][p] x[ci][p + off(t)]: M = Cout, N = Cin, K = pixels, both operands read from global
//          memory in MFMA operand order (8 consecutive pixels of one plane row = 16 bytes per lane; the two shifted copies a row
//          needs for kw = 0 / 2 are made in registers from the aligned 16 bytes and the two neighbouring pixels; a band is walked
//          column block by column block, rows inside, so each step loads ONE new x row and keeps the other two).  One wave owns a
//          32 x 32 (co, ci) tile for all nine taps (9 accumulators), a workgroup 64 x 64; the grid is (tiles, row bands, images)
//          and each workgroup writes its part of the fp32 partial vector of its (image, band).  The partial vectors are added
//          over (image, band) in one fixed order by defer_sum under oss_set_defer_finish(1), by oss_conv3x3_dense_finish (the
//          same order) otherwise: no atomics, reruns are bit-identical.  db = sum dy is a launch of its own, one workgroup per
//          output channel, summed in fp64 and rounded once (oss_conv3x3_dense_dbias_kernel says why).
//          Partial buffer: batch * bands * 9 Cin Cout floats with bands <= min(H, max(1, ceil(512 / (batch * tiles))))
//          (conv3x3_dense_wgrad_partial_floats), i.e. never more than batch * H vectors and about 512 / tiles for large planes.
// Fast path (VEC): 16-byte aligned base pointers, batch / channel strides multiples of 8 elements and W % 8 == 0 -- then every
// image row starts 16-byte aligned and 8-pixel groups are whole.  Anything else takes the element-wise loaders (same arithmetic).
#include "oss_device.h"
#include "oss_host.h"
#include "oss_mfma.h"

namespace oss {

namespace {

constexpr int kDensePC = 34;   // staged tile: 32 image columns + the halo

template <typename T> __device__ __forceinline__ uint32_t bits16(const T *p) { return (uint32_t)p->v; }

// the nine A operands of output row `o` for input channels k0 .. k0 + 7 (k0 = chunk + 8 * lane half)
template <typename T, bool WT>
__device__ __forceinline__ void dense_wfrags(const float *__restrict__ w, int o, int k0, int K, int M, bool wvec, s16x8 (&a)[9]) {
    float f[72];   // [j][t]
    if constexpr (!WT) {
        const float *p = w + ((size_t)o * K + k0) * 9;   // K % 16 == 0: the whole chunk exists
        if (wvec) {
#pragma unroll
            for (int q = 0; q < 18; ++q) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(p + 4 * q);
                f[4 * q] = v.x; f[4 * q + 1] = v.y; f[4 * q + 2] = v.z; f[4 * q + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 72; ++q) f[q] = p[q];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = k0 + j;
            const float *p = w + ((size_t)min(k, K - 1) * M + o) * 9;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const float v = p[8 - t];
                f[j * 9 + t] = k < K ? v : 0.f;
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 8; ++j) a[t][j] = to_bits<T>(f[j * 9 + t]);
}

// one (pixel, channel pair) of the staged tile, element-wise
template <typename T>
__device__ __forceinline__ uint32_t dense_pair(const T *__restrict__ xb, int c, int K, int gh, int gw, int H, int W, int64_t xsc) {
    if (gh < 0 || gh >= H || gw < 0 || gw >= W) return 0u;
    const T *p = xb + (int64_t)c * xsc + (int64_t)gh * W + gw;
    const uint32_t lo = c < K ? bits16(p) : 0u;
    const uint32_t hi = c + 1 < K ? bits16(p + xsc) : 0u;
    return lo | (hi << 16);
}

// channels c0 .. c0 + 15 of image rows h0 - 1 .. h0 + PR - 2, columns w0 - 1 .. w0 + 32 -> tile[pixel][16 channels]
template <typename T, int PR, bool VEC>
__device__ __forceinline__ void dense_stage(uint32_t *tile, const T *__restrict__ xb, int c0, int K, int h0, int w0, int H, int W,
                                            int64_t xsc, int tid) {
    if constexpr (!VEC) {
        for (int it = tid; it < PR * kDensePC * 8; it += 256) {
            const int cp = it & 7, pix = it >> 3;
            const int pr = pix / kDensePC, pc = pix - pr * kDensePC;
            tile[pix * 8 + cp] = dense_pair<T>(xb, c0 + 2 * cp, K, h0 - 1 + pr, w0 - 1 + pc, H, W, xsc);
        }
    } else {
        // interior: 8 pixels of two channels per item (two 16-byte loads, eight 4-byte LDS writes).  Items run channel pair,
        // then tile row, then pixel group, so that a 32-lane half writes 4 tile rows (1088 bytes apart): 2-way on the 32 write
        // banks instead of the 4-way of 4 pixel groups (256 bytes apart)
        for (int it = tid; it < PR * 32; it += 256) {
            const int cp = it & 7, q = it >> 3;
            const int pr = q % PR, g = q / PR;
            const int gh = h0 - 1 + pr, gw = w0 + 8 * g, c = c0 + 2 * cp;
            u32x4 va = {0u, 0u, 0u, 0u}, vb = {0u, 0u, 0u, 0u};
            if (gh >= 0 && gh < H && gw < W) {
                const T *p = xb + (int64_t)c * xsc + (int64_t)gh * W + gw;
                if (c < K) va = *reinterpret_cast<const u32x4 *>(p);
                if (c + 1 < K) vb = *reinterpret_cast<const u32x4 *>(p + xsc);
            }
            uint32_t *d = tile + (pr * kDensePC + 1 + 8 * g) * 8 + cp;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                d[(2 * k) * 8] = (va[k] & 0xffffu) | (vb[k] << 16);
                d[(2 * k + 1) * 8] = (va[k] >> 16) | (vb[k] & 0xffff0000u);
            }
        }
        // the two halo columns
        for (int it = tid; it < PR * 16; it += 256) {
            const int cp = it & 7, side = (it >> 3) & 1, pr = it >> 4;
            const int pc = side ? kDensePC - 1 : 0;
            tile[(pr * kDensePC + pc) * 8 + cp] = dense_pair<T>(xb, c0 + 2 * cp, K, h0 - 1 + pr, w0 - 1 + pc, H, W, xsc);
        }
    }
}

}  // namespace

// grid (pixel tiles: tiles_w x ceil(H / (4 WN)), ceil(M / (32 WM)), batch)
template <typename T, int WM, bool WT, bool VEC>
__global__ void __launch_bounds__(256)
oss_conv3x3_dense_kernel(const T *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias, T *__restrict__ y, int K,
                         int M, int H, int W, int tiles_w, int64_t xsb, int64_t xsc, int64_t ysb, int64_t ysc, int wvec) {
    constexpr int WN = 4 / WM, TH = 4 * WN, PR = TH + 2;
    constexpr int kTileWords = PR * kDensePC * 8 > 2048 ? PR * kDensePC * 8 : 2048;   // the epilogue stages 4 x 2 KiB in it
    __shared__ __attribute__((aligned(16))) uint32_t tile[kTileWords];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WM, wn = wave / WM;
    const int r = lane & 31, hh = lane >> 5;
    const int tw = blockIdx.x % tiles_w, th = blockIdx.x / tiles_w;
    const int h0 = th * TH, w0 = tw * 32;
    const int b = blockIdx.z;
    const int m0 = (blockIdx.y * WM + wm) * 32;
    const int o = min(m0 + r, M - 1);   // rows past M shadow the last one and are not stored
    const bool live = m0 < M && h0 + wn * 4 < H;   // wave-uniform
    const T *xb = x + b * xsb;
    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;
    for (int c0 = 0; c0 < K; c0 += 16) {
        s16x8 a[9];
        dense_wfrags<T, WT>(w, o, c0 + 8 * hh, K, M, wvec != 0, a);
        __syncthreads();   // the previous chunk has been read
        dense_stage<T, PR, VEC>(tile, xb, c0, K, h0, w0, H, W, xsc, tid);
        __syncthreads();
        if (live) {
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                s16x8 bf[6];
#pragma unroll
                for (int q = 0; q < 6; ++q)
                    bf[q] = *reinterpret_cast<const s16x8 *>(tile + ((wn * 4 + q) * kDensePC + r + kw) * 8 + 4 * hh);
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) acc[rr] = Mfma<T>::run(a[kh * 3 + kw], bf[rr + kh], acc[rr]);
            }
        }
    }
    T *yb = y + b * ysb;
    if constexpr (VEC) {
        // D has the pixel on the lane: through LDS (2 KiB per wave, [32 channels][32 pixels]) a lane gets 8 consecutive pixels of
        // one channel and stores 16 bytes instead of sixteen 2-byte values
        uint16_t *stg = reinterpret_cast<uint16_t *>(tile) + wave * 1024;
        __syncthreads();   // every wave has read the last chunk
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            if (live) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int ml = (i & 3) + 8 * (i >> 2) + 4 * hh;
                    const float bv = bias ? to_f32(from_f32<T>(bias[min(m0 + ml, M - 1)])) : 0.f;
                    stg[ml * 32 + r] = from_f32<T>(acc[rr][i] + bv).v;
                }
            }
            __syncthreads();
            const int gh = h0 + wn * 4 + rr;
            if (live && gh < H) {
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const int ml = (lane >> 2) + 16 * half, gw = w0 + 8 * (lane & 3);
                    if (m0 + ml < M && gw < W)
                        *reinterpret_cast<u32x4 *>(yb + (int64_t)(m0 + ml) * ysc + (int64_t)gh * W + gw) =
                            *reinterpret_cast<const u32x4 *>(stg + ml * 32 + 8 * (lane & 3));
                }
            }
            __syncthreads();
        }
    } else {
        const int gw = w0 + r;
        if (!live || gw >= W) return;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int gh = h0 + wn * 4 + rr;
            if (gh >= H) break;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int m = m0 + (i & 3) + 8 * (i >> 2) + 4 * hh;
                if (m < M) yb[(int64_t)m * ysc + (int64_t)gh * W + gw] = from_f32<T>(acc[rr][i] + (bias ? to_f32(from_f32<T>(bias[m])) : 0.f));
            }
        }
    }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------
namespace {

// columns p .. p + 7 of a plane row (zeros outside the image)
template <typename T, bool VEC>
__device__ __forceinline__ u32x4 dense_row8(const T *__restrict__ plane, int h, int p, int H, int W) {
    u32x4 q = {0u, 0u, 0u, 0u};
    if (h < 0 || h >= H || p >= W) return q;
    const T *row = plane + (int64_t)h * W;
    if constexpr (VEC) {
        q = *reinterpret_cast<const u32x4 *>(row + p);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = p + j;
            if (c >= 0 && c < W) q[j >> 1] |= bits16(row + c) << (16 * (j & 1));
        }
    }
    return q;
}

// the three column-shifted copies of that row: out[kw] holds columns p + kw - 1 .. p + kw + 6
template <typename T, bool VEC>
__device__ __forceinline__ void dense_row8x3(const T *__restrict__ plane, int h, int p, int H, int W, s16x8 (&out)[3]) {
    if constexpr (VEC) {
        const u32x4 q = dense_row8<T, true>(plane, h, p, H, W);
        uint32_t lo = 0u, hi = 0u;
        if (h >= 0 && h < H && p < W) {
            const T *row = plane + (int64_t)h * W;
            if (p > 0) lo = bits16(row + p - 1);
            if (p + 8 < W) hi = bits16(row + p + 8);
        }
        const u32x4 l = {(q.x << 16) | lo, (q.y << 16) | (q.x >> 16), (q.z << 16) | (q.y >> 16), (q.w << 16) | (q.z >> 16)};
        const u32x4 rgt = {(q.x >> 16) | (q.y << 16), (q.y >> 16) | (q.z << 16), (q.z >> 16) | (q.w << 16), (q.w >> 16) | (hi << 16)};
        out[0] = __builtin_bit_cast(s16x8, l);
        out[1] = __builtin_bit_cast(s16x8, q);
        out[2] = __builtin_bit_cast(s16x8, rgt);
    } else {
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) out[kw] = __builtin_bit_cast(s16x8, dense_row8<T, false>(plane, h, p + kw - 1, H, W));
    }
}

}  // namespace

// grid (ci_tiles x ceil(Cout / 64), row bands, batch); part[(b * bands + band) * pvec + (co * Cin + ci) * 9 + t], pvec = 9 Cin Cout
template <typename T, bool VEC>
__global__ void __launch_bounds__(256)
oss_conv3x3_dense_wgrad_kernel(const T *__restrict__ x, const T *__restrict__ dy, float *__restrict__ part, int Cin, int Cout, int H,
                               int W, int band_rows, int ci_tiles, int64_t xsb, int64_t xsc, int64_t gsb, int64_t gsc, size_t pvec) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int ct = blockIdx.x % ci_tiles, ot = blockIdx.x / ci_tiles;
    const int co0 = ot * 64 + (wave & 1) * 32, ci0 = ct * 64 + (wave >> 1) * 32;
    if (co0 >= Cout || ci0 >= Cin) return;   // wave-uniform; the kernel has no barrier
    const int band = blockIdx.y, b = blockIdx.z;
    const T *gp = dy + b * gsb + (int64_t)min(co0 + r, Cout - 1) * gsc;
    const T *xp = x + b * xsb + (int64_t)min(ci0 + r, Cin - 1) * xsc;
    f32x16 acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;
    const int hb = band * band_rows, he = min(H, hb + band_rows);
    // column block outside, rows inside: the three x rows of a step are the previous step's last two and ONE new row
    for (int s = 0; s < W; s += 16) {
        const int p = s + 8 * hh;
        s16x8 rows[3][3];
        dense_row8x3<T, VEC>(xp, hb - 1, p, H, W, rows[0]);
        dense_row8x3<T, VEC>(xp, hb, p, H, W, rows[1]);
        for (int h = hb; h < he; ++h) {
            dense_row8x3<T, VEC>(xp, h + 1, p, H, W, rows[2]);
            const u32x4 g = dense_row8<T, VEC>(gp, h, p, H, W);
            const s16x8 a = __builtin_bit_cast(s16x8, g);
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) acc[kh * 3 + kw] = Mfma<T>::run(a, rows[kh][kw], acc[kh * 3 + kw]);
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                rows[0][kw] = rows[1][kw];
                rows[1][kw] = rows[2][kw];
            }
        }
    }
    float *pb = part + ((size_t)b * gridDim.y + band) * pvec;
    const int ci = ci0 + r;
    if (ci < Cin) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int co = co0 + (i & 3) + 8 * (i >> 2) + 4 * hh;
            if (co < Cout) {
                float *d = pb + ((size_t)co * Cin + ci) * 9;
#pragma unroll
                for (int t = 0; t < 9; ++t) d[t] = acc[t][i];
            }
        }
    }
}

// db[co] = sum over images and pixels of dy[co]: one workgroup per channel, fp64 sums in a fixed order and ONE rounding, written
// directly (no partials).  The band partials of the main kernel cannot give this: the check this project holds weight-gradient sums
// to (at most 4 x the error of a plain fp32 sum) asks for the exact value whenever that sum happens to be exact, as it is for the few
// hundred 16-bit terms of a small plane, and no fp32 order over partial sums guarantees that.
template <typename T, bool VEC>
__global__ void __launch_bounds__(1024)
oss_conv3x3_dense_dbias_kernel(const T *__restrict__ dy, float *__restrict__ db, int B, int H, int W, int64_t gsb, int64_t gsc) {
    __shared__ double red[1024];
    const int tid = threadIdx.x;
    const int64_t P = (int64_t)H * W;
    double s = 0.0;
    for (int b = 0; b < B; ++b) {
        const T *p = dy + b * gsb + (int64_t)blockIdx.x * gsc;
        if constexpr (VEC) {
#pragma unroll 4
            for (int64_t i = (int64_t)tid * 8; i < P; i += 8192) {   // W % 8 == 0: whole groups
                float v[8];
                load_v<T, 8>(p + i, v);
                s += (((double)v[0] + v[1]) + ((double)v[2] + v[3])) + (((double)v[4] + v[5]) + ((double)v[6] + v[7]));
            }
        } else {
            for (int64_t i = tid; i < P; i += 1024) s += (double)to_f32(p[i]);
        }
    }
    red[tid] = s;
    __syncthreads();
    for (int st = 512; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    if (tid == 0) db[blockIdx.x] = (float)red[0];
}

// partial vectors added over (image, band) in the order of the deferred finishing launch (oss_sum_partials_kernel, oss_optim.hip:
// 4 interleaved slices of 4 interleaved sums, combined pairwise), so that a step gives the same bits with and without
// oss_set_defer_finish
__global__ void __launch_bounds__(256)
oss_conv3x3_dense_finish(const float *__restrict__ part, float *__restrict__ dw, int K, size_t pvec, size_t nw) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nw) return;
    float a[4][4];
#pragma unroll
    for (int sl = 0; sl < 4; ++sl)
#pragma unroll
        for (int j = 0; j < 4; ++j) a[sl][j] = 0.f;
    for (int k = 0; k < K; k += 16) {
#pragma unroll
        for (int q = 0; q < 16; ++q) a[q & 3][q >> 2] += k + q < K ? part[(size_t)(k + q) * pvec + i] : 0.f;
    }
    float r[4];
#pragma unroll
    for (int sl = 0; sl < 4; ++sl) r[sl] = (a[sl][0] + a[sl][1]) + (a[sl][2] + a[sl][3]);
    dw[i] = (r[0] + r[1]) + (r[2] + r[3]);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
static bool dense_vec(int W, std::initializer_list<const void *> ptrs, std::initializer_list<int64_t> strides) {
    if (W % 8 != 0) return false;
    for (const void *p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) & 15u) return false;
    for (int64_t st : strides)
        if (st % 8 != 0) return false;
    return true;
}

int conv3x3_dense_ok(oss_dtype io, int Cin, int Cout, int H, int W) {
    if (!io_ok<IO_16>(io)) return 0;
    if (Cin < 16 || Cin % 16 != 0 || Cin > 16384 || Cout < 5 || Cout > 16384) return 0;
    if (H < 1 || W < 1 || H > 32768 || W > 32768) return 0;   // every grid axis and every in-plane index stays far inside its limits
    return 1;
}

// waves along the output channels: the choice that pads M least, the larger one on a tie
static int dense_wm(int M) {
    int best = 4, pad = (M + 127) / 128 * 128;
    for (int wm : {2, 1}) {
        const int p = (M + 32 * wm - 1) / (32 * wm) * (32 * wm);
        if (p < pad) { pad = p; best = wm; }
    }
    return best;
}

template <typename T, bool WT>
static int dense_launch(const void *x, const float *w, const float *bias, void *y, int B, int K, int M, int H, int W, int64_t xsb,
                        int64_t xsc, int64_t ysb, int64_t ysc, hipStream_t s) {
    const int wm = dense_wm(M), th = 4 * (4 / wm);
    const int tiles_w = (W + 31) / 32;
    const dim3 grid((unsigned)tiles_w * ((H + th - 1) / th), (M + 32 * wm - 1) / (32 * wm), B);
    const bool vec = dense_vec(W, {x, y}, {xsb, xsc, ysb, ysc});
    const int wvec = (reinterpret_cast<uintptr_t>(w) & 15u) == 0;
#define OSS_DENSE_GO(WM_, V_)                                                                                                   \
    hipLaunchKernelGGL((oss_conv3x3_dense_kernel<T, WM_, WT, V_>), grid, dim3(256), 0, s, reinterpret_cast<const T *>(x), w, bias, \
                       reinterpret_cast<T *>(y), K, M, H, W, tiles_w, xsb, xsc, ysb, ysc, wvec)
    if (wm == 4) { if (vec) OSS_DENSE_GO(4, true); else OSS_DENSE_GO(4, false); }
    else if (wm == 2) { if (vec) OSS_DENSE_GO(2, true); else OSS_DENSE_GO(2, false); }
    else { if (vec) OSS_DENSE_GO(1, true); else OSS_DENSE_GO(1, false); }
#undef OSS_DENSE_GO
    return (int)hipGetLastError();
}

int conv3x3_dense_fwd(oss_dtype io, const void *x, const float *w, const float *bias, void *y, int B, int Cin, int Cout, int H, int W,
                      int64_t xsb, int64_t xsc, int64_t ysb, int64_t ysc, hipStream_t s) {
    if (!conv3x3_dense_ok(io, Cin, Cout, H, W) || B <= 0 || B > 65535) return OSS_ERR_SHAPE;
    return io_dispatch<IO_16>(io, [&](auto tag) {
        return dense_launch<typename decltype(tag)::type, false>(x, w, bias, y, B, Cin, Cout, H, W, xsb, xsc, ysb, ysc, s);
    });
}

// dx[ci] = sum_co sum_t W[co][ci][8 - t] dy[co][p + off(t)]: the forward body with the roles of Cin and Cout swapped
int conv3x3_dense_dgrad(oss_dtype io, const void *dy, const float *w, void *dx, int B, int Cin, int Cout, int H, int W, int64_t gsb,
                        int64_t gsc, int64_t dsb, int64_t dsc, hipStream_t s) {
    if (!conv3x3_dense_ok(io, Cin, Cout, H, W) || B <= 0 || B > 65535) return OSS_ERR_SHAPE;
    return io_dispatch<IO_16>(io, [&](auto tag) {
        return dense_launch<typename decltype(tag)::type, true>(dy, w, nullptr, dx, B, Cout, Cin, H, W, gsb, gsc, dsb, dsc, s);
    });
}

// rows per band: about 512 workgroups in all (two per CU), never more bands than rows
static int dense_band_rows(int B, int Cin, int Cout, int H) {
    const long tiles = (long)((Cin + 63) / 64) * ((Cout + 63) / 64);
    long bands = (512 + (long)B * tiles - 1) / ((long)B * tiles);
    if (bands < 1) bands = 1;
    if (bands > H) bands = H;
    return (int)((H + bands - 1) / bands);
}

size_t conv3x3_dense_wgrad_partial_floats(int B, int Cin, int Cout, int H, int W) {
    (void)W;
    const int rows = dense_band_rows(B, Cin, Cout, H);
    return (size_t)B * ((H + rows - 1) / rows) * ((size_t)Cin * Cout * 9);
}

int conv3x3_dense_wgrad(oss_dtype io, const void *x, const void *dy, float *dw, float *db, float *part, int B, int Cin, int Cout, int H,
                        int W, int64_t xsb, int64_t xsc, int64_t gsb, int64_t gsc, hipStream_t s) {
    if (!conv3x3_dense_ok(io, Cin, Cout, H, W) || B <= 0 || B > 65535) return OSS_ERR_SHAPE;
    const int rows = dense_band_rows(B, Cin, Cout, H), bands = (H + rows - 1) / rows;
    const size_t nw = (size_t)Cin * Cout * 9, pvec = nw;
    if ((size_t)B * bands > 0x7fffffffu) return OSS_ERR_SHAPE;   // unreachable: B <= 65535, bands <= 32768
    const int ci_tiles = (Cin + 63) / 64;
    const dim3 grid((unsigned)ci_tiles * ((Cout + 63) / 64), bands, B);
    const bool vec = dense_vec(W, {x, dy}, {xsb, xsc, gsb, gsc});
#define OSS_DENSE_WG(V_)                                                                                                            \
    do {                                                                                                                            \
    hipLaunchKernelGGL((oss_conv3x3_dense_wgrad_kernel<TT, V_>), grid, dim3(256), 0, s, reinterpret_cast<const TT *>(x),              \
                       reinterpret_cast<const TT *>(dy), part, Cin, Cout, H, W, rows, ci_tiles, xsb, xsc, gsb, gsc, pvec);                          \
    if (db)                                                                                                                         \
        hipLaunchKernelGGL((oss_conv3x3_dense_dbias_kernel<TT, V_>), dim3(Cout), dim3(1024), 0, s, reinterpret_cast<const TT *>(dy), db, \
                           B, H, W, gsb, gsc);                                                                                      \
    } while (0)
    const int rc = io_dispatch<IO_16>(io, [&](auto tag) {
        using TT = typename decltype(tag)::type;
        if (vec) OSS_DENSE_WG(true); else OSS_DENSE_WG(false);
        return (int)hipGetLastError();
    });
#undef OSS_DENSE_WG
    if (rc != 0) return rc;
    if (defer_finish())
        defer_sum(part, B * bands, pvec, nw, dw, nw, nullptr);
    else
        hipLaunchKernelGGL(oss_conv3x3_dense_finish, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, part, dw, B * bands, pvec, nw);
    return (int)hipGetLastError();
}

}  // namespace oss
