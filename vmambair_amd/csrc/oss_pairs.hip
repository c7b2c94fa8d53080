// oss_pairs.hip -- the training batches, cut on the device: a pool of decoded image pairs resident in HBM, a counter-based draw
// of (pair, top, left, augmentation) and ONE gather launch that crops, flips / transposes, reorders the channels and converts a
// whole batch of LQ and GT patches.  No host work per batch, no copy from the host, no atomics; both launches can be captured.
//
// What the reference does on the host, one image at a time, in DataLoader workers:
//   paired_random_crop   Deraining/basicsr/data/transforms.py:24-83   top ~ U[0, h_lq - p], left ~ U[0, w_lq - p]; the GT patch starts
//                        at (top * scale, left * scale) with side p * scale
//   augment              :136-200   hflip, vflip, transpose, each with probability 1/2, in that order          (SR trees)
//   random_augmentation  :223-275   one of 8 modes of np.rot90 / np.flipud, uniformly                          (Deraining)
//   img2tensor           utils/img_util.py:9-40 on img.astype(np.float32) / 255.: HWC -> CHW, BGR -> RGB, one fp32 division
//   EnlargedSampler      every rank takes perm[rank::world] of a per-epoch permutation
// Both augmentations are the uniform distribution over the dihedral group of the square; one 3-bit code names its elements:
// bit 0 hflip, bit 1 vflip, bit 2 transpose, applied in that order (out = T ? F^T : F, F[y][x] = S[v ? H-1-y : y][h ? W-1-x : x]).
//
// Pool: one flat uint8 buffer of HWC images (1 or 3 channels) and an int64 table, one row per pair: gt_offset, lq_offset, lq_h,
// lq_w (GT = scale x LQ).  Offsets are bytes and 64-bit everywhere: DIV2K sub-images with their x4 LQ are 23 GB.
//
// oss_pairs_draw_kernel (one workgroup): sample b of the call has per-rank position q = c + b (c = the sample counter in device
// memory), global position g = q * world + rank, epoch g div n and pair perm_epoch(g mod n).  perm_epoch is a keyed bijection of
// [0, n) in registers -- a 4-round Feistel network over the next even number of bits with cycle walking, round function one word
// of Philox4x32-10 -- so every pair is seen once per epoch over all ranks without a permutation array or a sort.  top, left and the
// code come from one Philox block keyed by the seed with g as counter; integers in [0, m) are (uint64(r) * m) >> 32.  Every thread
// reads c, the workgroup meets at a barrier, then one thread stores c + batch: replays of a captured launch walk on.
//
// oss_pairs_gather_kernel, grid (tiles of the LQ patch + tiles of the GT patch, batch), 256 threads, one 32 x 32 pixel source tile:
//   1. load: a tile row is a run of <= 96 bytes at ANY byte alignment (left * channels).  A thread takes one 4-byte word of the
//      run's aligned cover: words that lie inside the run are one global_load_dword, the ragged head and tail are byte loads of
//      the bytes inside -- nothing outside the rectangle is ever read.  Each byte is divided by 255 (correctly rounded fp32
//      division, what the reference's NumPy does) and stored planar into LDS, tile[channel][row][33]: the channel swap happens in
//      that store.  Consecutive lanes store to consecutive pixels of a row: at most 2-way on ds_write_b32, which is free.
//   2. store: 32 consecutive lanes write 32 consecutive floats of ONE destination row (descending lane order under hflip, which
//      coalesces the same), 256 bytes per wave-instruction.  Without the transpose bit they read tile[c][a][lane] (consecutive
//      banks), with it tile[c][lane][a] -- stride 33 dwords, 32 distinct banks of ds_read_b32's 32-lane groups: the row padding
//      makes the transposed read conflict-free, so global reads run along source rows and global writes along destination rows
//      for all 8 codes.
// A rectangle that does not fit its image (or a pair index / offset outside the pool) is clamped, what cannot be read is written
// as 0 and *clamped is set to 1 (a plain store of the same value from whoever sees it): a defence, the host layer validates.
//
//
// The Deraining tree's loader (paired_image_dataset.py:101-113, train.py:213-271) does two more things, both folded into the same
// two launches by a sibling of the draw and a second instantiation of the gather; the plain forms keep their device code:
//   padding              utils/img_util.py:148-164: both images extended at the bottom and right to gt_size by cv2.BORDER_REFLECT
//                        (fedcba|abcdefgh|hgfedcb): index i >= n reads r = i mod 2n, r < n ? r : 2n - 1 - r -- periodic, so an image
//                        below gt_size / 2 is covered.  Nothing is stored: oss_pairs_gather_kernel<C, PairPadArgs> reads rows and columns
//                        at or beyond the image through that map.  A tile row's in-image columns keep the aligned-word path; the
//                        reflected columns run backwards in memory and are byte loads, one pixel per thread.
//   progressive window   every iteration cuts ONE window [x0 : x0 + m, y0 : y0 + m] (x0 rows, y0 columns), common to the batch, out of
//                        the augmented gt_size patches.  With (wr, wc) = transpose ? (y0, x0) : (x0, y0) that is the ordinary sample
//                        of side m at (top + (vflip ? G - m - wr : wr), left + (hflip ? G - m - wc : wc)) with the same code, which is
//                        what oss_pairs_draw_window_kernel emits: the gather never reads the large patch to produce the small one.
//                        x0, y0 = words 0, 1 of one more Philox block per call, counter (g0 lo, g0 hi, "wind", 0), g0 the global
//                        position of the call's first sample; (uint64(r) * (G - m)) >> 32 never yields G - m, as int((G - m) *
//                        random()) never does.
//
// hipcc -Rpass-analysis=kernel-resource-usage, gfx950: see DESIGN.md 4.4d.  Timings: profiles/pairs_kernel_timing.txt.
#include "oss_host.h"
#include "oss_philox.h"   // Philox4x32-10, host and device from one text

#include <type_traits>

namespace oss {

constexpr uint32_t kTagPerm = 0x7065726du, kTagCrop = 0x63726f70u;   // "perm", "crop": word 3 / word 2 of the two counter forms
constexpr uint32_t kTagWind = 0x77696e64u;                           // "wind": word 2 of the per-call window block

// keyed bijection of [0, n): 4 Feistel rounds on 2 * half bits (4^half >= n), walked until the value is back inside [0, n)
__host__ __device__ inline uint32_t pairs_perm(uint32_t x, uint32_t n, uint64_t epoch, uint32_t k0, uint32_t k1) {
    int half = 1;
    while (half < 16 && ((uint64_t)1 << (2 * half)) < n) ++half;
    const uint32_t mask = (1u << half) - 1u;
    do {
        uint32_t l = x >> half, r = x & mask;
        for (uint32_t round = 0; round < 4; ++round) {
            const uint32_t f = philox4x32_10(r, round | ((uint32_t)(epoch >> 32) << 8), (uint32_t)epoch, kTagPerm, k0, k1).v[0];
            const uint32_t t = l ^ (f & mask);
            l = r, r = t;
        }
        x = (l << half) | r;
    } while (x >= n);
    return x;
}

__global__ void __launch_bounds__(256)
oss_pairs_draw_kernel(const int64_t *__restrict__ table, int n, int64_t *counter, int *__restrict__ samples, int batch, int patch,
                      uint32_t k0, uint32_t k1, int rank, int world, int code_mask) {
    const uint64_t c = (uint64_t)*counter;
    __syncthreads();                                   // every thread has read c ...
    if (threadIdx.x == 0) *counter = (int64_t)(c + (uint64_t)batch);   // ... before it moves
    for (int b = threadIdx.x; b < batch; b += 256) {
        const uint64_t g = (c + (uint64_t)b) * (uint64_t)world + (uint64_t)rank;
        const uint64_t epoch = g / (uint64_t)n;
        const uint32_t pair = pairs_perm((uint32_t)(g - epoch * (uint64_t)n), (uint32_t)n, epoch, k0, k1);
        const Philox4 r = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), kTagCrop, 0u, k0, k1);
        const int64_t mh = table[4 * (int64_t)pair + 2] - patch + 1, mw = table[4 * (int64_t)pair + 3] - patch + 1;
        const uint32_t uh = mh < 1 ? 1u : (uint32_t)mh, uw = mw < 1 ? 1u : (uint32_t)mw;   // a too-small image: the gather clamps and flags
        samples[4 * b + 0] = (int)pair;
        samples[4 * b + 1] = (int)(((uint64_t)r.v[0] * uh) >> 32);
        samples[4 * b + 2] = (int)(((uint64_t)r.v[1] * uw) >> 32);
        samples[4 * b + 3] = (int)(r.v[2] >> 29) & code_mask;
    }
}

// the two-stage draw: a crop of side `full` from the image padded to `pad`, then the call's common window of side `patch` inside the
// augmented crop, emitted as one sample of side `patch`.  full == patch and pad == 0: the samples of oss_pairs_draw_kernel
__global__ void __launch_bounds__(256)
oss_pairs_draw_window_kernel(const int64_t *__restrict__ table, int n, int64_t *counter, int *__restrict__ samples, int batch, int patch,
                             int full, int pad, uint32_t k0, uint32_t k1, int rank, int world, int code_mask) {
    const uint64_t c = (uint64_t)*counter;
    __syncthreads();                                   // every thread has read c ...
    if (threadIdx.x == 0) *counter = (int64_t)(c + (uint64_t)batch);   // ... before it moves
    const uint64_t g0 = c * (uint64_t)world + (uint64_t)rank;
    const Philox4 win = philox4x32_10((uint32_t)g0, (uint32_t)(g0 >> 32), kTagWind, 0u, k0, k1);
    const uint32_t span = (uint32_t)(full - patch);
    const int wx0 = (int)(((uint64_t)win.v[0] * span) >> 32), wy0 = (int)(((uint64_t)win.v[1] * span) >> 32);   // rows, columns
    for (int b = threadIdx.x; b < batch; b += 256) {
        const uint64_t g = (c + (uint64_t)b) * (uint64_t)world + (uint64_t)rank;
        const uint64_t epoch = g / (uint64_t)n;
        const uint32_t pair = pairs_perm((uint32_t)(g - epoch * (uint64_t)n), (uint32_t)n, epoch, k0, k1);
        const Philox4 r = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), kTagCrop, 0u, k0, k1);
        const int64_t mh = max(table[4 * (int64_t)pair + 2], (int64_t)pad) - full + 1;
        const int64_t mw = max(table[4 * (int64_t)pair + 3], (int64_t)pad) - full + 1;
        const uint32_t uh = mh < 1 ? 1u : (uint32_t)mh, uw = mw < 1 ? 1u : (uint32_t)mw;   // a too-small image: the gather clamps and flags
        const int code = (int)(r.v[2] >> 29) & code_mask;
        const int wr = (code & 4) ? wy0 : wx0, wc = (code & 4) ? wx0 : wy0;
        samples[4 * b + 0] = (int)pair;
        samples[4 * b + 1] = (int)(((uint64_t)r.v[0] * uh) >> 32) + ((code & 2) ? (int)span - wr : wr);
        samples[4 * b + 2] = (int)(((uint64_t)r.v[1] * uw) >> 32) + ((code & 1) ? (int)span - wc : wc);
        samples[4 * b + 3] = code;
    }
}

// ---- gather -------------------------------------------------------------------------------------------------------------------
constexpr int kPairTile = 32, kPairPitch = kPairTile + 1;

struct PairArgs {
    const uint8_t *pool;
    const int64_t *table;
    const int *samples;
    float *lq, *gt;
    int *clamped;
    int64_t pool_bytes;
    int n_pairs, ph, pw, scale, swap, lq_tiles, lq_tiles_x, gt_tiles_x;
};
struct PairPadArgs : PairArgs {                             // the padded form is chosen by its argument block; the plain one keeps its layout
    int pad;                                                // the side (LQ pixels) the images are reflected up to
};

// cv2.BORDER_REFLECT at the far edge: fedcba|abcdefgh|hgfedcb, any number of periods
__device__ inline int pairs_reflect(int i, int n) {
    if (i < n) return i;                                    // every index of an image that needs no padding
    const int r = i % (2 * n);
    return r < n ? r : 2 * n - 1 - r;
}

template <int C, typename Args>
__global__ void __launch_bounds__(256)
oss_pairs_gather_kernel(const Args p) {
    constexpr bool PAD = std::is_same<Args, PairPadArgs>::value;
    constexpr int kWords = (kPairTile * C + 3) / 4 + 1;     // 4-byte words that cover a tile row at the worst alignment
    __shared__ float tile[C][kPairTile][kPairPitch];
    const int t = threadIdx.x, b = blockIdx.y;
    const bool is_gt = (int)blockIdx.x >= p.lq_tiles;
    const int tidx = is_gt ? (int)blockIdx.x - p.lq_tiles : (int)blockIdx.x;
    const int tiles_x = is_gt ? p.gt_tiles_x : p.lq_tiles_x;
    const int s = is_gt ? p.scale : 1;
    const int PH = p.ph * s, PW = p.pw * s;                 // the patch in this image's pixels
    const int r0 = (tidx / tiles_x) * kPairTile, x0 = (tidx % tiles_x) * kPairTile;

    // the sample and its image, clamped to what exists
    bool bad = false;
    int pair = p.samples[4 * b], top = p.samples[4 * b + 1], left = p.samples[4 * b + 2], code = p.samples[4 * b + 3];
    if (pair < 0 || pair >= p.n_pairs) pair = pair < 0 ? 0 : p.n_pairs - 1, bad = true;
    const int64_t *row = p.table + 4 * (int64_t)pair;
    const int64_t off = row[is_gt ? 0 : 1];
    int64_t lqh = row[2], lqw = row[3];
    if (lqh < 0 || lqh > (1 << 24)) lqh = 0, bad = true;
    if (lqw < 0 || lqw > (1 << 24)) lqw = 0, bad = true;
    int H = (int)lqh * s, W = (int)lqw * s;                 // the image
    if (off < 0 || off > p.pool_bytes || (int64_t)H * W * C > p.pool_bytes - off) H = 0, W = 0, bad = true;
    if ((code & ~7) || ((code & 4) && p.ph != p.pw)) code &= 3, bad = true;
    // PAD: the image as the reference's padding() extends it (an image without bytes stays empty: nothing to reflect)
    int VH = H, VW = W;
    if constexpr (PAD) {
        if (H > 0 && W > 0) VH = max(H, p.pad * s), VW = max(W, p.pad * s);
    }
    const int EH = min(PH, VH), EW = min(PW, VW);           // rows / columns of the patch that can be read
    const int64_t y64 = (int64_t)top * s, x64 = (int64_t)left * s;
    if (EH < PH || EW < PW || y64 < 0 || x64 < 0 || y64 > VH - EH || x64 > VW - EW) bad = true;
    const int y0 = (int)min(max(y64, (int64_t)0), (int64_t)(VH - EH)), xl = (int)min(max(x64, (int64_t)0), (int64_t)(VW - EW));
    if (bad && t == 0) *p.clamped = 1;
    const int th = min(max(EH - r0, 0), kPairTile), tw = min(max(EW - x0, 0), kPairTile);
    const int tin = PAD ? min(max(W - (xl + x0), 0), tw) : tw;   // columns of the tile that lie inside the image

    // 1. source rows -> LDS
    const uint8_t *src = p.pool + off + ((int64_t)(y0 + r0) * W + xl + x0) * C;
    const int nbytes = tin * C;
    for (int idx = t; idx < kPairTile * kWords; idx += 256) {
        const int r = idx / kWords, j = idx - r * kWords;
        if (r >= th) break;
        const uint8_t *run = PAD ? p.pool + off + ((int64_t)pairs_reflect(y0 + r0 + r, H) * W + xl + x0) * C : src + (int64_t)r * W * C;
        const int head = (int)(reinterpret_cast<uintptr_t>(run) & 3);
        const int k0 = 4 * j - head;                        // position in the run of this word's first byte
        if (k0 >= nbytes) continue;
        uint32_t w = 0;
        if (k0 >= 0 && k0 + 4 <= nbytes) {
            w = *reinterpret_cast<const uint32_t *>(run + k0);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (k0 + i >= 0 && k0 + i < nbytes) w |= (uint32_t)run[k0 + i] << (8 * i);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = k0 + i;
            if (k >= 0 && k < nbytes) {
                const int x = k / C, c = k - x * C;
                tile[(C == 3 && p.swap) ? 2 - c : c][r][x] = (float)((w >> (8 * i)) & 255u) / 255.0f;
            }
        }
    }
    if constexpr (PAD) {                                    // the reflected columns: one pixel per thread, bytes of the image only
        if (tin < tw) {
            const uint8_t *img = p.pool + off;
            for (int idx = t; idx < kPairTile * kPairTile; idx += 256) {
                const int r = idx / kPairTile, x = idx % kPairTile;
                if (r >= th || x < tin || x >= tw) continue;
                const uint8_t *px = img + ((int64_t)pairs_reflect(y0 + r0 + r, H) * W + pairs_reflect(xl + x0 + x, W)) * C;
#pragma unroll
                for (int c = 0; c < C; ++c) tile[(C == 3 && p.swap) ? 2 - c : c][r][x] = (float)px[c] / 255.0f;
            }
        }
    }
    __syncthreads();

    // 2. LDS -> destination rows
    const bool hf = code & 1, vf = code & 2, tr = code & 4;
    const int DW = tr ? PH : PW;
    float *dst = (is_gt ? p.gt : p.lq) + (int64_t)b * C * PH * PW;
    for (int e = t; e < C * kPairTile * kPairTile; e += 256) {
        const int c = e / (kPairTile * kPairTile), a = (e / kPairTile) % kPairTile, lane = e % kPairTile;
        const int r = tr ? lane : a, x = tr ? a : lane;
        if (r0 + r >= PH || x0 + x >= PW) continue;
        const float v = (r < th && x < tw) ? tile[c][r][x] : 0.0f;
        const int fy = vf ? PH - 1 - (r0 + r) : r0 + r, fx = hf ? PW - 1 - (x0 + x) : x0 + x;
        const int i = tr ? fx : fy, jj = tr ? fy : fx;
        dst[((int64_t)c * PH * PW) + (int64_t)i * DW + jj] = v;
    }
}

static inline int pair_tiles(int n) { return (n + kPairTile - 1) / kPairTile; }

static int pairs_ok(int channels, int scale, int ph, int pw, int batch) {
    if ((channels != 1 && channels != 3) || scale < 1 || scale > 64 || ph < 1 || pw < 1 || batch < 1 || batch > 65535) return 0;
    if ((int64_t)ph * scale > (1 << 20) || (int64_t)pw * scale > (1 << 20)) return 0;
    const int64_t tiles = (int64_t)pair_tiles(ph) * pair_tiles(pw) + (int64_t)pair_tiles(ph * scale) * pair_tiles(pw * scale);
    return tiles <= 65535;
}

template <typename Args>
static int pairs_gather_launch(const void *pool, int64_t pool_bytes, const int64_t *table, int n_pairs, const int *samples, float *lq,
                               float *gt, int *clamped, int batch, int channels, int patch_h, int patch_w, int scale, int swap_rb,
                               int pad_to, oss_stream_t stream) {
    if (!pool || !table || !samples || !lq || !gt || !clamped) return OSS_ERR_NULL;
    if (!pairs_ok(channels, scale, patch_h, patch_w, batch) || n_pairs < 1 || pool_bytes < 1) return OSS_ERR_SHAPE;
    Args p;
    p.pool = static_cast<const uint8_t *>(pool), p.table = table, p.samples = samples, p.lq = lq, p.gt = gt, p.clamped = clamped;
    p.pool_bytes = pool_bytes, p.n_pairs = n_pairs, p.ph = patch_h, p.pw = patch_w, p.scale = scale, p.swap = swap_rb ? 1 : 0;
    p.lq_tiles_x = pair_tiles(patch_w), p.gt_tiles_x = pair_tiles(patch_w * scale);
    p.lq_tiles = pair_tiles(patch_h) * p.lq_tiles_x;
    if constexpr (std::is_same<Args, PairPadArgs>::value) p.pad = pad_to;
    const dim3 grid(p.lq_tiles + pair_tiles(patch_h * scale) * p.gt_tiles_x, batch);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (channels == 3) hipLaunchKernelGGL((oss_pairs_gather_kernel<3, Args>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((oss_pairs_gather_kernel<1, Args>), grid, dim3(256), 0, s, p);
    return (int)hipGetLastError();
}

}  // namespace oss

using namespace oss;

extern "C" {

int oss_pairs_philox(const uint32_t *counter, const uint32_t *key, uint32_t *out) {
    if (!counter || !key || !out) return OSS_ERR_NULL;
    const Philox4 r = philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1]);
    for (int i = 0; i < 4; ++i) out[i] = r.v[i];
    return OSS_OK;
}

int oss_pairs_ok(int channels, int scale, int patch_h, int patch_w, int batch) {
    return pairs_ok(channels, scale, patch_h, patch_w, batch);
}

int oss_pairs_draw(const int64_t *table, int n_pairs, int64_t *counter, int *samples, int batch, int patch, int64_t seed, int rank,
                   int world, int flags, oss_stream_t stream) {
    if (!table || !counter || !samples) return OSS_ERR_NULL;
    if (n_pairs < 1 || batch < 1 || patch < 1 || world < 1 || rank < 0 || rank >= world || (flags & ~(OSS_PAIRS_HFLIP | OSS_PAIRS_ROT)))
        return OSS_ERR_SHAPE;
    const int code_mask = ((flags & OSS_PAIRS_HFLIP) ? 1 : 0) | ((flags & OSS_PAIRS_ROT) ? 6 : 0);
    hipLaunchKernelGGL(oss_pairs_draw_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), table, n_pairs, counter,
                       samples, batch, patch, (uint32_t)(uint64_t)seed, (uint32_t)((uint64_t)seed >> 32), rank, world, code_mask);
    return (int)hipGetLastError();
}

int oss_pairs_draw_window(const int64_t *table, int n_pairs, int64_t *counter, int *samples, int batch, int patch, int full_patch,
                          int pad_to, int64_t seed, int rank, int world, int flags, oss_stream_t stream) {
    if (!table || !counter || !samples) return OSS_ERR_NULL;
    if (n_pairs < 1 || batch < 1 || patch < 1 || full_patch < patch || full_patch > (1 << 20) || pad_to < 0 || pad_to > (1 << 20) ||
        world < 1 || rank < 0 || rank >= world || (flags & ~(OSS_PAIRS_HFLIP | OSS_PAIRS_ROT)))
        return OSS_ERR_SHAPE;
    const int code_mask = ((flags & OSS_PAIRS_HFLIP) ? 1 : 0) | ((flags & OSS_PAIRS_ROT) ? 6 : 0);
    hipLaunchKernelGGL(oss_pairs_draw_window_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), table, n_pairs,
                       counter, samples, batch, patch, full_patch, pad_to, (uint32_t)(uint64_t)seed, (uint32_t)((uint64_t)seed >> 32),
                       rank, world, code_mask);
    return (int)hipGetLastError();
}

int oss_pairs_gather(const void *pool, int64_t pool_bytes, const int64_t *table, int n_pairs, const int *samples, float *lq, float *gt,
                     int *clamped, int batch, int channels, int patch_h, int patch_w, int scale, int swap_rb, oss_stream_t stream) {
    return pairs_gather_launch<PairArgs>(pool, pool_bytes, table, n_pairs, samples, lq, gt, clamped, batch, channels, patch_h, patch_w,
                                      scale, swap_rb, 0, stream);
}

int oss_pairs_gather_padded(const void *pool, int64_t pool_bytes, const int64_t *table, int n_pairs, const int *samples, float *lq,
                            float *gt, int *clamped, int batch, int channels, int patch_h, int patch_w, int scale, int swap_rb,
                            int pad_to, oss_stream_t stream) {
    // the reference pads LQ and GT by the same pixel count: a pair only at scale 1
    if (pad_to < 0 || pad_to > (1 << 20) || (pad_to > 0 && scale != 1)) return OSS_ERR_SHAPE;
    return pairs_gather_launch<PairPadArgs>(pool, pool_bytes, table, n_pairs, samples, lq, gt, clamped, batch, channels, patch_h, patch_w,
                                     scale, swap_rb, pad_to, stream);
}

}  // extern "C"
