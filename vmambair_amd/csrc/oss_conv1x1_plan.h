// oss_conv1x1_plan.h -- what a 1x1-convolution call (forward / input gradient) launches, decided in ONE place.
//
// Plain C++17 without HIP types: the kernels' translation units (oss_conv1x1.hip, oss_conv1x1_wg.hip, oss_conv1x1_f32.hip), the C
// ABI (oss_capi.hip) and a host-only program (tools/conv1x1_plan_walk.cpp) include it.  conv1x1_plan is a pure function of a
// Conv1x1Call: shape, strides, the low 4 address bits of the tensors, which optional pointers are null, and the two test-only
// overrides (oss_conv1x1_set_wg) passed in as values -- it reads no globals.  The launchers compute a plan and switch on it to the
// instantiation; oss_conv1x1_describe returns the same plan without launching.  The weight-gradient launches and the pack launch
// are not planned here.
#pragma once
#include "../../include/vmambair_oss.h"
#include "oss_scan_plan.h"   // kMaxLdsBytes

#include <algorithm>
#include <stddef.h>
#include <stdint.h>

namespace oss {

// ---- thresholds, each next to the measurement it comes from ---------------------------------------------------------------------
// waves a launch of the whole-K pixel-pair kernels aims for (row tiles are dealt to more workgroups until it is reached):
// 1024 / 2048 / 4096: 177.0 / 176.2 / 175.0 images/s (profiles/r02_conv1x1_pipeline.txt)
constexpr long kPairTargetWaves = 1024;
// the `reuse` kernel (32 pixels per wave): enough waves to fill 256 CUs x 4 SIMDs twice, otherwise as few activation re-loads as
// possible
constexpr long kReuseTargetWaves = 2048;
// the K-chunked pixel-pair kernel accumulates up to kPairkMaxTiles row tiles per workgroup: the fewest re-loads that still give
// this many waves
constexpr long kPairkTargetWaves = 4096;
constexpr int kPairkMaxTiles = 3;
// fp32 tiles: a call with fewer one-wave tiles than this leaves every wave alone on its SIMD (a 1x1 convolution at batch 8 is 768
// tiles for 1024 SIMDs: 57 us per launch against ~5 us of matrix time, profiles/r04_ab_fp32_kernels.txt)
constexpr long kF32TileWaves = 3072;
// workgroup-level kernel: a workgroup per CU.  K = 96 / 192 want 128 pixels per workgroup when that still gives one, K <= 48 wants
// 64 until there are kWgNarrowTiles 128-pixel tiles; a launch with fewer workgroups than CUs (Deraining levels 1.. at batch 4) loses
// to the wave-level kernels unless its row tiles are split over more workgroups (tools/conv_wg_bench.py, and inside the SR and
// Deraining steps)
constexpr long kWgCus = 256;
constexpr long kWgNarrowTiles = 1024;
constexpr int kWgNarrowMaxK = 48;
constexpr int kPairwMaxK = 512;           // oss_conv1x1_pairw_kernel: KMAX, its LDS weight tile
constexpr int kMaxGridYZ = 65535;         // hipLaunchKernel: grid dimensions y and z
// split != 0 selects the split-bf16 products of the forward / input-gradient family (the weight-gradient family has its own
// switch in oss_conv1x1_f32x3.h; DESIGN.md 4.4, profiles/fp32_matmul_high_ab.txt)
constexpr bool kF32SplitGemm = true;

// ---- the call and the plan --------------------------------------------------------------------------------------------------------
// y[b, m, p] = sum_k W(m, k) x[b, k, p];  W(m, k) = w[m * ws_m + k * ws_k]:  forward M = cout, K = cin, (ws_m, ws_k) = (cin, 1);
// input gradient M = cin, K = cout, (ws_m, ws_k) = (1, cin).  x: (B, K, P) with strides (xsb, xsk); y: (B, M, P) contiguous.
struct Conv1x1Call {
    oss_dtype io;                 // OSS_F32 | OSS_F16 | OSS_BF16 (OSS_F32_BF16X3 arrives as OSS_F32 + f32_split)
    int B, M, K, P;
    int64_t xsb, xsk, ws_m, ws_k;
    unsigned x_lo, y_lo, w_lo, res_lo, wimg_lo;   // address & 15
    bool has_bias, has_res, has_wimg;
    bool f32_split;
    bool ln;                      // a LayerNorm fused in front (ln_conv1x1_wg): the workgroup-level kernel or nothing
    int wg_on, wg_pixels;         // oss_conv1x1_set_wg: 0 = never the workgroup-level kernel; 64 | 128 = its tile width, 0 = by shape
};
enum Conv1x1Family {
    CONV1X1_WG = 0,      // oss_conv1x1_wg_kernel<T, KS, WT, PT, RES, PF, LN, WIMG>
    CONV1X1_PAIR,        // oss_conv1x1_pair_kernel<T, KS, WT, WVEC, RES, PF, WIMG>
    CONV1X1_PAIRW,       // oss_conv1x1_pairw_kernel<T>
    CONV1X1_PAIRK,       // oss_conv1x1_pairk_kernel<T, 8, MT, WT, WVEC, WIMG>
    CONV1X1_REUSE,       // oss_conv1x1_reuse_kernel<T, KS, WT>
    CONV1X1_GENERIC,     // oss_conv1x1_kernel<T>
    CONV1X1_F32_TILE64,  // oss_conv1x1_f32_kernel<2, false, X3>
    CONV1X1_F32_TILE32,  // oss_conv1x1_f32_kernel<1, false, X3>
    CONV1X1_F32_SPLITK,  // oss_conv1x1_f32_kernel<1, true, X3>
};
struct Conv1x1Plan {
    Conv1x1Family family;
    int ks, mt;                   // template arguments; the ones a family does not have are 0
    bool wt, wvec, res, pf, wimg, ln, x3;
    int pt;                       // pixels per workgroup
    unsigned grid[3];
    int block;
    size_t lds_bytes;             // dynamic LDS
    int per, nz;                  // 32-row tiles per workgroup; wg: row-tile groups (gridDim.z)
};

// ---- workgroup-level kernel -----------------------------------------------------------------------------------------------------
constexpr int kWgXPad = 32;
// activation tile, fp32 output staging tiles (sized for their widest pitch, PT + 16), the LayerNorm weight / bias image
constexpr size_t conv1x1_wg_lds_bytes(int K, int pt, bool res) {
    return (size_t)K * 2 * (pt + kWgXPad) + (size_t)4 * 32 * (res ? 4 : 2) * (pt + 16) + 2 * (size_t)K * sizeof(float);
}
// built for the widths a power-of-two-times-{1,3} base width gives (K = 16, 32, 48, 64, 96, 128, 192: dim 16 / 32 / 48 / 64 and
// their doublings); K = 80, 112, 144, 160, 176 stay on the wave-level kernels (round 5: 80 instantiations nobody launched)
constexpr bool conv1x1_wg_ks_built(int ks) { return ks == 1 || ks == 2 || ks == 3 || ks == 4 || ks == 6 || ks == 8 || ks == 12; }
constexpr bool conv1x1_wg_pf(int ks) { return ks <= 6; }
constexpr bool conv1x1_io16(oss_dtype io) { return io == OSS_F16 || io == OSS_BF16; }
// does the workgroup-level kernel take the shape?  lo: address & 15 of x, y, w and res, or-ed
inline bool conv1x1_wg_takes(oss_dtype io, int M, int K, int P, int64_t xsb, int64_t xsk, unsigned lo, bool has_res) {
    // The fused skip connection (RES) is written and parity-green, but inside the training step it measured SLOWER than the
    // wave-level kernel (10.6 vs 9.4 us at 96 -> 96: the residual arrives cold from HBM behind the fp32 LDS round trip), so
    // those calls stay where they were and the RES instantiations are not built.
    if (has_res || !conv1x1_io16(io)) return false;
    if (K % 16 != 0 || K < 16 || K > 192 || P % 128 != 0 || M < 1 || !conv1x1_wg_ks_built(K / 16)) return false;
    if (xsb % 8 != 0 || xsk % 8 != 0 || (lo & 15u)) return false;
    return conv1x1_wg_lds_bytes(K, 128, has_res) <= kMaxLdsBytes;
}
// the input gradient + the backward of the LayerNorm in front (oss_conv1x1_dgrad_lnbwd_kernel): M = dim rows, K = cout.
// (An any-K form for project_in after norm2 -- K = 2 hidden = 510, 64-pixel workgroups, weights fetched in chunks of 8 k-steps --
// was built, parity-green, and measured slower inside the step: 219.2 against 221.7 images/s with the two separate kernels.)
inline bool conv1x1_lnbwd_takes(oss_dtype io, int M, int K, int P) {
    if (!conv1x1_io16(io)) return false;
    if (K % 16 != 0 || K < 2 * M || K > 192 || M < 1 || M > 128 || P % 128 != 0) return false;
    return K / 16 != 1 && conv1x1_wg_ks_built(K / 16);
}
inline int conv1x1_lnbwd_pixels(int B, int P) { return (long)B * (P / 128) >= kWgCus ? 128 : 64; }

inline void conv1x1_wg_plan(const Conv1x1Call &c, bool wt, Conv1x1Plan &pl) {
    const long t128 = (long)c.B * (c.P / 128);
    pl.family = CONV1X1_WG;
    pl.pt = c.wg_pixels ? c.wg_pixels : ((c.K <= kWgNarrowMaxK && t128 < kWgNarrowTiles) || t128 < kWgCus ? 64 : 128);
    const long wgs = (long)c.B * (c.P / pl.pt);
    const int groups = ((c.M + 31) / 32 + 3) / 4;           // row tiles in units of a workgroup's four waves
    pl.nz = (int)std::max<long>(1, std::min<long>(groups, (kWgCus + wgs - 1) / wgs));
    pl.per = 4 * ((groups + pl.nz - 1) / pl.nz);
    pl.ks = c.K / 16;
    pl.wt = wt; pl.pf = conv1x1_wg_pf(pl.ks); pl.ln = c.ln; pl.wimg = c.has_wimg;
    pl.grid[0] = c.P / pl.pt; pl.grid[1] = c.B; pl.grid[2] = pl.nz;
    pl.block = 256;
    pl.lds_bytes = conv1x1_wg_lds_bytes(c.K, pl.pt, c.has_res);
}

// ---- wave-level 16-bit kernels ----------------------------------------------------------------------------------------------------
// PF of the whole-K pixel-pair kernel (the next tile's operands in flight during the current tile): the raw fp32 fragments of two
// tiles fit up to 6 k-steps, the 16-bit fragments of an image up to 8
constexpr bool conv1x1_pair_pf(int ks, bool wimg) { return ks <= (wimg ? 8 : 6); }
// row tiles per workgroup that still give `target` waves when `waves_p` waves cover the pixels of one row tile
inline int conv1x1_tiles_per_wg(long target, long waves_p, int mt) {
    const int split = (int)std::max<long>(1, std::min<long>(mt, (target + waves_p - 1) / waves_p));
    return (mt + split - 1) / split;
}
// The forward's weight tile through LDS (oss_conv1x1_pairw_kernel) instead of per-lane fp32 loads.  per == 0: asked before the
// whole-K / K-chunk split, for rows that are not 16-byte aligned (K = 127, the EFFN hidden width at dim 48; K = 255 likewise);
// per > 0: asked by the K-chunk form with its row tiles per workgroup -- one tile leaves nothing for the chunk kernel to reuse.
inline bool conv1x1_pairw_takes(const Conv1x1Call &c, bool plain, bool wvec, int per) {
    if (c.has_wimg || !plain || c.K > kPairwMaxK || (c.w_lo & 15u)) return false;
    return per == 0 ? (!wvec && c.K > 16 * 3) : per == 1;
}

inline void conv1x1_wave_plan(const Conv1x1Call &c, bool wt, bool plain, Conv1x1Plan &pl) {
    const int M = c.M, K = c.K, P = c.P, B = c.B;
    const int mt = (M + 31) / 32;
    const bool small_index = c.xsk < (1 << 24) && (size_t)M * K < (1u << 30);
    const bool w16 = (c.w_lo & 15u) == 0;
    pl.block = 256;
    pl.grid[1] = B;
    // pixel-pair form: even P, even row strides, 4-byte aligned bases
    if (P % 2 == 0 && c.xsk % 2 == 0 && c.xsb % 2 == 0 && small_index && (wt || plain) && ((c.x_lo | c.y_lo) & 3u) == 0) {
        const bool wvec = plain && K % 8 == 0 && w16;
        const long waves_p = (long)B * ((P + 63) / 64);
        pl.pt = 256;
        pl.grid[0] = (P + 255) / 256;
        // with an image WT / WVEC are ignored by the kernels and left false
        pl.wimg = c.has_wimg; pl.wt = wt && !pl.wimg; pl.wvec = wvec && !wt && !pl.wimg;
        if (conv1x1_pairw_takes(c, plain, wvec, 0)) pl.family = CONV1X1_PAIRW;
        else if (K <= 16 * 12) {
            // whole K in registers: enough workgroups to fill the chip, otherwise as few activation re-loads as possible
            pl.family = CONV1X1_PAIR;
            pl.per = conv1x1_tiles_per_wg(kPairTargetWaves, waves_p, mt);
            pl.ks = K <= 16 * 3 ? 3 : K <= 16 * 6 ? 6 : K <= 16 * 8 ? 8 : 12;   // K = 127: 8, no duplicate k-steps
            pl.pf = conv1x1_pair_pf(pl.ks, pl.wimg);
            pl.res = c.has_res;
        } else {
            // K in chunks of 128: up to 3 row tiles accumulate per workgroup (fewest re-loads that still fill the chip)
            int per = kPairkMaxTiles;
            while (per > 1 && waves_p * ((mt + per - 1) / per) < kPairkTargetWaves) --per;
            per = std::min(per, mt);
            if (conv1x1_pairw_takes(c, plain, wvec, per)) pl.family = CONV1X1_PAIRW;
            else { pl.family = CONV1X1_PAIRK; pl.ks = 8; pl.mt = pl.per = per; }
        }
        if (pl.family == CONV1X1_PAIRW) { pl.per = 1; pl.wt = pl.wvec = false; }
    } else if (K <= 16 * 12 && small_index && (wt || (plain && K % 8 == 0 && w16))) {
        pl.family = CONV1X1_REUSE;
        pl.pt = 128;
        pl.grid[0] = (P + 127) / 128;
        pl.per = conv1x1_tiles_per_wg(kReuseTargetWaves, (long)B * ((P + 31) / 32), mt);
        pl.ks = K <= 16 * 6 ? 6 : 12;
        pl.wt = wt;
    } else {
        pl.family = CONV1X1_GENERIC;
        pl.pt = 128;
        pl.grid[0] = (P + 127) / 128;
        pl.per = 1;
    }
    pl.grid[2] = (mt + pl.per - 1) / pl.per;
}

// ---- fp32 I/O ---------------------------------------------------------------------------------------------------------------------
// The GEMM of oss_conv1x1_f32.hip: bg = batch x G products of (M x K) (K x P); G > 1 are the x_proj / dt_proj products of the four
// scan directions.  aligned: every tensor base 16-byte aligned and every stride a multiple of 4 (the caller knows its tensors).
inline int conv1x1_f32_plan(int M, int K, int P, long bg, bool aligned, bool split, Conv1x1Plan &pl) {
    pl = Conv1x1Plan{};
    if (M < 1 || K < 1 || P < 4 || P % 4 != 0 || !aligned || bg <= 0 || bg > kMaxGridYZ) return OSS_ERR_SHAPE;
    pl.x3 = split && kF32SplitGemm;
    const long px = (P + 127) / 128;
    const long waves64 = px * ((M + 63) / 64) * bg, waves32 = px * ((M + 31) / 32) * bg;
    pl.pt = 128;
    pl.block = 64;
    if (waves64 >= kF32TileWaves && M > 32) {   // plenty of tiles: 64-row tiles, one wave each
        pl.family = CONV1X1_F32_TILE64;
        pl.mt = 2;
    } else if (waves32 >= kF32TileWaves || K < (pl.x3 ? 64 : 32)) {   // 32-row tiles, one wave each (a short K has nothing to split: x3 works in rounds of 16)
        pl.family = CONV1X1_F32_TILE32;
        pl.mt = 1;
    } else {                                    // few tiles: four waves per tile, a quarter of K each, summed through LDS
        pl.family = CONV1X1_F32_SPLITK;
        pl.mt = 1;
        pl.block = 256;
        pl.lds_bytes = sizeof(float) * 3 * 16 * 64 * 4;   // [3 waves][16 quads][64 lanes][4]
    }
    pl.per = pl.mt;
    pl.grid[0] = (unsigned)px; pl.grid[1] = (M + 32 * pl.mt - 1) / (32 * pl.mt); pl.grid[2] = (unsigned)bg;
    return pl.grid[1] > (unsigned)kMaxGridYZ ? OSS_ERR_SHAPE : OSS_OK;
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------------
inline int conv1x1_plan(const Conv1x1Call &c, Conv1x1Plan &pl) {
    pl = Conv1x1Plan{};
    if (c.B <= 0 || c.M <= 0 || c.K <= 0 || c.P <= 0) return OSS_ERR_SHAPE;
    const bool wt = (c.ws_m == 1 && c.ws_k == c.M);          // input gradient: weights read transposed
    const bool plain = (c.ws_k == 1 && c.ws_m == c.K);
    const bool wg = (wt || plain) && conv1x1_wg_takes(c.io, c.M, c.K, c.P, c.xsb, c.xsk, c.x_lo | c.y_lo | c.w_lo | c.res_lo, c.has_res);
    if (c.ln || (wg && c.wg_on)) {
        if (!wg || (c.wimg_lo & 15u)) return OSS_ERR_SHAPE;
        conv1x1_wg_plan(c, wt, pl);
    } else if (c.io == OSS_F32) {
        const bool aligned = ((c.x_lo | c.y_lo | c.res_lo) & 15u) == 0 && c.xsb % 4 == 0 && c.xsk % 4 == 0;
        return conv1x1_f32_plan(c.M, c.K, c.P, c.B, aligned, c.f32_split, pl);
    } else if (conv1x1_io16(c.io)) {
        conv1x1_wave_plan(c, wt, plain, pl);
    } else {
        return OSS_ERR_SHAPE;
    }
    if (pl.grid[1] > (unsigned)kMaxGridYZ || pl.grid[2] > (unsigned)kMaxGridYZ || pl.lds_bytes > kMaxLdsBytes) return OSS_ERR_SHAPE;
    return OSS_OK;
}

}  // namespace oss
