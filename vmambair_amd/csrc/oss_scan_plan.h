// oss_scan_plan.h -- what a selective-scan call launches, decided in ONE place.
//
// Plain C++17 without HIP types: the kernels' translation units, the C ABI (oss_capi.hip) and a host-only program
// (tools/scan_plan_walk.cpp) include it.  scan_fwd_plan / scan_bwd_plan are pure functions of the parameter block's integers
// and of which of its pointers are null (workspace, hs, dt_weight, dD, ddelta_bias, ddt, ddt_weight), plus the one test-only
// global g_carry_split.  The launchers (oss_scan_fwd.hip, oss_scan_bwd.hip) branch on a plan and on nothing else; the workspace
// size queries and oss_scan_*_describe are built from the same helpers, so the three cannot drift apart.
#pragma once
#include "../../include/vmambair_oss.h"

#include <algorithm>
#include <atomic>
#include <stddef.h>

namespace oss {

constexpr int kScanChunk = 256;  // time steps between saved states in x (oss_scan_chunk())
constexpr int kNB = 16;          // states per LDS tile
constexpr int kMaxDtRank = 8;    // fused-delta form: rank of the dt factor (include/vmambair_oss.h: dt_weight)
constexpr int kMaxSegments = 64; // time segments / carry slots per row
constexpr size_t kMaxLdsBytes = 160 * 1024;   // gfx950: 160 KiB per workgroup
// lane states (include/vmambair_oss.h: hs): entries per (batch, row, state) line, one per 8 scan steps, padded to whole 512-step chunks
constexpr size_t lane_state_stride(int seqlen) { return (size_t)(((seqlen + 7) / 8 + 63) & ~63); }
// padded LDS tiles of the forward (oss_device.h: tile_off_pad): floats between the quad planes, floats per state row
constexpr int tile_plane_pad(int items) { return 128 / items; }
constexpr int tile_row_pad(int lpr, int items) { return lpr * items + (items / 4) * tile_plane_pad(items); }
// slab of the round-2 backward (oss_scan_bwd_v2.h: SlabQ)
constexpr int kSlabK = 288;            // floats between the two quads of a lane
constexpr int kSlabA = 2 * kSlabK;     // floats per (row, dB | dC) array

// ---- kernel shapes ------------------------------------------------------------------------------------------------------------
// forward variants: (lanes per row, items per lane, waves per workgroup)
//   0: 64 x 8  x 8   (TC  512,  8 rows/WG)   many waves for small batches
//   1: 32 x 16 x 8   (TC  512, 16 rows/WG)
//   2: 16 x 16 x 4   (TC  256, 16 rows/WG)   fewest scan steps, needs many rows
//   3: 64 x 16 x 8   (TC 1024,  8 rows/WG)
//   4: 64 x 4  x 4   (TC  256,  4 rows/WG)   short sequences / few rows per group; every other number means 4, and so does a
//                                            launch whose tiles + per-row carries do not fit the LDS (large dstate)
//   6: 64 x 16 x 12  (TC 1024, 12 rows/WG): row counts that give <= 256 such workgroups
struct ScanFwdShape {
    int variant, lpr, items, waves;
    constexpr int rows() const { return waves * (64 / lpr); }
    constexpr int chunk() const { return lpr * items; }
    size_t lds_bytes(int dstate) const { return sizeof(float) * (2 * (size_t)kNB * tile_row_pad(lpr, items) + 3 * (size_t)dstate * rows()); }
};
constexpr ScanFwdShape kScanFwdSmall = {4, 64, 4, 4};
constexpr ScanFwdShape kScanFwdShapes[] = {{0, 64, 8, 8}, {1, 32, 16, 8}, {2, 16, 16, 4}, {3, 64, 16, 8}, {6, 64, 16, 12}, kScanFwdSmall};
// backward variants (0 and 2..9 were removed in round 4 and mean 1):
//   1: round-1 kernel, 64 lanes x 4 items, 4 rows/WG, 16 states per LDS tile (TC 256, 40 KiB LDS): short sequences, few rows
//      per group and dstate > 64 (the round-2 kernel keeps one lane per state); never cut in time
//  10: round-2 kernel (oss_scan_bwd_v2.h), 12 rows/WG (128 KiB LDS)   11: 8 rows/WG   12: 6 rows/WG   13: 4 rows/WG
struct ScanBwdShape { int variant, rows, chunk; };
constexpr int kBwd1TileStates = 16, kBwd2TileStates = 4;   // states per LDS tile of the round-1 / round-2 kernel
constexpr ScanBwdShape kScanBwdSmall = {1, 4, 256};
constexpr ScanBwdShape kScanBwdShapes[] = {kScanBwdSmall, {10, 12, 512}, {11, 8, 512}, {12, 6, 512}, {13, 4, 512}};

// ---- variant heuristics -------------------------------------------------------------------------------------------------------
// The forward/backward kernels are VALU-bound, so the cheapest variant in instructions per
// (element, state) wins as long as the launch still fills 256 CUs x 4 SIMDs with >= 2 waves.
inline int scan_fwd_pick_variant(int batch, int dim, int seqlen, int dstate, int n_groups, int elem_bytes) {
    (void)dstate; (void)elem_bytes;
    const int rows_per_group = dim / n_groups;
    const long rows = (long)batch * dim;
    if (seqlen <= 256 || rows_per_group < 8) return (rows_per_group >= 16 && rows >= 4096) ? 2 : 4;
    // 16 lanes per row (4 rows per wave): fewest scan steps, but only rows/4 waves
    if (rows_per_group % 16 == 0 && rows / 4 >= 2048) return 2;
    if (rows_per_group % 16 == 0 && rows / 2 >= 2048) return 1;
    // long sequences whose 12-row tiles leave CUs idle (RealSR tiles at batch 1: u:(1,384,25600) is 32 workgroups; Deraining
    // level 0 at batch 4: 64): the widest workgroup, cut into time segments by scan_pick_segments until the CUs are covered
    // (u:(1,384,25600) f16 0.129 ms in 9 segments against 0.354 ms for one 8-row workgroup per tile; u:(4,192,16384) bf16
    // 0.139 in 4 segments against 0.222 -- profiles/r03_segment_sweep.txt)
    // (u:(1,768,6400) f16: 0.070 ms in 4 segments against 0.093.  At exactly 128 such workgroups -- u:(8,192,4096), u:(4,384,4096) --
    // variant 3 stayed ahead until round 5; with the local pass cut finer than the main launch (oss_scan_set_carry_split) two
    // segments of the 12-row form win there too: u:(4,384,4096) bf16 0.059 against 0.064 ms, profiles/r05_sweep_batch4_scan_variants_and_segments.txt)
    if (seqlen >= 4096 && rows_per_group % 12 == 0 && (long)batch * n_groups * (rows_per_group / 12) <= 128) return 6;
    // <= one 8-row workgroup per CU and a long sequence: 16 items per lane (half the chunk hand-overs; u:(8,192,4096)
    // bf16 0.065 ms against 0.077, profiles/r01_sweep_v4_bwd_variants.txt)
    if (seqlen >= 1024 && (long)batch * n_groups * ((rows_per_group + 7) / 8) <= 256) return 3;
    // 12-row workgroups when they give <= one workgroup per CU (u:(8,384,4096) bf16: 0.081 ms against 0.113)
    if (seqlen >= 1024 && rows_per_group >= 12 && (long)batch * n_groups * ((rows_per_group + 11) / 12) <= 256) return 6;
    return 0;
}

inline int scan_bwd_pick_variant(int batch, int dim, int seqlen, int dstate, int n_groups) {
    const int rows_per_group = dim / n_groups;
    // short sequences, few rows per group, dstate > 64 (the round-2 kernel keeps one lane per state): the round-1 kernel
    if (seqlen <= 256 || rows_per_group < 8 || dstate > 64) return 1;
    const long wgs = (long)batch * n_groups * ((rows_per_group + 7) / 8);
    // round-2 kernel (oss_scan_bwd_v2.h) from here on: u:(8,192,4096) 0.172 ms against 0.203 for the round-1 kernel,
    // u:(8,384,4096) 0.235 against 0.284 (profiles/r02_scan_bwd_v2_experiments.txt)
    // long sequences whose 12-row tiles leave CUs idle: 12-row workgroups cut into time segments (scan_pick_segments) instead
    // of ever smaller row tiles -- a third of the dB / dC partial tiles of the 4-row form and three waves per SIMD
    // (u:(4,192,16384) bf16: 0.328 + 0.029 ms in 4 segments against 0.590 + 0.087 for variant 13; u:(1,384,25600) f16:
    // 0.293 + 0.022 in 9 segments against 1.316 -- profiles/r03_segment_sweep.txt)
    // (u:(8,192,4096) bf16, 128 such workgroups: 0.166 + 0.015 ms in 2 segments against 0.168 + 0.020 for variant 11)
    if (seqlen >= 2048 && rows_per_group % 12 == 0 && (long)batch * n_groups * (rows_per_group / 12) < 192) return 10;
    // very few rows (Deraining level 0 at batch 4: 96 8-row workgroups for 256 CUs): 4-row workgroups spread the same waves over
    // twice the CUs, one wave per SIMD instead of two (u:(4,192,16384): 0.585 ms against 0.684)
    if (wgs <= 128 && rows_per_group % 4 == 0) return 13;
    if (wgs <= 256) return 11;
    // more rows per workgroup: fewer dB / dC partial tiles and an even load (u:(8,384,4096) bf16: 0.271 ms against
    // 0.355; u:(32,384,4096): 1.07 against 1.14)
    return rows_per_group >= 12 ? 10 : 11;
}

// ---- time segments ------------------------------------------------------------------------------------------------------------
// Time-segmented launches (oss_scan_fwd.hip: FwdSeg, oss_scan_bwd_v2.h: BwdSeg).  seg_req: -1 = heuristic, 0 / 1 = never,
// n > 1 = n segments (clamped to the number of chunks).
// Segments of a launch that has `wgs` workgroups (one per CU at a time for the wide variants) over `n_chunks` chunks when
// it is not cut in time.  Cost model in units of one chunk of one workgroup: rounds over the 256 CUs x chunks per segment x
// (1 + ovh), where ovh is the extra sweep a segmented launch pays (forward: the B side of the step again, ~0.55 of a pass;
// backward: the reverse recurrence alone, ~0.3).  Launches that already put a workgroup on every CU are left alone, and a
// larger segment count has to win by 5 % to be taken.
constexpr double kFwdSegOverhead = 0.55, kBwdSegOverhead = 0.3;
inline int scan_pick_segments(long wgs, int n_chunks, int seg_req, double ovh) {
    if (seg_req == 0 || seg_req == 1 || n_chunks < 2 || wgs <= 0) return 1;
    if (seg_req > 1) return std::min(std::min(seg_req, n_chunks), kMaxSegments);
    if (wgs >= 256) return 1;
    int best = 1;
    double best_cost = (double)n_chunks;
    for (int s = 2; s <= std::min(n_chunks, 16); ++s) {
        const int cps = (n_chunks + s - 1) / s;
        if ((n_chunks + cps - 1) / cps != s) continue;   // not a segment count this chunk count can have
        const double rounds = (double)((wgs * s + 255) / 256);
        const double cost = rounds * cps * (1.0 + ovh);
        if (cost < 0.95 * best_cost) { best = s; best_cost = cost; }
    }
    return best;
}

// bytes of n_slots (product, state) carry pairs per (batch, row, state)
inline size_t scan_carry_bytes(int batch, int dim, int dstate, int n_slots) {
    return sizeof(float) * 2 * (size_t)batch * dim * dstate * n_slots;
}
// carry slots per row that the workspace queries size for: one per chunk of the variant, at most kMaxSegments
inline int scan_max_slots(int n_chunks) { return std::min(n_chunks, kMaxSegments); }

// pieces of the first (local / carry) launch per main segment: the largest piece count c <= forced (forced > 0), or with
// wgs * (n_seg - 1) * c <= 512 (heuristic), whose n_seg * c carry slots fit what the workspace queries allow.  A main segment
// of cps chunks is cut into c pieces of ceil(cps / c) chunks, the last one shorter (oss_scan_set_carry_split)
inline std::atomic<int> g_carry_split{0};   // test-only global (oss_scan_set_carry_split); a call's own field wins over it
inline int scan_carry_split(long wgs, int n_seg, int cps, int n_chunks, int per_call = 0) {
    if (n_seg <= 1) return 1;
    const int forced = per_call > 0 ? per_call : g_carry_split.load();
    int csub = 1;
    for (int c = 2; c <= cps; ++c) {
        const int ccps = (cps + c - 1) / c, pieces = (cps + ccps - 1) / ccps;   // pieces of ccps chunks, the last one shorter
        if (n_seg * pieces > scan_max_slots(n_chunks)) break;
        if (forced > 0 ? pieces <= forced : wgs * (n_seg - 1) * pieces <= 512) csub = pieces;
    }
    return csub;
}

// the five segment numbers of FwdSeg / BwdSeg: n_seg segments of cps chunks; the first launch cuts each into csub pieces of ccps
// chunks, n_cseg = n_seg * csub carry slots per row
struct ScanSegs { int n_seg, cps, csub, ccps, n_cseg; };
// The candidates of a launch with `wgs` workgroups over `n_chunks` chunks, in the order the workspace ladder tries them: the
// picked segments with the finer carry split, the same segments with csub = 1, unsegmented.  fused_delta: never cut in time.
struct ScanSegLadder { ScanSegs step[3]; };
inline ScanSegLadder scan_seg_ladder(long wgs, int n_chunks, int seg_req, double ovh, bool fused_delta, int carry_split) {
    const ScanSegs none = {1, n_chunks, 1, n_chunks, 1};
    ScanSegs fine = none;
    const int n_req = fused_delta ? 1 : scan_pick_segments(wgs, n_chunks, seg_req, ovh);
    if (n_req > 1) {
        fine.cps = (n_chunks + n_req - 1) / n_req;
        fine.n_seg = (n_chunks + fine.cps - 1) / fine.cps;
        fine.csub = scan_carry_split(wgs, fine.n_seg, fine.cps, n_chunks, carry_split);
        fine.ccps = (fine.cps + fine.csub - 1) / fine.csub;
        fine.n_cseg = fine.n_seg * fine.csub;
    }
    ScanSegs coarse = fine;
    coarse.csub = 1; coarse.ccps = coarse.cps; coarse.n_cseg = coarse.n_seg;
    return {{fine, coarse, none}};
}

// ---- backward workspace -------------------------------------------------------------------------------------------------------
// layout (float offsets from the workspace pointer):
//   [bc, dA)   dB/dC (+ d dt-factor) partials  [batch][group][tile][2 N + rp][L]   (bf16 partials use the front half)
//   dA partials [wbatch][dim][N], dD and ddelta_bias partials [wbatch][dim] each, dt-weight partials [wbatch][dim][kMaxDtRank]
//   (fused-delta form only: rp = dt_rank > 0), then the reverse-carry pairs of a time-segmented launch.
// wbatch = batch * n_seg: one weight-gradient partial per (batch, segment, row).
inline size_t ws_bc_floats(int batch, int G, int tiles, int N, int L, int RP = 0) {
    return (size_t)batch * G * tiles * (2 * N + RP) * L;
}
struct ScanBwdWs {
    size_t bc, dA, dD, db, dW, carry;   // dW: meaningful when rp > 0
    int tiles, rp, wbatch;
    size_t need_bytes;
};
inline ScanBwdWs scan_bwd_ws(int batch, int dim, int seqlen, int dstate, int n_groups, int rows_per_wg, int rp, const ScanSegs &sg) {
    ScanBwdWs w;
    w.tiles = (dim / n_groups + rows_per_wg - 1) / rows_per_wg;
    w.rp = rp;
    w.wbatch = batch * sg.n_seg;
    const size_t rows = (size_t)w.wbatch * dim;
    w.bc = 0;
    w.dA = ws_bc_floats(batch, n_groups, w.tiles, dstate, seqlen, rp);
    w.dD = w.dA + rows * dstate;
    w.db = w.dD + rows;
    w.dW = w.db + rows;
    w.carry = w.dW + (rp ? rows * kMaxDtRank : 0);
    w.need_bytes = sizeof(float) * w.carry + (sg.n_seg > 1 ? scan_carry_bytes(batch, dim, dstate, sg.n_cseg) : 0);
    return w;
}

// ---- the plans ----------------------------------------------------------------------------------------------------------------
struct ScanFwdPlan {
    ScanFwdShape kernel;   // the instantiation that runs, after the LDS remap
    bool fused_delta;      // FD: delta evaluated from the rank-R factor
    int tiles, n_chunks;   // row tiles per group, chunks of kernel.chunk() steps
    long wgs;              // batch * groups * tiles: workgroups of an unsegmented launch
    size_t lds_bytes;      // dynamic LDS of every launch of the call
    ScanSegs seg;
    size_t need_bytes;     // of the caller's workspace (the carry pairs)
};
struct ScanBwdPlan {
    ScanBwdShape kernel;   // after the remaps; kernel.variant >= 10: the round-2 kernel
    bool fused_delta, bf16_partials, lane_states, slab_q;
    int tiles, n_chunks;
    long wgs;
    size_t lds_bytes;      // of the main kernel
    ScanSegs seg;
    ScanBwdWs ws;          // carving of the caller's workspace; ws.wbatch = batch * n_seg, ws.need_bytes
};

inline int scan_plan_shape_ok(const oss_scan_fwd_params &p) {
    if (p.batch <= 0 || p.dim <= 0 || p.seqlen <= 0 || p.dstate <= 0 || p.n_groups <= 0 || p.dim % p.n_groups != 0) return OSS_ERR_SHAPE;
    if (p.dt_weight && (p.dt_rank < 1 || p.dt_rank > kMaxDtRank)) return OSS_ERR_SHAPE;
    return OSS_OK;
}

inline int scan_fwd_plan(const oss_scan_fwd_params &p, oss_dtype io, int variant, int seg_req, ScanFwdPlan &pl) {
    (void)io;
    if (const int rc = scan_plan_shape_ok(p)) return rc;
    pl.kernel = kScanFwdSmall;
    for (const ScanFwdShape &s : kScanFwdShapes)
        if (s.variant == variant) pl.kernel = s;
    // large dstate: tiles + per-row carries no longer fit 160 KiB -> the small-shape variant (4 rows, 256-step chunks)
    if (pl.kernel.lds_bytes(p.dstate) > kMaxLdsBytes) pl.kernel = kScanFwdSmall;
    pl.lds_bytes = pl.kernel.lds_bytes(p.dstate);
    if (pl.lds_bytes > kMaxLdsBytes) return OSS_ERR_SHAPE;
    pl.fused_delta = p.dt_weight != nullptr;
    pl.tiles = (p.dim / p.n_groups + pl.kernel.rows() - 1) / pl.kernel.rows();
    pl.wgs = (long)p.batch * p.n_groups * pl.tiles;
    pl.n_chunks = (p.seqlen + pl.kernel.chunk() - 1) / pl.kernel.chunk();
    // the carry slots are per LOCAL-pass piece.  A caller's workspace that holds the main segments' slots but not the finer
    // pieces' keeps the segments and drops the finer split; only one that does not hold even those (or none) goes unsegmented
    for (const ScanSegs &sg : scan_seg_ladder(pl.wgs, pl.n_chunks, seg_req, kFwdSegOverhead, pl.fused_delta, p.tune_carry_split).step) {
        pl.seg = sg;
        pl.need_bytes = sg.n_seg > 1 ? scan_carry_bytes(p.batch, p.dim, p.dstate, sg.n_cseg) : 0;
        if (sg.n_seg == 1 || (p.workspace && pl.need_bytes <= p.workspace_bytes)) break;
    }
    return OSS_OK;
}

inline int scan_bwd_plan(const oss_scan_bwd_params &p, oss_dtype io, int variant, int seg_req, ScanBwdPlan &pl) {
    const oss_scan_fwd_params &f = p.f;
    if (const int rc = scan_plan_shape_ok(f)) return rc;
    pl.fused_delta = f.dt_weight != nullptr;
    if (pl.fused_delta) {   // delta computed inside the scan: round-2 kernels only
        if (f.dstate > 64 || !p.ddt || !p.ddt_weight) return OSS_ERR_SHAPE;
        if (variant < 10) variant = 13;
    }
    if (variant >= 10 && f.dstate > 64) variant = 1;   // the round-2 kernel keeps one lane per state
    pl.kernel = kScanBwdSmall;
    for (const ScanBwdShape &s : kScanBwdShapes)
        if (s.variant == variant) pl.kernel = s;
    const bool round2 = pl.kernel.variant >= 10;
    const int rows = pl.kernel.rows, TC = pl.kernel.chunk;
    // bf16 row-tile partials (oss_scan_bwd_v2.h: kPartialsBf16Ok): only when THIS call asks for them (tune_partials == 2);
    // lane states saved by the forward pass (f.hs): the kernels that load them instead of re-running the forward recurrence
    pl.bf16_partials = round2 && !pl.fused_delta && io == OSS_BF16 && p.tune_partials == 2 && !f.hs;
    pl.lane_states = round2 && !pl.fused_delta && !pl.bf16_partials && f.hs != nullptr;
    pl.slab_q = round2 && !pl.fused_delta && !(pl.lane_states && rows > 8);   // oss_scan_bwd2_kernel: SQ
    pl.tiles = (f.dim / f.n_groups + rows - 1) / rows;
    pl.wgs = (long)f.batch * f.n_groups * pl.tiles;
    pl.n_chunks = (f.seqlen + TC - 1) / TC;
    if (round2)   // two tile buffers, two slab buffers (+ dt weights | + two buffers of this wave's lane states)
        pl.lds_bytes = sizeof(float) * (4 * (size_t)kBwd2TileStates * TC + 4 * (size_t)rows * (pl.slab_q ? kSlabA : TC) +
                                        (pl.fused_delta ? rows * kMaxDtRank : 0) + (pl.lane_states ? 2 * (size_t)rows * kBwd2TileStates * 64 : 0));
    else          // tiles, one slab, the per-row state tables
        pl.lds_bytes = sizeof(float) * (2 * (size_t)kBwd1TileStates * TC + 2 * (size_t)rows * TC + 3 * (size_t)f.dstate * rows + rows);
    if (pl.lds_bytes > kMaxLdsBytes) return OSS_ERR_SHAPE;
    // room for the main segments' carry pairs but not the finer pieces': csub = 1; a caller that sized the workspace for the
    // unsegmented form: one segment; less than that is an error
    const int rp = pl.fused_delta ? f.dt_rank : 0;
    for (const ScanSegs &sg : scan_seg_ladder(pl.wgs, pl.n_chunks, round2 ? seg_req : 1, kBwdSegOverhead, pl.fused_delta, f.tune_carry_split).step) {
        pl.seg = sg;
        pl.ws = scan_bwd_ws(f.batch, f.dim, f.seqlen, f.dstate, f.n_groups, rows, rp, sg);
        if (p.workspace && pl.ws.need_bytes <= p.workspace_bytes) return OSS_OK;
    }
    return OSS_ERR_WORKSPACE;
}

// ---- workspace size queries: the worst case over the variants, every one with as many carry slots as it has chunks -----------
inline size_t scan_fwd_workspace_bytes(int batch, int dim, int seqlen, int dstate, int n_groups) {
    if (batch <= 0 || dim <= 0 || seqlen <= 0 || dstate <= 0 || n_groups <= 0 || dim % n_groups) return 0;
    size_t worst = 0;
    for (const ScanFwdShape &s : kScanFwdShapes) {
        const int slots = scan_max_slots((seqlen + s.chunk() - 1) / s.chunk());
        if (slots > 1) worst = std::max(worst, scan_carry_bytes(batch, dim, dstate, slots));
    }
    return worst;
}
// ... and with the partial rows and dt-weight partials of the fused-delta form at its largest rank.  The round-1 kernel is
// sized like the 4-row round-2 kernel (generous: it never segments), as every release so far has done.
inline size_t scan_bwd_workspace_bytes(int batch, int dim, int seqlen, int dstate, int n_groups) {
    if (batch <= 0 || dim <= 0 || seqlen <= 0 || dstate <= 0 || n_groups <= 0 || dim % n_groups) return 0;
    size_t worst = 0;
    for (const ScanBwdShape &s : kScanBwdShapes) {
        if (s.variant < 10) continue;
        const int n_chunks = (seqlen + s.chunk - 1) / s.chunk, slots = scan_max_slots(n_chunks);
        const ScanSegs sg = {slots, (n_chunks + slots - 1) / slots, 1, (n_chunks + slots - 1) / slots, slots};
        worst = std::max(worst, scan_bwd_ws(batch, dim, seqlen, dstate, n_groups, s.rows, kMaxDtRank, sg).need_bytes);
    }
    return worst;
}

}  // namespace oss
