// oss_conv1x1_f32x3.h -- the "high" precision mode of the fp32 GEMM-shaped products (OSS_F32_BF16X3): fp32 tensors, every product on
// v_mfma_f32_32x32x16_bf16 with both operands split into two bfloat16 numbers.  gfx950 has no xf32 / TF32 matrix instruction; this
// is the substitute torch.set_float32_matmul_precision("high") documents.  Included by oss_conv1x1_f32.hip, whose F32Gemm and
// clamped-address loads are used here and whose GEMM kernel, launchers and finishing sum serve both modes; the exact products
// there stay the default.
//
// Contract, per fp32 operand value a:   hi = bf16_rne(a),   lo = bf16_rne(a - float(hi))   (the subtraction is exact in fp32);
// |a - hi - lo| <= 2^-16 |a|.  Every product accumulates  hi_w lo_x,  lo_w hi_x,  hi_w hi_x  (in that order, small terms first)
// into ONE fp32 accumulator and drops lo_w lo_x (<= 2^-16 |w||x|):
//     |y_high - y| <= (3 * 2^-16 + (K + 2) * 2^-23) * sum_k |w_k||x_k|            
// Operands that are bf16-exact (small integers) have lo = 0 and give the exact kernels' results bit for bit.
// Where a - hi is not finite (a = +-inf / NaN, or |a| so large that hi rounds to infinity) the value travels in lo ALONE:
// hi = 0, lo = bf16_rne(a).  With the infinity in hi_x the cross term lo_w hi_x would be an infinity of lo_w's sign -- which is
// as often the opposite of w's -- or 0 * inf, and the sum a NaN; in lo_x it meets hi_w only, and the output is the infinity
// (or NaN) the exact kernels give, in the same places.
// Matrix time per 16 channels of a 32-row x 128-pixel tile: 12 MFMAs of 32 cycles = 384 cycles against 32 x 64 = 2048 of
// v_mfma_f32_32x32x2_f32; the split itself is 3-4 vector instructions per value, which is why an activation value is split ONCE per
// wave and reused by all its row tiles and pixel groups.
#pragma once
#include "oss_mfma.h"

namespace oss {

// The weight-gradient family and the forward / input-gradient family are switched separately: a family that is not faster on split
// bf16 would stay on the exact kernel under "high" too.  Both are (profiles/fp32_matmul_high_ab.txt).
// (kF32SplitGemm, the forward / input-gradient family's switch, is a launch decision: oss_conv1x1_plan.h)
constexpr bool kF32SplitWgrad = true;

// Two values -> packed hi and lo.  The finite case costs five instructions per pair (cvt_pk, shift, and, packed subtract, cvt_pk);
// `bad` turns NaN when a remainder is not finite (r * 0 is NaN exactly then) and the caller then repairs its round (below).
__device__ __forceinline__ void split_bf16x2(float a, float b, uint32_t &hi, uint32_t &lo, float &bad) {
    hi = pack2<bf16_t>(a, b);   // one v_cvt_pk_bf16_f32: round to nearest even, NaN stays NaN
    const float ra = a - __uint_as_float(hi << 16), rb = b - __uint_as_float(hi & 0xffff0000u);
    lo = pack2<bf16_t>(ra, rb);
    bad = __builtin_fmaf(ra, 0.f, bad);
    bad = __builtin_fmaf(rb, 0.f, bad);
}
// ... and the repair of a pair whose remainder was not finite (lo is then NaN or +-inf, hi still holds bf16(a)): that value
// moves into lo (see the contract above).  Works on the packed operands, so nothing else has to stay in registers for it.
__device__ __forceinline__ void carry_nonfinite_in_lo(uint32_t &hi, uint32_t &lo) {
    const uint32_t m = ((lo & 0x7f80u) == 0x7f80u ? 0xffffu : 0u) | ((lo & 0x7f800000u) == 0x7f800000u ? 0xffff0000u : 0u);
    lo = (lo & ~m) | (hi & m);
    hi &= ~m;
}
// 8 fp32 values -> the hi and the lo MFMA operand (8 x bf16 each)
__device__ __forceinline__ void split_bf16x8(const float (&v)[8], s16x8 &hi, s16x8 &lo, float &bad) {
    uint32_t h[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) split_bf16x2(v[2 * i], v[2 * i + 1], h[i], l[i], bad);
    hi = __builtin_bit_cast(s16x8, u32x4{h[0], h[1], h[2], h[3]});
    lo = __builtin_bit_cast(s16x8, u32x4{l[0], l[1], l[2], l[3]});
}
__device__ __forceinline__ void carry_nonfinite_in_lo(s16x8 &hi, s16x8 &lo) {
    u32x4 h = __builtin_bit_cast(u32x4, hi), l = __builtin_bit_cast(u32x4, lo);
    uint32_t hh[4] = {h.x, h.y, h.z, h.w}, ll[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) carry_nonfinite_in_lo(hh[i], ll[i]);
    hi = __builtin_bit_cast(s16x8, u32x4{hh[0], hh[1], hh[2], hh[3]});
    lo = __builtin_bit_cast(s16x8, u32x4{ll[0], ll[1], ll[2], ll[3]});
}
__device__ __forceinline__ void unpack8(const f32x4 (&q)[2], float (&c)[8]) {
    c[0] = q[0].x; c[1] = q[0].y; c[2] = q[0].z; c[3] = q[0].w; c[4] = q[1].x; c[5] = q[1].y; c[6] = q[1].z; c[7] = q[1].w;
}
// did any lane of the wave meet a non-finite remainder?  (wave-uniform: the branch on it does not diverge)
__device__ __forceinline__ bool wave_any_bad(float bad) { return __builtin_amdgcn_ballot_w64(bad != bad) != 0; }
__device__ __forceinline__ f32x16 mfma_bf16(s16x8 a, s16x8 b, f32x16 c) { return Mfma<bf16_t>::run(a, b, c); }

// ---- forward / input gradient -------------------------------------------------------------------------------------------------
// The product loop of oss_conv1x1_f32_kernel<MT, SPLIT, true> (oss_conv1x1_f32.hip: same tiles -- one wave = 32 MT rows x 128
// pixels --, same grid, same wave split and epilogue as the exact kernel) over this wave's channels [kbeg, K).
// v_mfma_f32_32x32x16_bf16 wants, per lane, A[i = l & 31][k = 8 (l >> 5) + j] and B[k = 8 (l >> 5) + j][col = l & 31], j < 8: a
// lane loads the 16-byte pixel quad 4 (l & 31) .. + 3 of the EIGHT channel rows k0 + 8 (l >> 5) + j and feeds four MFMA groups,
// one per pixel of the quad (the instruction does not care which pixel is "column l & 31"), and eight weights of its row.
// A round is 16 channels; the loads of round r + 1 are in flight during the MFMAs of round r.  K tails read the zero quad.
template <int MT>
__device__ __forceinline__ void gemm_f32_bf16x3_loop(const F32Gemm &a, f32x16 (&acc)[MT][4], const float *xb, const float *const (&wr)[MT],
                                                     const bool (&mok)[MT], bool pok, int kbeg, int K, int kg) {
    f32x4 xv[8];        // the round as loaded: channel k0 + 8 kg + j, the lane's four pixels
    float av[MT][8];    // W(row of tile t, k0 + 8 kg + j)
    // The lane's row pointers walk along K (one 64-bit add per round) and the rows of a round are reached by adding the stride (a scalar)
    // eight times: the 64-bit multiply per load of `row k -> address` costs more vector
    // instructions than the split itself, and at 384 matrix cycles per round this loop is bound by its vector instructions.
    const float *xrow = xb + (int64_t)(kbeg + 8 * kg) * a.xsk;
    const float *wrow[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) wrow[t] = wr[t] + (int64_t)(kbeg + 8 * kg) * a.wsk;
    auto load_x = [&](int k0) {   // (rows past K: the address is formed but never read -- the zero quad is)
        const float *p = xrow;
#pragma unroll
        for (int j = 0; j < 8; ++j, p += a.xsk) xv[j] = quad_or_zero(p, k0 + 8 * kg + j < K && pok);
        xrow += 16 * a.xsk;
    };
    auto load_w = [&](int k0) {
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const float *p = wrow[t];
#pragma unroll
            for (int j = 0; j < 8; ++j, p += a.wsk) av[t][j] = float_or_zero(p, k0 + 8 * kg + j < K && mok[t]);
            wrow[t] += 16 * a.wsk;
        }
    };
    s16x8 xh[4], xl[4], wh[MT], wl[MT];
    auto split_round = [&]() {   // every value once: the four pixel groups and the MT row tiles share the results
        float bad = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float c[8] = {xv[0][q], xv[1][q], xv[2][q], xv[3][q], xv[4][q], xv[5][q], xv[6][q], xv[7][q]};
            split_bf16x8(c, xh[q], xl[q], bad);
        }
#pragma unroll
        for (int t = 0; t < MT; ++t) split_bf16x8(av[t], wh[t], wl[t], bad);
        if (wave_any_bad(bad)) {   // an infinity or a NaN among the round's operands (rare)
#pragma unroll
            for (int q = 0; q < 4; ++q) carry_nonfinite_in_lo(xh[q], xl[q]);
#pragma unroll
            for (int t = 0; t < MT; ++t) carry_nonfinite_in_lo(wh[t], wl[t]);
        }
    };
    // The activations of round r + 1 are requested before the MFMAs of round r, its weights (small, cache-resident) once the first
    // third of them has released the registers of xl: accumulators + operands + a whole raw round would not fit 256 registers at MT = 2.
    // (the prefetches are unconditional -- a round past K reads the zero quad -- for the reason given at the exact loop)
    load_x(kbeg);
    load_w(kbeg);
    for (int k0 = kbeg; k0 < K; k0 += 16) {
        split_round();
        __builtin_amdgcn_sched_barrier(0);
        load_x(k0 + 16);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[t][q] = mfma_bf16(wh[t], xl[q], acc[t][q]);
        __builtin_amdgcn_sched_barrier(0);
        load_w(k0 + 16);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[t][q] = mfma_bf16(wl[t], xh[q], acc[t][q]);
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[t][q] = mfma_bf16(wh[t], xh[q], acc[t][q]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------
// oss_rows_f32_wgrad_kernel's product (same arguments, tiles, grid and partial layout; the finishing sum is shared): the
// contraction runs over pixels and both operands are rows of an NCHW tensor, so a lane's eight consecutive pixels
// p + 8 (l >> 5) .. + 7 of its row ARE the bf16 operand layout -- two 16-byte loads per row and 16-pixel step.
template <int TM, int TN>
__global__ void __launch_bounds__(256)
oss_rows_f32_wgrad_bf16x3_kernel(const float *__restrict__ a, const float *__restrict__ bm, float *__restrict__ part, int M, int N, int P,
                                 int G, int GB, int64_t asb, int64_t asg, int64_t asm_, int64_t bsb, int64_t bsg, int64_t bsn, int NB) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, kg = lane >> 5;
    const int b = blockIdx.y / G, g = blockIdx.y - b * G, slab = blockIdx.x;
    const int mt = (M + 32 * TM - 1) / (32 * TM), nt = (NB + 32 * TN - 1) / (32 * TN);
    const int tile = blockIdx.z * 4 + wave;
    if (tile >= mt * nt) return;
    const int m0 = (tile / nt) * 32 * TM, n0 = (tile % nt) * 32 * TN;
    const int pbeg = slab * kF32WgradSlab, pend = min(P, pbeg + kF32WgradSlab);
    const float *ab = a + b * asb + g * asg, *bb = bm + b * bsb + (g % GB) * bsg;
    const float *ar[TM], *br[TN];
    bool aok[TM], bok[TN], bone[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = m0 + 32 * i + col;
        aok[i] = m < M;
        ar[i] = ab + (int64_t)(aok[i] ? m : 0) * asm_;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + 32 * j + col;
        bone[j] = n == N && NB > N;   // the virtual all-ones row: its column of the product is the bias gradient (1 = hi, lo = 0)
        bok[j] = n < N || bone[j];
        br[j] = bb + (int64_t)(n < N ? n : 0) * bsn;
    }
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // rounds of U 16-pixel steps, the next round's loads in flight during the current round's splits and MFMAs (two register sets)
    constexpr int U = 2;
    auto load_round = [&](int p, f32x4 (&av)[U][TM][2], f32x4 (&bv)[U][TN][2]) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int pp = p + 16 * u + 8 * kg + 4 * h;
                const bool ok = pp < pend;          // P % 4 == 0: a lane's quad is inside or outside as a whole
                const int pc = ok ? pp : pbeg;      // (a quad past the end reads the slab's first one and is zeroed)
#pragma unroll
                for (int i = 0; i < TM; ++i) av[u][i][h] = quad_or_zero(ar[i] + pc, ok && aok[i]);
#pragma unroll
                for (int j = 0; j < TN; ++j) bv[u][j][h] = quad_one_or_zero(br[j] + pc, ok && bok[j], bone[j]);
            }
    };
    auto mfma_round = [&](const f32x4 (&av)[U][TM][2], const f32x4 (&bv)[U][TN][2]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            s16x8 ah[TM], al[TM], bh[TN], bl[TN];
            float c[8], bad = 0.f;   // the lane's eight pixels of a row
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                unpack8(av[u][i], c);
                split_bf16x8(c, ah[i], al[i], bad);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                unpack8(bv[u][j], c);
                split_bf16x8(c, bh[j], bl[j], bad);
            }
            if (wave_any_bad(bad)) {   // an infinity or a NaN among the step's operands (rare)
#pragma unroll
                for (int i = 0; i < TM; ++i) carry_nonfinite_in_lo(ah[i], al[i]);
#pragma unroll
                for (int j = 0; j < TN; ++j) carry_nonfinite_in_lo(bh[j], bl[j]);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[i][j] = mfma_bf16(ah[i], bl[j], acc[i][j]);
                    acc[i][j] = mfma_bf16(al[i], bh[j], acc[i][j]);
                    acc[i][j] = mfma_bf16(ah[i], bh[j], acc[i][j]);
                }
        }
    };
    f32x4 a0[U][TM][2], b0[U][TN][2], a1[U][TM][2], b1[U][TN][2];
    load_round(pbeg, a0, b0);   // (prefetches unconditional, rounds past the slab read the zero quad)
    for (int p = pbeg; p < pend; p += 32 * U) {
        load_round(p + 16 * U, a1, b1);
        __builtin_amdgcn_sched_barrier(0);
        mfma_round(a0, b0);
        __builtin_amdgcn_sched_barrier(0);
        load_round(p + 32 * U, a0, b0);
        __builtin_amdgcn_sched_barrier(0);
        if (p + 16 * U < pend) mfma_round(a1, b1);
        __builtin_amdgcn_sched_barrier(0);
    }
    const size_t pvec = (size_t)G * M * N + (NB > N ? M : 0);   // one partial vector per (batch, slab): [G][M][N], then the M bias sums
    float *pb = part + (size_t)(b * gridDim.x + slab) * pvec + (size_t)g * M * N;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + 32 * j + col;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * kg;
                if (m < M && n < N) pb[(size_t)m * N + n] = acc[i][j][r];
                else if (m < M && n == N && NB > N) pb[(size_t)M * N + m] = acc[i][j][r];   // (G == 1)
            }
        }
}

}  // namespace oss
