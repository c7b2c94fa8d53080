// oss_channel.hip -- the channel branch of SS2D_1 (the two channel-direction scans of the Omni Selective Scan,
// SRGAN/VmambaIR/archs/MambaSISR6_arch.py:438-483,495-496; RealSR rank-R form MambaRealSR11_arch.py:758-817):
//   pooled[b, l] = mean over pixels of y2[b, l]                (l runs over the d_inner channels: L = d_inner)
//   seq[i, l]    = cin_w[i] pooled[l] + cin_b[i]               (the 1 -> dc_inner lift; identity for RealSR)
//   z[k, c, l]   = sum_i xc_proj[k, c, i] seq[i, l];  dts[k, i, l] = sum_r dtc_w[k, i, r] z[k, r, l]
//   y[k, i, :]   = selective scan of row (k, i) over l (k = 1: from l = L-1 down to 0), A = -exp(Ac_logs), D = Dsc
//   yc[l]        = sum_i cout_w[i] (y[0, i, l] + y[1, i, l]) + cout_b;   c = LayerNorm_l(yc)
//   out          = y2 * c + y2   ("mul_add")   or   y2 + c   ("add")
// Everything between the pooling and the gate is a few thousand numbers per image.  The reference (and any
// op-by-op port) spends ~15 launches forward and ~20 backward on it; here: one workgroup per image does the
// whole thing in one launch per direction of autograd, plus row reductions / row-affine passes over the
// (B, d, H, W) tensor at both ends.  fp32 throughout (the RealSR tree forces fp32 here even under AMP).
//
// The lift and the two projections are affine in the pooled scalar p = pooled[l], so they are never formed as arrays: a coefficient
// table, a function of the parameters only, is built once per launch in LDS
//   u_i(l)     = cw[i] p + cb[i]                                   (cw = cin_w, cb = cin_b; 1 and 0 for RealSR)
//   z[k, c, l] = za[k, c] p + zb[k, c]      za = sum_i xc_proj[k, c, i] cw[i],   zb likewise from cb
//   dts[k,i,l] = ta[k, i] p + tb[k, i]      ta = sum_r dtc_w[k, i, r] za[k, r],  tb likewise from zb
// and the scan lanes evaluate B, C, u and delta = softplus(ta p + tb + bias) of their own steps from p with one FMA each.  The
// backward returns gradients of the coefficients (sums over l of d z * p and of d z, and so on), and a last small phase maps those
// to the parameter slots: O(dc Rc) work per output instead of O(L).
//
// Scan layout inside the workgroup: wave = (direction k, one of four groups of 4 states); lane q of a 128-step chunk owns the steps
// 2q and 2q + 1 of the direction's walk.  Per (row, state): the lane's two steps from a zero state, one 64-lane scan of the
// recurrence monoid (oss_device.h: segment_scan4_64), and the chunk carry read from lane 63.  Sums over a group's states stay in the
// lane; sums over the four groups (and over the waves) go through LDS and are added in a fixed order, so reruns are bit-identical.
// The states h[row, l, n] of every step are kept in HBM for the backward recurrence (it needs h_{t-1}; 8 x 768 x 16 floats per
// image at most); B, C, u and delta are recomputed there from the pooled vector.
#include "oss_device.h"
#include "oss_host.h"

namespace oss {

constexpr int kChN = 16;  // dc_state of every reference config
constexpr int kChU = 8;   // scan steps whose operands are fetched together
constexpr int kChNT = 512;  // threads per workgroup: 8 waves = 2 directions x 4 time segments
constexpr int kChRed = 8;   // floats of the block-sum scratch

template <int NT>
__device__ __forceinline__ float block_sum(float v, float *red /*[kChRed]*/, int tid) {
    static_assert(NT == 256 || NT == 512, "block_sum: 4 or 8 waves");
    const float w = segment_sum_to_last<64>(v);
    __syncthreads();  // red may still be read from a previous call
    if ((tid & 63) == 63) red[tid >> 6] = w;
    __syncthreads();
    float t = (red[0] + red[1]) + (red[2] + red[3]);
    if constexpr (NT == 512) t += (red[4] + red[5]) + (red[6] + red[7]);
    return t;
}

// sum over the rows i of a direction (lanes n, 16 + n, 32 + n, 48 + n); every lane gets the total
__device__ __forceinline__ float sum_over_rows(float v, int lane) {
    v += __int_as_float(__builtin_amdgcn_ds_bpermute((lane ^ 16) << 2, __float_as_int(v)));
    v += __int_as_float(__builtin_amdgcn_ds_bpermute((lane ^ 32) << 2, __float_as_int(v)));
    return v;
}

// the affine coefficient table of one launch (the file's header comment): [za 2 Cc | zb 2 Cc | ta 2 dc | tb 2 dc | cw dc | cb dc]
__host__ __device__ inline int chan_tab_floats(int dc, int Cc) { return 4 * Cc + 6 * dc; }
struct ChanTab {
    float *za, *zb, *ta, *tb, *cw, *cb;
    __device__ ChanTab(float *t, int dc, int Cc) { za = t; zb = za + 2 * Cc; ta = zb + 2 * Cc; tb = ta + 2 * dc; cw = tb + 2 * dc; cb = cw + dc; }
};

// za, zb of column col = k Cc + c
__device__ __forceinline__ void chan_zcoef(const oss_chan_params &p, int col, float &a, float &b) {
    const bool lift = p.cin_w != nullptr;
    a = 0.f; b = 0.f;
    for (int i = 0; i < p.dc; ++i) {
        const float w = p.Wxc[col * p.dc + i];
        a = __builtin_fmaf(w, lift ? p.cin_w[i] : 1.f, a);
        b = __builtin_fmaf(w, lift ? p.cin_b[i] : 0.f, b);
    }
}

// One entry per thread, counted from the LAST thread down: the first threads are the ones busy with the pooled sums / the LayerNorm
// backward of the same phase.  A ta / tb entry forms the za / zb of its dt columns itself instead of waiting for them behind a
// barrier.  Both kernels call this, so the backward recomputes exactly the forward's B, C, u and delta.
template <int NT>
__device__ __forceinline__ void chan_coef_table(const oss_chan_params &p, float *tab, int tid) {
    const int dc = p.dc, Cc = p.Cc, Rc = p.Rc;
    const ChanTab T(tab, dc, Cc);
    for (int o = NT - 1 - tid; o < 2 * Cc + 3 * dc; o += NT) {
        if (o < 2 * Cc) {
            float a, b;
            chan_zcoef(p, o, a, b);
            T.za[o] = a; T.zb[o] = b;
        } else if (o < 2 * Cc + 2 * dc) {
            const int row = o - 2 * Cc, k = row / dc;
            float a = 0.f, b = 0.f;
            for (int r = 0; r < Rc; ++r) {
                float za, zb;
                chan_zcoef(p, k * Cc + r, za, zb);
                const float w = p.Wdtc[row * Rc + r];
                a = __builtin_fmaf(w, za, a);
                b = __builtin_fmaf(w, zb, b);
            }
            T.ta[row] = a; T.tb[row] = b;
        } else {
            const int i = o - 2 * Cc - 2 * dc;
            T.cw[i] = p.cin_w ? p.cin_w[i] : 1.f;
            T.cb[i] = p.cin_w ? p.cin_b[i] : 0.f;
        }
    }
}

// a wave-uniform value read from LDS: into a scalar register
__device__ __forceinline__ float wave_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// delta = softplus(ta p + tb + bias) of one (row, step); sg = its derivative in the argument
__device__ __forceinline__ float chan_delta(float ta, float tb, float bias, float pl, float &sg) {
    const float x = __builtin_fmaf(ta, pl, tb) + bias;
    float e;
    const float d = softplus_thr(x, e);
    sg = (x <= 20.f) ? e * __builtin_amdgcn_rcpf(1.f + e) : 1.f;
    return d;
}

// (round 4, measured and reverted: every parameter of the phases below requested in one batch at the top of the kernel, with clamped
// indices and stand-in pointers instead of `cond ? p[i] : 0` -- most of those loads are wave-uniform and were scalar loads already;
// 16.7 us per launch against 15.4 as it stood, profiles/r04_serial_loads.txt)
template <int NT>
__global__ void __launch_bounds__(NT)
oss_chan_fwd_kernel(oss_chan_params p) {
    extern __shared__ float sm[];
    const int b = blockIdx.x, tid = threadIdx.x, L = p.L, dc = p.dc, Cc = p.Cc, Rc = p.Rc;
    const bool lift = p.cin_w != nullptr;
    float *pls = sm;                 // [L]: the pooled vector
    float *ybuf = pls + L;           // [2 dc][L]
    float *ycs = ybuf + 2 * dc * L;  // [L]
    float *red = ycs + L;            // [kChRed]
    float *ypart = red + kChRed;     // [4][2 dc][L]: the state groups' partial sums of y
    float *tab = ypart + 4 * 2 * dc * L;   // [chan_tab_floats]
    chan_coef_table<NT>(p, tab, tid);
    // the pooled descriptor from the LayerNorm forward's per-workgroup output sums.  Few tiles (the training patches: 8 ... 32): one thread
    // per channel adds them in order.  Many tiles (an untiled 512 x 512 RealSR plane leaves 1024): that was 96 of the 512 threads busy with
    // 8 loads in flight each, 128 dependent rounds = most of a 61 us launch -- then NS threads per channel add contiguous runs of the
    // tiles, and the NS runs are added in order (a fixed order either way: reruns are bit-identical).  (round 6)
    const bool pool_runs = p.pool_part && p.n_part >= 64;   // (uniform)
    const int ns = max(1, min(8, NT / L));
    if (pool_runs) {
        const int per = (p.n_part + ns - 1) / ns;
        float *run = ypart;   // [ns][L] of its [4][2 dc][L]: free until the scans
        for (int idx = tid; idx < ns * L; idx += NT) {
            const int sub = idx / L, l = idx - sub * L;
            const int k0 = sub * per, k1 = min(p.n_part, k0 + per);
            const float *pp = p.pool_part + (size_t)b * p.n_part * L + l;
            float sum = 0.f;
            int k = k0;
            for (; k + 16 <= k1; k += 16) {
                float v[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) v[q] = pp[(size_t)(k + q) * L];
#pragma unroll
                for (int q = 0; q < 16; ++q) sum += v[q];
            }
            for (; k < k1; ++k) sum += pp[(size_t)k * L];
            run[idx] = sum;
        }
        __syncthreads();
    }
    for (int l = tid; l < L; l += NT) {
        float pl;
        if (pool_runs) {
            float sum = ypart[l];
            for (int sub = 1; sub < ns; ++sub) sum += ypart[sub * L + l];
            pl = sum * p.pool_scale;
            const_cast<float *>(p.pooled)[(size_t)b * L + l] = pl;   // kept for the backward
        } else if (p.pool_part) {
            const float *pp = p.pool_part + (size_t)b * p.n_part * L + l;
            float sum = 0.f;
            int k = 0;
            for (; k + 8 <= p.n_part; k += 8) {
                float v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = pp[(size_t)(k + q) * L];
#pragma unroll
                for (int q = 0; q < 8; ++q) sum += v[q];
            }
            for (; k < p.n_part; ++k) sum += pp[(size_t)k * L];
            pl = sum * p.pool_scale;
            const_cast<float *>(p.pooled)[(size_t)b * L + l] = pl;   // kept for the backward
        } else {
            pl = p.pooled[(size_t)b * L + l];
        }
        pls[l] = pl;
    }
    __syncthreads();   // pls and the coefficient table are complete (and the runs in ypart are consumed)
    // ---- the two channel-direction scans, time across the lanes (round 3) -------------------------------------------------
    // wave = (direction k, group of NPG states); lane p of a 128-step chunk owns steps 2p, 2p + 1 of the direction's walk.
    // Per (row, state): the two local steps, one 64-lane scan of the recurrence monoid (oss_device.h: segment_scan), the chunk
    // carry -- instead of a lane per (row, state) walking the steps one after the other (round 2: four 24-step segments per
    // direction, two passes each, every step paying cross-lane sums over the states and its own LDS round trips: 5.3 us of the
    // 13 us kernel at L = 96, 36.6 of 56.5 at L = 384).  Sums over the states of a group stay in the lane; the four groups'
    // partial sums of y go to LDS and are added in group order afterwards (fixed order: reruns are bit-identical).
    // Every operand of a step is one FMA away from the pooled scalar of that step; the coefficients are wave-uniform.
    static_assert(NT == 512, "wave = (direction, one of four state groups)");
    constexpr int GPD = NT / 128, NPG = kChN / GPD;   // state groups per direction, states per group
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    {
        const int k = wave / GPD, ng = wave - k * GPD, n0 = ng * NPG;
        const ChanTab T(tab, dc, Cc);
        float A2[4][NPG], carry[4][NPG], Dv[4], ta[4], tb[4], bias[4], cw[4], cb[4];
        float zaB[NPG], zbB[NPG], zaC[NPG], zbC[NPG];
#pragma unroll
        for (int nn = 0; nn < NPG; ++nn) {
            const int cB = k * Cc + Rc + n0 + nn, cC = cB + kChN;
            zaB[nn] = wave_uniform(T.za[cB]); zbB[nn] = wave_uniform(T.zb[cB]);
            zaC[nn] = wave_uniform(T.za[cC]); zbC[nn] = wave_uniform(T.zb[cC]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ic = min(i, dc - 1), row = k * dc + ic;
            Dv[i] = p.Dsc[row];
            bias[i] = p.dt_bias[row];
            ta[i] = wave_uniform(T.ta[row]); tb[i] = wave_uniform(T.tb[row]);
            cw[i] = wave_uniform(T.cw[ic]); cb[i] = wave_uniform(T.cb[ic]);
#pragma unroll
            for (int nn = 0; nn < NPG; ++nn) { A2[i][nn] = -__expf(p.A_logs[row * kChN + n0 + nn]) * kLog2e; carry[i][nn] = 0.f; }
        }
        const int nchunk = (L + 127) >> 7;
        for (int c = 0; c < nchunk; ++c) {
            const int t0 = c * 128 + 2 * lane;
            const bool v0 = t0 < L, v1 = t0 + 1 < L;
            const int tc0 = min(t0, L - 1), tc1 = min(t0 + 1, L - 1);
            const int l0 = k ? L - 1 - tc0 : tc0, l1 = k ? L - 1 - tc1 : tc1;
            const float p0 = pls[l0], p1 = pls[l1];
            float B0[NPG], B1[NPG], C0[NPG], C1[NPG];
#pragma unroll
            for (int nn = 0; nn < NPG; ++nn) {
                B0[nn] = __builtin_fmaf(zaB[nn], p0, zbB[nn]); B1[nn] = __builtin_fmaf(zaB[nn], p1, zbB[nn]);
                C0[nn] = __builtin_fmaf(zaC[nn], p0, zbC[nn]); C1[nn] = __builtin_fmaf(zaC[nn], p1, zbC[nn]);
            }
            float yv0[4], yv1[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                yv0[i] = 0.f; yv1[i] = 0.f;
                if (i < dc) {   // (uniform)
                    const int row = k * dc + i;
                    float sg;
                    float dl0 = chan_delta(ta[i], tb[i], bias[i], p0, sg), dl1 = chan_delta(ta[i], tb[i], bias[i], p1, sg);
                    dl0 = v0 ? dl0 : 0.f;   // a step past the end: a = 1, B u delta = 0 -- the identity
                    dl1 = v1 ? dl1 : 0.f;
                    const float u0 = __builtin_fmaf(cw[i], p0, cb[i]), u1 = __builtin_fmaf(cw[i], p1, cb[i]);
                    float hv0[NPG], hv1[NPG], a0[NPG], a1[NPG], b0[NPG], b1[NPG], P[NPG], h[NPG];
#pragma unroll
                    for (int nn = 0; nn < NPG; ++nn) {
                        a0[nn] = exp2_hw(dl0 * A2[i][nn]); a1[nn] = exp2_hw(dl1 * A2[i][nn]);
                        b0[nn] = dl0 * B0[nn] * u0; b1[nn] = dl1 * B1[nn] * u1;
                        P[nn] = a0[nn] * a1[nn]; h[nn] = __builtin_fmaf(a1[nn], b0[nn], b1[nn]);   // the lane's two steps from a zero state
                    }
                    segment_scan4_64(P, h);
#pragma unroll
                    for (int nn = 0; nn < NPG; ++nn) {
                        const float hp = shift_from_prev_lane(h[nn], 0.f, false), Pp = shift_from_prev_lane(P[nn], 1.f, false);
                        const float hin = __builtin_fmaf(Pp, carry[i][nn], hp);  // the state entering the lane's steps
                        const float h0 = __builtin_fmaf(a0[nn], hin, b0[nn]), h1 = __builtin_fmaf(a1[nn], h0, b1[nn]);
                        hv0[nn] = h0; hv1[nn] = h1;
                        yv0[i] = __builtin_fmaf(C0[nn], h0, yv0[i]);
                        yv1[i] = __builtin_fmaf(C1[nn], h1, yv1[i]);
                        carry[i][nn] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(h1), 63));
                    }
                    float *hr = p.hs + (((size_t)b * 2 * dc + row) * L) * kChN + n0;
                    static_assert(NPG == 4, "one 16-byte store per (row, step)");
                    if (v0) *reinterpret_cast<f32x4 *>(hr + (size_t)l0 * kChN) = f32x4{hv0[0], hv0[1], hv0[2], hv0[3]};
                    if (v1) *reinterpret_cast<f32x4 *>(hr + (size_t)l1 * kChN) = f32x4{hv1[0], hv1[1], hv1[2], hv1[3]};
                    if (ng == 0) { yv0[i] = __builtin_fmaf(Dv[i], u0, yv0[i]); yv1[i] = __builtin_fmaf(Dv[i], u1, yv1[i]); }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {   // the group's partial sums of y (group 0: + D u)
                if (i < dc) {
                    float *yr = ypart + (ng * 2 * dc + k * dc + i) * L;
                    if (v0) yr[l0] = yv0[i];
                    if (v1) yr[l1] = yv1[i];
                }
            }
        }
    }
    __syncthreads();
    for (int idx = tid; idx < 2 * dc * L; idx += NT)   // y = D u + the groups' sums over their states, in group order
        ybuf[idx] = ((ypart[idx] + ypart[2 * dc * L + idx]) + ypart[2 * 2 * dc * L + idx]) + ypart[3 * 2 * dc * L + idx];
    __syncthreads();
    float part = 0.f;
    for (int l = tid; l < L; l += NT) {
        float s = lift ? p.cout_b[0] : 0.f;
        for (int i = 0; i < dc; ++i) s = __builtin_fmaf(lift ? p.cout_w[i] : 1.f, ybuf[i * L + l] + ybuf[(dc + i) * L + l], s);
        ycs[l] = s;
        part += s;
    }
    for (int idx = tid; idx < 2 * dc * L; idx += NT) p.y[(size_t)b * 2 * dc * L + idx] = ybuf[idx];
    const float mu = block_sum<NT>(part, red, tid) / (float)L;
    float q = 0.f;
    for (int l = tid; l < L; l += NT) { const float d = ycs[l] - mu; q = __builtin_fmaf(d, d, q); }
    const float rstd = 1.0f / sqrtf(block_sum<NT>(q, red, tid) / (float)L + 1e-5f);
    for (int l = tid; l < L; l += NT) {
        p.yc[(size_t)b * L + l] = ycs[l];
        p.c[(size_t)b * L + l] = __builtin_fmaf((ycs[l] - mu) * rstd, p.cn_w[l], p.cn_b[l]);
    }
    if (tid == 0) { p.stat[b * 2] = mu; p.stat[b * 2 + 1] = rstd; }
}

// gradient slots of one image in gpart (B, NP); oss_chan_grad_floats() = NP
struct ChanSlots {
    int cnw, cnb, coutw, coutb, dA, dD, dbias, wdtc, wxc, cinw, cinb, total;
    __host__ __device__ ChanSlots(int L, int dc, int Rc, int Cc) {
        cnw = 0; cnb = L; coutw = 2 * L; coutb = coutw + dc; dA = coutb + 1; dD = dA + 2 * dc * kChN; dbias = dD + 2 * dc;
        wdtc = dbias + 2 * dc; wxc = wdtc + 2 * dc * Rc; cinw = wxc + 2 * Cc * dc; cinb = cinw + dc; total = cinb + dc;
    }
};

// per-wave sums over l of the coefficient gradients, [wave][kChCg]: d za / d zb of the group's B states (0, 4) and C states (8, 12),
// then per row i of the direction d ta (16), d tb (20), d cw (24), d cb (28)
constexpr int kChCg = 32;

template <int NT>
__global__ void __launch_bounds__(NT)
oss_chan_bwd_kernel(oss_chan_params p, const float *__restrict__ gc /*(B, L): grad of c*/, float *__restrict__ dpool,
                    float *__restrict__ gpart) {
    extern __shared__ float sm[];
    const int b = blockIdx.x, tid = threadIdx.x, L = p.L, dc = p.dc, Cc = p.Cc, Rc = p.Rc;
    const bool lift = p.cin_w != nullptr;
    const ChanSlots sl(L, dc, Rc, Cc);
    // the scan phase's layout (see there): wave = (direction, group of NPG states), lane = two steps of a 128-step chunk.  The
    // operands it reads from HBM -- the pooled scalars and the saved states, written by the forward pass milliseconds ago -- are
    // requested HERE for the first row of the first chunk, and from then on the states of the row that comes next (of the next
    // chunk after the last row) while a row is computed, in two alternating sets of registers: one memory latency under the
    // LayerNorm phase instead of one in front of every row.
    static_assert(NT == 512, "wave = (direction, one of four state groups)");
    constexpr int GPD = NT / 128, NPG = kChN / GPD, NW = NT / 64;
    static_assert(NPG == 4, "16-byte accesses of a group's states");
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int sk = wave / GPD, sng = wave - sk * GPD, sn0 = sng * NPG;
    struct RowOps { f32x4 h0, h1, h2; };   // the row's states after the lane's two steps and after the step before them
    auto chunk_pos = [&](int c, int &l0, int &l1, int &l2) {
        const int u0 = c * 128 + 2 * lane;
        const int c0 = min(u0, L - 1), c1 = min(u0 + 1, L - 1), c2 = min(u0 + 2, L - 1);
        l0 = sk ? c0 : L - 1 - c0; l1 = sk ? c1 : L - 1 - c1; l2 = sk ? c2 : L - 1 - c2;
    };
    auto fetch_row = [&](int c, int i, RowOps &o) {
        int l0, l1, l2;
        chunk_pos(c, l0, l1, l2);
        const float *hr = p.hs + (((size_t)b * 2 * dc + sk * dc + min(i, dc - 1)) * L) * kChN + sn0;
        o.h0 = *reinterpret_cast<const f32x4 *>(hr + (size_t)l0 * kChN);
        o.h1 = *reinterpret_cast<const f32x4 *>(hr + (size_t)l1 * kChN);
        o.h2 = *reinterpret_cast<const f32x4 *>(hr + (size_t)l2 * kChN);
    };
    auto fetch_pooled = [&](int c, float &p0, float &p1) {
        int l0, l1, l2;
        chunk_pos(c, l0, l1, l2);
        p0 = p.pooled[(size_t)b * L + l0];
        p1 = p.pooled[(size_t)b * L + l1];
    };
    RowOps hq[2];   // row i reads hq[i & 1]
    float pc0, pc1;
    fetch_pooled(0, pc0, pc1);
    fetch_row(0, 0, hq[0]);
    float *dys = sm;              // [L]   grad of yc
    float *red = dys + L;         // [kChRed]
    float *tab = red + kChRed;    // [chan_tab_floats]
    float *dpp = tab + chan_tab_floats(dc, Cc);   // [NW][L]: every wave's part of d pooled
    float *cgw = dpp + NW * L;    // [NW][kChCg]
    float *dza = cgw + NW * kChCg;   // [2 Cc]  sum over l of d z * p ...
    float *dzb = dza + 2 * Cc;    // [2 Cc]  ... and of d z
    float *dta = dzb + 2 * Cc;    // [2 dc]  the same of d dts (after softplus')
    float *dtb = dta + 2 * dc;    // [2 dc]
    float *gp = gpart + (size_t)b * sl.total;
    chan_coef_table<NT>(p, tab, tid);
    const float mu = p.stat[b * 2], rstd = p.stat[b * 2 + 1];
    float s1 = 0.f, s2 = 0.f;
    // g = gc * cn_w is the ROUNDED product in both loops (no contraction into the sums): m1 and m2 are means of exactly the values
    // the second loop subtracts them from, so a one-channel LayerNorm passes back an exact 0
    for (int l = tid; l < L; l += NT) {
#pragma clang fp contract(off)
        const float g0 = gc[(size_t)b * L + l], xh = (p.yc[(size_t)b * L + l] - mu) * rstd, g = g0 * p.cn_w[l];
        gp[sl.cnw + l] = g0 * xh;
        gp[sl.cnb + l] = g0;
        s1 += g;
        s2 = __builtin_fmaf(g, xh, s2);
    }
    const float m1 = block_sum<NT>(s1, red, tid) / (float)L;
    const float m2 = block_sum<NT>(s2, red, tid) / (float)L;
    for (int l = tid; l < L; l += NT) {
#pragma clang fp contract(off)
        const float xh = (p.yc[(size_t)b * L + l] - mu) * rstd, g = gc[(size_t)b * L + l] * p.cn_w[l];
        dys[l] = rstd * (g - m1 - xh * m2);
    }
    __syncthreads();   // dys and the coefficient table are complete
    const float *yb = p.y + (size_t)b * 2 * dc * L;
    const ChanTab T(tab, dc, Cc);
    // ---- both reverse recurrences, time across the lanes (round 3; the forward kernel's layout walked backwards) -----------
    // wave = (direction k, group of NPG states); lane p of a 128-step chunk owns the steps tau = 2p, 2p + 1 counted from the
    // END of the direction's walk (t = L - 1 - tau), so  dh_t = dy_t C_t + a_{t+1} dh_{t+1}  is a forward scan in tau with
    // the pair (a_{t+1}, dy_t C_t): one 64-lane scan per (row, state) and chunk instead of a serial walk with cross-lane sums
    // per step (round 2: 15 of the kernel's 27 us at L = 96, 61 of 103 at L = 384).  Sums over a group's states (d delta, du)
    // stay in the lane, and so does what follows from them and from dB, dC: softplus' is a factor per (row, step), so it applies
    // to the group's partial sum; the step's part of d pooled is a dot product with the wave's coefficients; the coefficient
    // gradients are sums over the steps, kept per lane and finished by one 64-lane sum each.  Nothing per step leaves the lane
    // but that part of d pooled.
    {
        const int k = sk, ng = sng, n0 = sn0;
        float Av[4][NPG], carry[4][NPG], carry_a[4][NPG], accA[4][NPG], cwv[4], Dv[4], ta[4], tb[4], bias[4], cw[4], cb[4];
        float zaB[NPG], zbB[NPG], zaC[NPG], zbC[NPG];
        float gzaB[NPG], gzbB[NPG], gzaC[NPG], gzbC[NPG], gta[4], gtb[4], gcw[4], gcb[4], accD[4];
#pragma unroll
        for (int nn = 0; nn < NPG; ++nn) {
            const int cB = k * Cc + Rc + n0 + nn, cC = cB + kChN;
            zaB[nn] = wave_uniform(T.za[cB]); zbB[nn] = wave_uniform(T.zb[cB]);
            zaC[nn] = wave_uniform(T.za[cC]); zbC[nn] = wave_uniform(T.zb[cC]);
            gzaB[nn] = 0.f; gzbB[nn] = 0.f; gzaC[nn] = 0.f; gzbC[nn] = 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ic = min(i, dc - 1), row = k * dc + ic;
            cwv[i] = i < dc ? (lift ? p.cout_w[i] : 1.f) : 0.f;
            Dv[i] = p.Dsc[row];
            bias[i] = p.dt_bias[row];
            ta[i] = wave_uniform(T.ta[row]); tb[i] = wave_uniform(T.tb[row]);
            cw[i] = wave_uniform(T.cw[ic]); cb[i] = wave_uniform(T.cb[ic]);
            gta[i] = 0.f; gtb[i] = 0.f; gcw[i] = 0.f; gcb[i] = 0.f; accD[i] = 0.f;
#pragma unroll
            for (int nn = 0; nn < NPG; ++nn) {
                Av[i][nn] = -__expf(p.A_logs[row * kChN + n0 + nn]);
                carry[i][nn] = 0.f; carry_a[i][nn] = 1.f; accA[i][nn] = 0.f;
            }
        }
        const int nchunk = (L + 127) >> 7;
        for (int c = 0; c < nchunk; ++c) {
            const int u0 = c * 128 + 2 * lane;                         // tau of the lane's first step
            const bool v0 = u0 < L, v1 = u0 + 1 < L, v2 = u0 + 2 < L;  // (tau + 2: the step before the lane's second one)
            const int c0 = min(u0, L - 1), c1 = min(u0 + 1, L - 1);
            // position along the channel axis of step tau: direction 0 walks l upwards (t = l), direction 1 downwards
            const int l0 = k ? c0 : L - 1 - c0, l1 = k ? c1 : L - 1 - c1;
            const float p0 = pc0, p1 = pc1;
            if (c + 1 < nchunk) fetch_pooled(c + 1, pc0, pc1);   // in flight while this chunk is computed
            float B0[NPG], B1[NPG];
#pragma unroll
            for (int nn = 0; nn < NPG; ++nn) { B0[nn] = __builtin_fmaf(zaB[nn], p0, zbB[nn]); B1[nn] = __builtin_fmaf(zaB[nn], p1, zbB[nn]); }
            const float dys0 = v0 ? dys[l0] : 0.f, dys1 = v1 ? dys[l1] : 0.f;
            float dp0 = 0.f, dp1 = 0.f;   // the wave's part of d pooled at the lane's two steps
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (i < dc) {   // (uniform)
                    // the row after this one goes to the other register set.  An odd dc wraps from the last row to row 0 of the
                    // next chunk in the SAME set: that request waits until this row is done with it.
                    const bool last = i + 1 == dc, wrap_same = last && (i & 1) == 0;
                    if (!last) fetch_row(c, i + 1, hq[(i + 1) & 1]);
                    else if (!wrap_same && c + 1 < nchunk) fetch_row(c + 1, 0, hq[0]);
                    const RowOps hr = hq[i & 1];
                    float sg0, sg1;
                    float dl0 = chan_delta(ta[i], tb[i], bias[i], p0, sg0), dl1 = chan_delta(ta[i], tb[i], bias[i], p1, sg1);
                    dl0 = v0 ? dl0 : 0.f;   // a step past the end: a = 1, nothing flows
                    dl1 = v1 ? dl1 : 0.f;
                    const float us0 = __builtin_fmaf(cw[i], p0, cb[i]), us1 = __builtin_fmaf(cw[i], p1, cb[i]);
                    const float dy0 = cwv[i] * dys0, dy1 = cwv[i] * dys1;
                    const float up0 = us0 * p0, up1 = us1 * p1, dyp0 = dy0 * p0, dyp1 = dy1 * p1;
                    float ddl0 = 0.f, ddl1 = 0.f, du0 = 0.f, du1 = 0.f;
                    float sB0 = 0.f, sB1 = 0.f, sC0 = 0.f, sC1 = 0.f;   // dot products of dB / (u delta) and dC / dy with the wave's za
                    float a0[NPG], a1[NPG], al0[NPG], g0[NPG], g1[NPG], P[NPG], h[NPG];
#pragma unroll
                    for (int nn = 0; nn < NPG; ++nn) {
                        a0[nn] = exp2_hw(dl0 * Av[i][nn] * kLog2e); a1[nn] = exp2_hw(dl1 * Av[i][nn] * kLog2e);
                        // the factor in front of the incoming dh at step tau is a of step tau - 1 (= t + 1)
                        al0[nn] = shift_from_prev_lane(a1[nn], carry_a[i][nn], false);
                        // (C of the two steps is formed here, per row, and not kept across the rows: registers)
                        g0[nn] = dy0 * __builtin_fmaf(zaC[nn], p0, zbC[nn]); g1[nn] = dy1 * __builtin_fmaf(zaC[nn], p1, zbC[nn]);
                        P[nn] = al0[nn] * a0[nn]; h[nn] = __builtin_fmaf(a0[nn], g0[nn], g1[nn]);
                    }
                    segment_scan4_64(P, h);
#pragma unroll
                    for (int nn = 0; nn < NPG; ++nn) {
                        const float A = Av[i][nn];
                        const float hp = shift_from_prev_lane(h[nn], 0.f, false), Pp = shift_from_prev_lane(P[nn], 1.f, false);
                        const float din = __builtin_fmaf(Pp, carry[i][nn], hp);   // a_{t+1} dh_{t+1} reaching the lane's first step
                        const float dh0 = __builtin_fmaf(al0[nn], din, g0[nn]), dh1 = __builtin_fmaf(a0[nn], dh0, g1[nn]);
                        carry[i][nn] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dh1), 63));
                        carry_a[i][nn] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a1[nn]), 63));
                        const float h0 = hr.h0[nn], h1 = hr.h1[nn];
                        const float hp0 = v1 ? h1 : 0.f, hp1 = v2 ? hr.h2[nn] : 0.f;   // the state BEFORE the step (0 before t = 0)
                        // dB = dh delta u and dC = dy h of the row go straight where they are needed (kept per step and state
                        // and summed over the rows first they are 16 more registers than this kernel has): d pooled through za,
                        // and the sums over the steps that are d za (weighted with p) and d zb
                        const float x0 = dh0 * dl0, x1 = dh1 * dl1;
                        sB0 = __builtin_fmaf(zaB[nn], x0, sB0); sB1 = __builtin_fmaf(zaB[nn], x1, sB1);
                        sC0 = __builtin_fmaf(zaC[nn], h0, sC0); sC1 = __builtin_fmaf(zaC[nn], h1, sC1);
                        gzaB[nn] = __builtin_fmaf(x0, up0, __builtin_fmaf(x1, up1, gzaB[nn]));
                        gzbB[nn] = __builtin_fmaf(x0, us0, __builtin_fmaf(x1, us1, gzbB[nn]));
                        gzaC[nn] = __builtin_fmaf(dyp0, h0, __builtin_fmaf(dyp1, h1, gzaC[nn]));
                        gzbC[nn] = __builtin_fmaf(dy0, h0, __builtin_fmaf(dy1, h1, gzbC[nn]));
                        ddl0 = __builtin_fmaf(dh0, __builtin_fmaf(A * a0[nn], hp0, B0[nn] * us0), ddl0);
                        ddl1 = __builtin_fmaf(dh1, __builtin_fmaf(A * a1[nn], hp1, B1[nn] * us1), ddl1);
                        du0 = __builtin_fmaf(x0, B0[nn], du0);
                        du1 = __builtin_fmaf(x1, B1[nn], du1);
                        accA[i][nn] = __builtin_fmaf(x0 * a0[nn], hp0, __builtin_fmaf(x1 * a1[nn], hp1, accA[i][nn]));
                    }
                    if (wrap_same && c + 1 < nchunk) fetch_row(c + 1, 0, hq[0]);
                    if (ng == 0) {   // the D path of y = ... + D u belongs to group 0, as in the forward kernel (dy = 0 past the end)
                        du0 = __builtin_fmaf(dy0, Dv[i], du0); du1 = __builtin_fmaf(dy1, Dv[i], du1);
                        accD[i] = __builtin_fmaf(dy0, us0, __builtin_fmaf(dy1, us1, accD[i]));
                    }
                    // the group's part of d dts: dh of a step past the end is not zero, its d delta is dropped here
                    const float gd0 = v0 ? ddl0 * sg0 : 0.f, gd1 = v1 ? ddl1 * sg1 : 0.f;
                    dp0 = __builtin_fmaf(ta[i], gd0, __builtin_fmaf(cw[i], du0, dp0));
                    dp1 = __builtin_fmaf(ta[i], gd1, __builtin_fmaf(cw[i], du1, dp1));
                    dp0 = __builtin_fmaf(us0, sB0, __builtin_fmaf(dy0, sC0, dp0));
                    dp1 = __builtin_fmaf(us1, sB1, __builtin_fmaf(dy1, sC1, dp1));
                    gta[i] = __builtin_fmaf(gd0, p0, __builtin_fmaf(gd1, p1, gta[i]));
                    gtb[i] += gd0 + gd1;
                    gcw[i] = __builtin_fmaf(du0, p0, __builtin_fmaf(du1, p1, gcw[i]));
                    gcb[i] += du0 + du1;
                }
            }
            if (v0) dpp[wave * L + l0] = dp0;
            if (v1) dpp[wave * L + l1] = dp1;
        }
        // the sums over the steps: dA_log per (row, state), dD per row (group 0), the wave's coefficient gradients
        float *cg = cgw + wave * kChCg;
#pragma unroll
        for (int nn = 0; nn < NPG; ++nn) {
            const float t0 = segment_sum_to_last<64>(gzaB[nn]), t1 = segment_sum_to_last<64>(gzbB[nn]);
            const float t2 = segment_sum_to_last<64>(gzaC[nn]), t3 = segment_sum_to_last<64>(gzbC[nn]);
            if (lane == 63) { cg[nn] = t0; cg[4 + nn] = t1; cg[8 + nn] = t2; cg[12 + nn] = t3; }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < dc) {
                const float t0 = segment_sum_to_last<64>(gta[i]), t1 = segment_sum_to_last<64>(gtb[i]);
                const float t2 = segment_sum_to_last<64>(gcw[i]), t3 = segment_sum_to_last<64>(gcb[i]);
                const float tD = segment_sum_to_last<64>(accD[i]);
                if (lane == 63) {
                    cg[16 + i] = t0; cg[20 + i] = t1; cg[24 + i] = t2; cg[28 + i] = t3;
                    if (ng == 0) gp[sl.dD + k * dc + i] = tD;
                }
#pragma unroll
                for (int nn = 0; nn < NPG; ++nn) {
                    const float tA = segment_sum_to_last<64>(accA[i][nn]);
                    if (lane == 63) gp[sl.dA + (k * dc + i) * kChN + n0 + nn] = tA * Av[i][nn];   // d/dA_log: A = -exp(A_log)
                }
            }
        }
    }
    __syncthreads();
    // ---- from the coefficient gradients to the parameter slots ---------------------------------------------------------------
    // sums over the four state groups of a direction, in group order
    auto group_sum = [&](int row, int off) {
        const float *q = cgw + (row / dc) * GPD * kChCg + off + row % dc;
        return ((q[0] + q[kChCg]) + q[2 * kChCg]) + q[3 * kChCg];
    };
    for (int o = tid; o < 2 * Cc + 2 * dc; o += NT) {
        if (o < 2 * Cc) {   // d za, d zb of column (k, c): the dt columns through dtc_projs, a B / C column from the wave that owns the state
            const int k = o / Cc, c = o - k * Cc;
            float a = 0.f, bb = 0.f;
            if (c < Rc) {
                for (int i = 0; i < dc; ++i) {
                    const float w = p.Wdtc[(k * dc + i) * Rc + c];
                    a = __builtin_fmaf(w, group_sum(k * dc + i, 16), a);
                    bb = __builtin_fmaf(w, group_sum(k * dc + i, 20), bb);
                }
            } else {
                const int n = (c - Rc) % kChN, isC = (c - Rc) / kChN;
                const float *q = cgw + (k * GPD + n / NPG) * kChCg + isC * 8 + n % NPG;
                a = q[0]; bb = q[4];
            }
            dza[o] = a; dzb[o] = bb;
        } else {
            const int row = o - 2 * Cc;
            const float a = group_sum(row, 16), bb = group_sum(row, 20);
            dta[row] = a; dtb[row] = bb;
            gp[sl.dbias + row] = bb;
        }
    }
    for (int l = tid; l < L; l += NT) {   // d pooled: the waves' parts in wave order
        float s = dpp[l];
#pragma unroll
        for (int w = 1; w < NW; ++w) s += dpp[w * L + l];
        dpool[(size_t)b * L + l] = s;
    }
    // gradients of conv_cout (sums over l of dyc * (y0 + y1), and of dyc): wave o does output o; slot dc = the bias
    if (wave <= dc) {
        const int o = wave;
        float a = 0.f;
        if (lift) {
            for (int l = lane; l < L; l += 64)
                a = o < dc ? __builtin_fmaf(dys[l], yb[o * L + l] + yb[(dc + o) * L + l], a) : a + dys[l];
        }
        const float t = segment_sum_to_last<64>(a);
        if (lane == 63) gp[sl.coutw + o] = t;
    }
    __syncthreads();
    const int n_wdtc = 2 * dc * Rc, n_wxc = 2 * Cc * dc;
    for (int o = tid; o < n_wdtc + n_wxc; o += NT) {
        if (o < n_wdtc) {
            const int row = o / Rc, r = o - row * Rc, col = (row / dc) * Cc + r;
            gp[sl.wdtc + o] = __builtin_fmaf(dta[row], T.za[col], dtb[row] * T.zb[col]);
        } else {
            const int q = o - n_wdtc, i = q % dc, kc = q / dc;
            gp[sl.wxc + q] = __builtin_fmaf(dza[kc], T.cw[i], dzb[kc] * T.cb[i]);
        }
    }
    // conv_cin: wave i the weight, wave 4 + i the bias: the direct part (the eight waves' d cw / d cb in wave order) plus the part
    // through xc_proj (lanes across the 2 Cc columns)
    {
        const int i = wave & 3, isb = wave >> 2;
        if (i < dc) {
            const float *dz = isb ? dzb : dza;
            float s = 0.f;
            if (lift) {
                for (int kc = lane; kc < 2 * Cc; kc += 64) s = __builtin_fmaf(p.Wxc[kc * dc + i], dz[kc], s);
            }
            const float t = segment_sum_to_last<64>(s);
            const float *q = cgw + 24 + isb * 4 + i;
            float d = q[0];
#pragma unroll
            for (int w = 1; w < NW; ++w) d += q[w * kChCg];
            if (lane == 63) gp[sl.cinw + isb * dc + i] = lift ? d + t : 0.f;
        }
    }
}

// gsum[j] = sum_b gpart[b][j] in batch order
__global__ void __launch_bounds__(256)
oss_chan_grad_finish(const float *__restrict__ gpart, float *__restrict__ gsum, int B, int NP) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= NP) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += gpart[(size_t)b * NP + j];
    gsum[j] = s;
}

// out[row] = alpha * sum_p a[row, p] * (bmul ? bmul[row, p] : 1);  rows = batch * channels, planes contiguous
template <typename T>
__global__ void __launch_bounds__(256)
oss_rowsum_kernel(const T *__restrict__ a, const T *__restrict__ bmul, float *__restrict__ out, int C, int P, int64_t asb,
                  int64_t asc, int64_t bsb, int64_t bsc, float alpha) {
    __shared__ float red[4];
    const int row = blockIdx.x, b = row / C, c = row - b * C, tid = threadIdx.x;
    const T *ap = a + b * asb + c * asc;
    const T *bp = bmul ? bmul + b * bsb + c * bsc : nullptr;
    float s = 0.f;
    const bool vec = (P % 8 == 0) && ((reinterpret_cast<uintptr_t>(ap) | reinterpret_cast<uintptr_t>(bp)) & 15u) == 0;
    if (vec) {
        // two 2048-element pieces per trip, all four loads requested before the first product (round 4: one piece per trip with the
        // second operand behind `if (bp)` was load -> wait -> load -> wait, twice over at P = 4096)
        const T *bq = bp ? bp : ap;   // no second operand: any readable address, the value is not used
        for (int p = tid * 8; p < P; p += 4096) {
            const bool two = p + 2048 < P;
            const int p2 = two ? p + 2048 : p;
            float a0[8], b0[8], a1[8], b1[8];
            load_items<8>(ap + p, 8, true, a0);
            load_items<8>(bq + p, 8, true, b0);
            load_items<8>(ap + p2, 8, true, a1);
            load_items<8>(bq + p2, 8, true, b1);
#pragma unroll
            for (int i = 0; i < 8; ++i) s = bp ? __builtin_fmaf(a0[i], b0[i], s) : s + a0[i];
            if (two) {
#pragma unroll
                for (int i = 0; i < 8; ++i) s = bp ? __builtin_fmaf(a1[i], b1[i], s) : s + a1[i];
            }
        }
    } else {
        for (int p = tid; p < P; p += 256) s = bp ? __builtin_fmaf(to_f32(ap[p]), to_f32(bp[p]), s) : s + to_f32(ap[p]);
    }
    const float t = block_sum<256>(s, red, tid);
    if (tid == 0) out[row] = t * alpha;
}

// y[row, p] = x[row, p] * (mul ? 1 + mul[row] : 1) + (add ? alpha * add[row] : 0)
template <typename T>
__global__ void __launch_bounds__(256)
oss_row_affine_kernel(const T *__restrict__ x, const float *__restrict__ mul, const float *__restrict__ add, T *__restrict__ y,
                      int C, int P, int64_t xsb, int64_t xsc, float alpha) {
    const int row = blockIdx.y, b = row / C, c = row - b * C;
    const T *xp = x + b * xsb + c * xsc;
    T *yp = y + (size_t)row * P;
    // (round 4) the two per-row scalars and the row's data: three independent loads, requested together (`mul ? 1 + mul[row] : 1` was
    // a branch + load + wait of its own, twice, in front of the data load: three dependent round trips in a 5 us kernel)
    const float *mp = mul ? mul + row : reinterpret_cast<const float *>(x), *ap = add ? add + row : mp;   // stand-ins: readable
    const float mv = *mp, av = *ap;
    const int p = (blockIdx.x * 256 + threadIdx.x) * 8;
    if (p >= P) return;
    const bool vec = (P % 8 == 0) && ((reinterpret_cast<uintptr_t>(xp) | reinterpret_cast<uintptr_t>(yp)) & 15u) == 0;
    float v[8];
    const int valid = min(8, P - p);
    load_items<8>(xp + p, valid, vec, v);
    const float sc = mul ? 1.f + mv : 1.f, sh = add ? alpha * av : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = __builtin_fmaf(v[i], sc, sh);
    store_items<8>(yp + p, valid, vec, v);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
size_t chan_grad_floats(int L, int dc, int Rc, int Cc) { return (size_t)ChanSlots(L, dc, Rc, Cc).total; }

constexpr size_t kChanLdsMax = 160 * 1024;   // the whole LDS of a CU: one workgroup per image, a handful of images
static int chan_enable_lds(const void *kern, size_t bytes) {
    if (bytes <= 48 * 1024) return 0;
    return (int)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kChanLdsMax);
}

static int chan_check(const oss_chan_params &p) {
    if (p.B <= 0 || p.L <= 0 || p.dc < 1 || p.dc > 4 || p.Rc < 1 || p.Cc != p.Rc + 2 * kChN) return OSS_ERR_SHAPE;
    if (!p.pooled || !p.Wxc || !p.Wdtc || !p.dt_bias || !p.A_logs || !p.Dsc || !p.cn_w || !p.cn_b || !p.hs || !p.y ||
        !p.yc || !p.stat || !p.c)
        return OSS_ERR_NULL;
    if ((p.cin_w != nullptr) != (p.cout_w != nullptr)) return OSS_ERR_NULL;
    if (p.cin_w && (!p.cin_b || !p.cout_b)) return OSS_ERR_NULL;
    return 0;
}

// floats of LDS the kernels keep per image (ops/channel.py: chan_supported repeats the forward's, the larger one)
static size_t chan_fwd_lds_floats(const oss_chan_params &p) {
    return (size_t)(10 * p.dc + 2) * p.L + kChRed + chan_tab_floats(p.dc, p.Cc);   // pooled, y, yc, the four groups' parts of y
}
static size_t chan_bwd_lds_floats(const oss_chan_params &p) {
    return (size_t)(1 + kChNT / 64) * p.L + kChRed + chan_tab_floats(p.dc, p.Cc) + (kChNT / 64) * kChCg + 4 * (size_t)p.Cc + 4 * p.dc;
}

int chan_fwd(const oss_chan_params &p, hipStream_t s) {
    if (int e = chan_check(p)) return e;
    const size_t smem = sizeof(float) * chan_fwd_lds_floats(p);
    if (smem > kChanLdsMax) return OSS_ERR_SHAPE;
    if (int e = chan_enable_lds(reinterpret_cast<const void *>(oss_chan_fwd_kernel<kChNT>), smem)) return e;
    hipLaunchKernelGGL((oss_chan_fwd_kernel<kChNT>), dim3(p.B), dim3(kChNT), smem, s, p);
    return (int)hipGetLastError();
}

int chan_bwd(const oss_chan_params &p, const float *gc, float *dpool, float *gsum, float *scratch, hipStream_t s) {
    if (int e = chan_check(p)) return e;
    if (!gc || !dpool || !gsum || !scratch) return OSS_ERR_NULL;
    const size_t smem = sizeof(float) * chan_bwd_lds_floats(p);
    if (smem > kChanLdsMax || sizeof(float) * chan_fwd_lds_floats(p) > kChanLdsMax) return OSS_ERR_SHAPE;
    if (int e = chan_enable_lds(reinterpret_cast<const void *>(oss_chan_bwd_kernel<kChNT>), smem)) return e;
    const size_t np = chan_grad_floats(p.L, p.dc, p.Rc, p.Cc);
    float *gpart = scratch;   // (B, np): the per-image gradient vectors
    hipLaunchKernelGGL((oss_chan_bwd_kernel<kChNT>), dim3(p.B), dim3(kChNT), smem, s, p, gc, dpool, gpart);
    if (defer_finish())
        defer_sum(gpart, p.B, np, np, gsum, np, nullptr);
    else
        hipLaunchKernelGGL(oss_chan_grad_finish, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s, gpart, gsum, p.B, (int)np);
    return (int)hipGetLastError();
}

size_t chan_bwd_scratch_floats(int B, int L, int dc, int Rc, int Cc) { return (size_t)B * chan_grad_floats(L, dc, Rc, Cc); }

int rowsum(oss_dtype io, const void *a, const void *bmul, float *out, int B, int C, int P, int64_t asb, int64_t asc, int64_t bsb,
           int64_t bsc, float alpha, hipStream_t s) {
    return io_dispatch(io, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(oss_rowsum_kernel<T>, dim3(B * C), dim3(256), 0, s, reinterpret_cast<const T *>(a), reinterpret_cast<const T *>(bmul),
                           out, C, P, asb, asc, bsb, bsc, alpha);
        return (int)hipGetLastError();
    });
}

int row_affine(oss_dtype io, const void *x, const float *mul, const float *add, void *y, int B, int C, int P, int64_t xsb,
               int64_t xsc, float alpha, hipStream_t s) {
    return io_dispatch(io, [&](auto tag) {
        using T = typename decltype(tag)::type;
        if ((long)B * C > 65535) return OSS_ERR_SHAPE;
        hipLaunchKernelGGL(oss_row_affine_kernel<T>, dim3((P + 2047) / 2048, B * C), dim3(256), 0, s, reinterpret_cast<const T *>(x), mul, add,
                           reinterpret_cast<T *>(y), C, P, xsb, xsc, alpha);
        return (int)hipGetLastError();
    });
}

}  // namespace oss
