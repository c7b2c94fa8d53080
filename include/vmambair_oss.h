/*
 * vmambair_oss.h -- C ABI of the MI355X (gfx950) Omni-Selective-Scan core.
 *
 * This is the drop-in boundary for the one native module the reference's archs import:
 *     import selective_scan_cuda_core          (reference: SRGAN/VmambaIR/archs/MambaSISR6_arch.py:22,
 *                                               Deraining/basicsr/models/archs/mamber32_arch.py:18,
 *                                               RealSR/VmambaIR/archs/MambaRealSR11_arch.py:24,32)
 * whose two entry points are pybind11 functions
 *     fwd(u, delta, A, B, C, D, delta_bias, delta_softplus, nrows) -> [out, x]
 *     bwd(u, delta, A, B, C, D, delta_bias, dout, x, delta_softplus, nrows)
 *            -> [du, ddelta, dA, dB, dC, dD, ddelta_bias]
 * (reference: Mamba/kernels/selective_scan/csrc/selective_scan/cus/selective_scan.cpp:157-164,
 *  241-250,351-354).  Behind those, the reference fills a parameter struct of sizes, element
 * strides and raw pointers (selective_scan.h:26-90, SSMParamsBase / SSMParamsBwd) and launches
 * one kernel per I/O dtype on a caller-supplied stream
 * (cus/selective_scan_core_fwd.cu:6-8, cus/selective_scan_core_bwd.cu:6-8).
 *
 * The functions below are what a binding for that module links against: plain pointers, sizes,
 * element strides and a HIP stream -- no torch types.  The binding layer (ours:
 * vmambair_amd/_capi.py + selective_scan_cuda_core.py; a maintainer's: INTEGRATION.md) does the
 * shape/dtype checks and allocates outputs exactly as cus/selective_scan.cpp:165-220,256-327.
 *
 * All device pointers must live on the device that is current when the call is made.  Calls are
 * asynchronous on `stream`, never synchronise the host, and are re-entrant.
 * Return value: 0 on success, a negative OSS_ERR_* for a rejected argument, or a positive
 * hipError_t if the launch failed.
 *
 * The ctypes binding (vmambair_amd/_capi.py) is READ from this file by vmambair_amd/_cheader.py, which is no C parser, so
 * everything between the extern "C" braces keeps to this subset (anything else is a load-time error there, never skipped):
 *   #define OSS_NAME <int> | (<int>);   typedef enum { NAME = <int>, ... } name;   typedef void *name;
 *   typedef struct { <type> [*]field, [*]field; ... } name;   -- scalar, pointer and earlier-struct fields; no arrays, bit-fields, unions
 *   <ret> oss_name(<type> [*[*]][name], ...);   -- also (void); no function pointers, arrays or varargs
 *   types: int, int64_t, size_t, float, double, long long, the typedefs above, and pointers to anything
 */
#ifndef VMAMBAIR_OSS_H
#define VMAMBAIR_OSS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OSS_OK 0
#define OSS_ERR_NULL (-1)        /* a required pointer is NULL                               */
#define OSS_ERR_SHAPE (-2)       /* batch/dim/seqlen/dstate/n_groups invalid (dim % groups)   */
#define OSS_ERR_DSTATE (-3)      /* dstate > OSS_MAX_DSTATE (reference: selective_scan.cpp:191) */
#define OSS_ERR_WORKSPACE (-4)   /* workspace missing or too small                           */

#define OSS_MAX_DSTATE 256

/* I/O element type of u, delta, B, C, out, dout, du, ddelta (the reference's input_t);
 * A, D, delta_bias, x and every weight gradient are always float (weight_t). */
typedef enum {
    OSS_F32 = 0, OSS_F16 = 1, OSS_BF16 = 2,
    /* (ABI 8) NOT an element type but a per-call precision selector: "fp32 tensors, products on split bf16".  Accepted by exactly six
     * entry points -- oss_conv1x1_fwd / _dgrad / _wgrad, oss_proj_fwd / _dgrad / _wgrad -- where it means OSS_F32 tensors whose
     * GEMM-shaped products run on v_mfma_f32_32x32x16_bf16 with each fp32 operand value a taken as hi + lo, hi = bf16(a),
     * lo = bf16(a - hi) (lo = 0 where a - hi is not finite), three products per pair (lo hi, hi lo, hi hi; lo lo is dropped) into
     * one fp32 accumulator, fp32 epilogues:  |y - y_exact| <= (3 * 2^-16 + (K + 2) * 2^-23) * sum_k |w_k||x_k|.  gfx950 has no
     * xf32 / TF32 matrix instruction; this is what torch.set_float32_matmul_precision("high") describes.  Same shapes, alignment
     * rules, scratch sizes and error returns as OSS_F32; calls the exact fp32 matrix-core kernels decline (and that then run on
     * the vector-ALU kernels) are not affected by the selector.  Deterministic (fixed summation order, no atomics).  Every other
     * entry point rejects the value (OSS_ERR_SHAPE, or 0 from an *_ok query).  oss_f32_matmul_modes() & 2 says the library has it. */
    OSS_F32_BF16X3 = 3
} oss_dtype;

/* Opaque stream handle: a hipStream_t (NULL = the default stream). */
typedef void *oss_stream_t;

/* Mirrors SSMParamsBase (selective_scan.h:26-66).  Strides are in ELEMENTS; the last (time)
 * dimension of u, delta, B, C, out must be contiguous (selective_scan.cpp:183-199). */
typedef struct {
    int batch, dim, seqlen, dstate, n_groups;
    int delta_softplus;
    /* Omni-scan direction handling without materialising the four flattenings:
     *   rev_group_start : rows of groups g >= rev_group_start are scanned from t = L-1 down to 0, i.e.
     *                     every time-indexed tensor of those rows/groups (u, delta, B, C, out, dout,
     *                     du, ddelta, dB, dC) is read and written mirrored in time.  n_groups (or
     *                     any value >= n_groups) = none: the reference's plain call.
     *   u_row_mod       : when > 0, row d reads u[:, d % u_row_mod, :] (du still has `dim` rows), so
     *                     that directions k and k+2 share one copy of the activations.  0 = off. */
    int rev_group_start, u_row_mod;
    /* a_log_form != 0: the `A` pointer holds A_log and the kernels use A = -exp(A_log) (the archs'
     * `As = -torch.exp(self.A_logs.float())`, MambaSISR6_arch.py:415); bwd then returns dA_log. */
    int a_log_form, reserved0_;
    int64_t u_batch_stride, u_d_stride;
    int64_t delta_batch_stride, delta_d_stride;
    int64_t out_batch_stride, out_d_stride;
    int64_t A_d_stride;                                  /* A is (dim, dstate), dstate stride 1 */
    int64_t B_batch_stride, B_group_stride, B_dstate_stride;
    int64_t C_batch_stride, C_group_stride, C_dstate_stride;
    const void *u, *delta;  /* (batch, dim, seqlen) io dtype                                   */
    const float *A;         /* (dim, dstate)                                                   */
    const void *B, *C;      /* (batch, n_groups, dstate, seqlen) io dtype                      */
    const float *D;         /* (dim) or NULL                                                   */
    const float *delta_bias;/* (dim) or NULL                                                   */
    void *out;              /* (batch, dim, seqlen) io dtype                                   */
    float *x;               /* (batch, dim, oss_scan_num_chunks(seqlen), 2*dstate) contiguous  */
    /* Delta computed INSIDE the scan (the archs' `dts = einsum(dts, dt_projs_weight)` followed by
     * the scan, SRGAN/VmambaIR/archs/MambaSISR6_arch.py:409-424): with dt_weight != NULL the `delta` pointer holds the
     * rank-dt_rank factor z: (batch, n_groups, >= dt_rank rows, seqlen) io dtype -- the first rows of x_dbl -- with element
     * strides (delta_batch_stride, dt_group_stride, dt_rank_stride), time contiguous (mirrored like B / C for groups >=
     * rev_group_start), and the kernels evaluate
     *     delta[b, d, t] = sum_r dt_weight[d * dt_rank + r] * z[b, group(d), r, t]        (fp32, r ascending)
     * so the (batch, dim, seqlen) delta tensor never exists.  delta_d_stride is ignored then.  dt_rank <= 8 (every
     * reference config where the fused form is used: D <= 128). */
    const float *dt_weight; /* (dim, dt_rank) float contiguous, or NULL = `delta` is the (batch, dim, seqlen) tensor */
    int dt_rank, reserved1_;
    int64_t dt_group_stride, dt_rank_stride;
    /* Optional scratch of oss_scan_fwd_workspace_bytes() bytes (no init needed) for oss_scan_fwd.  With it, calls whose
     * (batch, group, row tile) grid cannot fill the GPU (batch-1 inference tiles, few-row levels) are cut into time
     * segments that run as separate workgroups (two launches: segment-local pass, then the real pass from the folded
     * carries; oss_scan_set_segments).  NULL / too small = every row is walked by one workgroup, as the reference does
     * (cus/selective_scan_fwd_kernel.cuh:101-102).  Ignored by oss_scan_bwd (which has its own workspace). */
    void *workspace;
    size_t workspace_bytes;
    /* Optional lane states (round 3; oss_scan_features() & OSS_FEATURE_LANE_STATES -- in every library since round 6; a
     * library built without it ignores the field): oss_scan_lane_state_floats() floats, layout [batch][dim][dstate][L8] with
     * L8 = round_up(ceil(seqlen / 8), 64): entry k of a (batch, row, state) line is the state h ENTERING scan steps 8k .. 8k+7
     * (h after step 8k - 1; 0 for k = 0).  oss_scan_fwd writes them when hs != NULL (a by-product of its second pass);
     * oss_scan_bwd given the same buffer in f.hs reads them instead of re-running the forward recurrence and one lane scan per
     * state (round-2 kernels, dstate <= 64, not the fused-delta form) -- same gradients to fp32 round-off.  NULL = recompute
     * from `x`, as the reference's backward does (cus/selective_scan_bwd_kernel.cuh:184-186).  The torch layers carry the
     * buffer as a third tensor next to (out, x): selective_scan_fwd(..., want_hs) -> [out, x, hs], selective_scan_bwd(..., hs). */
    float *hs;
    /* Per-call launch tuning (round 6; ABI 7).  0 everywhere = the library's heuristics, which is what every product caller
     * passes (memset the struct).  These fields are the thread- and stream-safe way to force a launch shape; the process-global
     * setters further down (oss_scan_set_variant / _segments / _carry_split) exist for the test-suite and A-B timing scripts only
     * and are overridden by a non-zero field.
     *   tune_variant     : v + 1 forces kernel variant v of THIS call's direction (oss_scan_fwd: forward variants 0..7; in
     *                      oss_scan_bwd_params.f the field is ignored -- the backward's own tune_variant is used)
     *   tune_segments    : 1 = never cut the call in time, n > 1 = n time segments per row (clamped to the chunk count)
     *   tune_carry_split : n >= 1 = pieces per main segment of the local / reverse-carry pass (see oss_scan_set_carry_split);
     *                      oss_scan_bwd reads it from f.tune_carry_split */
    int tune_variant, tune_segments, tune_carry_split, reserved2_;
} oss_scan_fwd_params;

/* Mirrors SSMParamsBwd (selective_scan.h:68-90). */
typedef struct {
    oss_scan_fwd_params f;  /* f.out unused; f.x = the tensor fwd returned (required when
                               oss_scan_num_chunks(seqlen) > 1, selective_scan.cpp:310)          */
    int64_t dout_batch_stride, dout_d_stride;
    int64_t du_batch_stride, du_d_stride;
    int64_t ddelta_batch_stride, ddelta_d_stride;
    const void *dout;       /* (batch, dim, seqlen) io dtype                                   */
    void *du, *ddelta;      /* (batch, dim, seqlen) io dtype                                   */
    float *dA;              /* (dim, dstate) contiguous, overwritten                           */
    void *dB, *dC;          /* (batch, n_groups, dstate, seqlen) io dtype, overwritten (the cast of
                               selective_scan.cpp:347 is fused); contiguous unless
                               dBC_group_stride is set                                          */
    float *dD;              /* (dim) or NULL, overwritten                                      */
    float *ddelta_bias;     /* (dim) or NULL, overwritten                                      */
    void *workspace;        /* oss_scan_bwd_workspace_bytes() bytes of scratch, no init needed */
    size_t workspace_bytes;
    int dout_row_mod;       /* > 0: row d reads dout[:, d % dout_row_mod, :] (the merge hands the same
                               gradient to directions k and k + 2); 0 = off                        */
    int reserved_;
    int64_t dBC_group_stride; /* element stride between (batch, group) blocks of dB and of dC; the batch
                                 stride is n_groups times it.  0 = dstate * seqlen (contiguous).  Lets
                                 the caller have dB / dC written into the rows of a wider buffer.  */
    /* f.dt_weight != NULL (delta computed inside the scan): ddelta is not written; instead
     *   ddt[b, g, r, t]  = sum over the rows d of group g of dt_weight[d, r] * ddelta[b, d, t]   (io dtype; the dt rows of the
     *                      gradient of x_dbl -- with dBC_group_stride the kernel fills ALL rows of that gradient)
     *   ddt_weight[d, r] = sum over b, t of ddelta[b, d, t] * z[b, g, r, t]                       (float, (dim, dt_rank))
     * Only the round-2 kernels do this: dstate <= 64, 16-bit or float I/O, dt_rank <= 8. */
    void *ddt;
    float *ddt_weight;
    int64_t ddt_batch_stride, ddt_group_stride, ddt_rank_stride;
    /* per-call launch tuning of the backward (see oss_scan_fwd_params.tune_*): v + 1 forces backward variant v (1, 10..13);
     * 1 = never segment, n > 1 = n time segments.  0 = heuristic. */
    int tune_variant, tune_segments;
    /* row-tile partials of dB / dC (scratch between the main and the finishing kernel): 0 / 1 = fp32 (default: the reference's fp32
     * accumulation, cus/selective_scan_bwd_kernel.cuh:208-221, to the letter); 2 = bf16 partials at bf16 I/O (round-2 kernels, not the
     * fused-delta / lane-state forms; ignored elsewhere): half the scratch traffic, but every tile's partial is rounded to 8 bits of
     * mantissa before the tiles are summed -- an absolute error of 2^-9 x |partial| that can leave the reference's bf16 tolerance
     * when the tiles cancel.  An opt-in for callers who accept that (measured +1.7 % on the headline step). */
    int tune_partials, reserved3_;
    /* (round 6) The dt-factor gradient in the backward's finishing launch.  With finish_dt_weight != NULL (and f.dt_weight == NULL:
     * delta materialised, ddelta written as usual) the finishing kernel -- which already adds the row-tile partials of dB / dC --
     * also evaluates the adjoint of the archs' `dts = einsum("b k r l, k d r -> b k d l", dts, dt_projs_weight)`
     * (SRGAN/VmambaIR/archs/MambaSISR6_arch.py:411):
     *     ddt[b, g, r, t] = sum over the rows d of group g of finish_dt_weight[d * finish_dt_rank + r] * ddelta[b, d, t]
     * into `ddt` (element strides ddt_batch_stride / ddt_group_stride / ddt_rank_stride; normally the first rows of the gradient
     * of x_dbl that dBC_group_stride already points dB / dC into), in extra workgroups of the SAME launch: the two are independent
     * and memory-bound, so the block's backward has one launch less (oss_dt_dgrad_kernel of oss_proj_dgrad, which is then called
     * with ddts == NULL).  oss_scan_bwd_finish_dt_ok() says whether a shape qualifies (rank <= 8, seqlen % 4 == 0; 8 / 16-byte
     * aligned ddelta / ddt rows). */
    const float *finish_dt_weight;  /* (dim, finish_dt_rank) float contiguous, or NULL */
    int finish_dt_rank, reserved4_;
} oss_scan_bwd_params;

/* Time steps between two saved states in `x` (the reference's is 2048,
 * selective_scan.cpp:217; `x` is opaque to every caller, only our bwd reads it). */
int oss_scan_chunk(void);
int oss_scan_num_chunks(int seqlen);

/* Replaces selective_scan_fwd_cuda<1, input_t, float> (cus/selective_scan_fwd_kernel.cuh:174-207). */
size_t oss_scan_fwd_workspace_bytes(int batch, int dim, int seqlen, int dstate, int n_groups);   /* 0 when seqlen <= 256 */
size_t oss_scan_lane_state_floats(int batch, int dim, int seqlen, int dstate);                    /* size of `hs` */
int oss_scan_fwd(const oss_scan_fwd_params *p, oss_dtype io, oss_stream_t stream);

/* Replaces selective_scan_bwd_cuda<1, input_t, float> (cus/selective_scan_bwd_kernel.cuh:275-310)
 * plus the zero-fills and casts around it (cus/selective_scan.cpp:319-327,347). */
/* (the workspace size covers the fused-delta form with dt_rank <= 8 as well) */
size_t oss_scan_bwd_workspace_bytes(int batch, int dim, int seqlen, int dstate, int n_groups);
int oss_scan_bwd(const oss_scan_bwd_params *p, oss_dtype io, oss_stream_t stream);

/* What a call would launch, without launching it: oss_scan_fwd_describe / oss_scan_bwd_describe fill `out` with the plan that
 * oss_scan_fwd / oss_scan_bwd run for the same block, element type and test overrides.  Pure host arithmetic on the block's
 * integers and on which of its pointers are NULL (workspace, hs, dt_weight, dD, ddelta_bias, ddt, ddt_weight): the data pointers
 * are neither required nor read, only the shape rules of the entry points apply (same OSS_ERR_* codes, plus OSS_ERR_WORKSPACE
 * from the backward when no launch fits workspace_bytes).  An empty call (batch or seqlen 0) gives OSS_OK, variant -1, zeros. */
typedef struct {
    int variant;             /* the selected variant number: what oss_scan_last_variant reports after the call */
    int rows_per_workgroup;  /* of the kernel that runs (a variant that does not fit this shape runs another variant's kernel) */
    int chunk;               /* its time steps per chunk */
    int workgroups;          /* batch x groups x row tiles; a time-segmented launch runs workgroups x segments */
    int segments;            /* time segments per row: what oss_scan_last_segments reports (1 = unsegmented) */
    int chunks_per_segment;  /* the last segment may be shorter */
    int carry_pieces;        /* pieces per segment of the local / reverse-carry pass (oss_scan_set_carry_split) */
    int chunks_per_piece;    /* ceil(chunks_per_segment / carry_pieces); segments x carry_pieces carry slots per row */
    int lane_states;         /* backward: 1 = the kernels that load f.hs (oss_scan_last_lane_states) */
    int fused_delta;         /* 1 = delta evaluated inside the scan (dt_weight) */
    int bf16_partials;       /* backward: 1 = bf16 row-tile partials (tune_partials == 2 honoured) */
    int reserved_;
    size_t lds_bytes;        /* dynamic LDS per workgroup of the main kernel */
    size_t workspace_bytes;  /* of the caller's workspace this launch uses (<= the oss_scan_*_workspace_bytes query) */
} oss_scan_launch;
int oss_scan_fwd_describe(const oss_scan_fwd_params *p, oss_dtype io, oss_scan_launch *out);
int oss_scan_bwd_describe(const oss_scan_bwd_params *p, oss_dtype io, oss_scan_launch *out);

/* 1 when oss_scan_bwd_params.finish_dt_weight may be used at this length / rank (see the struct) */
int oss_scan_bwd_finish_dt_ok(int seqlen, int dt_rank);

/* 1 when the fused-delta form (oss_scan_fwd_params.dt_weight) covers this SS2D_1 shape: 16-bit I/O on the matrix-core
 * projection kernels (which may then be called with dts / ddts == NULL), dt_rank <= 8, dstate <= 64, seqlen >= 512
 * (shorter sequences take the small-shape kernels, which read delta). */
int oss_scan_fused_dt_ok(oss_dtype io, int batch, int D, int C, int R, int dstate, int seqlen);

/* ---- PROCESS-GLOBAL tuning overrides: test-suite / A-B timing scripts ONLY ------------------------------------------------
 * The three setters below mutate process-wide state that every later call from every thread and stream reads; they are not a
 * product interface.  An integrator who needs a particular launch shape sets the per-call fields
 * oss_scan_fwd_params.tune_* / oss_scan_bwd_params.tune_* instead, which win over these.
 * Kernel-variant override: -1 = heuristic (default).  Forward variants 0..7, backward variants 0..13
 * (tables in oss_scan_fwd.hip / oss_scan_bwd.hip; 8 and 9 = two states per pass in packed fp32, oss_scan_bwd_pair.h; 10..13 =
 * the round-2 kernel, oss_scan_bwd_v2.h).  An
 * unknown number falls back to the small-shape variant. */
void oss_scan_set_variant(int fwd_variant, int bwd_variant);
int oss_scan_last_variant(int which /* 0 fwd, 1 bwd */);
/* Time segments per row of the next launches (tuning / tests): -1 = heuristic (segments only when the launch would leave
 * most CUs without a workgroup), 0 or 1 = never, n > 1 = n segments (clamped to the number of chunks of the kernel variant;
 * the backward segments only its round-2 kernels, variants 10..13, dstate <= 64, and never the fused-delta form).
 * oss_scan_last_segments: what the last call used (1 = unsegmented). */
void oss_scan_set_segments(int fwd_segments, int bwd_segments);
int oss_scan_last_segments(int which /* 0 fwd, 1 bwd */);
/* (round 5) A time-segmented call runs a cheap first launch -- the forward's segment-local pass, the backward's reverse-carry
 * pass -- whose per-segment (product, state) pairs the main launch folds.  That first launch has its own, FINER segmentation: each main
 * segment's cps chunks are cut into pieces of ceil(cps / split) chunks (ANY split: the last piece is shorter or empty and an empty
 * piece keeps the identity pair), one workgroup and one pair slot per piece, so that it fills the CUs the main launch's segment
 * count was chosen for.  0 = heuristic (default: up to 512 workgroups), 1 = as coarse as the main launch (rounds 2-4).  Results
 * differ from split = 1 only in how the carries are associated (fp32 round-off).  The pair slots live in the caller's workspace:
 * size it with oss_scan_fwd_workspace_bytes / oss_scan_bwd_workspace_bytes (they cover min(chunks, 64) slots per row and state);
 * a workspace that holds the main segments' slots but not the finer pieces' makes the launch fall back to split = 1, and one
 * that does not even hold those to the unsegmented launch. */
void oss_scan_set_carry_split(int split);
/* 1 when the last oss_scan_bwd call ran the kernels that load the forward pass's lane states (f.hs), else 0 */
int oss_scan_last_lane_states(void);

/* Depth-wise 3x3 convolution, stride 1, zero padding 1, of the OSS block: SS2D_1.conv2d
 * (SRGAN/VmambaIR/archs/MambaSISR6_arch.py:286-294) and the EFFN dwconv (:209); both are
 * nn.Conv2d(C, C, 3, padding=1, groups=C).  x, y, dy, dx: (batch, C, H, W) io dtype with contiguous
 * H*W planes and element strides (batch, channel); weight (C, 9) and bias (C) float (bias may be
 * NULL).  oss_dwconv3x3_fwd computes y = conv(x) + bias; with flip = 1 it applies the mirrored taps,
 * i.e. the input gradient dx = conv_transpose(dy).  oss_dwconv3x3_wgrad overwrites dweight (C, 9)
 * and dbias (C, or NULL) with the sums over batch and pixels; `partials` is batch*C*10 floats of
 * scratch (no init needed).
 * Fused activation (SS2D_1: x = act(conv2d(x)), MambaSISR6_arch.py:486): with pre_silu != NULL (contiguous (batch, C, H, W))
 * the forward stores the convolution there and y = silu(convolution); the weight-gradient call given the same pre_silu
 * uses dy * silu'(pre_silu) as the gradient reaching the convolution and also writes it to dpre (contiguous), which is then
 * the input of the flip = 1 call that produces dx. */
int oss_dwconv3x3_fwd(oss_dtype io, const void *x, const float *weight, const float *bias, void *y, void *pre_silu, int batch,
                      int channels, int height, int width, int64_t x_batch_stride, int64_t x_channel_stride,
                      int64_t y_batch_stride, int64_t y_channel_stride, int flip, oss_stream_t stream);
int oss_dwconv3x3_wgrad(oss_dtype io, const void *x, const void *dy, float *dweight, float *dbias, float *partials,
                        const void *pre_silu, void *dpre, int batch, int channels, int height, int width,
                        int64_t x_batch_stride, int64_t x_channel_stride, int64_t dy_batch_stride, int64_t dy_channel_stride,
                        oss_stream_t stream);

/* The depth-wise convolution fused with the element-wise step that follows it, without ever storing the convolution
 * (16-bit io, and OSS_F32 since ABI 6 / round 4; oss_dwconv3x3_fused_ok(io, H, W, 1 | 2) says whether a shape qualifies: width % 8 == 0,
 * and 1 (silu) or 2 (gate) planes of (H + 2) x W elements fit the 160 KiB LDS of a workgroup; pointers 16-byte aligned and strides
 * multiples of 8 elements, else OSS_ERR_SHAPE).
 *   oss_dwconv3x3_silu_fwd: y = silu(conv(x) + bias)                         (SS2D_1: x = act(conv2d(x)), MambaSISR6_arch.py:486)
 *   oss_dwconv3x3_silu_bwd: dx, dweight, dbias of it from x and dy -- the convolution is recomputed from the rows of x the
 *                           weight gradient reads anyway, dy * silu' stays in LDS between the two passes of ONE launch
 *   oss_dwgate_fwd:         out (batch, hidden, H, W) = gelu(x1) * x2 with x1, x2 = the two channel halves of
 *                           conv(t) + bias, t (batch, 2 hidden, H, W)         (FeedForward.forward, MambaSISR6_arch.py:213-217)
 *                           The forward streams (nothing LDS-resident) and takes every plane oss_dwgate_fwd_ok accepts: width a multiple
 *                           of 8 and <= 512, any height -- the inference path of planes the backward's form cannot hold
 *   oss_dwgate_bwd:         dt, dweight (2 hidden, 9), dbias of it from t and dout, one launch
 * partials: batch * channels * 10 floats of scratch (channels = 2 hidden for the gate); dbias may be NULL.  The gradients that
 * reach the convolution are rounded to the io type before both uses, as the separate kernels hand them over. */
int oss_dwconv3x3_fused_ok(oss_dtype io, int height, int width, int channels_per_workgroup);
int oss_dwconv3x3_silu_fwd(oss_dtype io, const void *x, const float *weight, const float *bias, void *y, int batch, int channels,
                           int height, int width, int64_t x_batch_stride, int64_t x_channel_stride, int64_t y_batch_stride,
                           int64_t y_channel_stride, oss_stream_t stream);
int oss_dwconv3x3_silu_bwd(oss_dtype io, const void *x, const float *weight, const float *bias, const void *dy, void *dx,
                           float *dweight, float *dbias, float *partials, int batch, int channels, int height, int width,
                           int64_t x_batch_stride, int64_t x_channel_stride, int64_t dy_batch_stride, int64_t dy_channel_stride,
                           int64_t dx_batch_stride, int64_t dx_channel_stride, oss_stream_t stream);
int oss_dwgate_fwd_ok(oss_dtype io, int height, int width);

/* The whole second half of an OSS block, forward only (inference), as ONE launch:
 *   out = x + project_out( gelu(x1) * x2 ),  x1, x2 = dwconv3x3( project_in( norm2(x) ) ).chunk(2)
 * (FeedForward.forward, SRGAN/VmambaIR/archs/MambaSISR6_arch.py:201-218; the block's `x = x + self.ffn(self.norm2(x))`, :513-516;
 * LayerNorm :144-195 -- norm_bias NULL = the BiasFree form.)  The 2 hidden-channel and hidden-channel intermediates never reach memory;
 * they are rounded to the io type where the launch-per-layer chain (oss_conv1x1_fwd with norm, oss_dwgate_fwd, oss_conv1x1_fwd with
 * residual) stores them, so the two forms agree to the rounding of the last accumulation.  No biases on the three convolutions (no
 * reference config has them: `bias: False` in every options file).
 *   x, out: (batch, channels, H, W) of the io type (OSS_F16 / OSS_BF16), rows contiguous, 16-byte aligned, strides multiples of 8
 * With HP = hidden rounded up to a multiple of 16 and every padding row / column ZERO (the kernel's loop has no masks):
 *   w_in:   (2 HP, channels) of the io type -- project_in.weight rounded once by the caller (in inference a constant): rows
 *           0 .. hidden - 1 = its first half (x1), rows HP .. HP + hidden - 1 = its second half (x2)
 *   w_dw:   (2 HP, 9) float -- dwconv.weight in the same row order
 *   w_out:  (channels, HP) of the io type -- project_out.weight
 * oss_effn_fwd_ok: channels in {32, 48, 64, 96}, width a multiple of 8; anything else (and every training call) stays on the chain. */
int oss_effn_fwd_ok(oss_dtype io, int channels, int hidden, int height, int width);
/* w_in / w_dw / w_out of oss_effn_fwd from the module's float parameters (project_in.weight (2 hidden, channels), dwconv.weight
 * (2 hidden, 9), project_out.weight (channels, hidden)) in ONE launch: an inference graph captures it in front of the forward and
 * so never replays stale copies after the parameters changed in place. */
int oss_effn_round_weights(oss_dtype io, const float *project_in, const float *dwconv, const float *project_out, void *w_in, float *w_dw,
                           void *w_out, int channels, int hidden, oss_stream_t stream);
int oss_effn_fwd(oss_dtype io, const void *x, const float *norm_weight, const float *norm_bias, const void *w_in, const float *w_dw,
                 const void *w_out, void *out, int batch, int channels, int hidden, int height, int width, int64_t x_batch_stride,
                 int64_t x_channel_stride, int64_t out_batch_stride, int64_t out_channel_stride, float eps, oss_stream_t stream);
int oss_dwgate_fwd(oss_dtype io, const void *t, const float *weight, const float *bias, void *out, int batch, int hidden,
                   int height, int width, int64_t t_batch_stride, int64_t t_channel_stride, int64_t out_batch_stride,
                   int64_t out_channel_stride, oss_stream_t stream);
int oss_dwgate_bwd(oss_dtype io, const void *t, const float *weight, const float *bias, const void *dout, void *dt,
                   float *dweight, float *dbias, float *partials, int batch, int hidden, int height, int width,
                   int64_t t_batch_stride, int64_t t_channel_stride, int64_t dout_batch_stride, int64_t dout_channel_stride,
                   int64_t dt_batch_stride, int64_t dt_channel_stride, oss_stream_t stream);

/* The same convolution + silu together with cross_scan_2d's two forward flattenings (MambaSISR6_arch.py:399-404, 486): the scans of
 * SS2D_1 read silu(conv2d(x)) row-major AND column-major, and their input gradient comes back as one tensor per flattening.
 *   oss_dwconv3x3_silu_flat2_fwd: x2 (batch, 2, channels, H * W) contiguous = [silu(conv(x) + bias) | the same planes transposed,
 *                                 element (h, w) at w * H + h] -- what oss_dwconv3x3_silu_fwd + oss_cross_scan2 produce, bit for bit
 *   oss_dwconv3x3_silu_flat2_bwd: as oss_dwconv3x3_silu_bwd with dy(h, w) = g2[:, 0](h, w) + g2[:, 1](w, h) rounded to the io type --
 *                                 what oss_cross_merge2 + oss_dwconv3x3_silu_bwd produce, bit for bit; g2 (batch, 2, channels, H * W)
 * oss_dwconv3x3_flat2_ok(io, H, W): fused_ok(io, H, W, 1), H % 8 == 0, W / 8 a power of two <= 32; else OSS_ERR_SHAPE. */
int oss_dwconv3x3_flat2_ok(oss_dtype io, int height, int width);
int oss_dwconv3x3_silu_flat2_fwd(oss_dtype io, const void *x, const float *weight, const float *bias, void *x2, int batch, int channels,
                                 int height, int width, int64_t x_batch_stride, int64_t x_channel_stride, oss_stream_t stream);
int oss_dwconv3x3_silu_flat2_bwd(oss_dtype io, const void *x, const float *weight, const float *bias, const void *g2, void *dx,
                                 float *dweight, float *dbias, float *partials, int batch, int channels, int height, int width,
                                 int64_t x_batch_stride, int64_t x_channel_stride, int64_t dx_batch_stride, int64_t dx_channel_stride,
                                 oss_stream_t stream);

/* 1x1 convolutions of the OSS block (in_conv / out_conv / project_in / project_out,
 * MambaSISR6_arch.py:205,211,281,329) as MFMA GEMMs on NCHW tensors; io = OSS_BF16 or OSS_F16 (fp32
 * I/O is rejected with OSS_ERR_SHAPE: it stays on the vendor conv).  weight: float (Cout, Cin)
 * contiguous (master weights, converted in the loader); x / dy: (batch, C, pixels) io dtype, pixels
 * contiguous, element strides (batch, channel); y / dx contiguous.
 *   fwd  : y  = W x + bias (+ residual, contiguous like y: the skip connection of the block, MambaSISR6_arch.py:515-516)
 *   dgrad: dx = W^T dy
 *   wgrad: dweight (Cout, Cin) float = sum_{b,p} dy x^T and, when dbias != NULL, dbias (Cout) float =
 *          sum_{b,p} dy (an all-ones row appended to x inside the kernel); `partials` =
 *          oss_conv1x1_wgrad_partial_floats() floats of scratch. */
int oss_conv1x1_fwd(oss_dtype io, const void *x, const float *weight, const float *bias, const void *residual, void *y,
                    int batch, int cout, int cin, int pixels, int64_t x_batch_stride, int64_t x_channel_stride,
                    oss_stream_t stream);
int oss_conv1x1_dgrad(oss_dtype io, const void *dy, const float *weight, void *dx, int batch, int cout, int cin, int pixels,
                      int64_t dy_batch_stride, int64_t dy_channel_stride, oss_stream_t stream);
size_t oss_conv1x1_wgrad_partial_floats(int batch, int cout, int cin, int pixels);
/* Pre-packed 16-bit weight images of oss_conv1x1_fwd / oss_conv1x1_dgrad.  The weights change once per optimizer step, yet every
 * wave of every launch narrows the fp32 matrix again; an IMAGE holds the matrix operand of one direction already narrowed to the
 * io type (the loaders' round-to-nearest-even), zero-padded to whole tiles and in MFMA fragment order.  For the (M x K) product
 * operand W(m, k), KSTEPS = ceil(K / 16), tile t < ceil(M / 32), k-step s < KSTEPS, lane l < 64, e < 8:
 *   image[((t * KSTEPS + s) * 64 + l) * 8 + e] = W(32 t + (l & 31), 16 s + 8 (l >> 5) + e)      (0 outside M x K)
 *   forward image:        M = cout, K = cin,  W(m, k) = weight[m * cin + k]
 *   input-gradient image: M = cin,  K = cout, W(m, k) = weight[k * cin + m]
 * i.e. ceil(M / 32) * ceil(K / 16) * 1024 bytes each (oss_conv1x1_fwd_image_bytes / _dgrad_image_bytes), 16-byte aligned.
 * oss_conv1x1_pack_weights writes the images of MANY weights in one launch from a table in DEVICE memory of
 * oss_conv1x1_pack_row_bytes() bytes per row; oss_conv1x1_pack_fill (host only, no GPU work) writes the
 * oss_conv1x1_pack_rows(cout, cin) rows of ONE weight and both of its images into host memory and returns their number (< 0: an
 * error code); the caller concatenates the rows of all weights and copies them to the device once.  The launch reads the
 * table and the weights when it RUNS: no host synchronisation, capturable into a hipGraph, replays repack from the live weights.
 * The images are only as current as the last pack launch: whoever changes a weight must pack again before the next _packed call.
 *   oss_conv1x1_fwd_packed / oss_conv1x1_dgrad_packed: oss_conv1x1_fwd / _dgrad with the image of their direction.  The pixel-pair
 *   kernels (even pixel count, 4-byte aligned tensors) and the workgroup-level kernels then fetch their weight fragments from the
 *   image -- same products added in the same order, results bit-identical to the fp32-weight call; the remaining kernel forms
 *   (odd pixel counts, unaligned tensors) read `weight` as before.
 *   oss_ln_conv1x1_fwd_packed (forward image): the same for the LayerNorm-fused forward declared below; shapes and every other
 *   argument as there.  (oss_conv1x1_dgrad_ln_bwd has no packed form: it measured no gain.)
 *   image == NULL or io == OSS_F32 / OSS_F32_BF16X3: exactly the unpacked entry point. */
size_t oss_conv1x1_fwd_image_bytes(int cout, int cin);
size_t oss_conv1x1_dgrad_image_bytes(int cout, int cin);
size_t oss_conv1x1_pack_row_bytes(void);
int oss_conv1x1_pack_rows(int cout, int cin);
int oss_conv1x1_pack_fill(void *rows, const float *weight, void *fwd_image, void *dgrad_image, int cout, int cin);
int oss_conv1x1_pack_weights(oss_dtype io, const void *table, int n_rows, oss_stream_t stream);
int oss_conv1x1_fwd_packed(oss_dtype io, const void *x, const float *weight, const void *fwd_image, const float *bias,
                           const void *residual, void *y, int batch, int cout, int cin, int pixels, int64_t x_batch_stride,
                           int64_t x_channel_stride, oss_stream_t stream);
int oss_conv1x1_dgrad_packed(oss_dtype io, const void *dy, const float *weight, const void *dgrad_image, void *dx, int batch,
                             int cout, int cin, int pixels, int64_t dy_batch_stride, int64_t dy_channel_stride,
                             oss_stream_t stream);
int oss_ln_conv1x1_fwd_packed(oss_dtype io, const void *x, const float *ln_weight, const float *ln_bias, float eps, void *n, float *mean,
                              float *rstd, const float *weight, const void *fwd_image, const float *bias, void *y, int batch, int cout,
                              int cin, int pixels, int64_t x_batch_stride, int64_t x_channel_stride, oss_stream_t stream);
/* Tuning override of oss_conv1x1_wgrad / oss_proj_wgrad: MFMA tiles per wave, 0 = 1 x 1 (default), 12 / 21 / 22 = rows x columns
 * of 32 x 32 tiles (fewer re-reads of the operands, fewer waves).  Same results up to the summation order; the library starts
 * at 0. */
/* Workgroup-level form of oss_conv1x1_fwd / oss_conv1x1_dgrad without residual (oss_conv1x1_wg.hip): cin % 16 == 0, cin <= 192,
 * pixels % 128 == 0, 16-byte aligned tensors; anything else returns OSS_ERR_SHAPE (callers then use the wave-level kernels).
 * transposed_weight = 1: weight is (cin, cout) row-major, i.e. the call is the input gradient of a (cin, cout) convolution. */
int oss_conv1x1_wg(oss_dtype io, const void *x, const float *weight, const float *bias, void *y, int batch, int cout, int cin,
                   int pixels, int64_t x_batch_stride, int64_t x_channel_stride, int transposed_weight, oss_stream_t stream);
/* LayerNorm over channels followed by a 1x1 convolution as ONE launch (norm1 -> in_conv, norm2 -> project_in of the OSS block,
 * MambaSISR6_arch.py:514-516 with :144-195, :205, :281): n = LN(x) (weight, bias or NULL for the BiasFree form, eps), written out
 * together with mean / rstd (batch, pixels) for the backward passes (oss_ln_nchw_bwd, oss_conv1x1_wgrad take them as before), and
 * y = W n + bias.  Shapes of oss_conv1x1_wg: cin % 16 == 0, cin <= 192, pixels % 128 == 0, 16-bit io, 16-byte aligned tensors;
 * oss_ln_conv1x1_ok says whether (io, cout, cin, pixels) qualifies. */
int oss_ln_conv1x1_ok(oss_dtype io, int cout, int cin, int pixels);
int oss_ln_conv1x1_fwd(oss_dtype io, const void *x, const float *ln_weight, const float *ln_bias, float eps, void *n, float *mean,
                       float *rstd, const float *weight, const float *bias, void *y, int batch, int cout, int cin, int pixels,
                       int64_t x_batch_stride, int64_t x_channel_stride, oss_stream_t stream);
/* The backward of that pair's activation path as ONE launch: dn = W^T dy (oss_conv1x1_dgrad) never leaves the CU, the LayerNorm
 * backward (oss_ln_nchw_bwd: x, mean, rstd, + skip_grad, d weight / d bias through `partials` =
 * oss_conv1x1_dgrad_ln_bwd_partial_floats(batch, cin, pixels) floats and the usual (deferred) finishing sum) runs on it in LDS.
 * Shapes: cin <= 128, cout % 16 == 0, 2 cin <= cout <= 192, pixels % 128 == 0 (oss_conv1x1_dgrad_ln_bwd_ok); x, skip_grad, dx contiguous
 * (batch, cin, pixels); dy (batch, cout, pixels) with element strides.  The weight gradient stays oss_conv1x1_wgrad on n. */
int oss_conv1x1_dgrad_ln_bwd_ok(oss_dtype io, int cout, int cin, int pixels, int batch);
size_t oss_conv1x1_dgrad_ln_bwd_partial_floats(int batch, int cin, int pixels);
int oss_conv1x1_dgrad_ln_bwd(oss_dtype io, const void *dy, const float *weight, const void *x, const float *ln_weight, int ln_has_bias,
                             const float *mean, const float *rstd, const void *skip_grad, void *dx, float *dln_weight, float *dln_bias,
                             float *partials, int batch, int cout, int cin, int pixels, int64_t dy_batch_stride,
                             int64_t dy_channel_stride, oss_stream_t stream);
/* A-B switches of the dispatch inside oss_conv1x1_fwd / _dgrad: on = 0 never takes the workgroup-level kernel (the
 * library starts with on = 1); pixels = 64 | 128 forces its tile width, 0 = by grid size (the start value) */
void oss_conv1x1_set_wg(int on, int pixels);
/* What oss_conv1x1_fwd_packed (input_gradient = 0) / oss_conv1x1_dgrad_packed (1) would launch for these arguments and the
 * switches above, without launching it: the plan of csrc/oss_conv1x1_plan.h that the launchers themselves run.  Pure host
 * arithmetic on the shape, the strides, the low 4 address bits of x, weight, image, residual and y and on which of image / bias /
 * residual are NULL; nothing is dereferenced.  x / y are dy / dx of the input gradient, which ignores bias and residual; image ==
 * NULL or fp32 io: the unpacked entry point.  Returns what the entry point would return before its launch (OSS_ERR_*). */
typedef struct {
    int family;        /* kernel: 0 wg (workgroup-level), 1 pair, 2 pairw, 3 pairk, 4 reuse, 5 generic (16-bit io);
                        * 6 f32_tile64, 7 f32_tile32, 8 f32_splitk (fp32 io) */
    int ks, mt;        /* template arguments of the instantiation; 0 where the family has none: k-steps held in registers, row tiles */
    int wt, wvec, res, pf, wimg, pt, x3;   /* pt: pixels per workgroup (wg: the PT argument) */
    int per, nz;       /* 32-row tiles per workgroup; wg: row-tile groups = grid_z */
    int grid_x, grid_y, grid_z, block;
    size_t lds_bytes;  /* dynamic LDS per workgroup */
} oss_conv1x1_launch;
int oss_conv1x1_describe(int input_gradient, oss_dtype io, const void *x, const float *weight, const void *image, const float *bias,
                         const void *residual, const void *y, int batch, int cout, int cin, int pixels, int64_t x_batch_stride,
                         int64_t x_channel_stride, oss_conv1x1_launch *out);
void oss_conv1x1_wgrad_set_tile(int mode);
/* pixels per partial product of the GROUPED weight-gradient launch (oss_flush_wgrads), in units of 512: the library starts at 4;
 * 1 reproduces the one-problem launches bit for bit, larger values write fewer partial vectors */
void oss_conv1x1_wgrad_set_span(int mult);
int oss_conv1x1_wgrad(oss_dtype io, const void *dy, const void *x, float *dweight, float *dbias, float *partials, int batch,
                      int cout, int cin, int pixels, int64_t dy_batch_stride, int64_t dy_channel_stride,
                      int64_t x_batch_stride, int64_t x_channel_stride, oss_stream_t stream);

/* The two in-block projections of the spatial branch (MambaSISR6_arch.py:406-411), omni form, and the
 * flattenings around them.  Layouts (all contiguous, io dtype): x2 (batch, 2, D, L) = the row-major
 * and column-major flattenings of the (batch, D, H, W) activations (k = 0, 1;
 * directions 2, 3 are the same rows walked backwards by the scan); xdbl (batch, 4, C, L) with
 * C = R + 2 dstate rows per direction: R dt rows, then B, then C of the scan; dts (batch, 4, D, L).
 * Weights are float: x_proj_weight (4, C, D), dt_projs_weight (4, D, R).
 *   oss_cross_scan2 : x (batch, D, H, W) of in_type (contiguous planes, element strides batch / channel)
 *                     -> x2 of out_type        (replaces the stack / transpose / flip of :395-404)
 *   oss_cross_merge2: dx (batch, D, H, W) = g2[:, 0] + transpose(g2[:, 1])   (its adjoint)
 *   oss_proj_fwd    : xdbl[b,k,c,:] = sum_d x_proj_weight[k,c,d] x2[b,k%2,d,:], rounded to io;
 *                     dts[b,k,d,:]  = sum_r dt_projs_weight[k,d,r] xdbl[b,k,r,:]
 *   oss_proj_dgrad  : dxdbl holds dB / dC of the scan backward in its rows c >= R on entry; the dt rows
 *                     are filled with dt_projs_weight^T ddts, then
 *                     dx2[b,j] = sum_{k in {j,j+2}} (x_proj_weight[k]^T dxdbl[b,k] + du[b,k]) (du may be NULL)
 *   oss_proj_wgrad  : both weight gradients (float, overwritten) as split-K MFMA products; io =
 *                     OSS_BF16 / OSS_F16 only (OSS_ERR_SHAPE for float: callers use a vendor GEMM);
 *                     partials = oss_proj_wgrad_partial_floats() floats of scratch. */
int oss_cross_scan2(oss_dtype in_type, oss_dtype out_type, const void *x, void *x2, int batch, int D, int height, int width,
                    int64_t x_batch_stride, int64_t x_channel_stride, oss_stream_t stream);
int oss_cross_merge2(oss_dtype io, const void *g2, void *dx, int batch, int D, int height, int width, oss_stream_t stream);
int oss_proj_fwd(oss_dtype io, const void *x2, const float *x_proj_weight, const float *dt_projs_weight, void *xdbl, void *dts,
                 int batch, int D, int C, int R, int seqlen, oss_stream_t stream);
int oss_proj_dgrad(oss_dtype io, const void *ddts, void *dxdbl, const void *du, const float *x_proj_weight,
                   const float *dt_projs_weight, void *dx2, int batch, int D, int C, int R, int seqlen, oss_stream_t stream);
size_t oss_proj_wgrad_partial_floats(int batch, int D, int C, int R, int seqlen);
/* 16-bit I/O runs oss_proj_fwd / _dgrad on the matrix cores (MFMA); float I/O, or force_vector_alu != 0
 * (tests, A-B timing), on the vector-ALU kernels.  Same results up to the summation order. */
void oss_proj_set_path(int force_vector_alu);
/* A-B switch of the dispatch inside oss_proj_fwd: with 16-bit I/O, dts != NULL, R <= 8, D % 16 == 0, D <= 192, seqlen a multiple of
 * the 64- or 128-step tile and 16-byte aligned tensors, x_proj and dt_proj run as ONE launch (oss_proj_fwd_dt_kernel: the dt
 * projection is an epilogue on the tile of xdbl still in LDS) -- bit-identical to the two launches.  on = 0 never takes it (the
 * library starts with on = 1); on = 64 | 128 forces its tile width, 1 = by grid size */
void oss_proj_set_one_launch(int on);
/* 1 when oss_proj_fwd may be called with dts == NULL / oss_proj_dgrad with ddts == NULL at this shape (the matrix-core projection
 * kernels: 16-bit I/O, even seqlen, D <= 768, 2 C <= 256, R <= 32, and the vector-ALU path not forced) -- i.e. when the dt rows of
 * the gradient of x_dbl may come from somewhere else (oss_scan_bwd_params.finish_dt_weight, the fused-delta form) */
int oss_proj_rows_optional_ok(oss_dtype io, int batch, int D, int C, int R, int seqlen);
int oss_proj_wgrad(oss_dtype io, const void *x2, const void *xdbl, const void *dxdbl, const void *ddts, float *dx_proj_weight,
                   float *ddt_projs_weight, float *partials, int batch, int D, int C, int R, int seqlen, oss_stream_t stream);

/* Channel branch of SS2D_1 (MambaSISR6_arch.py:438-483; RealSR form MambaRealSR11_arch.py:758-817) between the
 * pooled descriptor and the gate vector c, one launch per direction of autograd (oss_channel.hip).  All float.
 * L = d_inner (the scan runs over the channels), dc = dc_inner (1 for the RealSR form, then cin_* / cout_* are
 * NULL and seq = pooled), Rc = the channel dt rank, Cc = Rc + 32 (dc_state is 16 in every reference config). */
typedef struct {
    int B, L, dc, Rc, Cc, reserved_;
    const float *pooled;            /* (B, L): mean of y2 over the pixels                                   */
    const float *cin_w, *cin_b;     /* conv_cin (dc) weight / bias, or NULL                                  */
    const float *Wxc;               /* xc_proj_weight (2, Cc, dc)                                            */
    const float *Wdtc;              /* dtc_projs_weight (2, dc, Rc)                                          */
    const float *dt_bias;           /* dtc_projs_bias (2 dc)                                                 */
    const float *A_logs;            /* Ac_logs (2 dc, 16)                                                    */
    const float *Dsc;               /* (2 dc)                                                                */
    const float *cout_w, *cout_b;   /* conv_cout (dc) weight / (1) bias, or NULL                             */
    const float *cn_w, *cn_b;       /* channel_norm weight / bias (L)                                        */
    float *hs;                      /* (B, 2 dc, L, 16) saved: the scan state after every step               */
    float *y;                       /* (B, 2 dc, L)    saved: scan outputs (direction 1 stored un-flipped)   */
    float *yc;                      /* (B, L)          saved: LayerNorm input                                */
    float *stat;                    /* (B, 2)          saved: LayerNorm mean, rstd                           */
    float *c;                       /* (B, L)          OUT: the gate vector                                  */
    /* oss_chan_fwd only.  pool_part != NULL: `pooled` is an OUTPUT -- pooled[b, l] = pool_scale * sum_k pool_part[b, k, l] over the
     * n_part per-workgroup output sums oss_ln_nchw_fwd_pool left (summed in k order) -- instead of an input.                 */
    const float *pool_part;         /* (B, n_part, L) or NULL                                                */
    int n_part;
    float pool_scale;               /* 1 / (H W)                                                             */
} oss_chan_params;
int oss_chan_fwd(const oss_chan_params *p, oss_stream_t stream);
/* gc: gradient of c (B, L).  OUT dpooled (B, L); grads: oss_chan_grad_floats() floats = the parameter gradients
 * summed over the batch in batch order, laid out [cn_w L | cn_b L | cout_w dc | cout_b 1 | Ac_logs 2 dc 16 |
 * Dsc 2 dc | dt_bias 2 dc | Wdtc 2 dc Rc | Wxc 2 Cc dc | cin_w dc | cin_b dc]; scratch:
 * oss_chan_bwd_scratch_floats() floats. */
size_t oss_chan_grad_floats(int L, int dc, int Rc, int Cc);
size_t oss_chan_bwd_scratch_floats(int B, int L, int dc, int Rc, int Cc);
int oss_chan_bwd(const oss_chan_params *p, const float *gc, float *dpooled, float *grads, float *scratch, oss_stream_t stream);
/* out[b, c] = alpha * sum_p a[b, c, p] * (bmul ? bmul[b, c, p] : 1)  (pooling, and the gate's gradient);
 * y[b, c, p] = x[b, c, p] * (mul ? 1 + mul[b, c] : 1) + (add ? alpha * add[b, c] : 0)  (the gate and its adjoint).
 * a, bmul, x: io dtype, contiguous planes, element strides (batch, channel); y contiguous. */
int oss_rowsum(oss_dtype io, const void *a, const void *bmul, float *out, int batch, int channels, int pixels,
               int64_t a_batch_stride, int64_t a_channel_stride, int64_t b_batch_stride, int64_t b_channel_stride, float alpha,
               oss_stream_t stream);
int oss_row_affine(oss_dtype io, const void *x, const float *mul, const float *add, void *y, int batch, int channels,
                   int pixels, int64_t x_batch_stride, int64_t x_channel_stride, float alpha, oss_stream_t stream);

/* Gate of the EFFN (MambaSISR6_arch.py:213-217): h (batch, 2, half_elems) = the two channel halves of
 * dwconv(project_in(x)) (halves contiguous, element batch stride given); out (batch, half_elems) = gelu(h[:, 0]) * h[:, 1]
 * with the exact (erf) gelu; bwd writes the gradient of both halves, dh (batch, 2, half_elems) contiguous. */
int oss_gelu_gate_fwd(oss_dtype io, const void *h, void *out, int batch, size_t half_elems, int64_t h_batch_stride,
                      oss_stream_t stream);
int oss_gelu_gate_bwd(oss_dtype io, const void *h, const void *dout, void *dh, int batch, size_t half_elems,
                      int64_t h_batch_stride, int64_t dout_batch_stride, oss_stream_t stream);

/* Deferred finishing.  Every two-stage reduction of the backward kernels (split-K slabs of oss_conv1x1_wgrad /
 * oss_proj_wgrad, per-workgroup partials of oss_ln_nchw_bwd, oss_dwconv3x3_wgrad, oss_chan_bwd) normally ends with a
 * small finishing launch that adds the partial vectors in a fixed order (~12 such launches per OSS block).  After
 * oss_set_defer_finish(1) those launches are not issued: each call registers its reduction with the library instead
 * (scratch buffers and gradient outputs must then stay alive and unread), and oss_flush_finishes runs ALL of them as
 * one launch: it writes the chunk table (oss_deferred_chunks() entries of sizeof(oss_sum_chunk) bytes, one per <= 1024
 * outputs) into host_table (pinned; must stay alive if the call is captured into a hipGraph), copies it to
 * device_table on the stream and launches the summation there.  Same fixed summation order on every run.
 * oss_set_defer_finish(0/1) also drops whatever was registered and not flushed. */
typedef struct {
    const void *src;   /* partial vector 0 */
    void *dst;         /* output of element j0 */
    int64_t stride;    /* floats between consecutive partial vectors */
    int j0, n, K, reserved_;
} oss_sum_chunk;
void oss_set_defer_finish(int on);
size_t oss_deferred_chunks(void);
int oss_flush_finishes(void *host_table, void *device_table, size_t capacity_chunks, oss_stream_t stream);
/* (round 6) only the FIRST max_chunks registered chunks (registration order = the order of the backward); 0 = all.  The rest stays
 * registered.  With oss_flush_wgrads_n: the gradients of the layers whose backward ran first can be finished -- and handed to the
 * data-parallel all-reduce -- while the remaining groups are still being flushed (vmambair_amd/train_graph.py: grad_buckets). */
int oss_flush_finishes_n(void *host_table, void *device_table, size_t capacity_chunks, size_t max_chunks, oss_stream_t stream);

/* Deferred weight gradients.  After oss_set_defer_wgrad(1), oss_conv1x1_wgrad and the x_proj / dt_proj products of oss_proj_wgrad
 * (16-bit I/O) do not launch: each call records its problem (operands, partial buffer and outputs must stay alive and unread)
 * and -- with oss_set_defer_finish(1) -- its finishing sum; oss_flush_wgrads then runs EVERY recorded product as one grouped
 * launch (the descriptor table, oss_deferred_wgrad_table_bytes() bytes, goes through host_table -- pinned, kept alive when
 * the call is captured into a hipGraph -- to device_table).  Call it before oss_flush_finishes.  With
 * oss_conv1x1_wgrad_set_span(1) the results are bit-identical to the one-launch-per-product form (same tiles, same partial
 * layout, same summation order); the default span (4: a workgroup walks four 512-pixel pieces into one accumulator, a quarter
 * of the partial vectors) changes the order of the fp32 additions -- equal to round-off, bit-identical from run to run.
 * A product recorded while oss_set_defer_finish is off is rejected (OSS_ERR_WORKSPACE): its finishing sum would read partials
 * that do not exist before the flush.
 * oss_set_defer_wgrad(0/1) also drops whatever was recorded and not flushed. */
void oss_set_defer_wgrad(int on);
size_t oss_deferred_wgrads(void);
size_t oss_deferred_wgrad_table_bytes(void);
int oss_flush_wgrads(void *host_table, void *device_table, size_t capacity_bytes, oss_stream_t stream);
/* only the FIRST max_products recorded products (recording order = the order of the backward: last layers first); 0 = all */
int oss_flush_wgrads_n(void *host_table, void *device_table, size_t capacity_bytes, size_t max_products, oss_stream_t stream);

/* Adam + EMA of the training step (MambaSISR_model.py:120-147: torch.optim.Adam without amsgrad / weight decay,
 * then ema = decay * ema + (1 - decay) * param) as one elementwise launch over a chunk table in device memory:
 * one entry per <= OSS_ADAM_CHUNK consecutive elements of one parameter tensor (all float; ema may be NULL).
 * state: 4 floats in device memory {step count, 1 - beta1^t, 1 - beta2^t, learning rate} (the fourth is read only with
 * lr < 0; a caller that always passes lr >= 0 may hand over 3); the call advances the step
 * count first (so the launch pair can be replayed inside a hipGraph).  lr >= 0: the learning rate of this call (baked into
 * a captured launch); lr < 0: the kernel reads state[3], which the host may rewrite between replays -- the reference
 * trainings change the rate during a run (MultiStepLR, SRGAN/options/MambaSISR15_x4.yml:84-87;
 * CosineAnnealingRestartCyclicLR every iteration, Deraining/Deraining/Options/Deraining_mamber33.yml:81-85). */
#define OSS_ADAM_CHUNK 2048
typedef struct {
    void *param;
    const void *grad;
    void *exp_avg, *exp_avg_sq, *ema;
    int n, reserved_;
} oss_adam_chunk;
int oss_adam_ema_step(const oss_adam_chunk *chunks, int n_chunks, float *state, float lr, float beta1, float beta2, float eps,
                      float ema_decay, oss_stream_t stream);
/* The Deraining tree's step (Deraining/basicsr/models/image_restoration_model.py:121-167): torch.optim.AdamW (decoupled
 * decay: param *= 1 - lr * weight_decay before the Adam update) after clip_grad_norm_(params, 0.01).  grad_scale (device
 * memory, one float, or NULL) multiplies every gradient inside the launch: the caller computes
 * min(1, max_norm / (total_norm + 1e-6)) on the device, so nothing is read back and the step stays graph-capturable.
 * ema_decay as above (entries with ema == NULL skip it: the Deraining YAML sets no EMA). */
int oss_adamw_ema_step(const oss_adam_chunk *chunks, int n_chunks, float *state, float lr, float beta1, float beta2, float eps,
                       float weight_decay, float ema_decay, const float *grad_scale, oss_stream_t stream);

/* Cross-merge of the four spatial directions (MambaSISR6_arch.py:427-430) on the omni scan's
 * un-flipped outputs: out (batch, 4, D, H*W) io dtype contiguous (directions 0/2 row-major, 1/3
 * column-major) -> y (batch, D, H, W) float = ((o0 + o2) + T o1) + T o3, the reference's association
 * order.  batch * D must be < 65536. */
int oss_merge4(oss_dtype io, const void *out, float *y, int batch, int D, int height, int width, oss_stream_t stream);

/* Per-pixel LayerNorm over the channel axis, NCHW in / NCHW out (LayerNorm of the OSS block,
 * SRGAN/VmambaIR/archs/MambaSISR6_arch.py:144-195: biased variance, eps inside the sqrt; bias == NULL
 * selects the BiasFree form x / sqrt(var + eps) * w).  x: (batch, C, pixels) of type x_type with element
 * strides (batch, channel), pixels contiguous; y (and dgate) contiguous (batch, C, pixels) of y_type;
 * gate of y_type with its own (batch, channel) strides; weight / bias / dweight / dbias float (C).
 * gate != NULL fuses y = LN(x) * silu(gate)
 * (SS2D_1: y1 * act(z), :488-493).  mean / rstd: (batch, pixels) float, written by fwd, read by bwd.
 * bwd: partials = oss_ln_nchw_bwd_partial_floats(batch, channels, pixels) floats of scratch
 * (per-workgroup dweight / dbias sums, combined in a fixed order by a finishing kernel).  skip_grad (x_type,
 * contiguous like dx, or NULL) is added to dx: the gradient arriving over the block's skip connection.
 * dgate_batch_stride: element stride between the images of dgate (0 = channels * pixels): SS2D_1 splits one tensor into x | z
 * (MambaSISR6_arch.py:487), and the gradient of the gate z is written straight into its half of that tensor's gradient. */
size_t oss_ln_nchw_bwd_partial_floats(int batch, int channels, int pixels);
int oss_ln_nchw_fwd(oss_dtype x_type, oss_dtype y_type, const void *x, const float *weight, const float *bias,
                    const void *gate, void *y, float *mean, float *rstd, int batch, int channels, int pixels,
                    int64_t x_batch_stride, int64_t x_channel_stride, int64_t gate_batch_stride,
                    int64_t gate_channel_stride, float eps, oss_stream_t stream);
/* oss_ln_nchw_fwd that also leaves, per workgroup of 128 pixels and channel, the sum of its OUTPUT values (as stored) in pool_part
 * (batch, oss_ln_nchw_fwd_pool_tiles(...), channels): the pooled descriptor of SS2D_1's channel branch without a pass over y
 * (oss_chan_params.pool_part).  _pool_tiles returns 0 for shapes that do not take the 128-pixel form (odd pixels / strides). */
int oss_ln_nchw_fwd_pool_tiles(int channels, int pixels, int64_t x_batch_stride, int64_t x_channel_stride, int64_t gate_batch_stride,
                               int64_t gate_channel_stride);
int oss_ln_nchw_fwd_pool(oss_dtype x_type, oss_dtype y_type, const void *x, const float *weight, const float *bias,
                         const void *gate, void *y, float *mean, float *rstd, float *pool_part, int batch, int channels, int pixels,
                         int64_t x_batch_stride, int64_t x_channel_stride, int64_t gate_batch_stride,
                         int64_t gate_channel_stride, float eps, oss_stream_t stream);
int oss_ln_nchw_bwd(oss_dtype x_type, oss_dtype y_type, const void *x, const float *weight, const float *bias,
                    const void *gate, const void *dy, const float *mean, const float *rstd, void *dx, void *dgate,
                    float *dweight, float *dbias, float *partials, const void *skip_grad, int batch, int channels, int pixels,
                    int64_t x_batch_stride, int64_t x_channel_stride, int64_t gate_batch_stride,
                    int64_t gate_channel_stride, int64_t dgate_batch_stride, oss_stream_t stream);
/* The same with the incoming gradient taken as dy * (1 + dy_mul[b, c]) + add_scale * dy_add[b, c] (both (batch, channels) float;
 * dy_mul NULL: no factor): the backward of SS2D_1's channel gate  out = y2 * c + y2 | y2 + c,  c = f(mean_hw(y2))
 * (MambaSISR6_arch.py:495-496) is  d y2 = g * (1 + c) | g  +  d pooled / (H W), an affine map per (image, channel) of the gradient g
 * that reaches `out` -- applied here on load instead of in a pass of its own (oss_row_affine) that writes d y2 only for this
 * kernel to read it back. */
int oss_ln_nchw_bwd_affine(oss_dtype x_type, oss_dtype y_type, const void *x, const float *weight, const float *bias,
                           const void *gate, const void *dy, const float *dy_mul, const float *dy_add, float add_scale,
                           const float *mean, const float *rstd, void *dx, void *dgate, float *dweight, float *dbias, float *partials,
                           const void *skip_grad, int batch, int channels, int pixels, int64_t x_batch_stride,
                           int64_t x_channel_stride, int64_t gate_batch_stride, int64_t gate_channel_stride,
                           int64_t dgate_batch_stride, oss_stream_t stream);

/* Optional per-launch timing of the two scan kernels (bench.py's roofline leg): when enabled every
 * main forward / backward kernel launch is bracketed by HIP events recorded on the launch stream.
 * oss_prof_collect synchronises those events and returns, for one bucket (which: 0 = forward
 * kernel, 1 = backward main kernel, 2 = backward finishing kernel; variant; io dtype), the summed kernel time, the number of launches
 * and the summed ALGORITHMIC bytes (SURVEY.md section 8d formulas).
 * Returns 0, or OSS_ERR_SHAPE for a bucket out of range. */
void oss_prof_enable(int on);
void oss_prof_reset(void);
/* variant 16 + v: the time-segmented launches of kernel variant v (carry / local pass included in the call's time) */
int oss_prof_collect(int which, int variant, oss_dtype io, double *total_ms, long long *launches,
                     double *algorithmic_bytes);
/* ... plus the kernel's OWN algorithmic bytes (tensors the omni form shares between directions counted once); which = 2
 * selects the backward's finishing kernel (time only). */
int oss_prof_collect2(int which, int variant, oss_dtype io, double *total_ms, long long *launches, double *algorithmic_bytes,
                      double *own_bytes);

/* HBM copy-kernel (float4 read+write) used by bench.py to measure the achievable bandwidth in
 * the same run as the scan kernels; copies n_bytes (multiple of 16) from src to dst. */
int oss_hbm_copy(const void *src, void *dst, size_t n_bytes, oss_stream_t stream);

/* Launches an empty kernel named oss_prof_marker_begin (which = 1) / oss_prof_marker_end (2) on `stream`: bench.py brackets
 * its timed region with them so that tools/prof_summary.py can cut a rocprofv3 kernel trace down to the steady-state
 * replays (no warm-up, capture or vendor solver search). */
int oss_prof_marker(int which, oss_stream_t stream);

/* Hash of the sources the scan kernels are compiled from (oss_scan_*.hip/.h, oss_device.h), fixed at build time.  PMC
 * counter records under profiles/ carry the id of the build they were measured on; bench.py reports counters only when it
 * matches the loaded library ("stale" otherwise). */
const char *oss_scan_build_id(void);

const char *oss_version(void);

/* Dense 3x3 convolutions (stride 1, zero padding 1, NCHW) with a THIN side -- at most 4 channels in or out: the layers the UNets
 * open and close with (OverlapPatchEmbed conv(3 -> 48), SRGAN/VmambaIR/archs/MambaSISR6_arch.py:520-528; the x4 tail's last
 * conv(96 -> 3) at the output resolution, archs/common.py:45-60; Mamber32.output, Deraining/basicsr/models/archs/
 * mamber32_arch.py:608).  HBM-bound stencils, not GEMMs: 16-bit I/O, fp32 master weights (cout, cin, 3, 3) and bias, fp32
 * accumulation, 8 pixels per lane.  oss_conv3x3_thin_ok says whether a shape qualifies (bf16 / fp16, width % 8 == 0,
 * min(cin, cout) <= 4); pointers 16-byte aligned, plane strides (elements) multiples of 8, planes contiguous.
 *   fwd:   y = conv(x) + bias
 *   dgrad: dx = the transposed convolution of dy
 *   wgrad: dweight (cout, cin, 3, 3) and -- cout <= 4 only -- dbias, through `partial`
 *          (oss_conv3x3_thin_wgrad_partial_floats floats, no init): one partial vector per image, added in batch order by the
 *          deferred finishing launch (oss_set_defer_finish) or right away. */
int oss_conv3x3_thin_ok(oss_dtype io, int cin, int cout, int height, int width);
int oss_conv3x3_thin_fwd(oss_dtype io, const void *x, const float *weight, const float *bias, void *y, int batch, int cin, int cout,
                         int height, int width, int64_t x_batch_stride, int64_t x_channel_stride, int64_t y_batch_stride,
                         int64_t y_channel_stride, oss_stream_t stream);
int oss_conv3x3_thin_dgrad(oss_dtype io, const void *dy, const float *weight, void *dx, int batch, int cin, int cout, int height,
                           int width, int64_t dy_batch_stride, int64_t dy_channel_stride, int64_t dx_batch_stride,
                           int64_t dx_channel_stride, oss_stream_t stream);
size_t oss_conv3x3_thin_wgrad_partial_floats(int batch, int cin, int cout);
int oss_conv3x3_thin_wgrad(oss_dtype io, const void *x, const void *dy, float *dweight, float *dbias, float *partial, int batch, int cin,
                           int cout, int height, int width, int64_t x_batch_stride, int64_t x_channel_stride, int64_t dy_batch_stride,
                           int64_t dy_channel_stride, oss_stream_t stream);

/* The GEMM-shaped dense 3x3 convolutions (stride 1, zero padding 1, NCHW) of the UNet skeleton on the matrix cores: Downsample
 * conv(n -> n/2), Upsample conv(n -> 2n) and the x4 tail's two conv(n -> 4n) (vmambair_amd/archs.py).  16-bit I/O, fp32 master
 * weights (cout, cin, 3, 3) and bias narrowed to the I/O type where they are loaded, fp32 accumulation, one rounding after the bias.
 * oss_conv3x3_dense_ok is a pure host query: 1 for bf16 / fp16, cin % 16 == 0 (16 .. 16384), 5 <= cout <= 16384 and
 * 1 <= height, width <= 32768 (odd widths included), else 0; a call on an accepted shape with 1 <= batch <= 65535 never fails to
 * launch, anything else returns OSS_ERR_SHAPE.  Batch and channel strides (elements) are free, planes are contiguous.  With 16-byte
 * aligned pointers, strides that are multiples of 8 and width % 8 == 0 the loaders use 16-byte accesses, element-wise ones otherwise.
 *   fwd:   y = conv(x) + bias
 *   dgrad: dx = the transposed convolution of dy (the forward kernel with the weights read transposed and mirrored)
 *   wgrad: dweight (cout, cin, 3, 3) through `partial` (oss_conv3x3_dense_wgrad_partial_floats floats, no init): one partial vector of
 *          9 cin cout floats per (image, row band) -- at most batch * height vectors, about 512 workgroups' worth for large planes --
 *          added in that order by the deferred finishing launch (oss_set_defer_finish) or right away.  With dbias != NULL also
 *          dbias = sum dy, by a launch of its own that sums in fp64 and rounds once.  No atomics: reruns are bit-identical. */
int oss_conv3x3_dense_ok(oss_dtype io, int cin, int cout, int height, int width);
int oss_conv3x3_dense_fwd(oss_dtype io, const void *x, const float *weight, const float *bias, void *y, int batch, int cin, int cout,
                          int height, int width, int64_t x_batch_stride, int64_t x_channel_stride, int64_t y_batch_stride,
                          int64_t y_channel_stride, oss_stream_t stream);
int oss_conv3x3_dense_dgrad(oss_dtype io, const void *dy, const float *weight, void *dx, int batch, int cin, int cout, int height,
                            int width, int64_t dy_batch_stride, int64_t dy_channel_stride, int64_t dx_batch_stride,
                            int64_t dx_channel_stride, oss_stream_t stream);
size_t oss_conv3x3_dense_wgrad_partial_floats(int batch, int cin, int cout, int height, int width);
int oss_conv3x3_dense_wgrad(oss_dtype io, const void *x, const void *dy, float *dweight, float *dbias, float *partial, int batch, int cin,
                            int cout, int height, int width, int64_t x_batch_stride, int64_t x_channel_stride, int64_t dy_batch_stride,
                            int64_t dy_channel_stride, oss_stream_t stream);

/* The reference's validation metrics of a batch of image pairs, on the device, in one call: the mean squared error behind
 * calculate_psnr (Deraining/basicsr/metrics/psnr_ssim.py:9-63) and the mean SSIM of _ssim (psnr_ssim.py:66-99; Deraining/Deraining/
 * utils.py:31-78) or _ssim_cly (psnr_ssim.py:184-222), with 11 x 11 Gaussian window (sigma 1.5), C1 = (0.01 * 255)^2,
 * C2 = (0.03 * 255)^2, all moments and the quotient in fp64.
 *   a, b      (batch, channels, height, width), channels 1 or 3 in R, G, B order, element strides for batch / channel / row, column
 *             stride 1 (cropped views need no copy); io = fp32 / fp16 / bf16
 *   out       (batch, 2) doubles: mean squared error over the cropped planes, mean SSIM.  PSNR = 10 log10(255^2 / mse)
 *   partials  oss_image_metrics_partial_doubles(...) doubles of scratch, no init: one (squared error, SSIM sum) pair per workgroup,
 *             added in a fixed order by a second small launch of the same call -- no atomics, reruns are bit-identical, no host
 *             read-back, capturable into a hipGraph
 *   crop_border pixels are dropped on every side first (psnr_ssim.py:46-48, :276-278)
 *   flags     OSS_METRIC_QUANTISE   the values are network outputs in [0, 1]: clamp, * 255, round half to even on load, in fp32
 *                                   (tensor2img, SRGAN/VmambaIR/utils/img_util.py:68-92); clear: already in [0, 255] units
 *             OSS_METRIC_Y          channels == 3 only: both metrics on the BT.601 luma of to_y_channel (metrics/metric_util.py:
 *                                   34-47, utils/matlab_functions.py:207-238): / 255 in fp32, dot product in fp64, + 16, / 255, cast
 *                                   to fp32, * 255; the squared difference is then taken in fp32 and summed in fp64 as
 *                                   calculate_psnr does.  Clear with 3 channels: the mean over the three per-channel SSIMs
 *                                   (utils.calculate_ssim:46-51) and the squared error over all three
 *             OSS_METRIC_REPLICATE  every cropped pixel is a window centre, neighbours outside the cropped plane are clamped to its
 *                                   edge (_ssim_cly, cv2.BORDER_REPLICATE); clear: only the (height' - 10)(width' - 10) windows
 *                                   inside the cropped plane (_ssim), which needs height', width' >= 11
 * oss_image_metrics_ok is a pure host query: 1 when the shape and flags are taken.  OSS_ERR_NULL for a NULL pointer, OSS_ERR_SHAPE
 * for channels not in {1, 3}, Y with one channel, crop_border >= half a side, valid mode on a cropped plane under 11 pixels, or a
 * launch grid beyond the device limits (batch * planes > 65535, height' > 16 * 65535). */
#define OSS_METRIC_QUANTISE 1
#define OSS_METRIC_Y 2
#define OSS_METRIC_REPLICATE 4
int oss_image_metrics_ok(oss_dtype io, int channels, int height, int width, int crop_border, int flags);
size_t oss_image_metrics_partial_doubles(int batch, int channels, int height, int width, int crop_border);
int oss_image_metrics(oss_dtype io, const void *a, const void *b, double *out, double *partials, int batch, int channels,
                      int height, int width, int64_t a_batch_stride, int64_t a_channel_stride, int64_t a_row_stride,
                      int64_t b_batch_stride, int64_t b_channel_stride, int64_t b_row_stride, int crop_border, int flags,
                      oss_stream_t stream);

/* The features of the reference's NIQE, the no-reference quality metric (Deraining/basicsr/metrics/niqe.py:10-140), of a batch of
 * images on the device, in one launch (oss_niqe.hip): the plane is cropped to whole 96 x 96 blocks from the top-left and every
 * block gives 18 features at scale 1 and 18 at scale 2 (the plane halved by 2 x 2 means, blocks of 48 x 48) -- per scale an AGGD
 * fit of the block of the MSCN map (7 x 7 window, 'nearest' border) and of its product with the block rolled by [0, 1], [1, 0],
 * [1, 1], [1, -1] inside itself.  The multivariate-Gaussian distance of niqe.py:142-155 is left to the host (36 x 36, per image).
 *   a         (batch, channels, height, width), channels 1 or 3 in R, G, B order, element strides for batch / channel / row, column
 *             stride 1 (cropped views need no copy); io = fp32 / fp16 / bf16
 *   tables    (4, OSS_NIQE_GRID) doubles in DEVICE memory on the grid gam = arange(0.2, 10.001, 0.001) of estimate_aggd_param: gam,
 *             r_gam = G(2/gam)^2 / (G(1/gam) G(3/gam)) (increasing), sqrt(G(1/gam) / G(3/gam)), G(2/gam) / G(1/gam).  The caller
 *             computes them once in double; no gamma function is evaluated on the device
 *   window    the 7 x 7 window of the pristine model, 49 doubles in HOST memory, row-major, as scipy.ndimage.convolve receives it
 *             (the launcher flips it); read before the call returns
 *   out       (batch, blocks, OSS_NIQE_FEATURES) doubles, blocks = (height' / 96) * (width' / 96) in the reference's order
 *             (block column outer, block row inner); features 0-17 scale 1, 18-35 scale 2: alpha, (beta_l + beta_r) / 2, then
 *             four times alpha, mean, beta_l, beta_r.  A block whose MSCN values are all zero has alpha 0.2 and NaN elsewhere,
 *             as in the reference (argmin of an all-NaN array)
 *   crop_border pixels are dropped on every side first (niqe.py:200-201)
 *   flags     OSS_METRIC_QUANTISE, OSS_METRIC_Y as for oss_image_metrics; the metric is defined on ONE plane, so three channels
 *             need OSS_METRIC_Y and one channel must not set it
 * Dtypes follow the reference: fp32 planes, every window sum 49 products and additions in fp64 rounded once to fp32, the other
 * steps up to the MSCN map and the products single correctly rounded fp32 operations, the moments fp64 sums of those fp32 values
 * in a fixed order (the reference sums them in fp32: its features are 1e-7 away).  No atomics, no scratch: reruns are
 * bit-identical, an image's result does not depend on the batch, no host read-back, capturable into a hipGraph.
 * oss_niqe_features_ok is a pure host query: 1 when the element type, shape and flags are taken.  OSS_ERR_NULL for a NULL pointer,
 * OSS_ERR_SHAPE for io no element type, channels not in {1, 3}, OSS_METRIC_Y that does not go with the channels, an unknown flag, a
 * cropped plane under 96 pixels on a side, or a launch grid beyond the device limits (batch > 65535, blocks > 2^31 - 1). */
#define OSS_NIQE_BLOCK 96
#define OSS_NIQE_FEATURES 36
#define OSS_NIQE_GRID 9801
int oss_niqe_features_ok(int channels, int height, int width, int crop_border, int flags, oss_dtype io);
int oss_niqe_features(oss_dtype io, const void *a, const double *tables, const double *window, double *out, int batch, int channels,
                      int height, int width, int64_t a_batch_stride, int64_t a_channel_stride, int64_t a_row_stride, int crop_border,
                      int flags, oss_stream_t stream);

/* The two custom operators of the RealSR degradation pipeline on the device (oss_degrade.hip; MambaRealSR.feed_data,
 * RealSR/VmambaIR/models/MambaRealSR_model.py:146-263): filter2D and USMSharp of the basicsr package.  All tensors are dense fp32
 * (batch, channels, H, W), sums are fp32; out must not overlap img.  An axis of n elements is padded by k / 2 with torch's 'reflect'
 * rule inside the load (index -v for v < 0, 2n - 2 - v from n on); no padded copy exists.
 *   oss_filter2d    out[b,c,y,x] = sum_ij kernel[b or 0][i][j] * pad[b,c,y+i,x+j]: cross-correlation, no flip.  kernel is
 *                   (kernels, k, k) with kernels == 1 (shared) or == batch (one per sample, shared by its channels), k odd <= 21.
 *                   A workgroup finds the non-zero bounding box of its kernel on the device and leaves the zero taps out, which
 *                   changes nothing for finite input.  epilogue: OSS_FILTER_NONE; OSS_FILTER_CLAMP = clamp to [0, 1];
 *                   OSS_FILTER_QUANTISE = clamp(rint(x * 255), 0, 255) / 255 with round-half-even and the division as torch
 *                   evaluates it on the device, q * fp32(1 / 255), so that it equals torch's expression there bit for bit.  One launch.
 *   oss_filter_sep  the same correlation with the rank-1 kernel g g^T of one odd vector g (k <= 63): a row pass into scratch
 *                   (oss_filter_sep_scratch_floats floats), a column pass into out.  Two launches.
 *   oss_usm_sharp   blur = filter_sep(img); residual = img - blur; mask = (|residual| * 255 > threshold) as 0 / 1;
 *                   soft = filter_sep(mask); sharp = clip(img + weight * residual, 0, 1); out = img + soft * (sharp - img), which is
 *                   soft * sharp + (1 - soft) * img and returns img itself where weight == 0 or the mask is empty.  Four launches;
 *                   mask (may be NULL) receives the 0 / 1 mask; scratch: oss_usm_scratch_floats floats, no init.
 * Nothing is allocated or read back: every call can be captured into a hipGraph.  The three size queries are pure host calls and
 * the support queries: 0 when the shape is not taken -- k even, k < 1 or above the limit, H <= k / 2 or W <= k / 2 (one
 * reflection is then not enough), a dimension < 1 or above 2^24, kernels neither 1 nor batch, more than 2^31 - 1 workgroups.
 * The entry points return OSS_ERR_SHAPE for the same and for an unknown epilogue, OSS_ERR_NULL for a missing pointer, without a
 * launch. */
#define OSS_FILTER_NONE 0
#define OSS_FILTER_CLAMP 1
#define OSS_FILTER_QUANTISE 2
#define OSS_FILTER2D_MAX_K 21
#define OSS_FILTER_SEP_MAX_K 63
size_t oss_filter2d_workgroups(int64_t batch, int64_t channels, int64_t h, int64_t w, int k, int64_t kernels);
int oss_filter2d(const float *img, const float *kernel, float *out, int64_t batch, int64_t channels, int64_t h, int64_t w, int k,
                 int64_t kernels, int epilogue, oss_stream_t stream);
size_t oss_filter_sep_scratch_floats(int64_t batch, int64_t channels, int64_t h, int64_t w, int k);
int oss_filter_sep(const float *img, const float *g, float *out, float *scratch, int64_t batch, int64_t channels, int64_t h,
                   int64_t w, int k, oss_stream_t stream);
size_t oss_usm_scratch_floats(int64_t batch, int64_t channels, int64_t h, int64_t w, int k);
int oss_usm_sharp(const float *img, const float *g, float *out, float *mask, float *scratch, int64_t batch, int64_t channels,
                  int64_t h, int64_t w, int k, float weight, float threshold, oss_stream_t stream);

/* DiffJPEG, the JPEG step of the same pipeline (oss_jpeg.hip; MambaRealSR_model.py:189-191, :234-241; basicsr.utils.diffjpeg), as
 * one launch: img (batch, 3, h, w) dense fp32 in [0, 1] -> out of the same shape, which must not overlap img.
 *   factor     per sample: (q < 50 ? 5000 / q : 200 - 2 q) / 100 in fp32.  quality != NULL: q = quality[b], batch fp32 values in
 *              DEVICE memory that the kernel reads (no host read, so a captured launch follows later writes to them);
 *              quality == NULL: q = quality_scalar for every sample, converted on the host.  q = 100 gives factor 0 and NaN output,
 *              as in the package.
 *   compress   zero padding at the bottom and right to H, W = multiples of 16 (inside the load); p = 255 x; Y, Cb, Cr with the
 *              package's fp32 matrix; Cb, Cr averaged over 2 x 2; per 8 x 8 block F = DCT-II(block - 128), orthonormal;
 *              c = rint(F / (T * factor)) with round-half-even, T = the luminance table transposed / the chrominance table
 *   decompress c * (T * factor), inverse DCT, + 128, Cb and Cr replicated 2 x 2, the package's inverse matrix, clamp to [0, 255],
 *              * fp32(1 / 255) (torch's division of a device tensor by 255), cropped to h x w by guarded stores
 *   flags      OSS_JPEG_CLAMP_INPUT: x is clamped to [0, 1] first (:190, :235, :240); OSS_JPEG_QUANTISE: the epilogue
 *              clamp(rint(x * 255), 0, 255) / 255 of :248, with the bits of OSS_FILTER_QUANTISE; OSS_JPEG_DIFF_ROUND:
 *              c = rint(v) + (v - rint(v))^3, the package's differentiable rounding (the forward value only: no backward exists)
 *   coef_y, coef_cb, coef_cr   each may be NULL (nothing is written): the quantised coefficients c as fp32 in the layout of
 *              basicsr's CompressJpeg, (batch, H W / 64, 8, 8) and twice (batch, H W / 256, 8, 8), blocks row-major over the
 *              padded plane, [u][v] = [vertical][horizontal] frequency
 * Nothing is allocated or read back.  oss_jpeg_workgroups is a pure host call and the support query: 0 for a dimension < 1 or
 * above 2^24 or more than 2^31 - 1 macroblocks (16 x 16).  oss_jpeg_roundtrip returns OSS_ERR_SHAPE for the same and for an unknown
 * flag, OSS_ERR_NULL when img or out is missing, without a launch. */
#define OSS_JPEG_CLAMP_INPUT 1
#define OSS_JPEG_QUANTISE 2
#define OSS_JPEG_DIFF_ROUND 4
size_t oss_jpeg_workgroups(int64_t batch, int64_t h, int64_t w);
int oss_jpeg_roundtrip(const float *img, const float *quality, float quality_scalar, float *out, float *coef_y, float *coef_cb,
                       float *coef_cr, int64_t batch, int64_t h, int64_t w, int flags, oss_stream_t stream);

/* The two noise steps of the same pipeline (oss_noise.hip; MambaRealSR_model.py:177-187, :209-219; basicsr.data.degradations:
 * generate_ / add_ / random_generate_ / random_add_ gaussian_noise_pt and poisson_noise_pt), without a host read.  img, out: dense
 * fp32 (batch, channels, h, w); out must not be img.  Per element, in fp32 and in the package's operation order:
 *   Gaussian  noise = (n_c * sigma_b / 255) * (1 - g_b) + (n_g[y, x] * sigma_b / 255) * g_b, n_c standard normal per element, n_g ONE
 *             (h, w) standard normal field shared by all samples and channels, as in the package
 *   Poisson   (channels == 3) q = clamp(rint(255 x), 0, 255) / 255; vals_b = the next power of two >= the number of distinct levels
 *             255 q in sample b over all channels; noise = poisson(q * vals_b) / vals_b - q; the grey field of a sample likewise from
 *             g = clamp(rint(255 (0.2989 R + 0.587 G + 0.114 B)), 0, 255) / 255 and its own vals, one count per pixel shared by
 *             the three channels; noise = (noise * (1 - g_b) + noise_grey * g_b) * scale_b
 *   out = epilogue(img + noise), or epilogue(noise) with OSS_NOISE_ONLY (generate_*; img may then be NULL for Gaussian)
 *   sigma_b / scale_b, g_b   sigma[b] / scale[b] and gray[b] from (batch,) fp32 arrays in DEVICE memory; a NULL array stands for the
 *             scalar sigma_lo / scale_lo resp. gray_scalar.  OSS_NOISE_DRAW_PARAMS (random_*): both are drawn by the kernel,
 *             sigma_b = u (hi - lo) + lo and g_b = (u' < gray_scalar) with u, u' uniform in [0, 1) with 24 bits; the arrays are not read.
 *             The grey term is always evaluated and mixed with its weight (the package skips it after a host read when all g_b
 *             are 0: the same value).
 *   epilogue  OSS_NOISE_CLIP: clamp to [0, 1]; OSS_NOISE_ROUNDS: rint(x * 255) / 255; both: clamp(rint(x * 255), 0, 255) / 255;
 *             OSS_NOISE_QUANTISE: then clamp(rint(x * 255), 0, 255) / 255 with the bits of OSS_FILTER_QUANTISE (/ 255 as torch
 *             evaluates it on the device)
 *   params    may be NULL; else fp32, (2, batch) for Gaussian: sigma_b, g_b as used; (4, batch) for Poisson: scale_b, g_b, vals_b of
 *             the colour levels, vals_b of the grey levels
 *   OSS_NOISE_RAW   the samplers alone.  Gaussian: out = n_c (img unused, may be NULL).  Poisson: img holds lambda (clamped to
 *             256) per element, out receives the count drawn with that element's colour draws; any channels, no scratch.
 *             gray_scalar > 0 selects the grey draws instead: n_g[y, x] of every element, resp. the counts with the grey tag and
 *             element = flat index (the grey counts of a (batch, 3, h, w) call when img is its (batch, 1, h, w) lambda field).
 * Random stream: every word is a word of Philox4x32-10 with key (seed lo, seed hi) and counter (element lo, element hi [8 bits] | call
 * hi << 8, tag << 24 | draw, call lo); tags 0x63 colour, 0x67 grey, 0x70 parameters (element = b, words 0 and 1).  Gaussian: element
 * = flat index / 4 (colour) or (y w + x) / 4 (grey, no sample index), draw 0, the normals of the 4 elements by Box-Muller on the word
 * pairs (0, 1) and (2, 3): u1 = (word + 1/2) 2^-32, r = sqrt(-2 ln u1) (ln u1 as log1p(-(~word + 1/2) 2^-32) for word >= 2^31),
 * theta = 2 pi word' 2^-32, (r cos theta, r sin theta).
 * Poisson: element = flat index (colour) or b h w + pixel (grey); lambda < OSS_NOISE_POISSON_SWITCH: inversion by sequential search in
 * fp64 from u = (word 0 of draw 0 + 1/2) 2^-32, at most OSS_NOISE_INVERSION_MAX steps; else PTRS (Hoermann 1993), round i with
 * the words 2 (i & 1), 2 (i & 1) + 1 of draw i / 2 as ((word >> 9) + 1/2) 2^-23, at most OSS_NOISE_PTRS_MAX_ROUNDS rounds (then
 * floor(lambda): probability below 1e-13).
 *   state     two int64 in DEVICE memory: seed, call.  The kernels read both; a one-thread launch after the sampling launch stores
 *             call + 1, so the next call -- or the next replay of a captured one -- draws other fields.  One call consumes one value.
 *   scratch   Poisson without OSS_NOISE_RAW: oss_noise_scratch_words(batch) = 16 batch uint32 words, zeroed by the entry point on
 *             the stream: per sample the 256-bit set of colour levels and the 256-bit set of grey levels, filled by a census launch.
 * Launches: Gaussian sampling + advance; Poisson memset + census + sampling + advance.  Nothing is allocated or read back.
 * oss_noise_workgroups(kind: 0 Gaussian, 1 Poisson, ...) is a pure host call and the support query: the sampling launch's
 * workgroups, 0 when refused -- an unknown kind or flag, a dimension < 1 or above 2^24, 2^40 or more elements, more than 2^31 - 1
 * workgroups, and for Poisson without OSS_NOISE_RAW channels != 3 or batch > 65535.  The entry points return OSS_ERR_SHAPE for the
 * same and for out == img, OSS_ERR_NULL for a missing out, state, scratch (where needed) or img (where needed), without a launch.
 * The *_host twins evaluate the same per-element text on the CPU with all pointers in HOST memory and (key, counter) = (seed, call)
 * as plain numbers; they advance nothing.  oss_noise_normals_host applies the normal transform alone to `blocks` groups of four GIVEN
 * words (host memory) -> four fp32 normals each, for the words no seed is known to produce (all-zero, all-one bits). */
#define OSS_NOISE_DRAW_PARAMS 1
#define OSS_NOISE_CLIP 2
#define OSS_NOISE_ROUNDS 4
#define OSS_NOISE_QUANTISE 8
#define OSS_NOISE_RAW 16
#define OSS_NOISE_ONLY 32
#define OSS_NOISE_POISSON_SWITCH 10
#define OSS_NOISE_INVERSION_MAX 64
#define OSS_NOISE_PTRS_MAX_ROUNDS 16
size_t oss_noise_workgroups(int kind, int64_t batch, int64_t channels, int64_t h, int64_t w, int flags);
size_t oss_noise_scratch_words(int64_t batch);
int oss_noise_gaussian(const float *img, float *out, int64_t *state, const float *sigma, const float *gray, float sigma_lo,
                       float sigma_hi, float gray_scalar, float *params, int64_t batch, int64_t channels, int64_t h, int64_t w,
                       int flags, oss_stream_t stream);
int oss_noise_poisson(const float *img, float *out, int64_t *state, const float *scale, const float *gray, float scale_lo,
                      float scale_hi, float gray_scalar, float *params, uint32_t *scratch, int64_t batch, int64_t channels, int64_t h,
                      int64_t w, int flags, oss_stream_t stream);
int oss_noise_normals_host(const uint32_t *words, float *out, int64_t blocks);
int oss_noise_gaussian_host(const float *img, float *out, int64_t key, int64_t counter, const float *sigma, const float *gray,
                            float sigma_lo, float sigma_hi, float gray_scalar, float *params, int64_t batch, int64_t channels,
                            int64_t h, int64_t w, int flags);
int oss_noise_poisson_host(const float *img, float *out, int64_t key, int64_t counter, const float *scale, const float *gray,
                           float scale_lo, float scale_hi, float gray_scalar, float *params, uint32_t *scratch, int64_t batch,
                           int64_t channels, int64_t h, int64_t w, int flags);

/* The reference's pixel losses with their gradients on the device (oss_pixel_loss.hip): L1Loss, MSELoss, PSNRLoss (with toY) and
 * CharbonnierLoss of Deraining/basicsr/models/losses/losses.py:26-122 with the weighting and reduction of weight_reduce_loss
 * (losses/loss_util.py:25-54).  lw = loss_weight, d = pred - target, n = batch * channels * plane:
 *   OSS_LOSS_L1, OSS_LOSS_MSE   lw * sum(term) / n with term = |d| or d^2; OSS_LOSS_SUM: lw * sum(term).  With a weight
 *                               (OSS_LOSS_WEIGHT: (batch, channels, H, W); OSS_LOSS_WEIGHT_1CH: (batch, 1, H, W), broadcast over the
 *                               channels by the kernel) term * w, and the mean divides by sum(w), resp. channels * sum(w)
 *                               (loss_util.py:47-52).  d|d| / dd = sign(d) with sign(0) = 0, as torch
 *   OSS_LOSS_CHARBONNIER        sum(sqrt(d^2 + eps^2)) / n; loss_weight is accepted and unused, as in the reference (losses.py:114-122)
 *   OSS_LOSS_PSNR               lw * (10 / ln 10) * mean_b ln(mse_b + 1e-8), mse_b = the mean of d^2 over image b (losses.py:109);
 *                               OSS_LOSS_TOY (channels == 3): on y = (k0 R + k1 G + k2 B + 16) / 255 with k = the fp32 values of
 *                               65.481, 128.553, 24.966 (losses.py:92, :102-105) -- dy is formed from the three differences, the
 *                               + 16 cancels -- and mse_b over the H W pixels
 *   pred      (batch, channels, H, W) dense, fp32 / fp16 / bf16 (pred_io); plane = H * W
 *   target    the same shape, dense, fp32 or pred's type (target_io)
 *   weight    fp32, dense, NULL unless one of the two weight flags is set (L1 and MSE only)
 *   loss      one fp32 scalar in device memory, rounded once from the fp64 result
 *   stats     oss_pixel_loss_stat_doubles(...) doubles the forward writes and the backward reads: the denominator of the mean
 *             (1 for OSS_LOSS_SUM), or for PSNR mse_b per image
 *   partials  oss_pixel_loss_partial_doubles(...) doubles of scratch, no init
 * Arithmetic order: every element is widened to fp32, d and the term (and term * w) are fp32, every sum is fp64.  A workgroup owns
 * 2048 consecutive elements (for PSNR: of one image) and writes one fp64 partial (two with a weight: sum term * w, sum w) after a
 * fixed reduction; a second, single-workgroup launch of the same call adds the partials in a fixed order.  No atomics: reruns are
 * bit-identical, no host read-back, capturable into a hipGraph.  oss_pixel_loss_bwd is one launch: dpred (pred's type) =
 * grad_output (one fp32 scalar in device memory) * d loss / d pred, each value formed in fp32 and rounded once.
 * oss_pixel_loss_partial_doubles is a pure host query and the support query: 0 when the combination is not taken -- pred_io or
 * target_io no element type, a 16-bit target that is not pred's type, an unknown kind or flag, a weight or OSS_LOSS_SUM with
 * Charbonnier / PSNR, both weight flags, OSS_LOSS_TOY without PSNR or with channels != 3, a dimension < 1 or more than 2^31 - 1
 * workgroups.  The entry points return OSS_ERR_SHAPE for the same, OSS_ERR_NULL for a missing pointer. */
#define OSS_LOSS_L1 0
#define OSS_LOSS_MSE 1
#define OSS_LOSS_CHARBONNIER 2
#define OSS_LOSS_PSNR 3
#define OSS_LOSS_SUM 1
#define OSS_LOSS_TOY 2
#define OSS_LOSS_WEIGHT 4
#define OSS_LOSS_WEIGHT_1CH 8
size_t oss_pixel_loss_partial_doubles(int kind, int flags, oss_dtype pred_io, oss_dtype target_io, int64_t batch, int64_t channels,
                                      int64_t plane);
size_t oss_pixel_loss_stat_doubles(int kind, int flags, int64_t batch, int64_t channels, int64_t plane);
int oss_pixel_loss_fwd(int kind, int flags, oss_dtype pred_io, oss_dtype target_io, const void *pred, const void *target,
                       const float *weight, float *loss, double *stats, double *partials, int64_t batch, int64_t channels,
                       int64_t plane, float loss_weight, float eps, oss_stream_t stream);
int oss_pixel_loss_bwd(int kind, int flags, oss_dtype pred_io, oss_dtype target_io, const void *pred, const void *target,
                       const float *weight, const double *stats, const float *grad_output, void *dpred, int64_t batch,
                       int64_t channels, int64_t plane, float loss_weight, float eps, oss_stream_t stream);

/* Training batches cut on the device (oss_pairs.hip): a pool of decoded image pairs resident in device memory, a counter-based draw
 * and one gather launch per batch -- paired_random_crop, augment / random_augmentation (Deraining/basicsr/data/transforms.py:24-83,
 * :136-200, :223-275), img2tensor(bgr2rgb, float32) of img / 255. (utils/img_util.py:9-40) and EnlargedSampler's rank-strided epoch
 * permutation, with no host work, no copy from the host, no atomics and no allocation: both calls can be captured into a hipGraph.
 *   pool      flat uint8 buffer of HWC images, `channels` (1 or 3) interleaved bytes per pixel, any byte alignment
 *   table     (n_pairs, 4) int64 in device memory: gt_offset, lq_offset (bytes into pool), lq_h, lq_w; the GT image is
 *             (scale lq_h, scale lq_w); with scale == 1 LQ and GT are still two images
 *   samples   (batch, 4) int in device memory: pair_index, top, left (LQ pixels), code; code bit 0 = horizontal flip, bit 1 =
 *             vertical flip, bit 2 = transpose, applied in that order (the 8 elements of the dihedral group: every mode of
 *             data_augmentation is exactly one code)
 * oss_pairs_draw (one single-workgroup launch) fills `samples`: it reads the sample counter c (*counter), gives sample b the
 * per-rank position q = c + b and the global position g = q * world + rank, epoch = g div n_pairs, pair = perm_epoch(g mod n_pairs)
 * -- a keyed bijection of [0, n_pairs): 4 Feistel rounds over the next even number of bits with cycle walking, round function
 * word 0 of Philox4x32-10 with key (seed lo, seed hi) and counter (half, round | epoch_hi << 8, epoch_lo, 0x7065726d) -- so all ranks
 * together see every pair once per epoch; top, left, code = words 0, 1, 2 of the Philox block with counter (g lo, g hi, 0x63726f70,
 * 0): top = (word * (lq_h - patch + 1)) >> 32, left likewise, code = (word >> 29) masked by flags (OSS_PAIRS_HFLIP admits bit 0,
 * OSS_PAIRS_ROT bits 1 and 2).  It stores c + batch after every thread has read c, so a replayed launch continues the sequence.
 * oss_pairs_gather writes lq (batch, channels, patch_h, patch_w) and gt (batch, channels, scale patch_h, scale patch_w), float,
 * contiguous, from ONE launch: value = float(byte) / 255.0f correctly rounded, channel order reversed when swap_rb != 0 and
 * channels == 3.  Rectangular patches (whole validation images) are taken with codes 0-3; bit 2 needs patch_h == patch_w.  The
 * kernel never reads outside an image: a rectangle, pair index or offset that does not fit is clamped, what cannot be read is
 * written as 0 and *clamped (an int in device memory the caller zeroed) is set to 1.
 * oss_pairs_ok is a pure host query: channels 1 or 3, 1 <= scale <= 64, 1 <= patch sides, scale * side <= 2^20, 1 <= batch <= 65535
 * and at most 65535 tiles of 32 x 32 pixels per sample (LQ + GT).  oss_pairs_philox evaluates one Philox4x32-10 block (4 counter
 * words, 2 key words -> 4 words) on the HOST from the text the kernels are compiled from.
 *
 * The Deraining tree's loader pads and its training loop cuts a second window (paired_image_dataset.py:101-113, utils/img_util.py:
 * 148-164, train.py:213-271); two sibling entry points do both in the same two launches, the two above are unchanged:
 * oss_pairs_draw_window: the two-stage draw.  Every image counts as extended to max(side, pad_to) (pad_to = 0: as it is); top and
 * left of a crop of side full_patch >= patch come from the words oss_pairs_draw uses, with range max(lq_h, pad_to) - full_patch + 1
 * (and lq_w likewise); ONE window per call comes from words 0, 1 of the Philox block with counter (g0 lo, g0 hi, 0x77696e64, 0), g0 =
 * c * world + rank the global position of the call's first sample: x0 = (word 0 * (full_patch - patch)) >> 32 (rows of the augmented
 * crop), y0 likewise (columns) -- the support {0 .. full_patch - patch - 1} of int((G - m) * random()), {0} when equal.  The sample
 * stored is the crop's window as one ordinary sample of side patch: with (wr, wc) = transpose ? (y0, x0) : (x0, y0), top + (vflip ?
 * full_patch - patch - wr : wr), left + (hflip ? full_patch - patch - wc : wc), and the same code.  All sizes in LQ pixels.  With
 * full_patch == patch and pad_to == 0 the samples are those of oss_pairs_draw, bit for bit; the counter is handled the same way.
 * oss_pairs_gather_padded: oss_pairs_gather on images extended at the bottom and right to max(side, pad_to) by cv2.BORDER_REFLECT
 * (fedcba|abcdefgh|hgfedcb): row or column i >= n of an image with n rows / columns is read at r = i mod 2n, r < n ? r : 2n - 1 - r
 * (periodic: an image smaller than pad_to / 2 is covered).  Nothing is stored and nothing outside the image's own bytes is read; a
 * rectangle that does not fit even the extended image is clamped, zero-filled and flagged as above.  The reference pads LQ and GT by
 * the same pixel count, which is a pair only at scale 1: pad_to > 0 needs scale == 1 (OSS_ERR_SHAPE otherwise); 0 <= pad_to <= 2^20. */
#define OSS_PAIRS_HFLIP 1
#define OSS_PAIRS_ROT 2
int oss_pairs_philox(const uint32_t *counter, const uint32_t *key, uint32_t *out);
int oss_pairs_ok(int channels, int scale, int patch_h, int patch_w, int batch);
int oss_pairs_draw(const int64_t *table, int n_pairs, int64_t *counter, int *samples, int batch, int patch, int64_t seed, int rank,
                   int world, int flags, oss_stream_t stream);
int oss_pairs_gather(const void *pool, int64_t pool_bytes, const int64_t *table, int n_pairs, const int *samples, float *lq, float *gt,
                     int *clamped, int batch, int channels, int patch_h, int patch_w, int scale, int swap_rb, oss_stream_t stream);
int oss_pairs_draw_window(const int64_t *table, int n_pairs, int64_t *counter, int *samples, int batch, int patch, int full_patch,
                          int pad_to, int64_t seed, int rank, int world, int flags, oss_stream_t stream);
int oss_pairs_gather_padded(const void *pool, int64_t pool_bytes, const int64_t *table, int n_pairs, const int *samples, float *lq,
                            float *gt, int *clamped, int batch, int channels, int patch_h, int patch_w, int scale, int swap_rb,
                            int pad_to, oss_stream_t stream);

/* Algorithmic bytes of the block's NON-scan launches, by kernel family (round 6; bench.py `roofline.non_scan`).  While counting
 * is on, every entry point of this header that launches a kernel adds the bytes its launch must move at minimum (each operand
 * read once, each result written once, fp32 master weights included, scratch partials not) to its family's counter -- host-side
 * bookkeeping only, so it also works while a hipGraph is being captured.  oss_prof_family_enable(1) clears the counters.
 * oss_prof_family: name, the '|'-separated substrings of the family's kernel names (for matching a kernel trace), bytes and
 * entry-point calls since counting was switched on.  The scan kernels have their own event profiler above (oss_prof_collect2). */
void oss_prof_family_enable(int on);
int oss_prof_family_count(void);
int oss_prof_family(int family, const char **name, const char **kernel_patterns, double *algorithmic_bytes, long long *calls);

/* Runtime-selected scan forms the loaded library contains.  Since round 6 every build has both (rounds 4-5 kept them behind
 * build flags): the fused-delta form of SURVEY.md 8f row 1 (chosen per call by oss_scan_fwd_params.dt_weight != NULL) and the
 * lane states (chosen per call by oss_scan_fwd_params.hs != NULL).  Both are parity-green against the oracle and measured
 * slower inside the training step, so the host layers leave them off unless asked.  A build that
 * compiled one out (-DOSS_WITHOUT_FUSED_DT / -DOSS_WITHOUT_LANE_STATES) rejects dt_weight with OSS_ERR_SHAPE, answers 0 from
 * oss_scan_fused_dt_ok() / oss_scan_lane_state_floats() and ignores `hs`. */
#define OSS_FEATURE_FUSED_DT 1
#define OSS_FEATURE_LANE_STATES 2
int oss_scan_features(void);

/* fp32 product modes of the six GEMM-shaped entry points (pure host query): bit 0 = exact fp32 MFMA (OSS_F32), bit 1 = split bf16
 * (OSS_F32_BF16X3). */
int oss_f32_matmul_modes(void);

/* ABI guard.  oss_scan_fwd_params / oss_scan_bwd_params / oss_chan_params cross the boundary BY POINTER, so a binding layer
 * compiled against another revision of this header would hand the kernels garbage pointers.  OSS_ABI_VERSION is bumped with
 * every change of a struct or of an entry point's argument list (9: the pre-packed weight images of the 1x1 convolutions,
 * oss_conv1x1_pack_* and the *_packed entry points; 10: oss_chan_params lost zt and dts, the channel kernels evaluate the
 * projections from the pooled vector; 11: the added entry point oss_proj_set_one_launch; 12: the added
 * entry points oss_jpeg_workgroups and oss_jpeg_roundtrip; 13: the added entry points oss_noise_workgroups,
 * oss_noise_scratch_words, oss_noise_gaussian, oss_noise_poisson, their *_host twins and oss_noise_normals_host; 14: the added entry point
 * oss_conv1x1_describe with its struct oss_conv1x1_launch); oss_abi_struct_bytes(which) is the library's own sizeof
 * (which: 0 = oss_scan_fwd_params, 1 = oss_scan_bwd_params, 2 = oss_chan_params; 0 for anything else).  Every binding layer
 * in this tree compares both with its own values when it loads and refuses to run on a mismatch: csrc_host/oss_torch_host.cpp
 * (through vmambair_amd/_host.py) with its compile-time ones, vmambair_amd/_capi.py with what it reads from this file -- the
 * number below is the only place to bump. */
#define OSS_ABI_VERSION 14
int oss_abi_version(void);
size_t oss_abi_struct_bytes(int which);

#ifdef __cplusplus
}
#endif
#endif /* VMAMBAIR_OSS_H */
