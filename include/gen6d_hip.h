/*
 * gen6d_hip.h — C ABI of libgen6d_hip.so: the hand-written gfx950 kernels behind the Gen6D inference hot path
 * (detector score-map correlation, selector viewpoint similarity, refiner feature-volume pose update).
 *
 * Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch tensors' data_ptr()); nothing is allocated,
 *     freed or synchronised inside; every call enqueues on the given hipStream_t and returns immediately;
 *   - return value: 0 on success, a negative G6D_E* code otherwise (never throws);
 *   - activations are CHANNELS-LAST fp32: [N][D][H][W][C] with an explicit channel stride `ld` (>= C, multiple of 4),
 *     so a layer can read from / write into a channel slice of a wider (concatenated) buffer;
 *   - conv weights are [Cout][taps][Cin] (the reference's [Cout][Cin][kd][kh][kw] permuted once at load time).
 *
 * The reference has no FFI: each entry point replaces a PyTorch op sequence of the reference, cited per function
 * as file:line relative to liuyuan-pal/Gen6D.  INTEGRATION.md shows the ctypes binding a maintainer would add.
 */
#ifndef GEN6D_HIP_H
#define GEN6D_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* g6d_stream_t; /* hipStream_t */

enum {
  G6D_OK = 0,
  G6D_EINVAL = -1,   /* bad shape / null pointer / misaligned pointer */
  G6D_ENOSPC = -2,   /* workspace too small */
  G6D_ELAUNCH = -3   /* hipLaunch error (hipGetLastError != success) */
};
/* Refusals.  Every launcher checks its arguments on the host BEFORE the first HIP call and refuses with G6D_EINVAL (G6D_ENOSPC for a
 * workspace or spectrum that is too small) and a message in g6d_last_error(): a NULL required pointer; a dimension or count < 1 (or beyond
 * its documented maximum); a row stride smaller than the row it holds (ld < C), or off the vector width where rows are read in 16-byte
 * pieces; a pointer that is not 16-byte aligned where the kernel reads or writes 8- / 16-byte pieces; an enumeration outside its values;
 * and sizes whose element offsets, work-item counts or grid sizes leave the type the launcher or the kernel computes them in (products
 * such as n * C, HW * C, hs * ws, dh * dw, rfn * C, N * H * W, fh * fw * C that pass 2^31 - 1 where they are formed as int; where a grid
 * is such a count rounded up to whole blocks, count + block - 1 must fit as well, e.g. n * C <= 2^31 - 256).  A refused call has
 * launched nothing.  The entry points the table reaches are those of elementwise, selector, detector, refiner_volume, warp, pose_chain,
 * track_health, split16 and the frame launchers, whose integer arithmetic was read line by line; the convolution, Winograd and correlation
 * families keep the byte and element bounds they state in their own messages (2^29 / 2^30 / 2^31 floats, 2 GB of filters).  tests/launch_contract.py holds the rules per entry point as a table, tests/test_launch_contract_cpu.py runs it. */

int g6d_abi_version(void);
/* last HIP error string of this thread ("" if none) */
const char* g6d_last_error(void);

/* Launch-policy knobs.  The library reads NO environment variable: every dispatch decision that tools/ and tests want to force (a kernel
 * variant for an A/B run, a constant of a split model for a sweep) is a named knob with the product default — conv_patch, tile_policy,
 * split_target, patch_pipe, corr_slots, sel_rowq, conv1_mfma, w43_split_max / _gain / w43_chunk_us, wino_debug, conv_wino43, wino_wide,
 * wino_split_max / _gain / _fix / _per, wino16_2w, conv_wino, conv_wino16, wino_min_work, w43_map, conv_pm, gemv_mfma, c16_ablate, conv16_halo, conv_narrow (gen6d_amd/csrc/common.hip lists meanings
 * and defaults).  Process-wide; reads and writes are relaxed atomics (a launch racing with g6d_set_knob sees the old or the new value):
 * set them before the launches they are meant to steer.  g6d_set_knob returns G6D_EINVAL for an unknown name; g6d_get_knob returns
 * -1e300 for one. */
int g6d_set_knob(const char* name, double value);
double g6d_get_knob(const char* name);
void g6d_reset_knobs(void);

/* Profiling aid: launches the empty kernel `g6d_marker_kernel` so a kernel trace can be cut to a region of interest. */
int g6d_marker(int id, g6d_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Generic implicit-GEMM convolution on fp32 MFMA (v_mfma_f32_32x32x2_f32), 1-D/2-D/3-D, stride, zero padding.
 * Replaces every dense conv / linear contraction of the hot path:
 *   detector  F.conv2d(que_x, ref_x) correlation            network/detector.py:222-224
 *             score/scale/offset heads                        network/detector.py:164-184,248-255
 *   selector  corr_conv_list (1,3,3) Conv3d stacks            network/selector.py:27-69,187
 *             corr_feats_conv, score_process, mlps, heads     network/selector.py:71-104,197-214
 *   refiner   RefineFeatureNet convs                          network/refiner.py:24-51
 *             RefineVolumeEncodingNet 3x3x3 convs             network/refiner.py:88-143
 * Fused into the operand loader: optional elementwise multiplier (selector query x reference product,
 * selector.py:183-186, never materialised), optional per-channel affine (the preceding InstanceNorm,
 * applied as x*scale+shift; padding stays exactly zero as in the reference where padding follows the norm) and ReLU.
 * Fused into the epilogue: bias, activation, per-(group,channel) sum / sum-of-squares for the FOLLOWING
 * InstanceNorm (fp64 accumulators).
 *   out[m][co] = act( bias[co] + sum_{tap,ci} X(m,tap,ci) * weight[co][tap][ci] )
 *   X = relu?( (in * mul?) * in_scale + in_shift ), 0 outside the input; mul and relu only together with in_scale / in_shift (the ReLU is
 *   the one that follows the InstanceNorm affine: in_relu or mul without in_scale is refused with G6D_EINVAL)
 * ---------------------------------------------------------------------------------------------------------------- */
/* Workspace (g6d_conv_igemm, g6d_corr2d_patch, g6d_wino_conv3x3): layers whose grid would not fill 256 CUs split their
 * reduction over more blocks.  The workspace holds G6D_WORKSPACE_COUNTER_BYTES of per-tile arrival counters followed by the
 * partial tiles; the block of a tile that arrives last adds the partials and runs the epilogue (no second kernel at any
 * split count).  Contract: 16-byte aligned, the first
 * G6D_WORKSPACE_COUNTER_BYTES are ZERO before the first call (every call leaves them zero), and the buffer is not shared
 * by launches that may run concurrently (one per stream).  NULL / 0 disables splitting. */
#define G6D_WORKSPACE_COUNTER_BYTES 16384

typedef struct G6dConv {
  const float* in;        /* [N][Di][Hi][Wi][ld_in] */
  const float* mul;       /* optional [Hi][Wi][Cin] (dense), broadcast over N and Di (one per image group with mul_group_images); NULL = none */
  const float* in_scale;  /* optional [in_affine_groups][Cin]; NULL = none */
  const float* in_shift;  /* same shape as in_scale */
  const float* weight;    /* [Cout][kd*kh*kw][Cin] */
  const float* bias;      /* [Cout] or NULL */
  float* out;             /* [N*Do*Ho*Wo][ld_out] */
  double* stats;          /* optional [stat_groups][Cout][2] (sum, sumsq), caller-zeroed; NULL = none */
  float* workspace;       /* split scratch (see "Workspace" below); may be NULL if workspace_bytes == 0 */
  size_t workspace_bytes;
  int32_t N, Di, Hi, Wi, Cin, ld_in;
  int32_t Do, Ho, Wo, Cout, ld_out;
  int32_t kd, kh, kw;
  int32_t sd, sh, sw;
  int32_t pd, ph, pw;
  int32_t in_relu;              /* apply ReLU after the input affine; non-zero needs in_scale / in_shift (G6D_EINVAL without them) */
  int32_t in_affine_per_n;      /* 0: one affine table for all N; k >= 1: image n uses table n / k (1 = a table per image; k = the
                                   hypothesis count D when N = qn * D images of a batched selector call share one table per query) */
  int32_t out_act;              /* 0 none, 1 ReLU, 2 LeakyReLU(0.1); anything else is refused.  Sizes: N, Di, Hi, Wi, Do, Ho, Wo, Cin, Cout, the
                                   kernel extents (<= 32) and the strides sd, sh, sw are >= 1, the paddings >= 0; Cin % 4 == 0,
                                   ld_in % 4 == 0, ld_in >= Cin, ld_out >= Cout; in, weight, mul and the affine tables 16-byte aligned */
  int32_t stat_rows_per_group;  /* output rows per statistics group (0 = all rows in one group) */
  int32_t split_k;              /* 0 = choose automatically; 1 = never split; >1 = force */
  int32_t math_mode;            /* 0 = fp32 MFMA (default, the parity path); 1 = bf16, 2 = fp16 operands with fp32 accumulation:
                                   v_mfma_f32_32x32x16_{bf16,f16}, opt-in speed mode graded separately (BASELINE configs[2], [4]);
                                   3 = fp32-CLASS arithmetic on the fp16 matrix cores, used by the fp32 path: the implicit-GEMM kernel's
                                   loader splits every fp32 operand (after the prologue) into an fp16 hi / lo pair, three
                                   v_mfma_f32_32x32x16_f16 per product (hi x hi + hi x lo + lo x hi).  Always the implicit-GEMM kernel
                                   (no Winograd / patch / narrow hand-off; weight_wino16 must be NULL), strided, 3-D, split-K and 1x1
                                   layers included; Cin % 8 == 0, Cout > 32, no `mul`.  Filters are split as weight * 2^w_exp, activations
                                   as x * 2^-e with e and the range record from g6d_conv_igemm_ex's G6dRange16;
                                   4 = mode 3 with PRE-SPLIT FILTERS (additive to ABI v12: values above 3 were rejected): `weight` points at
                                   [Cout][taps][Cin / 32][2][32] fp16 — per 32-channel chunk the 32 hi halves rn16(u), then the 32 lo halves
                                   rn16(u - hi), u = w * 2^w_exp: the bytes the chunk's fp32 values would occupy — and the loader copies them;
                                   activations, prologue, exponent and record as in 3; bit-identical to 3.  Cin % 32 == 0;
                                   5 = mode 4 with PRE-SPLIT ACTIVATIONS as well: `in` points at a pair map in the format of
                                   g6d_conv16_direct_multi's math_mode 3 and g6d_affine_split16 — [N][Di][Hi][Wi] pixels of ld_in 16-bit
                                   elements, a pixel's hi plane of Cin values at its start and its lo plane ld_in / 2 elements further on
                                   (dense: ld_in = 2 Cin; a channel slice of a wider dense map: that map's row, `in` at the slice's first hi
                                   value); ld_in % 16 == 0, ld_in >= 2 Cin, Cin % 32 == 0.  No prologue and no multiplier (in_scale,
                                   in_shift, in_relu, mul must be unset: the map's producer applied them); the map holds x * 2^-e with
                                   e = exps[slot_in] of g6d_conv_igemm_ex's G6dRange16, and the launch records nothing */
  const float* weight_wino;     /* optional: the same filters transformed for Winograd F(2x2,3x3), [kd][Cin/8][16][Cout][8] in the
                                   layout of g6d_wino_conv3x3 (per depth tap for 3x3x3).  When set and the layer is eligible
                                   (stride 1, "same" padding, maps >= 6x6, Cin % 8 == 0, Cout % 32 == 0, fp32), the launch runs on
                                   the Winograd kernel (2.25x fewer multiplications) with the same prologue / epilogue semantics;
                                   otherwise `weight` is used.  NULL = never. */
  /* Optional InstanceNorm finalisation inside the launch (needs `stats`): the block that finishes last turns the completed
     (sum, sumsq) table into the affine of the FOLLOWING InstanceNorm — scale = 1/sqrt(var + eps), shift = -mean * scale with
     mean = sum / fin_count, var = sumsq / fin_count - mean^2 — instead of a separate g6d_stats_finalize launch.
     fin_scale / fin_shift: [fin_groups][Cout] floats; fin_counter: one int32, ZERO before the launch (the launch leaves it zero).
     NULL fin_scale = off.  Not for statistics that are still to be summed over ranks. */
  float* fin_scale;
  float* fin_shift;
  int32_t* fin_counter;
  double fin_count, fin_eps;
  int32_t fin_groups;
  /* Query batching (round 3; reference API: network/selector.py:165-175 takes [qn,...] queries).  N = qn * k images, image
     n = q * k + d belongs to query q:
       in_image_mod = k      image n READS input image n % k — `in` holds k images (the selector's reference cache, shared by the
                             queries of the batch instead of being replicated); 0 = off (`in` holds N images)
       mul_group_images = k  `mul` is [ceil(N / k)][Hi][Wi][Cin] and image n is multiplied by mul[n / k] (the query's own feature
                             map); 0 = one multiplier for all images
     together with in_affine_per_n = k and stat_rows_per_group = k * Do * Ho * Wo every query keeps its own InstanceNorm. */
  int32_t in_image_mod;
  int32_t mul_group_images;
  int32_t w_exp;                /* math_mode 3: the filters are split as weight * 2^w_exp (an exact scaling, undone on the accumulators) so
                                   that the lo parts of small filters stay normal fp16 numbers — choose the largest w_exp <= 14 with
                                   max |weight| * 2^w_exp < 2048; not read in the other modes (the former reserved_ field: 0 = unscaled) */
  const void* weight_wino16;    /* optional, used when math_mode != 0: the Winograd-domain filters ROUNDED to the operand type of
                                   math_mode (bf16 / fp16), [kd][Cin/16][16][Cout][16] 16-bit values in the layout of
                                   g6d_wino16_conv3x3_multi's U16 (per depth tap for 3x3x3).  Eligible layers (as weight_wino, and
                                   Cin % 16 == 0, Cout % 64 == 0) then run on the 16-bit Winograd kernel instead of the direct kernels
                                   with 16-bit operands.  NULL = never. */
  const float* weight_wino43;   /* optional (ABI v8): the same filters transformed for Winograd F(4x4,3x3) in the layout of
                                   g6d_wino43_conv3x3_multi's U43, [kd * Cin/8][2][Cout/64][18][2][4][16][4] (per depth tap for 3x3x3).  When set
                                   and the layer is eligible (fp32, stride 1, "same" padding, maps >= 8x8, Cin % 8 == 0, Cout % 64 ==
                                   0, no multiplier) the launch runs on the F(4x4,3x3) kernel: 4x fewer multiplications than the direct
                                   form at ~5x the fp32 error of F(2x2,3x3) — set it only on layers whose parity budget has the room
                                   (the refiner's 32^3 volume layers); takes precedence over weight_wino.  NULL = never. */
} G6dConv;

int g6d_conv_igemm(const G6dConv* desc, g6d_stream_t stream);
/* g6d_conv_igemm with the range control of math_mode 3 (additive to ABI v12; G6dRange16 below; NULL = exponent 0, nothing recorded;
   a non-NULL range with another math_mode is G6D_EINVAL): the kernel is producer and consumer of its operand pairs, so ONE slot serves —
   the loader splits x * 2^-exps[slot_out] (x after the multiplier / affine / ReLU prologue; padding stays exactly zero), folds
   2^exps[slot_out] back into the accumulator scale, and records the largest |x| in rec[slot_out] (at most one atomicMax per block, only
   when it exceeds a coherent read of the record).  slot_in is not read.  math_mode 4: the same.  math_mode 5 is a consumer only: it
   reads the exponent of its pair map from exps[slot_in] (< 0: exponent 0), writes no record and does not read slot_out.
   Implementation note: the kernel takes the descriptor by value, and in math_mode 3 - 5 the launcher's private COPY of it carries the two
   device pointers &exps[slot_out] and &rec[slot_out] in `weight_wino16` / `weight_wino43`, fields this kernel never reads as filters (that
   keeps one kernel signature and the other modes' code unchanged).  The caller's descriptor is not modified, and a caller's own values in
   those two fields are not forwarded in math_mode 3 - 5 (weight_wino16 must be NULL, weight_wino43 is ignored). */
struct G6dRange16;
int g6d_conv_igemm_ex(const G6dConv* desc, const struct G6dRange16* range, g6d_stream_t stream);
/* Kernel family g6d_conv_igemm will run `desc` on (no launch): 0 generic implicit GEMM, 1 LDS-patch kernel, 2 Winograd F(2x2,3x3) kernel,
   3 Winograd F(4x4,3x3) kernel, 4 narrow-output kernel, 5 implicit GEMM on fp16 hi / lo pairs (math_mode 3, 4, 5) */
int g6d_conv_plan(const G6dConv* desc);
/* sizeof(G6dConv) as compiled into the library: bindings check their struct layout against it */
int g6d_sizeof_conv_desc(void);
/* The route g6d_conv_igemm will take with `desc` under the current knobs (additive to ABI v12; launches nothing, reads no operand, and is
   the launcher's own decision code, not a restatement of it).  Returns G6D_OK, or what the launch would refuse the descriptor with
   (G6D_EINVAL / G6D_ENOSPC and its message; the fields are then not meaningful).  tests/conv_sweep.py files its descriptors by it. */
typedef struct G6dConvRoute {
  int32_t family;          /* as g6d_conv_plan */
  int32_t bm, bn;          /* families 0 and 5: the tile, 128x128 / 128x64 / 128x32 / 64x64 output rows x channels; otherwise 0 */
  int32_t mode;            /* the loader prologue of the kernel that runs.  Families 0 and 5: 0 none, 1 affine with one table, 2 affine with a
                              table per image group, 3 multiplier + affine, 4 multiplier + affine per image group.  Families 1 - 3: the mode
                              their own launcher chooses (0 none, 1 affine, 2 affine per image group, 3 multiplier + affine; the LDS-patch
                              kernel reads one or many tables in mode 1).  Family 4: 0 */
  int32_t math_mode;       /* families 0 and 5: the descriptor's; otherwise 0 */
  int32_t splits;          /* blocks that share one output tile's reduction, after every clamp and rounding (1 = no split); families 1 - 3:
                              the count their launcher's own rule chooses, -1 if that launcher would refuse the layer */
  int32_t split_source;    /* 0 none (splits == 1), 1 forced by split_k > 1, 2 automatic, 3 automatic and then clamped by the workspace's
                              room or by the tile-counter limit (splits may be 1).  Families 1 - 3: 0 or 2 only — their launchers fold
                              the workspace's room into their own count and do not say whether it cut it */
  int32_t position_major;  /* families 0 and 5: 1 = position-major row order (knob conv_pm), 0 = row order */
} G6dConvRoute;
int g6d_conv_route(const G6dConv* desc, G6dConvRoute* route);
int g6d_sizeof_conv_route(void);

/* Stride-1 2-D cross-correlation without bias for Cout <= 32 with input-patch reuse in LDS: the detector's
 * F.conv2d(que_x0, ref_x0, padding=7) (network/detector.py:224), where the generic kernel is bound by re-loading the
 * activation tile for every one of the 225 taps.  in [H][W][ld_in], wgt [Cout][kh*kw][Cin], out [H*W][ld_out],
 * "same" zero padding (kh, kw odd, kw <= 31).  workspace: split scratch (see "Workspace"). */
int g6d_corr2d_patch(const float* in, int H, int W, int Cin, int ld_in, const float* wgt, int Cout, int kh, int kw,
                     float* out, int ld_out, float* workspace, size_t workspace_bytes, int math_mode /* as G6dConv.math_mode */,
                     g6d_stream_t stream);
/* The same correlation for up to 4 map sizes in one launch: the scales of the detector's image pyramid against the same reference
 * filters, N maps (the queries of a batch, network/detector.py:291-304 takes [qn,H,W,3]) per size; the tiles of all maps form one
 * flat work list (fewer splits, one launch).  Inputs within 2^30 floats of each other (g6d_corr2d_wino_multi,
 * g6d_corr2d_wino43_multi: 2^29), outputs within 2^31. */
typedef struct G6dCorrSeg {
  const float* in;        /* [N][H][W][ld_in] */
  float* out;             /* [N][H*W][ld_out] */
  int32_t H, W, ld_in, ld_out;
  int32_t N, reserved_;   /* N >= 1 maps of this size, dense one after the other */
} G6dCorrSeg;
int g6d_corr2d_patch_multi(const G6dCorrSeg* segs, int nseg, int Cin, const float* wgt, int Cout, int kh, int kw,
                           float* workspace, size_t workspace_bytes, int math_mode, g6d_stream_t stream);
/* The same correlation with 16-bit matrix-core operands on its own kernel (math_mode 1 = bf16, 2 = fp16; fp32 maps in and out, fp32
 * accumulation): the reference filters are rounded and laid out per unit on the host, once per object — w16 =
 * [(Cin/32) * kh units][kw][32 co][40 x 16 bit]: unit u holds the 32 channels of chunk u / kh at filter row u % kh, every (tap, co)
 * row is 32 channels + 8 values of zero padding (rows co >= Cout zero), and >= 1 KB of padding follows the last unit.  All kw weight
 * tiles of a unit are staged at once, so a wave runs its 2 kw MFMAs without a barrier (g6d_corr2d_patch_multi with math_mode != 0
 * keeps one hand-over per tap).  Cin % 32 == 0, Cout <= 32, odd kh, odd kw <= 15.  Replaces network/detector.py:222-224 in the
 * reduced-precision mode. */
int g6d_corr2d_patch16_multi(const G6dCorrSeg* segs, int nseg, int Cin, const void* w16, int Cout, int kh, int kw,
                             float* workspace, size_t workspace_bytes, int math_mode, g6d_stream_t stream);

/* The 15x15 level of the same correlation (network/detector.py:222-224) on the Winograd kernel of g6d_wino_conv3x3: the filter is
 * cut into kblocks x kblocks (= 5 x 5) blocks of 3x3 taps, out = sum_b conv3x3(in shifted by (3bi-6, 3bj-6), w_b), and the 25 blocks
 * accumulate in the F(2x2,3x3) transform domain: 2.25x fewer multiplications than g6d_corr2d_patch.  Maps as above (all with the
 * same ld_in); U = the sub-filter banks transformed on the host like g6d_wino_conv3x3's U, CHUNK-major [Cin/8][25][16][Cout][8]
 * (row c*25 + b = 8-channel chunk c of block b = 5*bi + bj, which holds w[:, 3bi..3bi+2, 3bj..3bj+2, :]: the 25 shifted visits of a
 * chunk are consecutive, so the window stays in L2); Cin % 8 == 0, Cout % 32 == 0. */
int g6d_corr2d_wino_multi(const G6dCorrSeg* segs, int nseg, int Cin, const float* U, int Cout, int kblocks, float* workspace,
                          size_t workspace_bytes, g6d_stream_t stream);

/* The same 15x15 correlation with the 25 blocks accumulated in the F(4x4,3x3) transform domain (ABI v8; kernel and filter layout of
 * g6d_wino43_conv3x3_multi): 225 taps cost 25 * 36 / 16 = 56.25 multiplications per output (F(2x2,3x3): 100).  U43 CHUNK-major
 * [Cin/8 * 25][2][Cout/CB][18][CB/32][4][16][4], row c*25 + b = chunk c of block b; Cin % 8 == 0, Cout % 32 == 0.
 * kblocks = 3 (ABI v9): a 9x9 "same" correlation as 3x3 blocks (rows c*9 + b, shifts 3bi-3, 3bj-3) — the 7x7 level of the detector
 * (F.conv2d(que_x1, ref_x1, padding=3)) with its filters zero-extended by one tap on every side: 20.25 multiplications instead of 49. */
int g6d_corr2d_wino43_multi(const G6dCorrSeg* segs, int nseg, int Cin, const float* U43, int Cout, int kblocks, float* workspace,
                            size_t workspace_bytes, g6d_stream_t stream);

/* InstanceNorm finalisation: stats[g][c] = (sum, sumsq) over `count` elements ->
 * scale = 1/sqrt(var+eps), shift = -mean*scale (biased variance; torch InstanceNorm{1,2,3}d, eps 1e-5,
 * network/selector.py:28-77, network/refiner.py:27-50,93-133). n = groups*channels, 1 <= n <= 2^31 - 256;
 * count > 0. */
int g6d_stats_finalize(const double* stats, int n, double count, double eps, float* scale, float* shift, g6d_stream_t stream);

/* y = pool2x2?( relu?( x*scale[c] + shift[c] ) ) on [N][H][W][C] channels-last rows (D folded into N).
 * pool: 0 none, 1 = 2x2 max (MaxPool3d (1,2,2), network/selector.py:34,41,56), 2 = full-window mean over HxW
 * (AvgPool3d (1,4,4), selector.py:76).  scale/shift may be NULL (identity; both or neither); affine_per_n = k >= 1: image n uses table n / k
 * (as G6dConv.in_affine_per_n), 0: one table.  C > 0 and C, ld_in, ld_out multiples of 4, ld_in >= C, ld_out >= C; in, out and the tables
 * 16-byte aligned; pool 1 needs even H and W; pool 2: H * W <= 2^31 - 1. */
int g6d_affine_act_pool(const float* in, int ld_in, const float* scale, const float* shift, int affine_per_n, int relu,
                        int pool, int N, int H, int W, int C, float* out, int ld_out, g6d_stream_t stream);

/* Bilinear up-sampling by an integer factor (align_corners=False, F.interpolate in network/refiner.py:74-75) of
 * relu?(x*scale+shift) on [N][H][W][C] -> [N][H*f][W*f][C] written with channel stride ld_out.  N, H, W > 0, factor >= 1; C, strides,
 * alignment and affine_per_n as g6d_affine_act_pool; H * factor and W * factor <= 2^31 - 1. */
int g6d_upsample_bilinear(const float* in, int ld_in, const float* scale, const float* shift, int affine_per_n,
                          int N, int H, int W, int C, int factor, float* out, int ld_out, g6d_stream_t stream);

/* VGG trunk glue for an NCHW caller (a trunk whose convolutions run elsewhere, e.g. tools/library_trunk.py's MIOpen A/B trunk; reference
 * pretrain_models.py:86-104 with BatchNorm folded): out = maxpool2x2?( relu?( in + bias[c] ) ) in one pass.  The product trunk
 * (g6d_vgg_conv1_pool_nhwc + g6d_wino_conv3x3* / g6d_wino43_conv3x3_multi) fuses this into its epilogues and does not call it. */
int g6d_bias_relu_pool_nchw(const float* in, const float* bias, int N, int C, int H, int W, int relu, int pool, float* out,
                            g6d_stream_t stream);

/* First trunk layer fused (reference network/pretrain_models.py:17-25,66-72: vgg11_bn features[0..3] with BatchNorm
 * folded): out = maxpool2x2( relu( conv3x3_pad1(in, w) + bias ) ).  in [N][3][H][W], w_oihw [64][3][3][3], bias [64],
 * out [N][64][H/2][W/2] (floor); Cin must be 3 and Cout 64.  Replaces the library convolution of that layer, its two
 * layout transposes and the g6d_bias_relu_pool_nchw pass over the full-resolution result. */
int g6d_vgg_conv1_pool(const float* in, int N, int H, int W, const float* w_oihw, const float* bias, int Cin, int Cout,
                       float* out, g6d_stream_t stream);

/* The same layer with a channels-last result [N][H/2][W/2][64] (input of g6d_wino_conv3x3). */
int g6d_vgg_conv1_pool_nhwc(const float* in, int N, int H, int W, const float* w_oihw, const float* bias, int Cin, int Cout,
                            float* out, g6d_stream_t stream);
/* The same on an image in [0,1]: torchvision Normalize ((x - mean[c]) / std[c]; mean, std: HOST arrays of 3 floats) applied
 * while the input tile is staged — replaces the two elementwise passes of img_norm in front of every trunk call. */
int g6d_vgg_conv1_pool_nhwc_norm(const float* in, int N, int H, int W, const float* w_oihw, const float* bias, int Cin, int Cout,
                                 const float* mean_host, const float* std_host, float* out, g6d_stream_t stream);
/* g6d_vgg_conv1_pool_nhwc(_norm) with a 16-BIT channels-last result [N][H/2][W/2][64] (ABI v11; math_mode 1 = bf16, 2 = fp16): the first
 * layer of the reduced-precision mode's 16-bit activation path (its output feeds g6d_conv16_direct_multi).  fp32 arithmetic, rounded
 * once in the epilogue.  math_mode 3: fp16 hi / lo pairs [N][H/2][W/2][2][64] (hi = rn16(v), lo = rn16(v - hi)), the input format of
 * g6d_conv16_direct_multi's math_mode 3 (the fp32 path's trunk).  mean_host / std_host: NULL = the input is already normalised. */
int g6d_vgg_conv1_pool_nhwc16(const float* in, int N, int H, int W, const float* w_oihw, const float* bias, int Cin, int Cout,
                              const float* mean_host, const float* std_host, void* out16, int math_mode, g6d_stream_t stream);


/* The 3x3 layers 64->128 ... 512->512 of the VGG-11-BN trunks (reference network/pretrain_models.py:9-31,61-72:
 * vgg11_bn features[4..28], BatchNorm folded) as Winograd F(2x2,3x3) on fp32 MFMA with the trunk's bias, ReLU and 2x2
 * max-pool fused into the epilogue; channels-last in and out.
 *   in   [N][H][W][ld_in], Cin % 8 == 0;  U = filters transformed on the host, [Cin/8][16][Cout][8] with
 *        U[c][4a+b][co][k ^ (co & 8 ? 4 : 0)] = (G g G^T)[a][b] of filter (co, 8c+k), G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]]
 *        (the two 4-channel halves of a row are swapped for co & 8: bank-conflict-free LDS image, the copy is lane-linear)
 *   y = conv3x3_pad1(in) + bias[co];  relu != 0: y = max(y, 0)
 *   out_full (optional) [N][H][W][ld_full] = y;  out_pool (optional) [N][H/2][W/2][ld_pool] = maxpool2x2(y) (floor)
 *   workspace (optional): small maps split the channel chunks over more blocks (see "Workspace")
 * One trunk layer = one launch: convolution, bias, ReLU, 2x2 max-pool and the channels-last layout in the kernel's epilogue. */
int g6d_wino_conv3x3(const float* in, int N, int H, int W, int Cin, int ld_in, const float* U, const float* bias, int Cout,
                     int relu, float* out_full, int ld_full, float* out_pool, int ld_pool, float* workspace,
                     size_t workspace_bytes, g6d_stream_t stream);

/* The same layer over up to 4 map sizes in one launch: the scales of the detector's image pyramid (network/detector.py:236-241)
 * share every trunk layer's filters, and the quarters of all segments form one flat work list, so the small scales fill the
 * blocks the large ones leave over.  All segments give the same kinds of output (out_full / out_pool both set or both NULL
 * across segments), their inputs lie within 2^29 floats of each other and their outputs of each kind within 2^31 (allocate them from
 * one buffer). */
typedef struct G6dWinoSeg {
  const float* in;        /* [N][H][W][ld_in] */
  float* out_full;        /* [N][H][W][ld_full] or NULL */
  float* out_pool;        /* [N][H/2][W/2][ld_pool] or NULL */
  int32_t N, H, W, ld_in, ld_full, ld_pool;
} G6dWinoSeg;
int g6d_wino_conv3x3_multi(const G6dWinoSeg* segs, int nseg, int Cin, const float* U, const float* bias, int Cout, int relu,
                           float* workspace, size_t workspace_bytes, g6d_stream_t stream);

/* Reduced-precision variant of g6d_wino_conv3x3_multi (opt-in speed mode as G6dConv.math_mode: 1 = bf16, 2 = fp16 operands, fp32
 * accumulation, fp32 activations in and out) on v_mfma_f32_32x32x16_{bf16,f16}: a chunk is 16 input channels, U16 = the filters
 * transformed AND rounded on the host, [Cin/16][16][Cout][16] 16-bit values (32 bytes per (a,b,co) row; rows with co & 8 carry their
 * two 16-byte halves swapped, as in g6d_wino_conv3x3's U); Cin % 16 == 0, Cout % 64 == 0. */
int g6d_wino16_conv3x3_multi(const G6dWinoSeg* segs, int nseg, int Cin, const void* U16, const float* bias, int Cout, int relu,
                             int math_mode, float* workspace, size_t workspace_bytes, g6d_stream_t stream);

/* Direct (implicit-GEMM) 3x3 / 3x3x3 "same" convolution on 16-BIT ACTIVATIONS (ABI v11, round 6): the kernel family of the VGG trunks
 * (reference network/pretrain_models.py:9-31,66-72; the detector's image pyramid network/detector.py:188-197,236-241; the refiner's
 * crops network/refiner.py:64-78).  v_mfma_f32_32x32x16_{bf16,f16}, fp32 accumulation; the activation tile of a K step goes
 * global -> LDS by DMA (zero padding = the buffer's out-of-range zero fill).
 *   math_mode 1 = bf16, 2 = fp16   the reduced-precision mode (BASELINE configs[2] / [4]): `in`, W16 and 16-bit outputs hold that type
 *   math_mode 3                    fp32-CLASS arithmetic on the fp16 matrix cores, used by the fp32 path: every operand is a PAIR of fp16
 *                                  values hi = rn16(x), lo = rn16(x - hi) (22+ significand bits; the MFMA keeps fp16 subnormals) and
 *                                  acc += a_hi b_hi + a_hi b_lo + a_lo b_hi — 3 MFMAs of 32 cycles per 16 channels against 8 x 64 cycles
 *                                  on the fp32 matrix cores.  Activations [pixel][2][C]: the hi plane, then the lo plane (ld >= 2 C).
 *   in     [N][D][H][W][ld_in] 16-bit channels-last (D = 1 for the 2-D layers), rows 16-byte aligned; Cin % 64 == 0 (pairs: % 32)
 *   W16    w_layout 0: [Cout][kd*9][Cin] rows, tap = (kz*3 + ky)*3 + kx (math_mode 1 / 2; both operand tiles staged through LDS)
 *          w_layout 1: FRAGMENT-major, read straight into registers one K step ahead (K step = BK = 64 channels, pairs 32, of one tap;
 *            steps ordered channel slice outermost, taps innermost):
 *            [Cout/128][Cin/BK * kd*9 steps][BK/16 ks][planes][4 groups j][64 lanes][8 values], value e of lane l =
 *            filter (co = 128 tile + 32 j + (l & 31), tap, ci = BK slice + 16 ks + 8 (l >> 5) + e); planes = 1, or 2 (hi, lo) for pairs
 *          Cout % 128 == 0 (fragment-major, 2-D: also Cout = 64, packed as one 128-channel tile whose upper half is zero);
 *          bias [Cout] fp32 or NULL
 *   y = acc_scale * conv(in, W16) + bias  (acc_scale: the filters may carry an exact power-of-two scale that keeps their lo parts
 *       normal; 0 = 1);  relu != 0: y = max(y, 0)
 *   out_full [N][D][H][W][ld_full] = y        element type full_type: 0 = not written, 1 = the 16-bit type (modes 1 / 2), 2 = fp32,
 *                                             3 = fp16 pairs [pixel][2][Cout] (mode 3; ld_full >= 2 Cout)
 *   out_pool [N][H/2][W/2][ld_pool] = maxpool2x2(y) (2-D only, H and W even)     element type pool_type, same coding
 *   stats (optional) [groups][Cout][2] fp64, zeroed by the caller: sum and sum of squares of y (fp32 values, before rounding) per
 *        (image group, channel) are ADDED; group of a pixel = (its index in [N][D][H][W]) / stat_rows_per_group (0 = one group).
 *        A 128-pixel tile is summed under ONE group, so groups are whole tiles; on the halo-patch kernel (fragment-major 2-D layers) whole
 *        images do, and where a tile holds several small images (8 x 8: two) a group may also be whole 64-pixel epilogue passes of the
 *        tile — one 8 x 8 image per group.  Groups smaller than a pass, or not aligned to one, are rejected (G6D_EINVAL)
 * Up to 4 map sizes per launch (the scales of the detector's pyramid) like g6d_wino_conv3x3_multi; all segments share D and the
 * kinds of output.  No workspace: the K loop is never split.  Cin, Cout >= 1; W16 16-byte aligned (g6d_corr16_multi too); ld_in, ld_full,
 * ld_pool multiples of 8 elements. */
typedef struct G6dConv16Seg {
  const void* in;
  void* out_full;
  void* out_pool;
  int32_t N, D, H, W, ld_in, ld_full, ld_pool;
} G6dConv16Seg;
int g6d_conv16_direct_multi(const G6dConv16Seg* segs, int nseg, int Cin, const void* W16, int w_layout, float acc_scale, const float* bias,
                            int Cout, int kd, int relu, int full_type, int pool_type, int math_mode, double* stats, int stat_rows_per_group,
                            g6d_stream_t stream);

/* The selector's query x reference product (network/selector.py:183-186) in the 16-bit activation format of g6d_conv16_direct_multi (ABI v12;
 * this and the other *_split16 hand-over passes: csrc/split16.hip, the formats: csrc/pair16.h):
 * out[(q D + d) P + px][plane][c] = split16((ref[d][px][c] * que[q][px][c]) * scale[q][c] + shift[q][c]); ref [D][P][C], que [qn][P][C], scale /
 * shift [qn][C] fp32; out 16-bit: [qn D P][C] for math_mode 1 (bf16) / 2 (fp16), [qn D P][2][C] fp16 hi / lo pairs for math_mode 3.  C % 8 == 0. */
int g6d_product_split16(const float* ref, const float* que, const float* scale, const float* shift, void* out, int qn, int D, int P, int C,
                        int math_mode, g6d_stream_t stream);

/* g6d_affine_act_pool (pool 0 / 1) with the result in the 16-bit activation format of g6d_conv16_direct_multi (ABI v12): [N][Ho][Wo][C] for
 * math_mode 1 (bf16) / 2 (fp16), [N][Ho][Wo][2][C] fp16 hi / lo pairs for math_mode 3 — the InstanceNorm affine + ReLU (+ 2x2 max-pool) between two
 * convs of the selector's stacks (network/selector.py:27-77) as a pass of its own, so that the next conv runs on the direct 16-bit kernel. */
int g6d_affine_split16(const float* in, int ld_in, const float* scale, const float* shift, int affine_per_n, int relu, int pool, int N, int H, int W,
                       int C, void* out, int math_mode, g6d_stream_t stream);

/* The detector's K x K correlation (network/detector.py:188-197,222-224: query feature map x the 32 reference-centre features) on 16-bit
 * activations, halo-patch kernel with the K^2 taps of a slice split over the eleven computing waves of a block (ABI v12;
 * csrc/corr16.hip, corr16_kernel).  segs[i]: in = [N][H][W][ld_in] of the mode's 16-bit type (mode 3: [pixel][2][Cin] fp16 hi / lo pairs), out_full = fp32
 * [N][H][W][ld_full] (ld_full >= 32), D = 1; out = acc_scale * sum_{ky,kx,c} in[y + ky - K/2][x + kx - K/2][c] * w[r][ky K + kx][c] with zero
 * padding.  W16 (host: ops.corr16_pack): [Cin / S][K K][2][64 lanes][8 values] 16-bit — S = 32 channels per slice and fragment f = the
 * slice's 16-channel group (modes 1 / 2), or S = 16 and f = hi / lo plane (mode 3); lane l of a fragment holds reference r = l & 31,
 * channels S c + (16 f for modes 1 / 2) + 8 (l >> 5) + e.  Cout = 32, k in {7, 15}, Cin % 32 == 0, up to 4 map sizes per launch. */
int g6d_corr16_multi(const G6dConv16Seg* segs, int nseg, int Cin, const void* W16, float acc_scale, int Cout, int k, int math_mode,
                     g6d_stream_t stream);

/* Range control of fp16 hi / lo PAIR maps (the math_mode 3 activations above; additive to ABI v12).  A pair map may hold v * 2^-e instead
 * of v: its exponent e sits in a small DEVICE table `exps` (int32, one slot per pair-producing call site of a network), so a captured graph
 * stays valid when the host rewrites an exponent between calls.  NULL range pointer (or the entry points without _ex) = today's unscaled maps.
 *   exps      NULL = every exponent 0
 *   rec       NULL = no record; else rec[slot_out] = max(rec[slot_out], max over the stored UNSCALED values v of bits(|v|)) — an integer
 *             max of the IEEE bits, so NaN > inf > every finite value (at most one atomicMax per wave; clear it with g6d_zero_bytes)
 *   slot_in   pair input read with exponent exps[slot_in] (the consumer multiplies its accumulator scale by 2^e_in); < 0 = exponent 0
 *   slot_out  pair outputs written as split16(v * 2^-exps[slot_out]) and recorded in rec[slot_out]; < 0 = unscaled, not recorded
 * Only the 16-bit pair outputs carry the exponent: fp32 outputs and fp64 statistics stay unscaled. */
typedef struct G6dRange16 {
  const int32_t* exps;
  uint32_t* rec;
  int32_t slot_in, slot_out;
} G6dRange16;
int g6d_conv16_direct_multi_ex(const G6dConv16Seg* segs, int nseg, int Cin, const void* W16, int w_layout, float acc_scale, const float* bias,
                               int Cout, int kd, int relu, int full_type, int pool_type, int math_mode, double* stats, int stat_rows_per_group,
                               const G6dRange16* range, g6d_stream_t stream);
/* The validation and kernel choice of g6d_conv16_direct_multi_ex WITHOUT a launch (no pointer is dereferenced, no HIP call): G6D_EINVAL with
 * the launch's message, else 0 = the per-tap kernels, 1 = the halo-patch kernel (statistics, if any, one group per tile), 2 = the halo-patch
 * kernel with statistics groups of whole epilogue passes inside a tile of several small images. */
int g6d_conv16_direct_plan(const G6dConv16Seg* segs, int nseg, int Cin, const void* W16, int w_layout, int Cout, int kd, int full_type, int pool_type,
                           int math_mode, double* stats, int stat_rows_per_group);
/* The whole choice behind g6d_conv16_direct_plan's answer (additive to ABI v12; launches nothing, reads no operand, and is the launcher's
   own decision code under the current knobs, not a restatement of it).  Returns G6D_OK, or G6D_EINVAL with the launch's message (the
   fields are then not meaningful).  tests/conv16_sweep.py files its cases by it. */
typedef struct G6dConv16Route {
  int32_t kernel;          /* g6d_conv16_direct_plan's answer: 0 per-tap kernels, 1 halo-patch kernel, 2 halo-patch with per-pass statistics */
  int32_t w_layout, math_mode, kd;     /* as passed */
  int32_t wm;              /* pixel tiles per block: 1 or 2 (per-tap kernels: 1) */
  int32_t half_tile;       /* 1: Cout = 64 packed as half of a 128-channel tile */
  int32_t folded;          /* 1: depth-folded 3x3x3 layer (w_layout 2) */
  int32_t tiles, nN, blocks;           /* 128-pixel tiles of the launch, channel blocks, blocks of the grid */
  struct {
    int32_t tile0;         /* first tile of the segment */
    int32_t tw_log2, tiles_x;          /* tile width and tiles per map row (halo-patch: c16g::halo_tiling's; per-tap: c16g::pick_tw's) */
    int32_t tpi;           /* halo-patch: tiles per image, 0 = banded tiles of whole small images; per-tap: 0 */
    int32_t segh_log2, bands;          /* halo-patch: rows per band and bands per tile (1 = tiles inside one image); per-tap: 0 */
  } seg[4];                /* segments past nseg: zeros */
} G6dConv16Route;
int g6d_conv16_direct_route(const G6dConv16Seg* segs, int nseg, int Cin, const void* W16, int w_layout, int Cout, int kd, int full_type, int pool_type,
                            int math_mode, double* stats, int stat_rows_per_group, G6dConv16Route* route);
int g6d_sizeof_conv16_route(void);
int g6d_corr16_multi_ex(const G6dConv16Seg* segs, int nseg, int Cin, const void* W16, float acc_scale, int Cout, int k, int math_mode,
                        const G6dRange16* range, g6d_stream_t stream);
int g6d_product_split16_ex(const float* ref, const float* que, const float* scale, const float* shift, void* out, int qn, int D, int P, int C,
                           int math_mode, const G6dRange16* range, g6d_stream_t stream);
int g6d_affine_split16_ex(const float* in, int ld_in, const float* scale, const float* shift, int affine_per_n, int relu, int pool, int N, int H,
                          int W, int C, void* out, int math_mode, const G6dRange16* range, g6d_stream_t stream);
int g6d_vgg_conv1_pool_nhwc16_ex(const float* in, int N, int H, int W, const float* w_oihw, const float* bias, int Cin, int Cout,
                                 const float* mean_host, const float* std_host, void* out16, int math_mode, const G6dRange16* range,
                                 g6d_stream_t stream);

/* Hand-over passes of the refiner's 2-D feature net to g6d_conv16_direct_multi (network/refiner.py:64-78; additive to ABI v12).  Their
 * output may be a CHANNEL SLICE of wider 16-bit rows — the three branches of the feature net write one `cat` map: `out` points at pixel 0 of
 * rows of ld_out 16-bit elements, the slice is channels [c_off, c_off + C), and for math_mode 3 the lo plane lies `plane` elements after the
 * hi plane (a dense pair map [pixel][2][C]: ld_out = 2 C, plane = C, c_off = 0; modes 1 / 2: one plane, `plane` is not read).  ld_out, plane
 * and c_off are multiples of 8; nothing else of a row is touched.  Slices of one map must be written with ONE slot_out.
 *   g6d_affine_split16_to          g6d_affine_split16_ex with such an output (the dense entry calls it)
 *   g6d_upsample_bilinear_split16  g6d_upsample_bilinear (x factor, the per-image affine applied to the four neighbours, same arithmetic)
 *   g6d_l2norm_split16             g6d_l2norm_rows (F.normalize over C, same arithmetic) of an fp32 tap in[rows][ld_in], C = 256 or 512,
 *                                  written as a dense 16-bit map instead of in place: [rows][C], or [rows][2][C] pairs */
int g6d_affine_split16_to(const float* in, int ld_in, const float* scale, const float* shift, int affine_per_n, int relu, int pool, int N, int H,
                          int W, int C, void* out, int ld_out, int plane, int c_off, int math_mode, const G6dRange16* range, g6d_stream_t stream);
int g6d_upsample_bilinear_split16(const float* in, int ld_in, const float* scale, const float* shift, int affine_per_n, int N, int H, int W, int C,
                                  int factor, void* out, int ld_out, int plane, int c_off, int math_mode, const G6dRange16* range,
                                  g6d_stream_t stream);
int g6d_l2norm_split16(const float* in, int ld_in, int rows, int C, void* out, int math_mode, const G6dRange16* range, g6d_stream_t stream);

/* g6d_wino_conv3x3_multi on the Winograd F(4x4,3x3) kernel (ABI v8, fp32 on v_mfma_f32_16x16x4_f32): 36 multiplications per 16
 * outputs — 4x fewer than the direct form, 1.78x fewer than F(2x2,3x3) — with the interpolation points (0, +-3/4, +-3/2, inf), whose
 * fp32 error is ~1.3e-6 of the output range at Cin = 512 (F(2x2,3x3): 2.5e-7; the textbook points 0, +-1, +-2: 4.6e-6).  Meant for the
 * layers whose parity budget has that room: the detector's image pyramid (network/pretrain_models.py:17-25, network/detector.py:188-197,
 * 236-241; headline detector parity 1.5e-6 of range against a 1e-4 bar).
 * U43 = the filters transformed on the host in fp64, [Cin/8][2][Cout/CB][18][CB/32][4][16][4] (CB = 64; 32 when Cout % 64):
 * U43[c][b / 3][blk][3a + b % 3][np][kg][lt][2 par + s] = (G g G^T)[a][b] of filter (co = CB blk + 32 np + 16 par + lt, ci = 8c + 2kg + s),
 * (a, b) = position in the 6x6 transform domain.  Per chunk of 8 input channels the two column halves (b < 3, b >= 3) are the units
 * the kernel stages in LDS: each half of a CB-channel block is one contiguous run (18 CB/32 KB) in the order of its LDS image, of which
 * lane (kg, lt) reads the 16 bytes [position][np][kg][lt] — its B operands for two 16-channel tiles.  Cin % 8 == 0, Cout % 64 == 0;
 * segments, bias, relu, outputs and workspace as g6d_wino_conv3x3_multi. */
int g6d_wino43_conv3x3_multi(const G6dWinoSeg* segs, int nseg, int Cin, const float* U43, const float* bias, int Cout, int relu,
                             float* workspace, size_t workspace_bytes, g6d_stream_t stream);

/* What the host chooses for a launch of one of the Winograd entry points under the current knobs (additive to ABI v12; launches nothing,
   reads no operand, makes no HIP call, and is the launchers' own validation and decision code, not a restatement of it): the entry's
   argument checks, the segment table, the plan (block form, split of the chunk list), the kernel instantiation and, for F(4x4,3x3), the
   block-id decode.  Returns G6D_OK, or G6D_EINVAL with the launch's message where the launch would be refused (the fields are then not
   meaningful).  `entry` says which launch is meant and how `segs` is read:
     0  g6d_wino_conv3x3_multi     G6dWinoSeg rows      3  g6d_wino43_conv3x3_multi   G6dWinoSeg rows
     1  g6d_wino_conv3x3           ONE G6dWinoSeg row    4  g6d_corr2d_wino_multi      G6dCorrSeg rows
        holding its scalar arguments (nseg = 1)          5  g6d_corr2d_wino43_multi    G6dCorrSeg rows
     2  g6d_wino16_conv3x3_multi   G6dWinoSeg rows
   U: the launch's filter pointer (only its value is checked); kblocks: entries 4 and 5, else 0; math_mode: entry 2, else 0; workspace,
   workspace_bytes: as handed to the launch.  tests/wino_sweep.py files its cases by it. */
typedef struct G6dWinoRoute {
  int32_t entry;           /* as passed */
  int32_t family;          /* the kernel: 0 F(2x2,3x3) fp32, 1 16-bit operands with one wave per SIMD, 2 16-bit operands with two waves per SIMD
                              (un-split trunk launches, knob wino16_2w), 3 F(4x4,3x3) */
  int32_t kd;              /* sub-filter blocks accumulated in the transform domain: 1, or kblocks^2 = 25 / 9 */
  int32_t wide;            /* family 0: 1 = blocks of two quarters x 128 channels (knob wino_wide); otherwise 0 */
  int32_t nq;              /* quarters (8x8 output pixels) of the flat list per block: 4, 2 (wide) or 8 (family 3) */
  int32_t nwn;             /* channel width of a block: families 0 - 2 in 32s (1, 2 or 4), family 3 in 16s (nt = 2 or 4) */
  int64_t grid2;           /* blocks x channel slices: the tile counters a split launch uses */
  int32_t blocks;          /* blocks over the quarter list */
  int32_t nchunks;         /* kd x input-channel chunks (8 channels; 16 for families 1 and 2) */
  int32_t splits;          /* parts of the chunk list = gridDim.z (1: no split) */
  int32_t chunks_per_split;       /* chunks of every part but the last, which has nchunks - (splits - 1) * chunks_per_split */
  int32_t map_mode;        /* family 3: the block-id decode that runs (knob w43_map; 0 whenever there is one channel slice); otherwise 0 */
  int32_t lds_bytes;       /* dynamic LDS asked for */
  struct { int32_t qstart, QH, QW; } seg[4];      /* first quarter of the segment in the flat list, quarters per map column / row;
                                                     segments past nseg: zeros */
} G6dWinoRoute;
int g6d_wino_multi_route(int entry, const void* segs, int nseg, int Cin, const void* U, int Cout, int kblocks, int math_mode,
                         const float* workspace, size_t workspace_bytes, G6dWinoRoute* route);
int g6d_sizeof_wino_route(void);

/* In-place L2 normalisation over C of channels-last rows x[rows][ld] (F.normalize eps 1e-12, network/selector.py:118,
 * network/refiner.py:69-71,165).  16-byte accesses when x is 16-byte aligned and ld % 4 == 0 (then C % 4 == 0 is required),
 * scalar accesses otherwise (the [qn][7] rows of the regressor output).  ld >= C, rows <= 2^31 - 4. */
int g6d_l2norm_rows(float* x, int rows, int C, int ld, g6d_stream_t stream);

/* NCHW (backbone output) -> channels-last, optionally L2-normalised over C (F.normalize eps 1e-12,
 * network/selector.py:118, network/refiner.py:69-71). out [N][H][W][ld_out], ld_out >= C; with l2norm C and ld_out are multiples of 4 and
 * out is 16-byte aligned; H * W <= 2^31 - 64, C <= 2^31 - 64, N * H * W <= 2^31 - 4 (grids of rounded-up counts). */
int g6d_nchw_to_nhwc(const float* in, int N, int C, int H, int W, int l2norm, float* out, int ld_out, g6d_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Selector similarity (network/selector.py:183-186,192-195 and the InstanceNorm3d(512) at :28,49,63).  The
 * query x reference product [C][D][HW] is never materialised.
 *   que   [HW][C]            L2-normalised query features (channels-last)
 *   refs  [D][HW][C]         reference cache, D = rfn*an with d = r*an + a
 * g6d_selector_ref_sums   (load time)  r1[hw][c] = sum_d refs, r2[hw][c] = sum_d refs^2      (fp64)
 * g6d_selector_prod_affine(query time) InstanceNorm affine of the product from r1/r2:
 *                                      mean_c = sum_hw q r1 / (D*HW), E[x^2]_c = sum_hw q^2 r2 / (D*HW)
 *                                      scale = 1/sqrt(var+eps), shift = -mean*scale           (exact algebra)
 * g6d_selector_scan       (query time) one coalesced streaming pass over refs, wavefront shuffle reductions:
 *                                      score_map[d][hw] = sum_c que*ref ;  vps[d] = sum_hw S^2 / max_hw S
 * ---------------------------------------------------------------------------------------------------------------- */
/* D, HW, C >= 1.  g6d_selector_ref_sums: HW * C <= 2^31 - 256 (the grid is formed as (HW * C + 255) / 256 in int).  g6d_selector_scan: C % 4 == 0, que and refs 16-byte aligned, D * HW <= 2^30. */
int g6d_selector_ref_sums(const float* refs, int D, int HW, int C, double* r1, double* r2, g6d_stream_t stream);
int g6d_selector_prod_affine(const float* que, const double* r1, const double* r2, int D, int HW, int C, double eps,
                             float* scale, float* shift, g6d_stream_t stream);
int g6d_selector_scan(const float* que, const float* refs, int D, int HW, int C, float* score_map, float* vps,
                      g6d_stream_t stream);
/* g6d_selector_scan + g6d_selector_prod_affine for all (<= 3) pyramid levels of a BATCH of qn <= 8 queries in ONE launch (+ a tiny
 * reduction launch): the reference cache is streamed once per batch.  Per level l: que[l] [qn][HW_l][C], refs[l] [D][HW_l][C],
 * r1[l] / r2[l] [HW_l][C], HW[l] <= 1024, score_maps[l] [qn][D][HW_l] (written; required); vps [qn][nlev][D], scale / shift
 * [qn][nlev][C]; Dg = global hypothesis count of the InstanceNorm statistics (= D unless the references are sharded over ranks). */
int g6d_selector_levels(int nlev, int qn, const float* const* que, const float* const* refs, const double* const* r1,
                        const double* const* r2, const int* HW, int D, int Dg, int C, double eps, float* const* score_maps,
                        float* vps, float* scale, float* shift, g6d_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Refiner feature-volume construction (network/refiner.py:183-206,208-247; network/operator.py:4-17), fused:
 * rotate the sn^3 grid by R_in, project every voxel into each reference view and the query view, bilinear-sample
 * (zeros padding, align_corners=False, coordinates normalised with the INPUT IMAGE size h_in x w_in), and reduce over
 * the references in registers (mean, unbiased std).  All pointers are device pointers.
 *   feats     [rfn+1][fh][fw][C]  channels-last feature maps; view rfn is the query
 *   projs     [rfn+1][12]         row-major 3x4 K*[R|t] per view (query last)
 *   rot_in    [9]                 row-major R_in (grid row-vector v is mapped to v @ R_in)
 *   lin       [sn]                torch.linspace(-1,1,sn)
 *   mean_in   [sn^3][2C]          cat[mean over refs, query sample]   (input of mean_embed)
 *   std       [sn^3][C]           1 <= rfn <= 8
 * fh * fw * C <= 2^31 - 1 (the tap offsets inside a view are ints).
 * C is any positive multiple of 4 (also below 4 * (rfn + 1) and off the 128-channel trips of a half-wave: every lane walks every
 * trip, lanes beyond C store nothing); fh, fw, h_in, w_in > 0, sn <= 256.  Anything else is refused with G6D_EINVAL.
 * ---------------------------------------------------------------------------------------------------------------- */
int g6d_refiner_volume(const float* feats, const float* projs, const float* rot_in, const float* lin, int rfn, int fh,
                       int fw, int C, int h_in, int w_in, int sn, float* mean_in, float* std, g6d_stream_t stream);
/* The same with intrinsics and poses given separately (ref_Ks [rfn][3][3], ref_poses [rfn][3][4], K_in [3][3], pose_in [3][4]):
 * the projections K @ pose of network/refiner.py:208-226 are formed inside the kernel and the rotation is read from pose_in.
 * batch >= 1 queries in one launch (the reference's forward takes [qn,...], refiner.py:249-269): every operand and both outputs
 * carry a leading [batch] axis (feats [batch][rfn+1][fh][fw][C], ... mean_in [batch][sn^3][2C], std [batch][sn^3][C]). */
int g6d_refiner_volume_kp(const float* feats, const float* ref_Ks, const float* ref_poses, const float* K_in, const float* pose_in,
                          const float* lin, int rfn, int fh, int fw, int C, int h_in, int w_in, int sn, float* mean_in, float* stdv,
                          int batch, g6d_stream_t stream);
/* g6d_refiner_volume_kp with both volumes written as fp16 hi / lo PAIR maps in the activation format of g6d_conv16_direct_multi, math_mode 3
 * (additive to ABI v12): mean_in16 [batch][sn^3][2][2C] and std16 [batch][sn^3][2][C] fp16 — per voxel the hi plane, then the lo plane; the
 * same gathers and arithmetic as the fp32 entry and the same number of bytes written.  Each map has its own exponent slot and range record
 * (range_mean / range_std: slot_out; NULL = unscaled and not recorded), the protocol of the elementwise pair producers above. */
int g6d_refiner_volume_kp_pairs(const float* feats, const float* ref_Ks, const float* ref_poses, const float* K_in, const float* pose_in,
                                const float* lin, int rfn, int fh, int fw, int C, int h_in, int w_in, int sn, void* mean_in16, void* std16,
                                int batch, const G6dRange16* range_mean, const G6dRange16* range_std, g6d_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Detector score assembly (network/detector.py:225-229,243-245,207-216): for one detection scale, take the three raw
 * correlation maps (level l at 1/(8*2^l) resolution, channels-last [h_l*w_l][rfn]), nearest-upsample levels 1,2 to
 * level-0 size, normalise ((x-mu_l)/sigma_l), clip to +-clip, bilinear-resize (align_corners=False) to (hs,ws) and
 * write channels [3*scale_idx .. 3*scale_idx+2] of stacked [hs*ws][rfn][nch].  batch >= 1 queries (network/detector.py:291-304
 * takes [qn,H,W,3]): s_l [batch][h_l*w_l][rfn], stacked [batch][hs*ws][rfn][nch].  hc, wc multiples of 4; hs, ws > 0; 0 <= scale_idx and
 * 3 * scale_idx + 3 <= nch; batch <= 65535; hs * ws <= 2^31 - 1 (the kernel's pixel index is an int) and ceil(hs * ws * rfn / 256) <= 2^31 - 1
 * (one grid).
 * ---------------------------------------------------------------------------------------------------------------- */
int g6d_detector_assemble(const float* s0, const float* s1, const float* s2, int hc, int wc, int rfn,
                          const float* mu_sigma /* HOST pointer: {mu0,sigma0,mu1,sigma1,mu2,sigma2} */, float clip, int hs, int ws,
                          int scale_idx, int nch, float* stacked, int batch, g6d_stream_t stream);

/* score_conv + max over references (network/detector.py:159-163,246-247): per (pixel, ref) MLP nch->64 (ReLU) ->64,
 * then max over rfn.  w0 [64][nch], b0[64], w1[64][64], b1[64]; out [P][64].  rfn <= 256, nch == 12, P <= 2^31 - 256. */
int g6d_detector_score_mlp_max(const float* stacked, int P, int rfn, int nch, const float* w0, const float* b0,
                               const float* w1, const float* b1, float* out, g6d_stream_t stream);

/* arg-max + decode (network/detector.py:84-121): scores [hs*ws], offset [hs*ws][2], scale [hs*ws] (channels-last);
 * result[0..1] = position (x,y) px, result[2] = 2^scale, result[3..4] = (x,y) cell of the peak (as float).
 * batch >= 1 queries: the maps of query b start b*hs*ws rows after those of query 0, result [batch][5].  Row strides in floats: ld_s >= 1,
 * ld_o >= 2, ld_c >= 1 (three dense maps of their own: 1, 2, 1); hs * ws <= 2^31 - 1. */
int g6d_detector_decode(const float* scores, int ld_s, const float* offset, int ld_o, const float* scale, int ld_c,
                        int hs, int ws, int pool_ratio, float* result, int batch, g6d_stream_t stream);
/* (ABI v10) The detector's image pyramid in one launch: F.interpolate(que_imgs, size=(h_k, w_k), mode='bilinear') (align_corners False;
 * network/detector.py:236-241) of src [planes = N*3][H][W] for up to 4 destination sizes -> dsts[k] [planes][hs[k]][ws[k]] (dense).
 * Source index as ATen: scale = in / out, src = scale * (dst + 0.5) - 0.5 clamped at 0. */
int g6d_resize_bilinear_pyramid(const float* src, int planes, int H, int W, int nscale, const int* hs, const int* ws,
                                float* const* dsts, g6d_stream_t stream);
/* (ABI v10) Stream-ordered zero fill of `bytes` bytes of device memory at a 16-byte aligned address (an own kernel: the runtime's memset node
 * lost writes inside captured graphs). */
int g6d_zero_bytes(void* ptr, size_t bytes, g6d_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Selector tail helpers (network/selector.py:201-214, network/attention.py:4-17,50-68).
 * ---------------------------------------------------------------------------------------------------------------- */
/* The tail helpers take `batch` >= 1 queries (selector.py:165-175 takes [qn,...]): row blocks of the queries follow each other.
 * InstanceNorm2d(3) of vps [batch][3][D] over D, written to channels c_off..c_off+2 of feats [batch*D][ld] (selector.py:201-202);
 * c_off >= 0, c_off + 3 <= ld, batch <= 65535 */
int g6d_vps_norm(const float* vps, int D, float* feats, int ld, int c_off, int batch, g6d_stream_t stream);
/* x[b*rfn+r][c] = max_a in[(b*rfn+r)*an+a][c] + embed[r][c]   (selector.py:204-205); ld_in >= C, ld_out >= C, batch <= 65535,
 * rfn * C <= 2^31 - 256, rfn * an <= 2^31 - 1 */
int g6d_max_an_add(const float* in, int ld_in, int rfn, int an, int C, const float* embed, float* out, int ld_out, int batch,
                   g6d_stream_t stream);
/* multi-head attention over n tokens with the reference's head split c -> (d=c/heads, head=c%heads), scale
 * 1/sqrt(C/heads): q,k,v [batch*n][ld] -> out [batch*n][ld_out] (ld >= C, ld_out >= C), attention among the n tokens of one
 * query (attention.py:4-17,60-64) */
int g6d_attention(const float* q, const float* k, const float* v, int ld, int n, int C, int heads, float* out,
                  int ld_out, int batch, g6d_stream_t stream);
/* LayerNorm over C per token with affine (attention.py:19-26): out may alias in; ld_in >= C, ld_out >= C */
int g6d_layernorm(const float* in, int ld_in, int n, int C, const float* gamma, const float* beta, float eps,
                  float* out, int ld_out, g6d_stream_t stream);
/* out = relu?(x*scale+shift) (+ residual) elementwise on [n][C] rows (selector.py:209); rows_per_group = k > 0: row r uses
 * table r / k of scale / shift [n/k][C] (one InstanceNorm1d per query of a batch), 0: one table.  scale and shift both or neither;
 * ld_in >= C, ld_out >= C, ld_res >= C when residual is given (not read otherwise); n * C <= 2^31 - 256 */
int g6d_affine_act_add(const float* in, int ld_in, const float* scale, const float* shift, int relu,
                       const float* residual, int ld_res, int n, int C, float* out, int ld_out, int rows_per_group,
                       g6d_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Inter-stage image warps of Gen6DEstimator.predict: cv2.warpAffine in transformation_crop
 * (utils/base_utils.py:646-655), cv2.warpPerspective in look_at_crop / normalize_reference_views
 * (utils/database_utils.py:8-25,54-110) and the rotated reference copies (estimator.py:150-164).
 * src uint8 [sh][sw][ch] (device); hinv: HOST pointer, row-major 3x3 destination->source pixel map (inverse of the
 * cv2 `M`/`H`); dst [dh][dw][ch] uint8 (out_float=0, round-to-nearest) or float32 * out_scale (out_float=1).
 * Bilinear, zero outside the source.  Exact float weights: cv2 quantises them to 1/32 px (<= 1-2 grey levels apart).
 * 1 <= ch <= 4; dh * dw <= 2^31 - 256 (g6d_warp_batch too).
 * ---------------------------------------------------------------------------------------------------------------- */
int g6d_warp_perspective(const unsigned char* src, int sh, int sw, int ch, const float* hinv, void* dst, int dh, int dw,
                         int out_float, float out_scale, g6d_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Device-resident inter-stage glue: what Gen6DEstimator.predict computes on the HOST between the
 * network calls, as single-launch kernels on device buffers (float32 in memory, float64 arithmetic), so that
 * detect -> crop -> select -> pose -> 3 x refine is one chain of launches without host synchronisation (hipGraph-capturable).
 * All pointers are DEVICE pointers.  3x3 matrices are row-major [9], poses row-major [3][4] = [12].
 * Every kernel takes a `batch` of queries (round 3): per-query operands and results are dense arrays with the query as leading axis
 * (det [batch][5], logits / angles [batch][rfn], que_K [batch][9], poses [batch][12], geo [batch][42+30*ref_num], ...); the reference
 * state (ref_poses, ref_Ks, center, norm, sub_poses, sub_Ks) is shared by the queries.
 * ---------------------------------------------------------------------------------------------------------------- */
/* det = result of g6d_detector_decode (x, y, 2^scale, ...) -> hinv[9]: destination->source map of
 * transformation_crop(que_img, position, 1/scale_r2q, 0, size) (estimator.py:184, utils/base_utils.py:646-655) */
int g6d_chain_crop_from_detection(const float* det, float size, float* hinv, int batch, g6d_stream_t stream);
/* arg-max viewpoint (first maximum) + estimate_pose_from_similarity_transform_compose (estimator.py:193-206,
 * utils/pose_utils.py:12-49,104-111): logits/angles [rfn], ref_poses [rfn][12], ref_Ks [rfn][9] -> pose_out[12],
 * sel_out[2] = (selected reference index, its in-plane angle) */
int g6d_chain_pose_from_selection(const float* det, const float* logits, const float* angles, int rfn, const float* ref_poses,
                                  const float* ref_Ks, const float* que_K, const float* center, float* pose_out, float* sel_out,
                                  int batch, g6d_stream_t stream);
/* Geometry of one refinement step before the network (network/refiner.py:275-313, utils/database_utils.py:54-139 on the
 * NormalizedDatabase): pose_in[12] in the database frame, que_K[9], norm[4] = (NormalizedDatabase.scale, offset xyz),
 * sub_poses [n_sub][12] / sub_Ks [n_sub][9] = normalised poses and intrinsics of the (FPS) reference subset, n_sub <= 128.
 * Writes ref_idx[ref_num] (the views most aligned with the warped input pose) and the record
 *   geo = K_warp[9] | pose_warp[12] | pose_rect[12] | ref_Ks[ref_num][9] | ref_poses[ref_num][12] | hinv[1+ref_num][9]
 * (42 + 30*ref_num floats; hinv[0] warps the query, hinv[1+k] reference k: inputs of g6d_warp_batch).
 * angle_step > 0 (radians; reference-feature caching): the in-plane alignment angle of every reference view is
 * snapped to multiples of angle_step, so that its aligned crop depends on (view, bucket) only; ref_bucket[ref_num] (optional)
 * receives round(angle / angle_step).  angle_step = 0: the reference's exact alignment. */
int g6d_chain_refine_prepare(const float* pose_in, const float* que_K, const float* norm, float size, float margin,
                             const float* sub_poses, const float* sub_Ks, int n_sub, int ref_num, float* geo, int* ref_idx,
                             float angle_step, int* ref_bucket, int batch, g6d_stream_t stream);
/* Refiner outputs (rotation[4] w-first, offset[2], log2 scale[1]) + the step's geo record -> refined pose in the database frame
 * (refiner.py:327-341: compose_sim_pose, pose_sim_to_pose_rigid with the polar factor of the SVD, un-rectify, denormalise). */
int g6d_chain_refine_update(const float* rot, const float* off, const float* scl, const float* geo, int geo_floats /* per query */,
                            const float* norm, float* pose_out, int batch, g6d_stream_t stream);
/* Batched g6d_warp_perspective with homographies and source selection in device memory, output in the layout the networks
 * take: dst [B][ch][dh][dw] float = rint(bilinear)/255 (the uint8 image cv2.warpPerspective would return, scaled to [0,1]);
 * image b reads `single` when idx == NULL or idx[b] < 0, else stack[idx[b]] (uint8 [.][sh][sw][ch]); hinv [B][9]. */
int g6d_warp_batch(const unsigned char* stack, const unsigned char* single, const int* idx, int B, int sh, int sw, int ch,
                   const float* hinv, float* dst, int dh, int dw, g6d_stream_t stream);

/* Small-batch linear layer, weight-streaming GEMV (network/refiner.py:153-166): out[b][o] = act(W[o].x[b] + bias[o]);
 * W [O][K] row-major, x [B][K], B <= 8; act as G6dConv.out_act (0, 1 or 2).  K % 4 == 0; x and W 16-byte aligned (g6d_linear_gemv_batch
 * too). */
int g6d_linear_gemv(const float* x, int B, int K, const float* W, const float* bias, int O, int act, float* out,
                    g6d_stream_t stream);

/* (ABI v9) The same layer for ANY number of right-hand sides (network/refiner.py:249-269 takes [qn, ...] queries).  Since v10 ONE pass over
 * the weights serves up to 32 rows of x: groups of 2..16 with O % 8 == 0 and K % 2048 == 0 run 8 output rows x one 2048-float K slice per
 * block with one or two groups of 8 rows of x against the block's weight values; groups of 17..32 with O % 32 == 0 and K % 1024 == 0 run
 * as a GEMM on the matrix cores (32 weight rows x 256 k per wave).  Partial sums are joined in slice order through `workspace`
 * (G6D_WORKSPACE_COUNTER_BYTES of counters, zero at rest, then <= O * K / 32 floats); anything else takes the row-per-block kernel of
 * g6d_linear_gemv. */
int g6d_linear_gemv_batch(const float* x, int B, int K, const float* W, const float* bias, int O, int act, float* out, float* workspace,
                          size_t workspace_bytes, g6d_stream_t stream);

/* Multi-stream tracking (gen6d_amd/tracking.py, reference predict.py:49-72); additive within ABI 12.  Per-stream state lives in tables
 * indexed by stream id: pose_table / smooth_table [streams][12] (last raw / smoothed pose), hist [streams][num][8][2] float64 (ring of
 * the projected box corners), hist_count [streams] (frames since the last reset).  slot_stream [batch]: the stream served by slot b, or
 * -1 for an unused slot; ids must index the tables (the caller checks them).
 * g6d_track_gather: pose_out[b][12] = the stream's last raw pose, or parking_pose[12] for an unused slot (a finite pose that looks at
 * the object, so that the refinement step of an unused slot stays finite and inside the fp16 pair range records). */
int g6d_track_gather(const float* pose_table, const int* slot_stream, const float* parking_pose, float* pose_out, int batch,
                     g6d_stream_t stream);
/* g6d_track_commit, one 64-thread block per used slot: pose [batch][12] (refined, unsmoothed), K [batch][9], box [8][3] (corner order
 * of the reference's pts_range_to_bbox_pts).  Writes the raw pose into the stream's table row, projects the box under it and pushes the
 * corners into the stream's ring (reset != 0: the count restarts first), averages the last min(count, num) frames with weights
 * exp(-(i/std)^2) (i = frames older than the newest), solves PnP on the averaged corners by Levenberg-Marquardt on (Rodrigues vector, t)
 * from the raw pose (<= 20 iterations), and writes the smoothed pose into smooth_table and out[b] = raw[12] | smoothed[12].
 * Unused slots write nothing.  1 <= num <= G6D_TRACK_MAX_NUM, std > 0. */
#define G6D_TRACK_MAX_NUM 64
int g6d_track_commit(const float* pose, const float* K, const int* slot_stream, int reset, const float* box, int num, float std,
                     float* pose_table, double* hist, int* hist_count, float* smooth_table, float* out, int batch, g6d_stream_t stream);

/* Track health (gen6d_amd/tracking.py HealthPolicy; the reference's predict.py loop has no counterpart: it feeds every
 * frame's pose into the next frame unconditionally); additive within ABI 12.  Two more per-stream tables: health [streams][4] int32 =
 * (status, bad, vbad, flags) and measures [streams][12] float32 = (u, v, z, d_px, rot_deg, shift, log2_scale, verify_shift,
 * verify_log2_scale, 0, 0, 0), the measures of the last evaluated candidate pose.  One thread per slot, float64 on the float32 inputs;
 * every comparison is !(x <= thr): a NaN fails, an infinite threshold disables its gate.  The policy travels by value, so a captured
 * graph holds it.
 * g6d_track_gate, before the gather: slot_eff[b] = slot_stream[b] when the slot is used, its stream is not LOST and the 12 floats of
 * its pose_table row are finite, else -1 (the gather then parks the slot like an unused one, so nothing non-finite reaches the networks).
 * A non-finite row of a stream that is not LOST sets status = LOST, flags = NONFINITE. */
enum { G6D_TRACK_NONE = 0, G6D_TRACK_TRACKING = 1, G6D_TRACK_SUSPECT = 2, G6D_TRACK_LOST = 3 };
enum { G6D_TRACK_NONFINITE = 1, G6D_TRACK_BEHIND = 2, G6D_TRACK_SMALL = 4, G6D_TRACK_LARGE = 8, G6D_TRACK_OUTSIDE = 16, G6D_TRACK_ROT = 32,
       G6D_TRACK_SHIFT = 64, G6D_TRACK_SCALE = 128, G6D_TRACK_VERIFY_POS = 256, G6D_TRACK_VERIFY_SCALE = 512 };
int g6d_track_gate(const float* pose_table, int32_t* health, const int* slot_stream, int* slot_eff, int batch, g6d_stream_t stream);
/* g6d_track_health, after the refinement and before the commit.  pose_prev [batch][12] (the gathered poses; NULL with reset != 0, an
 * acquisition), pose_new [batch][12], K [batch][9], pic [batch][2] int32 (picture (w, h) per slot; NULL: (W, H)), center [3], diameter
 * (the box diagonal).  Per used slot of slot_eff, with X = R center + t, z = X.z, f = (K00 + K11) / 2, (u, v) = (K X).xy / z,
 * d_px = f diameter / z:
 *   NONFINITE an entry of pose_new is not finite (ends the evaluation, measures 0);  BEHIND !(z > 0) (ends it too, only z is recorded);
 *   SMALL !(d_px >= min_px);  LARGE !(d_px <= max_px max(w, h));  OUTSIDE u outside [-margin d_px, w + margin d_px] or v likewise with h;
 *   without reset: ROT rot_deg = acos(clamp((tr(R_new R_prev^T) - 1) / 2, -1, 1)) 180 / pi, !(rot_deg <= max_rot_deg);
 *   SHIFT shift = hypot(u - u_prev, v - v_prev) / d_px under pose_prev and the same K;  SCALE log2_scale = |log2(z_prev / z)|, which also
 *   fails when !(z_prev > 0) (shift and log2_scale are then 0 and SHIFT is not evaluated).
 * State: NONFINITE or BEHIND -> LOST; any other bit -> bad += 1, LOST if bad >= patience else SUSPECT; no bit -> bad = 0, TRACKING; with
 * reset: any bit -> LOST else TRACKING, bad = vbad = 0.  flags bits 0..7 are replaced, 8..9 kept.  slot_commit[b] = the stream id when
 * the frame passed, slot_draw[b] = the stream id unless the stream is LOST after this frame, else -1 (also for unused slots). */
int g6d_track_health(const float* pose_prev, const float* pose_new, const float* K, const int32_t* pic, int W, int H, const int* slot_eff,
                     int reset, const float* center, double diameter, int patience, double min_px, double max_px, double margin,
                     double max_rot_deg, double max_shift, double max_log2_scale, int32_t* health, float* measures, int* slot_commit,
                     int* slot_draw, int batch, g6d_stream_t stream);
/* g6d_track_verify, the detector's independent check of the slots committed in this tick: det [batch][5] = (x, y, 2^scale, cell) as the
 * chain forms it (det[2] is the reference-to-query size ratio), the stream's committed raw pose from pose_table, ref_px = the object's
 * mean projected diameter over the reference views.  verify_shift = hypot(det.x - u, det.y - v) / d_px, verify_log2_scale =
 * |log2(det[2] ref_px / d_px)|; a failed check sets VERIFY_POS / VERIFY_SCALE and vbad += 1, LOST at vbad >= verify_patience; a passed
 * one clears both bits and vbad.  flags bits 0..7 are kept. */
int g6d_track_verify(const float* det, const float* pose_table, const float* K, const int* slot_commit, const float* center,
                     double diameter, double ref_px, double verify_shift, double verify_log2_scale, int verify_patience, int32_t* health,
                     float* measures, int batch, g6d_stream_t stream);

/* Frame ingest (gen6d_amd/ingest.py; reference prepare.py:16-42 video2image + predict.py:45,52-54); additive within ABI 12.  ONE launch
 * reads n camera-native frames (packed RGB / BGR / RGBA / BGRA or NV12, and the formats after NV12 listed at the enum below; any size, row
 * pitch and quarter-turn rotation), scales each to
 * out_w x out_h with the integer bilinear below, and writes the RGB picture into the top-left corner of image `slot` of
 * out [B][H][W][3] uint8 (canvas pixels outside the picture are written as 0) and the frame's K into K_out [B][3][3].  Slots that no frame
 * names are not touched; a frame whose slot lies outside [0, B) is skipped; two frames must not name the same slot.
 * The table lives in DEVICE memory (it changes with every call, so the launch stays outside captured graphs); the caller validates its
 * contents: planes cover height rows of pitch bytes, 1 <= width, height <= 8192, even sizes for the 4:2:0 formats and an even width for
 * 4:2:2, out_w <= W, out_h <= H.
 * Arithmetic (exact integers, the numpy restatement in tests/test_ingest_cpu.py is bit-identical): with wt x ht the scaled
 * picture before rotation ((out_w, out_h) for rotate 0 / 180, (out_h, out_w) for 90 / 270) and ws x hs the source,
 *   fx = clamp(floor((2x+1) * ws * 1024 / wt) - 1024, 0, (ws-1) * 2048), x0 = fx >> 11, a = fx & 2047, x1 = min(x0+1, ws-1), y likewise (b);
 *   each tap is converted to RGB, then per channel v = ((2048-a)(2048-b) p00 + a(2048-b) p01 + (2048-a) b p10 + a b p11 + 2^21) >> 22;
 *   NV12 tap: chroma UV[y>>1][x>>1], c = max(Y-16, 0), d = U-128, e = V-128, R = sat8((CY c + CVR e + 2^19) >> 20),
 *   G = sat8((CY c - CUG d - CVG e + 2^19) >> 20), B = sat8((CY c + CUB d + 2^19) >> 20) with round(k * 2^20) constants of BT.601 / BT.709
 *   limited range; canvas pixel (X, Y) of a picture turned clockwise by 90 is the unrotated (Y, ht-1-X), 180: (wt-1-X, ht-1-Y),
 *   270: (wt-1-Y, X). */
enum { G6D_FMT_RGB24 = 0, G6D_FMT_BGR24 = 1, G6D_FMT_RGBA32 = 2, G6D_FMT_BGRA32 = 3, G6D_FMT_NV12 = 4,
       /* additive within ABI 12 (the numpy restatement in tests/test_pixel_formats_cpu.py is bit-identical) */
       G6D_FMT_YUYV422 = 5,        /* packed 4:2:2, 2 bytes per pixel, a pair of pixels = Y0 U Y1 V; read and written */
       G6D_FMT_UYVY422 = 6,        /* packed 4:2:2, a pair = U Y0 V Y1; read and written */
       G6D_FMT_I420 = 7,           /* planar 4:2:0: Y, then U, then V; read and written */
       G6D_FMT_YV12 = 8,           /* planar 4:2:0: Y, then V, then U; read and written */
       G6D_FMT_P010 = 9,           /* NV12's layout with 16-bit little-endian samples, value = word >> 6; read only (G6dFrame) */
       G6D_FMT_GRAY8 = 10 };       /* one byte per pixel; read only (G6dFrame) */
/* The formats after NV12 and the full-range matrices.  Planar 4:2:0 (I420 / YV12) has two plane pointers: plane1 is the FIRST chroma
 * plane, pitch1 the chroma row pitch, and the second chroma plane starts at plane1 + pitch1 * (height / 2).  Three separately allocated
 * planes would need a third pointer, i.e. an ABI bump, and are out of scope.  matrix: 0 / 1 BT.601 / BT.709 limited range (constants and
 * results as they were, bit for bit), 2 / 3 BT.601 / BT.709 FULL range; valid for every YUV format, NV12 included, in G6dFrame and G6dSink.
 * Tap rules, exact integers; chroma is point-sampled as for NV12 (no siting interpolation); everything after a tap (the 11-bit blend,
 * the rotation, the mesh rule, the crop's float32 blend) is as written for the five formats above:
 *   4:2:2: luma at byte 2x of row y (YUYV) or 2x + 1 (UYVY), U and V from pair x >> 1 of the same row; even width, any height;
 *   I420 / YV12: Y[y][x] and chroma [y>>1][x>>1] of the two chroma planes; even sizes;
 *   limited range, 8 bit: the NV12 formula above with its constants, unchanged;
 *   full range, 8 bit: c = Y, d = U-128, e = V-128, R = sat8((2^20 c + CVR e + 2^19) >> 20), G = sat8((2^20 c - CUG d - CVG e + 2^19) >> 20),
 *     B = sat8((2^20 c + CUB d + 2^19) >> 20), (CVR, CUG, CVG, CUB) = round(k 2^20): BT.601 (1470104, 360853, 748826, 1858077) from
 *     (1.402, 0.344136, 0.714136, 1.772), BT.709 (1651297, 196424, 490864, 1945738) from (1.5748, 0.187324, 0.468124, 1.8556);
 *     every sum stays below 2^31 (2^20 255 + 1858077 128 + 2^19 = 5.06e8);
 *   P010: y10 = word >> 6, c = max(y10 - 64, 0) (limited) or y10 (full), d = u10 - 512, e = v10 - 512, the 8-bit constants of the
 *     matrix (CY = 1220542 limited, 2^20 full), >> 22 with rounding term 2^21.  c, d, e are four times their 8-bit values when the
 *     samples are v8 << 8, so such a frame converts to the NV12 result bit for bit.  The limited-range sums pass 2^31
 *     (1220542 959 + 2214593 511 + 2^21 = 2.30e9): they are EVALUATED IN 64-BIT, nothing is pre-shifted;
 *   GRAY8: R = G = B = the byte. */
typedef struct G6dFrame {          /* one per frame */
  const void* plane0;              /* packed pixels (RGB, 4:2:2, GRAY8), or the Y plane */
  const void* plane1;              /* NV12 / P010: interleaved UV plane; I420 / YV12: first chroma plane (above); else NULL */
  int32_t pitch0, pitch1;          /* bytes per source row */
  int32_t width, height;           /* source size in pixels, 1..8192 */
  int32_t format;                  /* G6D_FMT_* */
  int32_t rotate;                  /* 0 / 90 / 180 / 270 degrees clockwise */
  int32_t matrix;                  /* YUV formats: 0 BT.601, 1 BT.709 limited range; 2 BT.601, 3 BT.709 full range */
  int32_t slot;                    /* destination image index in `out`; outside [0, B): frame skipped */
  int32_t out_w, out_h;            /* size of the scaled AND rotated picture inside the canvas */
  float   K[9];                    /* intrinsics of the canvas picture, written to K_out[slot] */
} G6dFrame;
int g6d_frame_ingest(const G6dFrame* frames, int n, uint8_t* out, int B, int H, int W, float* K_out, g6d_stream_t stream);
int g6d_sizeof_frame_desc(void);

/* Lens undistortion inside the ingest launch (gen6d_amd/ingest.py `Lens`); additive within ABI 12.  g6d_frame_ingest_mesh is
 * g6d_frame_ingest with one G6dMesh per frame (meshes[i] belongs to frames[i]; the table lives in device memory, 8-byte aligned).  A frame
 * whose mesh has nodes == NULL takes the plain rule above, bit for bit; a tick that mixes plain and lens frames is one launch.
 * A mesh gives the SOURCE coordinate of every canvas pixel of the picture (the quarter turn already undone by whoever built it: the
 * frame's `rotate` is not used): node (c, r) sits at canvas pixel (g c, g r), g = 2^step_log2 in {2, 4, 8, 16}, and holds (x, y) in
 * 1/65536 source pixels, |value| <= 2^30; nx >= ceil(out_w / g) + 1, ny >= ceil(out_h / g) + 1.  Canvas pixel (X, Y) of the picture,
 * exact integers (the numpy restatement in tests/test_ingest_lens_cpu.py is bit-identical): i = X mod g, j = Y mod g,
 * m00 m01 / m10 m11 the nodes of its cell (m01 to the right, m10 below),
 *   S = (g-i)(g-j) m00 + i (g-j) m01 + (g-i) j m10 + i j m11 (64-bit), f = (S + 2^(s-1)) >> s (arithmetic) with s = 2 step_log2 + 5:
 *   fx from the x parts, fy from the y parts, in 1/2048 source pixels;
 *   fx < -1024, fx > (ws-1) 2048 + 1024, or the same for fy against hs: the pixel is (0, 0, 0) (a constant black border);
 *   else fx = clamp(fx, 0, (ws-1) 2048), x0 = fx >> 11, a = fx & 2047, x1 = min(x0+1, ws-1), y likewise; taps, NV12 conversion and
 *   blend as above. */
typedef struct G6dMesh {           /* one per frame */
  const int32_t* nodes;            /* [ny][nx][2] (x, y), device memory; NULL: the plain rule */
  int32_t nx, ny;                  /* nodes per row, rows */
  int32_t step_log2;               /* 1..4 */
  int32_t samples_log2;            /* the former `reserved` (0 everywhere before): read by g6d_frame_ingest_area alone, 0..3 (clamped), below */
} G6dMesh;
int g6d_frame_ingest_mesh(const G6dFrame* frames, const G6dMesh* meshes, int n, uint8_t* out, int B, int H, int W, float* K_out,
                          g6d_stream_t stream);
int g6d_sizeof_mesh_desc(void);

/* Area-filtered ingest (gen6d_amd/ingest.py minify="area"); additive within ABI 12, no struct changes.
 * g6d_frame_ingest_area is g6d_frame_ingest_mesh (the table, the slot rules, K_out, the black canvas outside the picture) with `meshes`
 * optional (NULL: no frame has a lens) and a filter where a picture shrinks.  A frame whose mesh has nodes is supersampled through the
 * mesh by the rule at the end of this comment; with samples_log2 = 0 (every caller before the field had a name) that is the mesh rule
 * above, bit for bit.  Lens and plain frames still mix in one call (with a mesh table the call is two kernels on `stream`: the second
 * takes the frames with samples_log2 > 0, and which those are is known on the device only).
 * Every frame without a mesh takes this rule per axis of the scaled picture before rotation (target extent T = wt or ht, source extent S = ws or
 * hs; the quarter turn maps canvas (X, Y) to the unrotated (tx, ty) as above), exact integers, restated bit-identically in
 * tests/test_minify_cpu.py:
 *   S <= T (the axis does not shrink): the plain rule's two taps (i0, 2048 - a) and (i1, a), D_axis = 2048;
 *   S >  T: target coordinate t covers [t S, (t+1) S) in units of 1/T source pixel, source pixel i covers [i T, (i+1) T): the taps are
 *     i = floor(t S / T) .. floor(((t+1) S - 1) / T) (the last is at most S - 1), w_i = min((i+1) T, (t+1) S) - max(i T, t S) in 1..T;
 *     the weights sum to S: D_axis = S;
 *   each tap is converted to 8-bit RGB by its format's tap rule above (all eleven formats, the four matrices, P010 in 64-bit);
 *   per channel Sigma = sum_y sum_x wy wx p, D = Dx Dy, v = floor((2 Sigma + D) / (2 D)): the weighted mean, rounded half up.
 * Two consequences.  1: with no shrinking axis D = 2^22 and v = (Sigma + 2^21) >> 22: a frame that does not shrink gives
 * g6d_frame_ingest's bytes exactly.  2: with S = k T on both axes every canvas pixel is the round-half-up mean of its k x k block of
 * converted source pixels; the box's centre is the bilinear rule's centre ((t + 0.5) S / T - 0.5), so the picture's K does not change.
 * Magnitudes: Sigma <= 255 * 2^26; a row's inner sum sum_x wx p <= 255 * 2^13 fits 32 bits; the sum over rows and 2 Sigma + D need 64.
 * A frame whose mesh has nodes (gen6d_amd/ingest.py Lens(minify="area"); restated bit-identically in
 * tests/test_ingest_lens_area_cpu.py): L = clamp(samples_log2, 0, 3), n = 2^L, g = 2^step_log2, G = 2 n g, s = 2 (1 + L + step_log2) + 5.
 * Canvas pixel (X, Y) of the picture is the mean of n x n sub-samples (k, l), k, l = 0 .. n-1, placed at canvas position
 * (X + (2k+1-n) / (2n), Y + (2l+1-n) / (2n)), centred on the pixel; exact integers:
 *   U = 2nX + 2k + 1 - n, V = 2nY + 2l + 1 - n (the position in units of 1/(2n) canvas pixel);
 *   c = clamp(floor(U / G), 0, nx - 2), i = U - c G; r = clamp(floor(V / G), 0, ny - 2), j = V - r G.  i and j are negative only at the
 *     picture's left / top edge, where the first cell is extrapolated over less than half a canvas pixel; nx >= ceil(out_w / g) + 1
 *     keeps floor(U / G) <= nx - 2 inside the picture (ny likewise);
 *   m00 m01 / m10 m11 the nodes (c, r), (c+1, r), (c, r+1), (c+1, r+1):
 *   S = (G-i)(G-j) m00 + i (G-j) m01 + (G-i) j m10 + i j m11 (64-bit), f = (S + 2^(s-1)) >> s (arithmetic): fx, fy in 1/2048 source pixels;
 *   the mesh rule's black test, clamp and four taps, unchanged; each tap converted by its format's tap rule (all eleven formats, the four
 *     matrices, P010 in 64-bit); per channel A = sum of the four 11-bit weight products w p.  The weights sum to 2^22 and A is NOT rounded;
 *     a black sample has A = 0;
 *   v = (sum_{k,l} A + 2^(21 + 2L)) >> (22 + 2L).
 * Magnitudes: A < 2^30, sum A < 2^37 (64-bit), |S| < 2^52.  Two consequences.  1: L = 0 gives U = 2X, G = 2g: S is four times the mesh
 * rule's S and s two more, so the result is the mesh rule's, bit for bit.  2: a lens that maps every canvas position to itself (a brown
 * lens with zero coefficients, new_K = K) over a source exactly k times the picture, k in {1, 2, 4, 8}, with n = k puts every sub-sample
 * on one source pixel with fraction 0: the result is the round-half-up mean of the k x k block, the bytes the rule above writes for the
 * same frame without a lens. */
int g6d_frame_ingest_area(const G6dFrame* frames, const G6dMesh* meshes /* may be NULL */, int n, uint8_t* out, int B, int H, int W,
                          float* K_out, g6d_stream_t stream);

/* Annotated frame output (gen6d_amd/emit.py; reference predict.py:60-72 + utils/draw_utils.py draw_bbox_3d); additive within ABI 12.
 * g6d_track_corners, one 64-thread block per slot: the box (box[8][3], corner order of pts_range_to_bbox_pts) projected in float64 (the
 * projection of g6d_track_commit) under row slot_stream[b] of `table` (pose_table or smooth_table, [streams][12]) and K[b][9]; every
 * coordinate rounded as floor(v + 0.5) -> pts[b][8][2] int32, valid[b] int32.  valid[b] = 0 (and pts[b] = 0) when the slot is unused
 * (slot_stream[b] < 0), when a corner's depth is <= 0 or a rounded coordinate lies outside [-8192, 16383] (NaN included); else 1. */
int g6d_track_corners(const float* table, const float* K, const int* slot_stream, const float* box, int32_t* pts, int32_t* valid,
                      int batch, g6d_stream_t stream);
/* g6d_frame_emit, the counterpart of g6d_frame_ingest: ONE launch writes n sinks.  Sink i shows image `slot` of imgs [B][H][W][3] uint8
 * RGB with the box of pts[box][slot] drawn on it, in the sink's format, into memory the caller names.  pts [sets][B][8][2] int32 and
 * valid [sets][B] int32 hold one or two corner sets (predict.py writes the raw and the smoothed picture of a frame); `box` names the set.
 * The table lives in DEVICE memory (it changes with every call, so the launch stays outside captured graphs); the caller validates its
 * contents: planes cover `height` rows of `pitch` bytes, 1 <= width, height <= 8192 (even for NV12), 0 <= pic_w <= W, 0 <= pic_h <= H,
 * 0 <= thickness, dot_radius <= 255, box < sets.  A sink whose slot lies outside [0, B) is skipped; sinks may share a slot but must not
 * overlap in memory.  No scaling, no rotation.
 * Exact integer rules (the numpy restatement in tests/test_emit_cpu.py is bit-identical).
 * Annotated RGB at picture pixel (x, y), corners q_j = pts[box][slot][j]; priority: edges, then discs, then the picture (draw_bbox_3d
 * draws its lines over its discs).  Nothing is drawn when box is not 0 or 1, valid[box][slot] == 0 or a corner lies outside
 * [-8192, 16383].
 *   disc j covers the pixel iff dot_radius >= 0 and (x-qx)^2 + (y-qy)^2 <= dot_radius^2                          -> dot_rgb
 *   edge (a, b) of 0-1 1-2 2-3 3-0 4-5 5-6 6-7 7-4 0-4 1-5 2-6 3-7, thickness > 0: d = q_b - q_a, p = (x, y) - q_a, L = d.d, s = p.d,
 *     t = min(max(s, 0), L), E = L |p|^2 - 2 t s + t^2; covered iff E <= floor(thickness^2 L / 4) (L > 0) or 4 |p|^2 <= thickness^2
 *     (L == 0): the pixel centre lies within thickness / 2 of the segment                                        -> line_rgb
 *     (64-bit: with 0 <= x, y < 8192 and corners in [-8192, 16383], |p| components <= 16383 and |d| components <= 24575, so
 *      L <= 1.21e9, L |p|^2 <= 6.5e17, |2 t s| <= 2.0e18, t^2 <= 1.5e18, thickness^2 L <= 7.9e13: every term and sum < 2^63)
 * Sink pixel (x, y) = the annotated picture pixel when x < pic_w and y < pic_h, else RGB (0, 0, 0) (a sink larger than the picture pads
 * black, a smaller one crops).  Packed formats: channel order as in the ingest, alpha 255.
 * NV12, limited range, round(k * 2^20) constants of the forward matrix (Y row 219/255 (Kr, Kg, Kb); Cb row 224/255 (-Kr/(2(1-Kb)),
 * -Kg/(2(1-Kb)), 1/2); Cr row 224/255 (1/2, -Kg/(2(1-Kr)), -Kb/(2(1-Kr)))):
 *   Y  = sat8((CYR R + CYG G + CYB B + 2^19 + 16 * 2^20) >> 20) per pixel;
 *   Cb = sat8((CBR sR + CBG sG + CBB sB + 2^21 + 128 * 2^22) >> 22), Cr likewise, once per 2 x 2 block from the channel sums sR, sG, sB of
 *   its four annotated sink pixels (the division by 4 is folded into the shift);
 *   BT.601 (Kr, Kb) = (0.299, 0.114):   CY = (269262, 528618, 102662), CB = (-155423, -305128, 460551), CR = (460551, -385654, -74897)
 *   BT.709 (Kr, Kb) = (0.2126, 0.0722): CY = (191455, 644067, 65019),  CB = (-105533, -355018, 460551), CR = (460551, -418321, -42230) */
/* Sinks of the formats after NV12 and of the full-range matrices (additive within ABI 12; restated in
 * tests/test_pixel_formats_cpu.py), exact integers:
 *   I420 / YV12 sinks hold exactly the Y, Cb, Cr values the NV12 sink of the same call would hold: the 2 x 2 channel-sum rule above with
 *   planar stores.  4:2:2 sinks: Y per pixel as for NV12; Cb = sat8((CBR sR + CBG sG + CBB sB + 2^20 + 128 * 2^21) >> 21), Cr likewise,
 *   once per horizontal pair from the channel sums of its two annotated sink pixels; even width, any height.
 *   Full range (matrix 2 / 3), round(k * 2^20) of (Kr, Kg, Kb) without the 219 / 224 scaling and without the +16:
 *   Y = sat8((CYR R + CYG G + CYB B + 2^19) >> 20), chroma as above with +128;
 *   BT.601: CY = (313524, 615514, 119538), CB = (-176932, -347356, 524288), CR = (524288, -439026, -85262)
 *   BT.709: CY = (222927, 749942, 75707),  CB = (-120138, -404150, 524288), CR = (524288, -476214, -48074)
 *   (both Y rows sum to 2^20); black padding of a full-range sink is Y = 0, chroma 128. */
typedef struct G6dSink {           /* one per destination */
  void* plane0;                    /* packed pixels (RGB, 4:2:2), or the Y plane */
  void* plane1;                    /* NV12: interleaved UV plane; I420 / YV12: first chroma plane, the second at plane1 + pitch1 * (height / 2); else NULL */
  int32_t pitch0, pitch1;          /* bytes per sink row */
  int32_t width, height;           /* sink size in pixels, 1..8192 (4:2:0: even; 4:2:2: even width) */
  int32_t format;                  /* G6D_FMT_* but P010 and GRAY8, which are read only: such a sink is not written */
  int32_t matrix;                  /* YUV formats: 0 BT.601, 1 BT.709 limited range; 2 BT.601, 3 BT.709 full range */
  int32_t slot;                    /* source image index in `imgs`; outside [0, B): sink skipped */
  int32_t pic_w, pic_h;            /* the picture inside the canvas (top-left corner), <= W, H */
  int32_t thickness, dot_radius;   /* draw_bbox_3d: 2, 2 */
  int32_t line_rgb, dot_rgb;       /* 0xRRGGBB; draw_bbox_3d: 0x0000FF, 0xFF0000 */
  int32_t box;                     /* corner set drawn: 0 or 1; anything else: no box */
} G6dSink;
int g6d_frame_emit(const G6dSink* sinks, int n, const uint8_t* imgs, int B, int H, int W, const int32_t* pts, const int32_t* valid,
                   g6d_stream_t stream);
int g6d_sizeof_sink_desc(void);

/* g6d_frame_emit_source, the source view of g6d_frame_emit (gen6d_amd/emit.py, Sink(view="source")); additive within ABI 12.  ONE launch
 * writes n sinks; sink i shows the camera's own picture frames[sinks[i].slot] (a G6dFrame table of nf records as g6d_frame_ingest
 * takes it, e.g. the one an ingest launch of the same tick read) with a box drawn in the SOURCE's pixel grid: the picture is the
 * frame's width x height at the sink's top-left corner, not scaled and not turned.  A sink whose `slot` lies outside [0, nf) is skipped.
 * The corners are pts[box][frames[slot].slot] of pts [sets][B][8][2] / valid [sets][B] (sets 1 or 2): the frame's own `slot` is its
 * canvas slot, so corner sets indexed like the canvas serve both views; they must have been projected with the SOURCE's intrinsics
 * (ingest.source_K).  A frame whose own slot lies outside [0, B) is drawn without a box.  Not read: the sink's pic_w / pic_h and the
 * frame's rotate, out_w, out_h and K.  max_w x max_h bounds the sinks' sizes (1..8192): it sizes the tile walk of the launch and never
 * changes a result.  Both tables live in DEVICE memory; the caller validates them as for g6d_frame_ingest and g6d_frame_emit.
 * Exact integer rules (the numpy restatement in tests/test_emit_source_cpu.py is bit-identical).
 * Source RGB at source pixel (x, y), 0 <= x < width, 0 <= y < height: the ingest's tap rule at an integer position, i.e. what
 * g6d_frame_ingest writes for a same-size, unturned frame (a = b = 0).  Packed formats: R, G, B by channel order (alpha ignored).
 * NV12: Y[y][x] and UV[y>>1][x>>1] through the inverse formulas above with the frame's matrix.
 * Annotation: g6d_frame_emit's rules unchanged, in source pixels: priority edges, discs, picture; the same edge and disc inequalities;
 * nothing is drawn when box is not 0 or 1, valid is 0 or a corner lies outside [-8192, 16383]; sizes <= 8192, so the 64-bit bound above
 * holds as written.
 * Sink pixel (x, y) = the annotated source pixel when x < width and y < height of the frame, else RGB (0, 0, 0).
 * Output: packed formats and NV12 by g6d_frame_emit's forward formulas on the annotated RGB, EXCEPT an NV12 frame into an NV12 sink
 * of the same matrix, which is a pass-through (call a pixel covered when an edge or a disc covers it):
 *   a Y sample of a sink pixel inside the picture that no primitive covers is the source's Y byte; a covered pixel's Y comes from the
 *   forward formula on line_rgb / dot_rgb;
 *   a UV pair whose 2 x 2 block lies inside the picture and has no covered pixel is the source's UV pair; a block with at least one
 *   covered pixel comes from the forward formula on the channel sums of its four annotated pixels, the uncovered ones contributing
 *   their converted source RGB;
 *   outside the picture Y = 16 and UV = (128, 128), what the forward formulas make of black.  Both pictures have even sizes and share
 *   the origin, so no block straddles the picture's edge.  A pass-through sink without a box is a byte copy of the picture.
 * With the formats after NV12 the pass-through is this rule for a frame and a sink of the SAME format among NV12, I420,
 * YV12, YUYV422, UYVY422 and the same `matrix` value, with the chroma block 2 x 2 for 4:2:0 and 2 x 1 (a horizontal pair of one row)
 * for 4:2:2, and Y = 0 outside the picture under a full-range matrix.  Any other pair goes through RGB, YUYV <-> UYVY and I420 <-> NV12
 * included.  For matrix values 0 / 1 on NV12 nothing changes. */
int g6d_frame_emit_source(const G6dSink* sinks, int n, const G6dFrame* frames, int nf, const int32_t* pts, const int32_t* valid, int sets,
                          int B, int max_w, int max_h, g6d_stream_t stream);

/* g6d_frame_crop, g6d_warp_batch's query crops cut from the camera-native frames (gen6d_amd/chain.py query_batch_source, DESIGN.md
 * §4.24); additive within ABI 12.  ONE launch fills dst [B][3][dh][dw] float32 in [0,1], the layout and the uint8-rounded values of
 * g6d_warp_batch.  hinv [B][9] maps crop pixels to pixels of the working-resolution canvas, as for g6d_warp_batch; slot b samples the
 * camera's own picture frames[rec[b]] (a G6dFrame table as g6d_frame_ingest takes it; the record's `slot` field is not used) through that
 * map composed with the inverse of the ingest's scaling and quarter turn.  A slot with rec[b] < 0 has no source: it takes g6d_warp_batch's
 * rule on imgs[b] (imgs [B][H][W][3] uint8, the canvases), bit for bit.  frames, rec, imgs and hinv live in DEVICE memory and are read when
 * the kernel runs (the launch can sit inside a captured graph); the caller validates the table as for g6d_frame_ingest and that
 * rec[b] names one of its records.
 * Rule of a slot with r = rec[b] >= 0, all in float32, with ws x hs the source and wt x ht the scaled picture before rotation
 * ((out_w, out_h) for rotate 0 / 180, (out_h, out_w) for 90 / 270) of frames[r], at crop pixel (x, y):
 *   1. (cx, cy) = (X, Y) / Wd of hinv[b] * (x, y, 1), with 1 / Wd taken as 0 when Wd == 0 (g6d_warp_batch's rule);
 *   2. the quarter turn undone (the ingest's rule above, read for real coordinates): rotate 0: (px, py) = (cx, cy), 90: (cy, ht-1-cx),
 *      180: (wt-1-cx, ht-1-cy), 270: (wt-1-cy, cx);
 *   3. fx = px * ax + bx (one fused multiply-add) with ax = (float)(ws / wt) and bx = 0.5f * ax - 0.5f, fy likewise with hs / ht: the inverse of the ingest's
 *      u' = (u + 0.5) * wt / ws - 0.5.  A same-size source has ax = 1, bx = 0 and fx = px exactly;
 *   4. g6d_warp_batch from here, on the source: fx = clamp(fx, -4, ws + 4), x0 = floor(fx), a = fx - x0, x1 = x0 + 1, y likewise (b);
 *      weights (1-a)(1-b), a(1-b), (1-a)b, ab; a tap outside the source contributes zero;
 *   5. each tap becomes RGB by the ingest's tap rules: packed formats by channel order (alpha ignored), NV12 through the integer
 *      conversion above with chroma UV[y>>1][x>>1] and the frame's matrix;
 *   6. per channel v = sum of weight * tap, dst = clamp(rint(v), 0, 255) / 255.
 * The sampler is the point-sampled bilinear of every warp here: a crop pixel that covers several source pixels aliases
 * (g6d_frame_crop_area below filters such a crop). */
int g6d_frame_crop(const G6dFrame* frames, const int32_t* rec, const uint8_t* imgs, int B, int H, int W, const float* hinv, float* dst,
                   int dh, int dw, g6d_stream_t stream);

/* g6d_frame_crop_area, g6d_frame_crop supersampled where the crop shrinks its source (chain.py query_batch_source minify="area",
 * DESIGN.md §4.26); additive within ABI 12.  g6d_frame_crop's arguments plus max_n in 1..8; everything is read from device memory when
 * the kernel runs, so the launch sits in a captured graph where g6d_frame_crop sits.
 * Per slot b, with the slot's view as above (the source record, or the identity on the canvas when rec[b] < 0: such slots are filtered
 * over their canvas), float32: P(.) = steps 1 - 3 of the rule above, the source position before the clamp; c = ((dw-1)/2, (dh-1)/2);
 *   m = max(|P(c + (1,0)) - P(c)|, |P(c + (0,1)) - P(c)|), Euclidean lengths in source pixels: how far a crop pixel reaches;
 *   n = min(floor(m + 0.5), max_n) if m is finite and m >= 1.5, else n = 1 (a NaN or infinite m of a degenerate map: one sample).
 * Per crop pixel (x, y), for i, j in 0 .. n-1: the sample at (x + (2i + 1 - n) / (2n), y + (2j + 1 - n) / (2n)) (offsets 0 when n = 1)
 * goes through steps 1 - 5 unchanged and gives the unrounded weighted sum v_ij per channel; dst = clamp(rint(sum v_ij / n^2), 0, 255) / 255.
 * With n = 1 the result is g6d_frame_crop's, bit for bit.  The order of the n^2 sum is not part of the contract.  max_n = 8 bounds the
 * work at 256 taps per crop pixel; beyond 8x the crop still aliases, at an eighth of the rate. */
int g6d_frame_crop_area(const G6dFrame* frames, const int32_t* rec, const uint8_t* imgs, int B, int H, int W, const float* hinv, float* dst,
                        int dh, int dw, int max_n, g6d_stream_t stream);

/* The detector's 15x15 correlation in the frequency domain (csrc/corr_fft.hip; network/detector.py:222-224 for batched
 * calls on the fp32 path); additive within ABI 12.  Overlap-save over T x T windows, T = 32, k = 15, V = T - k + 1 = 18: tile (ty, tx) of
 * a map owns output pixels (ty V .., tx V ..), its window starts k/2 pixels before them and is zero outside the map; a window has
 * bins = T (T/2 + 1) Hermitian bins, bin = ky (T/2 + 1) + kx.  The tiles of all segments form one flat list in segment, image, row, column
 * order (csrc/corr_fft_plan.h).  fp32 everywhere: three launches, each an entry point of its own, so that each is testable:
 *   g6d_corr_fft_fwd   segs[i].in [N][H][W][ld_in] (>= Cin channels, Cin % 32 == 0)  ->  X [bins][tiles][2][Cin], re plane then im plane
 *   g6d_corr_fft_gemm  Y [bins][tiles][2][32] = X' . B' per bin, B' [bins][2 Cin][64] = the conjugate filter spectrum as a real matrix:
 *                      row c (of Xr) = [Wr[.][c] | -Wi[.][c]], row Cin + c (of Xi) = [Wi[.][c] | Wr[.][c]] over the 32 references, with
 *                      W = rfft2 of the k x k filter zero-extended to T x T (tap (0, 0) at the origin); X and B' 16-byte aligned
 *   g6d_corr_fft_inv   Y  ->  inverse real FFT / T^2, positions [0, V)^2 of every tile to segs[i].out [N][H*W][ld_out] inside the map.
 * One launch addresses less than 2^31 bytes of X (G6D_ENOSPC beyond): g6d_corr_fft_plan answers, for the segments given, out[0..7] =
 * tiles, bins, V, bytes of X, bytes of Y, bytes of B', the tiles of one query (one map per segment) and the most queries a launch takes. */
int g6d_corr_fft_plan(const G6dCorrSeg* segs, int nseg, int Cin, int Cout, int k, int T, int64_t* out);
int g6d_corr_fft_fwd(const G6dCorrSeg* segs, int nseg, int Cin, int k, int T, float* X, g6d_stream_t stream);
int g6d_corr_fft_gemm(const float* X, const float* B, float* Y, int tiles, int Cin, int Cout, int T, g6d_stream_t stream);
int g6d_corr_fft_inv(const G6dCorrSeg* segs, int nseg, int Cout, int k, int T, const float* Y, g6d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GEN6D_HIP_H */
