// 3x3 stride-1 pad-1 convolution as Winograd F(2x2,3x3) on the fp32 matrix cores of gfx950 — the seven 64->128 ...
// 512->512 layers of the VGG-11-BN trunks (reference network/pretrain_models.py:9-31,61-72, BatchNorm folded), with the
// bias, ReLU and 2x2 max-pool of the trunk fused into the epilogue, channels-last in and out.
//
//   Y(2x2) = A^T [ sum_ci U_ci (.) V_ci ] A,   U = G g G^T (host, once per checkpoint),  V = B^T d B (4x4 input tile)
//
// i.e. 16 independent GEMMs  D_ab[tile][co] = sum_ci V_ab[tile][ci] * U_ab[ci][co]  with 2.25x fewer multiplications
// than the direct form.  Mapping to v_mfma_f32_32x32x2_f32 (M = tiles, N = co, K = ci):
//
//   block  = 256 threads = 4 waves = 64 Winograd tiles (four "quarters" of 4x4 tiles = 8x8 output pixels each, consecutive
//            entries of the flat list of all quarters of all images) x 64
//            output channels; wave (wm, wn) owns 32 tiles x 32 channels for ALL 16 (a,b) positions: 16 accumulator
//            tiles = 256 accumulator registers per lane, one wave per SIMD.  Because a lane holds all 16 D_ab of its
//            (tile, co) elements, the output transform, bias, ReLU and the 2x2 max-pool (= max over the 4 outputs of a
//            tile) are pure per-lane register arithmetic: no LDS exchange in the epilogue.
//   K loop = chunks of 8 input channels: the RAW 10x10 input patch of every quarter (not its 3.2x larger transform) is
//            staged in LDS through registers (zero padding + image borders masked there); the input transform runs in
//            registers on the fragment each lane reads (16 ds_read_b128 -> 32 vector add/sub -> 16 A fragments).  The
//            pre-transformed filters are stored [chunk][ab][co][8], so a block's 32 KB per chunk is 16 contiguous 2 KB
//            runs that go global -> LDS directly (global_load_lds_dwordx4, no VGPR round trip: the registers are spent on
//            accumulators).  Two LDS stages, one barrier per chunk; per wave and chunk 64 MFMAs against 32 ds_read_b128.
//   split  = small maps do not fill 256 CUs with 64-tile blocks and a block's K loop is serial (2-3 us per chunk): the
//            channel chunks are then split over gridDim.z; partial OUTPUT tiles (the output transform is linear) go to a
//            workspace and the block of a tile that arrives last adds them and applies bias / ReLU / max-pool / statistics.
//   K trick = as in conv_igemm.hip: lane-half h reads channels 4h..4h+3 of the chunk with one ds_read_b128 per operand;
//            MFMA s consumes channel s (lanes 0-31) and 4+s (lanes 32-63) for both operands.
//
// Numerics: fp32 throughout; F(2x2,3x3) has transform constants {0, +-1, +-1/2} only (same error class as the MIOpen
// Winograd solver the trunk ran on before).
//
// This unit: the fp32 kernel, the launcher of the whole F(2x2,3x3) family (wino_run: plan of wino_plan.h, then this kernel or
// wino16_launch of wino16_conv.hip) and the entry points.  wino_common.h: what the kernels of both units share.
#include "wino_common.h"
#include "seg_table.h"
#include <stdio.h>

namespace {

#ifndef WINO_M3_RAW_AUX
#define WINO_M3_RAW_AUX 0                   // cache policy of the raw pieces of the product layers (profiling builds: 2 = non-temporal)
#endif

// The same kernel also runs the stride-1 3x3 / 3x3x3 layers of the selector, the refiner feature net and the refiner volume
// net when g6d_conv_igemm finds pre-transformed filters in G6dConv.weight_wino (template parameters):
//   MODE  operand prologue applied when the raw patch is written to LDS, as in conv_igemm.hip: 0 none, 1 InstanceNorm
//         affine(+ReLU) with one table, 2 one table per image group (image / aff_div; LDS holds the tables of the block's four
//         quarters), 3 elementwise multiplier (selector query x reference product) + affine, tables per quarter as in 2 — a
//         batch of queries shares the reference images (img_mod) while each query brings its own multiplier map (mul_div) and
//         table; zero padding stays exactly zero.  The affine tables sit in LDS (loaded once per block).
//   KD    3: 3x3x3 layers as a 2-D Winograd over (h, w) with the three depth taps folded into the reduction: chunk c =
//         (kd, 8 input channels) reads depth slice d + kd - 1 — the transform-domain accumulators are shared, so the
//         multiplication count drops from 27 to 12 per output.
//         25: a 15x15 "same" correlation (the detector's reference-as-filter level, network/detector.py:222-224) as 5x5 blocks of 3x3
//         sub-filters: out = sum_{bi,bj} conv3x3(in shifted by (3bi-6, 3bj-6), w[3bi..3bi+2, 3bj..3bj+2]) — chunk c = (block, 8 input
//         channels) reads the raw patch at the block's shift, all 25 blocks accumulate in the same transform-domain accumulators:
//         225 taps cost 25 * 16 / 4 = 100 multiplications per output (2.25x fewer, as for a single 3x3).
//   NWN   output-channel width of a block in 32s: 2 = 64 channels / 4 waves; 1 = 32 channels / 2 waves (two such blocks share a
//         CU), used when 64-wide blocks would leave CUs idle (e.g. the 32^3 x 64 volume layers: 128 -> 256 blocks).
// Epilogue additions for those layers: per-(group, channel) sum / sum of squares of the outputs for the following
// InstanceNorm (float partials per block, one fp64 atomic per channel and run of equal groups).

// NWM = 32-tile rows of the block (quarters / 2): 2 = four quarters x 32*NWN channels (the default shape); 1 with NWN = 4 = two quarters x
// 128 channels — the same four waves, but one staged raw patch feeds twice the output channels: a layer's input is re-read Cout / 128
// instead of Cout / 64 times (trunk layers with Cout % 128 == 0).
template <int MODE, int KD, int NWN, int NWM = 2>
__global__ void __launch_bounds__(64 * NWM * NWN, 1) wino_conv3x3_kernel(const WinoArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int THREADS = 64 * NWM * NWN;
  constexpr int NQ = 2 * NWM;                                 // quarters per block
  constexpr int RAWF = NQ * WQ_PIX * WRAW_LD;                 // floats of the raw patch image
  constexpr int NPR = (200 * NQ + THREADS - 1) / THREADS;     // raw-patch pieces per thread and chunk (2, 4 or 7)
  constexpr int GL = 16 / NWM;                                // direct-to-LDS filter pieces per wave and chunk
  constexpr int WU_FLOATS = 16 * 32 * NWN * 8;                // [ab][co][8], lane-linear image of the global layout
  constexpr int WSTAGE = RAWF + WU_FLOATS + 4 * THREADS;   // raw patch, filter image, scratch row for the idle pieces of the last round
  constexpr int AFF0 = 2 * WSTAGE;                            // affine tables behind the stages: [G][Cin] scales, [G][Cin] shifts, [Cin] zeros
  constexpr int AFFG = MODE >= 2 ? NQ : 1;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / NWN, wn = wave % NWN;
  const int li = lane & 31, lh = lane >> 5;
  const int n0 = blockIdx.y * (32 * NWN);
  const int nc8 = p.Cin >> 3;                                             // 8-channel chunks per depth tap
  const int c_first = blockIdx.z * p.chunks_per_split;                    // this block's slice of the (kd, chunk) list
  const int c_last = min(KD * nc8, c_first + p.chunks_per_split) - 1;

  // ---- raw patch loader: pieces idx = tid + THREADS*j < 800 = 4 quarters x 100 positions x 2 halves of the 8-channel chunk
  int poff[NPR], lsto[NPR], moff[MODE == 3 ? NPR : 1], aoff[MODE != 0 ? NPR : 1];
  bool pval[NPR], live[NPR];
  unsigned dbits = 0;                                          // KD = 3: bit 2j / 2j+1 = piece j has a slice below / above
  unsigned smask[KD == 25 ? NPR : 1];                          // KD = 25: bits 0-4 / 8-12 = row / column of the piece inside the image under block shift b
  int rstep[KD == 25 ? NPR : 1];                               //          floats per block step along y (3 rows of the piece's map)
#pragma unroll
  for (int j = 0; j < NPR; ++j) {
    const int idx = tid + THREADS * j;
    const int q = idx / 200, r = idx - q * 200, pp = r >> 1, half = r & 1;
    const int py = pp / 10, px = pp - py * 10;
    const QGeo g = quarter_of(p, q < NQ ? q : 0, NQ);
    const int n = g.n;
    const int iy = g.oy0 + py - 1, ix = g.ox0 + px - 1;
    pval[j] = (idx < 200 * NQ) & g.valid & ((unsigned)iy < (unsigned)g.H) & ((unsigned)ix < (unsigned)g.W);
    const int n_in = p.img_mod > 0 ? ((n / p.D) % p.img_mod) * p.D + n % p.D : n;      // query batches share the input images
    poff[j] = pval[j] ? g.in_off + ((n_in * g.H + iy) * g.W + ix) * g.ld_in + 4 * half : 0;
    live[j] = idx < 200 * NQ;
    lsto[j] = live[j] ? (q * WQ_PIX + pp) * WRAW_LD + 4 * (half ^ ((py >> 1) & 1)) : RAWF + WU_FLOATS + 4 * tid;
    if constexpr (MODE == 3) moff[j] = pval[j] ? (((p.mul_div > 0 ? n / p.mul_div : 0) * p.H + iy) * p.W + ix) * p.Cin + 4 * half : 0;
    if constexpr (MODE != 0) aoff[j] = (MODE >= 2 ? (q < NQ ? q : 0) * p.Cin : 0) + 4 * half;
    if constexpr (KD == 3) { const int dd = n % p.D; dbits |= (unsigned)(dd > 0) << (2 * j) | (unsigned)(dd < p.D - 1) << (2 * j + 1); }
    if constexpr (KD == 25) {
      unsigned m = 0;
#pragma unroll
      for (int b = 0; b < 5; ++b)
        m |= (unsigned)((unsigned)(iy + 3 * b - 6) < (unsigned)g.H) << b | (unsigned)((unsigned)(ix + 3 * b - 6) < (unsigned)g.W) << (8 + b);
      smask[j] = ((idx < 200 * NQ) & g.valid) ? m : 0u;
      rstep[j] = 3 * g.W * g.ld_in;
      poff[j] = g.in_off + ((n * g.H + iy) * g.W + ix) * g.ld_in + 4 * half;      // the UNSHIFTED position (may lie outside: used under smask only)
    }
  }
  // Operand prologues without a select and (2-D layers) without per-chunk address arithmetic: every piece comes through a
  // bounds-checked buffer load — a piece outside the image (zero padding, masked quarter) asks for an offset beyond the tensor and the
  // hardware returns zeros — and the InstanceNorm SHIFT of such a piece is read from a row of zeros behind the tables, so that
  // raw * scale + shift (and ReLU of it) is exactly zero there, as the reference's padding behind the norm is.  2-D layers: the lane
  // offset of a piece and the LDS offset of its shift are constants of the piece, the chunk's channel offset is the instruction's
  // scalar / immediate offset.  (Round 4: per piece and chunk a `v ? off : 0` select and 64-bit address per load, 4 multiplies, 4 FMAs
  // and 4 selects beside the MFMAs — the MODE 3 / MODE 2 instantiations ran at 44-56 % MfmaUtil against 66 % for MODE 0.)
  unsigned pboff[KD == 1 ? NPR : 1];                          // byte offsets of the pieces for the buffer loads (beyond the tensor: zero)
  unsigned mboff[MODE == 3 ? NPR : 1];                        // ... into the multiplier maps
  int shoff[MODE != 0 ? NPR : 1];                             // LDS offset of the piece's shift values: its table, or the zero row
  if constexpr (KD == 1) {
#pragma unroll
    for (int j = 0; j < NPR; ++j) pboff[j] = pval[j] ? (unsigned)poff[j] << 2 : 0x80000000u;
  }
  if constexpr (MODE == 3) {
#pragma unroll
    for (int j = 0; j < NPR; ++j) mboff[j] = pval[j] ? (unsigned)moff[j] << 2 : 0x80000000u;
  }
  if constexpr (MODE != 0) {
#pragma unroll
    for (int j = 0; j < NPR; ++j) shoff[j] = pval[j] ? AFF0 + AFFG * p.Cin + aoff[j] : AFF0 + 2 * AFFG * p.Cin + (aoff[j] & 4);
  }
  const int slice = p.H * p.W * p.ld_in;                     // KD = 3: one depth step
  const auto in_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in), 0, p.in_bytes, 0x00020000);
  const auto mul_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(MODE == 3 ? p.mul : p.in), 0, MODE == 3 ? p.mul_bytes : p.in_bytes, 0x00020000);
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  f32x4 rp[NPR], rm[MODE == 3 ? NPR : 1];
  bool rv[NPR];                                               // validity of the piece for the chunk it was loaded for
  auto load_piece = [&](int j, int chunk) {
    // reduction order: depth taps outermost for KD = 3; for KD = 25 the 25 block shifts are INNERMOST (chunk-major): the shifted
    // windows of a block overlap almost completely, so the 25 visits of an 8-channel slice come while its lines are still in L2
    // (shift-major re-fetched the whole window from the fabric 25 times: 10.5 GB per launch against 0.33 GB of input)
    const int kd = KD == 25 ? chunk % 25 : (KD != 1 ? chunk / nc8 : 0), cc = KD == 25 ? chunk / 25 : (KD != 1 ? chunk - kd * nc8 : chunk);
    bool v = pval[j];
    int off = poff[j] + cc * 8;
    if constexpr (KD == 3) { v &= kd == 1 || ((dbits >> (2 * j + (kd >> 1))) & 1u) != 0; off += (kd - 1) * slice; }
    if constexpr (KD == 25) {                      // block (bi, bj) of the 15x15 filter: the patch shifted by (3bi - 6, 3bj - 6)
      const int bi = kd / 5, bj = kd - 5 * bi;
      v = ((smask[j] >> bi) & (smask[j] >> (8 + bj)) & 1u) != 0;
      off += (bi - 2) * rstep[j] + (bj - 2) * 3 * p.ld_in;
    }
    rv[j] = v;
    {
      // bounds-checked buffer load: pieces outside the image (zero padding, masked quarters) ask for an offset beyond the
      // tensor and get zeros from the hardware — no select when the piece goes to LDS; for 2-D layers the lane offset is a
      // constant of the piece and the chunk's channel offset is the instruction's scalar offset: no vector-ALU work at all
      u32x4 raw;
      if constexpr (KD == 1) raw = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(in_rsrc, pboff[j], cc * 32, (MODE == 3 ? WINO_M3_RAW_AUX : 0)));
      else raw = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(in_rsrc, v ? (unsigned)off << 2 : 0x80000000u, 0, 0));
      rp[j] = __builtin_bit_cast(f32x4, raw);
    }
    if constexpr (MODE == 3)      // (2-D layers only: g6d_wino_eligible)
      rm[j] = __builtin_bit_cast(f32x4, __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(mul_rsrc, mboff[j], cc * 32, 0)));
  };
  auto load_raw = [&](int chunk) {
#pragma unroll
    for (int j = 0; j < NPR; ++j) load_piece(j, chunk);
  };
  auto store_piece = [&](int j, int st, int chunk) {   // unconditional stores (a branch would serialise them behind one vmcnt(0) each);
    const int cc = KD == 25 ? chunk / 25 : (KD != 1 ? chunk % nc8 : chunk);       // the idle pieces of the last round go to a scratch row behind the stages
    {
      f32x4 v = rp[j];
      if constexpr (MODE != 0) {
        // packed: two v_pk_fma_f32 (+ two v_pk_mul_f32 for the multiplier) per piece; the shift comes from the zero row for a piece
        // outside the image (3-D layers: decided per chunk by the depth tap — one select on the LDS offset instead of four on the data)
        const int so = KD == 1 ? shoff[j] : (rv[j] ? shoff[j] : AFF0 + 2 * AFFG * p.Cin + (aoff[j] & 4));
        f32x4 sc = *reinterpret_cast<const f32x4*>(lds + AFF0 + aoff[j] + cc * 8);
        const f32x4 sh = *reinterpret_cast<const f32x4*>(lds + so + cc * 8);
        f32x2w s0 = {sc[0], sc[1]}, s1 = {sc[2], sc[3]};
        if constexpr (MODE == 3) { s0 = s0 * f32x2w{rm[j][0], rm[j][1]}; s1 = s1 * f32x2w{rm[j][2], rm[j][3]}; }
        const f32x2w r0 = __builtin_elementwise_fma(f32x2w{v[0], v[1]}, s0, f32x2w{sh[0], sh[1]});
        const f32x2w r1 = __builtin_elementwise_fma(f32x2w{v[2], v[3]}, s1, f32x2w{sh[2], sh[3]});
        v = f32x4{r0.x, r0.y, r1.x, r1.y};
        if (p.in_relu) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
      }
      f32x4* dst = reinterpret_cast<f32x4*>(__builtin_assume_aligned(lds + st * WSTAGE + lsto[j], 16));
      *dst = v;
    }
  };
  auto store_raw = [&](int st, int chunk) {
#pragma unroll
    for (int j = 0; j < NPR; ++j) store_piece(j, st, chunk);
  };
  if constexpr (MODE != 0) {                  // InstanceNorm affine tables -> LDS: [G][Cin] scales, then [G][Cin] shifts
    constexpr int G = MODE >= 2 ? NQ : 1;
    for (int i = tid; i < G * p.Cin; i += THREADS) {
      int g = 0;
      if constexpr (MODE >= 2) g = p.aff_div > 0 ? (quarter_of(p, i / p.Cin, NQ).n / p.D) / p.aff_div : 0;
      const int c = MODE >= 2 ? i % p.Cin : i;
      lds[AFF0 + i] = p.in_scale[g * p.Cin + c];
      lds[AFF0 + G * p.Cin + i] = p.in_shift[g * p.Cin + c];
    }
    for (int i = tid; i < p.Cin; i += THREADS) lds[AFF0 + 2 * G * p.Cin + i] = 0.f;      // the shifts of the pieces outside the image
    __syncthreads();
  }
  // ---- filter tiles: wave w moves (ab, half) pairs idx = 8w .. 8w+7, 1 KB (32 co x 32 B) per instruction
  // Direct-to-LDS copy in inline asm: with the builtin, hipcc books the copy on the LDS counter as well and then waits
  // lgkmcnt(0) in front of every fragment use (it cannot count mixed event types), which exposes the LDS latency of the
  // fragment requests just issued.  M0 = LDS byte address of the wave's 1 KB destination, each lane lands at +16*lane.
  const float* ubase = p.U + (size_t)n0 * 8;                 // wave-uniform; each lane adds 16 bytes x lane
  const unsigned lane16 = lane * 16;
  const unsigned lds_addr0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)lds;
  auto glds = [&](int chunk, int st, int idx) {
    const int ab = idx / NWN, h = idx % NWN;
    // wave-uniform source: a 64-bit base per chunk plus a 32-bit piece offset (two scalar adds per piece)
    const char* g = reinterpret_cast<const char*>(ubase) + (size_t)chunk * ((size_t)p.Cout * 512) + (unsigned)((ab * p.Cout + h * 32) * 32);
    const unsigned dst = __builtin_amdgcn_readfirstlane(lds_addr0 + 4u * (unsigned)(st * WSTAGE + RAWF + (ab * 32 * NWN + h * 32) * 8));
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane16), "s"(g), "s"(dst) : "memory");
  };
  auto load_u = [&](int chunk, int st) {
#pragma unroll
    for (int k = 0; k < GL; ++k) glds(chunk, st, wave * GL + k);
  };

  // ---- fragment bases
  const int tl = li & 15, ty = tl >> 2, tx = tl & 3;
  const int apos = ((2 * wm + (li >> 4)) * WQ_PIX + (2 * ty) * 10 + 2 * tx) * WRAW_LD;
  const int abase01 = apos + 4 * (lh ^ (ty & 1));            // patch rows 2ty, 2ty+1   ((py >> 1) & 1 == ty & 1)
  const int abase23 = apos + 4 * (lh ^ (ty & 1) ^ 1);        // patch rows 2ty+2, 2ty+3
  const int bbase = RAWF + (wn * 32 + li) * 8 + 4 * (lh ^ ((li >> 3) & 1));
  constexpr int USTRIDE = 32 * NWN * 8;                      // floats between (a,b) positions of the filter image

  f32x16 acc[16];
#pragma unroll
  for (int a = 0; a < 16; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

  load_u(c_first, 0);
  load_raw(c_first);
  store_raw(0, c_first);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  if (WINO_ABLATE == 9) { if (lds[tid] == 12345.f && p.out_pool) p.out_pool[tid] = lds[tid + 1]; return; }   // launch + prologue only
  // Software pipeline (one wave per SIMD: nothing but the wave's own instruction order hides latency).  The 16 MFMAs of
  // the LAST (a,b) group of chunk c-1 are deferred across the barrier with their operands held in registers (vD, uD):
  // chunk c opens with them, and every request of the chunk — the direct-to-LDS filter copies and the raw loads of
  // chunk c+1, the 16 raw-tile reads and the first 8 filter fragments of chunk c — is issued in the shadow of those MFMAs,
  // two to three memory instructions behind each.  Groups 0-2 then run back to back (the fragments of group g+2 are
  // requested at the start of group g), and the chunk ends by preparing vD / uD of its own last group.
  f32x4 vD[4], uD[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { vD[j] = f32x4{0.f, 0.f, 0.f, 0.f}; uD[j] = f32x4{0.f, 0.f, 0.f, 0.f}; }

  // Input transform V = B^T d B of (a,b) group `grp` (row combination a = grp of the raw rows, then the four column combinations)
  // as 16 packed two-float adds.  On this matrix pipe fp32 MFMAs and vector-ALU instructions do not overlap (measured,
  // tools/ubench/mfma_fill.hip: every VALU instruction beside v_mfma_f32_32x32x2_f32 costs its 4 issue cycles, the first one in an
  // MFMA gap 14; a packed add costs the same as a scalar one; LDS reads, scalar instructions and loads are nearly free): the
  // kernel therefore keeps the VALU count minimal and in ONE burst per group instead of spreading it over the gaps.
  auto xform = [&](int grp, const f32x4 (&dd)[4][4], f32x4 (&vv)[4]) {
    if (WABL(3)) {
#pragma unroll
      for (int q = 0; q < 4; ++q) vv[q] = dd[grp][q];
      return;
    }
    f32x2 rl[4], rh[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 &a = dd[grp == 0 ? 0 : grp == 2 ? 2 : 1][q], &b = dd[grp == 0 ? 2 : grp == 1 ? 2 : grp == 2 ? 1 : 3][q];
      if (grp == 1) { rl[q] = pk_add(lo2(a), lo2(b)); rh[q] = pk_add(hi2(a), hi2(b)); }
      else { rl[q] = pk_sub(lo2(a), lo2(b)); rh[q] = pk_sub(hi2(a), hi2(b)); }
    }
    vv[0] = cat2(pk_sub(rl[0], rl[2]), pk_sub(rh[0], rh[2]));
    vv[1] = cat2(pk_add(rl[1], rl[2]), pk_add(rh[1], rh[2]));
    vv[2] = cat2(pk_sub(rl[2], rl[1]), pk_sub(rh[2], rh[1]));
    vv[3] = cat2(pk_sub(rl[1], rl[3]), pk_sub(rh[1], rh[3]));
  };

  for (int cc = c_first; cc <= c_last; ++cc) {
    const int c = cc - c_first;                   // stage parity counts from the block's first chunk
    const float* S = lds + (c & 1) * WSTAGE;
    const int cn = min(cc + 1, c_last);           // the last chunk re-requests itself into the idle stage: no branches
    f32x4 d[4][4], ub[3][4], v[4];
    auto rd_d = [&](int i, int j) { if (!WABL(4)) d[i][j] = *reinterpret_cast<const f32x4*>(S + (i < 2 ? abase01 : abase23) + (i * 10 + j) * WRAW_LD); };
    auto rd_u = [&](int g, int j) { if (!WABL(4)) ub[g % 3][j] = *reinterpret_cast<const f32x4*>(S + bbase + (g * 4 + j) * USTRIDE); };
    // deferred group of chunk c-1 (gaps 0-15): every request of the chunk is issued in its shadow — the direct-to-LDS filter
    // pieces and the raw loads of chunk c+1 (the pieces first: invisible to the compiler's load counting, they must be OLDER
    // than the loads it waits for), the 16 raw-tile reads and the filter fragments of groups 0 and 1 of chunk c
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      // consecutive MFMAs go to DIFFERENT accumulators (k & 3): instructions issued between two MFMAs on the same accumulator
      // stretch the dependent pair
      acc[12 + (k & 3)] = __builtin_amdgcn_mfma_f32_32x32x2f32(vD[k & 3][k >> 2], uD[k & 3][k >> 2], acc[12 + (k & 3)], 0, 0, 0);
      if (!WABL(2)) {
        if (k < GL) glds(cn, (c & 1) ^ 1, wave * GL + k);
        else if (k - GL < NPR) load_piece(k - GL, cn);
      }
      if (k < 12) {                                // LDS requests in the order of first use: rows 0, 2, fragments 0, row 1, fragments 1, row 3
        const int j0 = 2 * (k & 1);
        if (k < 2) { rd_d(0, j0); rd_d(0, j0 + 1); }
        else if (k < 4) { rd_d(2, j0); rd_d(2, j0 + 1); }
        else if (k < 6) { rd_u(0, j0); rd_u(0, j0 + 1); }
        else if (k < 8) { rd_d(1, j0); rd_d(1, j0 + 1); }
        else if (k < 10) { rd_u(1, j0); rd_u(1, j0 + 1); }
        else { rd_d(3, j0); rd_d(3, j0 + 1); }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      xform(i, d, v);                              // one VALU burst, then 16 MFMAs with the remaining requests in their gaps
      if (i == 2 && !WABL(2)) store_raw((c & 1) ^ 1, cn);      // raw pieces of chunk c+1 -> LDS: requested ~40 gaps ago
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        acc[i * 4 + (m & 3)] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[m & 3][m >> 2], ub[i][m & 3][m >> 2], acc[i * 4 + (m & 3)], 0, 0, 0);
        if (i < 2 && m < 2) { rd_u(i + 2, 2 * m); rd_u(i + 2, 2 * m + 1); }
        if constexpr (GL == 16) {                    // 16 filter pieces fill the deferred group: the raw pieces follow in the first gaps of group 0
          if (i == 0 && m >= 2 && m - 2 < NPR && !WABL(2)) load_piece(m - 2, cn);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    xform(3, d, vD);                               // operands of this chunk's deferred group
#pragma unroll
    for (int q = 0; q < 4; ++q) uD[q] = ub[0][q];  // ub[3 % 3] holds the group-3 fragments
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the direct-to-LDS filter tiles of the next chunk have landed
    if (!WABL(1)) __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < 16; ++k)
    acc[12 + (k & 3)] = __builtin_amdgcn_mfma_f32_32x32x2f32(vD[k & 3][k >> 2], uD[k & 3][k >> 2], acc[12 + (k & 3)], 0, 0, 0);

  if (WINO_ABLATE == 7) {                             // no epilogue: one conditional dummy store keeps the accumulators alive
    float t = 0.f;
#pragma unroll
    for (int a = 0; a < 16; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) t += acc[a][r];
    if (t == 12345.f && p.out_pool) p.out_pool[tid] = t;
    return;
  }
  // ---------------------------------------------------------------- epilogue: A^T D A, bias, ReLU, stores, 2x2 max-pool
  const int co = n0 + wn * 32 + li;
  // output transform first: Y[r] = the 2x2 outputs {y00, y01, y10, y11} of accumulator row r (no bias yet)
  f32x4 Y[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float sr[2][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sr[0][j] = acc[0 + j][r] + acc[4 + j][r] + acc[8 + j][r];
      sr[1][j] = acc[4 + j][r] - acc[8 + j][r] - acc[12 + j][r];
    }
    Y[r] = f32x4{sr[0][0] + sr[0][1] + sr[0][2], sr[0][1] - sr[0][2] - sr[0][3], sr[1][0] + sr[1][1] + sr[1][2], sr[1][1] - sr[1][2] - sr[1][3]};
  }
  if (p.splits > 1) {
    // the output transform is linear: partial OUTPUT tiles go to the workspace as [split][tile][r][thread] 16-byte pieces, and
    // the block that arrives last adds them in split order (g6d_common.h) and carries on with bias / ReLU / pool / statistics
    constexpr int TILE = THREADS * 64;
    const int ntiles = gridDim.x * gridDim.y, tile = blockIdx.y * gridDim.x + blockIdx.x;
    float* part = p.ws + G6D_WS_COUNTERS + (size_t)tile * TILE + tid * 4;
    const size_t zstride = (size_t)ntiles * TILE;
#pragma unroll
    for (int r = 0; r < 16; ++r) g6d_store_wt(part + blockIdx.z * zstride + r * (THREADS * 4), Y[r]);
    if (!g6d_split_arrive(reinterpret_cast<int*>(p.ws) + tile, p.splits, reinterpret_cast<int*>(lds))) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) Y[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int z0 = 0; z0 < p.splits; z0 += 2) {
      f32x4 v[2][16];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) v[u][r] = *reinterpret_cast<const f32x4*>(part + (size_t)min(z0 + u, p.splits - 1) * zstride + r * (THREADS * 4));
#pragma unroll
      for (int r = 0; r < 16; ++r) Y[r] += v[0][r];
      if (z0 + 1 < p.splits) {
#pragma unroll
        for (int r = 0; r < 16; ++r) Y[r] += v[1][r];
      }
    }
  }
  const float bv = p.bias ? p.bias[co] : 0.f;
  const bool do_relu = p.relu != 0;
  const bool do_stats = p.stats != nullptr;
  const QGeo geo[2] = {quarter_of(p, 2 * wm, NQ), quarter_of(p, 2 * wm + 1, NQ)};      // the wave's two quarters
  float st1[2] = {0.f, 0.f}, st2[2] = {0.f, 0.f};       // statistics of this lane's column, per quarter of the wave
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    // accumulator row r of the 32x32 tile = tile (r&3) + 8*(r>>2) + 4*lh of the wave's 32
    const QGeo& g = geo[r >> 3];
    const int tyy = lh + 2 * ((r >> 2) & 1), txx = r & 3;
    const int n = g.n; const bool qv = g.valid;
    const int Hp = g.H >> 1, Wp = g.W >> 1;
    float y[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        y[a][b] = Y[r][2 * a + b] + bv;
        if (do_relu) y[a][b] = fmaxf(y[a][b], 0.f);
      }
    const int oy = g.oy0 + 2 * tyy, ox = g.ox0 + 2 * txx;
    if (p.out_full && qv) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
          if (oy + a < g.H && ox + b < g.W) {
            p.out_full[(size_t)g.full_off + ((size_t)(n * g.H + oy + a) * g.W + ox + b) * g.ld_full + co] = y[a][b];
            if (do_stats) { st1[r >> 3] += y[a][b]; st2[r >> 3] += y[a][b] * y[a][b]; }
          }
    }
    if (p.out_pool && qv) {
      const int py = oy >> 1, px = ox >> 1;
      if (py < Hp && px < Wp)
        p.out_pool[(size_t)g.pool_off + ((size_t)(n * Hp + py) * Wp + px) * g.ld_pool + co] = fmaxf(fmaxf(y[0][0], y[0][1]), fmaxf(y[1][0], y[1][1]));
    }
  }
  if (do_stats) {
    // lanes l and l+32 hold the same column; [quarter][column][2] float partials in LDS (the stages are free: every wave has
    // passed the last barrier of the K loop), then one fp64 atomic per column and run of quarters with the same group
    float* sred = lds;
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      st1[h] += __shfl_xor(st1[h], 32, 64);
      st2[h] += __shfl_xor(st2[h], 32, 64);
      if (lh == 0) {
        sred[((2 * wm + h) * 32 * NWN + wn * 32 + li) * 2] = st1[h];
        sred[((2 * wm + h) * 32 * NWN + wn * 32 + li) * 2 + 1] = st2[h];
      }
    }
    __syncthreads();
    if (tid < 32 * NWN) {
      double a1 = 0.0, a2 = 0.0;
      int cur = -1;
      for (int q = 0; q < NQ; ++q) {
        const QGeo qg = quarter_of(p, q, NQ);
        if (!qg.valid) break;
        const int g = p.stats_div > 0 ? (qg.n / p.D) / p.stats_div : 0;
        if (g != cur && cur >= 0) {
          double* st = p.stats + ((size_t)cur * p.Cout + n0 + tid) * 2;
          atomicAdd(st, a1); atomicAdd(st + 1, a2); a1 = a2 = 0.0;
        }
        cur = g;
        a1 += (double)sred[(q * 32 * NWN + tid) * 2];
        a2 += (double)sred[(q * 32 * NWN + tid) * 2 + 1];
      }
      if (cur >= 0) {
        double* st = p.stats + ((size_t)cur * p.Cout + n0 + tid) * 2;
        atomicAdd(st, a1); atomicAdd(st + 1, a2);
      }
    }
    if (p.fin.scale) {                          // InstanceNorm finalisation by the launch's last block (G6dConv.fin_*)
      __syncthreads();
      g6d_finalize_stats(p.fin, gridDim.x * gridDim.y, reinterpret_cast<int*>(lds));
    }
  }
}

// ---- launch: plan (wino_plan.h), instantiation
// The instantiation of a planned launch, chosen once (wino_prepare) for the launch and for g6d_wino_multi_route: family as
// G6dWinoRoute.family; NWN x NWM waves per block (wide: 4 x 1), the 16-bit kernels: wino16_pick's answer
struct WinoPick { int family, nwn, nwm; size_t lds_bytes; };

template <int MODE, int KD, int NWN, int NWM = 2>
int wino_launch_t(WinoArgs& a, long long blocks, const WinoPick& pick, hipStream_t stream) {
  constexpr int THREADS = 64 * NWM * NWN;
  g6d_allow_lds(reinterpret_cast<const void*>(&wino_conv3x3_kernel<MODE, KD, NWN, NWM>), (int)wplan::LDS_MAX);
  hipLaunchKernelGGL((wino_conv3x3_kernel<MODE, KD, NWN, NWM>), dim3((unsigned)blocks, a.Cout / (32 * NWN), a.splits), dim3(THREADS),
                     pick.lds_bytes, stream, a);
  return g6d_check_launch("wino_conv3x3");
}

template <int MODE, int KD>
int wino_launch_w(WinoArgs& a, long long blocks, const WinoPick& pick, hipStream_t stream) {
  return pick.nwn == 1 ? wino_launch_t<MODE, KD, 1>(a, blocks, pick, stream) : wino_launch_t<MODE, KD, 2>(a, blocks, pick, stream);
}

// The plan of one launch under the current knobs (wino_prepare; g6d_wino_route): completes a one-map argument block's segment list first
wplan::F2Plan wino_plan_of(WinoArgs& a, int mode, int kd, bool has_workspace, size_t workspace_bytes) {
  if (a.nseg == 0) {          // one map size: the launch's own fields
    a.nseg = 1;
    a.seg[0] = WinoSeg{0, a.N, a.H, a.W, 0, 0, 0, 0, 0, a.ld_in, a.ld_full, a.ld_pool};
  }
  // (the model's constants can be overridden for measurements)
  const wplan::F2Knobs knobs = {(int)g6d_knob(G6D_KNOB_WINO_WIDE), (int)g6d_knob(G6D_KNOB_WINO_SPLIT_MAX), g6d_knob(G6D_KNOB_WINO_SPLIT_GAIN),
                                g6d_knob(G6D_KNOB_WINO_SPLIT_FIX), g6d_knob(G6D_KNOB_WINO_SPLIT_PER)};
  return wplan::f2_plan(a.seg, a.nseg, a.img_mod > 0 ? (long long)a.img_mod * a.D : 0, a.mm, mode, kd, a.Cin, a.Cout,
                        wplan::room(has_workspace, workspace_bytes, G6D_WS_COUNTER_BYTES), G6D_WS_COUNTERS, knobs);
}

// Everything of a launch but the launch: the plan, the geometry / split fields of `a`, the instantiation.  G6D_EINVAL = refused (message
// set).  kd = 1, 3 or 25; mode as the kernel's MODE.
int wino_prepare(WinoArgs& a, int mode, int kd, const float* workspace, size_t workspace_bytes, wplan::F2Plan& pl, WinoPick& pick) {
  pl = wino_plan_of(a, mode, kd, workspace != nullptr, workspace_bytes);
  if (pl.error) { g6d_set_error(pl.error); return G6D_EINVAL; }
  a.QH = a.seg[0].QH; a.QW = a.seg[0].QW;
  a.qtotal = (int)pl.q.quarters;
  a.in_bytes = (unsigned)(pl.q.in_extent * 4);
  a.splits = pl.split.splits; a.chunks_per_split = pl.split.chunks_per_split; a.ws = const_cast<float*>(workspace);
  if (a.mm) {
    const wino::Pick16 p16 = wino16_pick(a, mode, kd);
    if (p16.error) { g6d_set_error(p16.error); return G6D_EINVAL; }
    pick = WinoPick{p16.two_waves ? 2 : 1, pl.shape.nwn, 2, p16.lds_bytes};
    return G6D_OK;
  }
  const int nwm = pl.shape.wide ? 1 : 2;
  pick = WinoPick{0, pl.shape.nwn, nwm, wplan::f2_lds_bytes(mode, pl.shape.nwn, nwm, a.Cin)};
  return G6D_OK;
}

int wino_run(WinoArgs& a, int mode, int kd, float* workspace, size_t workspace_bytes, hipStream_t stream) {
  wplan::F2Plan pl; WinoPick pick;
  if (int rc = wino_prepare(a, mode, kd, workspace, workspace_bytes, pl, pick)) return rc;
  if (g6d_knob(G6D_KNOB_WINO_DEBUG) == 1)
    fprintf(stderr, "wino %d seg, N=%d %dx%dx%d->%d kd=%d mode=%d: grid %lld x %d splits of %d chunks\n", a.nseg, a.N, a.H, a.W, a.Cin,
            a.Cout, kd, mode, pl.grid2, a.splits, a.chunks_per_split);
  const long long blocks = pl.blocks;
  if (a.mm) return wino16_launch(a, mode, kd, blocks, stream);
  if (kd == 25) return wino_launch_w<0, 25>(a, blocks, pick, stream);
  if (kd == 3) return mode == 2 ? wino_launch_w<2, 3>(a, blocks, pick, stream)
                    : mode == 1 ? wino_launch_w<1, 3>(a, blocks, pick, stream) : wino_launch_w<0, 3>(a, blocks, pick, stream);
  if (mode == 3) return wino_launch_w<3, 1>(a, blocks, pick, stream);
  if (mode == 2) return wino_launch_w<2, 1>(a, blocks, pick, stream);
  if (mode == 1) return wino_launch_w<1, 1>(a, blocks, pick, stream);
  if (pick.nwn == 4) return wino_launch_t<0, 1, 4, 1>(a, blocks, pick, stream);
  return wino_launch_w<0, 1>(a, blocks, pick, stream);
}

// What g6d_wino_multi_route reports of a prepared launch
void wino_report(const WinoArgs& a, int entry, int kd, const wplan::F2Plan& pl, const WinoPick& pick, G6dWinoRoute& r) {
  r = G6dWinoRoute{};
  r.entry = entry; r.family = pick.family; r.kd = kd; r.wide = pl.shape.wide; r.nq = pl.shape.nq; r.nwn = pl.shape.nwn;
  r.grid2 = pl.grid2; r.blocks = (int)pl.blocks; r.nchunks = pl.nchunks; r.splits = a.splits; r.chunks_per_split = a.chunks_per_split;
  r.lds_bytes = (int)pick.lds_bytes;
  for (int k = 0; k < a.nseg; ++k) { r.seg[k].qstart = a.seg[k].qstart; r.seg[k].QH = a.seg[k].QH; r.seg[k].QW = a.seg[k].QW; }
}

// The segment list and bases of a multi-map launch from its validated table (seg_table.h); the scalar fields = segment 0
void wino_segments(WinoArgs& a, const G6dSegTable& t) {
  wplan::segments(t, a.seg, a.nseg, a.in, a.out_full, a.out_pool);
  const G6dSeg& g = t.seg[0];
  a.N = g.N; a.H = g.H; a.W = g.W; a.ld_in = g.ld_in; a.ld_full = g.ld_full; a.ld_pool = g.ld_pool;
}

}  // namespace

// in [N][H][W][ld_in] channels-last (Cin % 8 == 0), U = pre-transformed filters [Cin/8][16][Cout][8] (see
// gen6d_amd/network/backbone.py: winograd_filters), bias [Cout] or NULL, Cout % 64 == 0.
//   y = conv3x3(in, pad 1) + bias; if relu: y = max(y, 0)
//   out_full (optional) [N][H][W][ld_full]   <- y
//   out_pool (optional) [N][H/2][W/2][ld_pool] <- 2x2 max-pool of y (floor, as F.max_pool2d)
//   workspace (optional): split partial outputs for grids that would not fill the chip (splits*N*H*W*Cout floats)
// Replaces features[4..27] of vgg11_bn (conv + folded BatchNorm + ReLU + MaxPool), network/pretrain_models.py:17-25,66-72.
static int wino_single_args(const float* in, int N, int H, int W, int Cin, int ld_in, const float* U, const float* bias, int Cout, int relu,
                            float* out_full, int ld_full, float* out_pool, int ld_pool, WinoArgs& a) {
  if (!in || !U || (!out_full && !out_pool) || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || (Cin & 7) || (ld_in & 3) || ld_in < Cin ||
      Cout <= 0 || (Cout & 63) || (out_full && ld_full < Cout) || (out_pool && (ld_pool < Cout || H < 2 || W < 2)) ||
      !g6d_aligned16(in) || !g6d_aligned16(U) || (long long)N * H * W * ld_in >= (1ll << 29)) {
    g6d_set_error("wino_conv3x3: bad args (Cin % 8 == 0, Cout % 64 == 0, 16-byte aligned operands)"); return G6D_EINVAL;
  }
  a = WinoArgs{};
  a.in = in; a.U = U; a.bias = bias; a.out_full = out_full; a.out_pool = out_pool;
  a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.ld_in = ld_in; a.Cout = Cout; a.ld_full = ld_full; a.ld_pool = ld_pool; a.relu = relu;
  a.D = 1;
  return G6D_OK;
}
extern "C" int g6d_wino_conv3x3(const float* in, int N, int H, int W, int Cin, int ld_in, const float* U, const float* bias,
                                int Cout, int relu, float* out_full, int ld_full, float* out_pool, int ld_pool,
                                float* workspace, size_t workspace_bytes, g6d_stream_t stream) {
  WinoArgs a;
  if (int rc = wino_single_args(in, N, H, W, Cin, ld_in, U, bias, Cout, relu, out_full, ld_full, out_pool, ld_pool, a)) return rc;
  return wino_run(a, 0, 1, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}

// The same layer over up to 4 map sizes in ONE launch (G6dWinoSeg, include/gen6d_hip.h): the scales of the detector's image
// pyramid (network/detector.py:236-241) run every trunk layer with the same filters.
static int wino_multi_args(const G6dWinoSeg* segs, int nseg, int Cin, const float* U, const float* bias, int Cout, int relu, WinoArgs& a) {
  if (!segs || nseg < 1 || nseg > wplan::MAX_SEG || !U || Cin <= 0 || (Cin & 7) || Cout <= 0 || (Cout & 63) || !g6d_aligned16(U)) {
    g6d_set_error("wino_conv3x3_multi: bad args (1..4 segments, Cin % 8 == 0, Cout % 64 == 0)"); return G6D_EINVAL;
  }
  G6dSegTable t;
  if (int rc = g6d_seg_table("wino_conv3x3_multi", "segment", G6D_SAME_KINDS, segs, nseg, Cin, Cout, G6D_REACH_BUFFER_LOAD, t)) return rc;
  a = WinoArgs{};
  a.U = U; a.bias = bias; a.Cin = Cin; a.Cout = Cout; a.relu = relu; a.D = 1;
  wino_segments(a, t);
  return G6D_OK;
}
extern "C" int g6d_wino_conv3x3_multi(const G6dWinoSeg* segs, int nseg, int Cin, const float* U, const float* bias, int Cout, int relu,
                                      float* workspace, size_t workspace_bytes, g6d_stream_t stream) {
  WinoArgs a;
  if (int rc = wino_multi_args(segs, nseg, Cin, U, bias, Cout, relu, a)) return rc;
  return wino_run(a, 0, 1, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}

// Reduced-precision variant of g6d_wino_conv3x3_multi (math_mode 1 = bf16, 2 = fp16 operands, fp32 accumulation and outputs): U16 =
// the filters transformed AND rounded on the host, [Cin/16][16][Cout][16] 16-bit values in the layout of g6d_wino_conv3x3's U with a
// chunk of 16 input channels (rows with co & 8 carry their two 16-byte halves swapped); Cin % 16 == 0, Cout % 64 == 0.
static int wino16_multi_args(const G6dWinoSeg* segs, int nseg, int Cin, const void* U16, const float* bias, int Cout, int relu, int math_mode,
                             WinoArgs& a) {
  if (!segs || nseg < 1 || nseg > wplan::MAX_SEG || !U16 || Cin <= 0 || (Cin & 15) || Cout <= 0 || (Cout & 63) || !g6d_aligned16(U16) ||
      (math_mode != 1 && math_mode != 2)) {
    g6d_set_error("wino16_conv3x3_multi: bad args (1..4 segments, Cin % 16 == 0, Cout % 64 == 0, math_mode 1 or 2)"); return G6D_EINVAL;
  }
  G6dSegTable t;
  if (int rc = g6d_seg_table("wino16_conv3x3_multi", "segment", G6D_SAME_KINDS, segs, nseg, Cin, Cout, G6D_REACH_BUFFER_LOAD, t)) return rc;
  a = WinoArgs{};
  a.U = reinterpret_cast<const float*>(U16); a.bias = bias; a.Cin = Cin; a.Cout = Cout; a.relu = relu; a.D = 1; a.mm = math_mode;
  wino_segments(a, t);
  return G6D_OK;
}
extern "C" int g6d_wino16_conv3x3_multi(const G6dWinoSeg* segs, int nseg, int Cin, const void* U16, const float* bias, int Cout, int relu,
                                        int math_mode, float* workspace, size_t workspace_bytes, g6d_stream_t stream) {
  WinoArgs a;
  if (int rc = wino16_multi_args(segs, nseg, Cin, U16, bias, Cout, relu, math_mode, a)) return rc;
  return wino_run(a, 0, 1, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}

// The detector's 15x15 reference-as-filter correlation (network/detector.py:222-224) on the Winograd kernel: 5x5 blocks of 3x3
// sub-filters accumulated in the transform domain (KD = 25 above) — 2.25x fewer multiplications than the direct form of
// g6d_corr2d_patch.  Maps as in g6d_corr2d_patch_multi (up to 4 sizes, N maps each); U = the 25 sub-filter banks transformed like
// g6d_wino_conv3x3's, CHUNK-major: [Cin/8 * 25][16][Cout][8], row c * 25 + b = 8-channel chunk c of block b = 5 bi + bj, which holds
// w[:, 3bi..3bi+2, 3bj..3bj+2, 8c..8c+7] (include/gen6d_hip.h, backbone.winograd_corr_filters; the kernel walks kd = chunk % 25 innermost).
static int wino_corr_args(const G6dCorrSeg* segs, int nseg, int Cin, const float* U, int Cout, int kblocks, WinoArgs& a) {
  if (!segs || nseg < 1 || nseg > wplan::MAX_SEG || !U || kblocks != 5 || Cin <= 0 || (Cin & 7) || Cout <= 0 || (Cout & 31) || !g6d_aligned16(U)) {
    g6d_set_error("corr2d_wino_multi: bad args (1..4 map sizes, 15x15 = 5 blocks, Cin % 8 == 0, Cout % 32 == 0)"); return G6D_EINVAL;
  }
  for (int k = 1; k < nseg; ++k)
    if (segs[k].ld_in != segs[0].ld_in) return g6d_bad_seg("corr2d_wino_multi", "map", G6D_SHARED_LD_IN);
  G6dSegTable t;
  if (int rc = g6d_seg_table("corr2d_wino_multi", "map", G6D_SHARED_LD_IN, segs, nseg, Cin, Cout, G6D_REACH_BUFFER_LOAD, t)) return rc;
  a = WinoArgs{};
  a.U = U; a.bias = nullptr; a.Cin = Cin; a.Cout = Cout; a.relu = 0; a.D = 1;
  wino_segments(a, t);
  return G6D_OK;
}
extern "C" int g6d_corr2d_wino_multi(const G6dCorrSeg* segs, int nseg, int Cin, const float* U, int Cout, int kblocks, float* workspace,
                                     size_t workspace_bytes, g6d_stream_t stream) {
  WinoArgs a;
  if (int rc = wino_corr_args(segs, nseg, Cin, U, Cout, kblocks, a)) return rc;
  return wino_run(a, 0, kblocks * kblocks, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}

// The host's choice for a launch of one of the entry points above or of wino43_conv.hip, without the launch (include/gen6d_hip.h): the
// entry's own argument checks and segment table, then wino_prepare — what the launch itself runs before hipLaunchKernelGGL
int g6d_w43_multi_route(bool corr, const void* segs, int nseg, int Cin, const void* U, int Cout, int kblocks, const float* workspace,
                        size_t workspace_bytes, G6dWinoRoute& route);      // (wino43_conv.hip)
extern "C" int g6d_wino_multi_route(int entry, const void* segs, int nseg, int Cin, const void* U, int Cout, int kblocks, int math_mode,
                                    const float* workspace, size_t workspace_bytes, G6dWinoRoute* route) {
  if (!route) { g6d_set_error("wino_multi_route: route expected"); return G6D_EINVAL; }
  if (entry < 0 || entry > 5) { g6d_set_error("wino_multi_route: entry 0 ... 5 expected"); return G6D_EINVAL; }
  if (entry == 3 || entry == 5) {
    const int rc = g6d_w43_multi_route(entry == 5, segs, nseg, Cin, U, Cout, kblocks, workspace, workspace_bytes, *route);
    route->entry = entry;
    return rc;
  }
  const G6dWinoSeg* ws = static_cast<const G6dWinoSeg*>(segs);
  const float* Uf = static_cast<const float*>(U);
  WinoArgs a;
  int rc, kd = 1;
  if (entry == 1) {
    if (!ws || nseg != 1) { g6d_set_error("wino_multi_route: one G6dWinoSeg row expected for g6d_wino_conv3x3"); return G6D_EINVAL; }
    rc = wino_single_args(ws->in, ws->N, ws->H, ws->W, Cin, ws->ld_in, Uf, nullptr, Cout, 0, ws->out_full, ws->ld_full, ws->out_pool, ws->ld_pool, a);
  } else if (entry == 0) rc = wino_multi_args(ws, nseg, Cin, Uf, nullptr, Cout, 0, a);
  else if (entry == 2) rc = wino16_multi_args(ws, nseg, Cin, U, nullptr, Cout, 0, math_mode, a);
  else { rc = wino_corr_args(static_cast<const G6dCorrSeg*>(segs), nseg, Cin, Uf, Cout, kblocks, a); kd = kblocks * kblocks; }
  if (rc) return rc;
  wplan::F2Plan pl; WinoPick pick;
  if ((rc = wino_prepare(a, 0, kd, workspace, workspace_bytes, pl, pick))) return rc;
  wino_report(a, entry, kd, pl, pick, *route);
  return G6D_OK;
}
extern "C" int g6d_sizeof_wino_route(void) { return (int)sizeof(G6dWinoRoute); }

// ---- the conv family on the Winograd kernel (called by g6d_conv_igemm when G6dConv.weight_wino is set)
// Eligible: kernel (1,3,3) on 2-D maps or (3,3,3), stride 1, "same" padding, Cin % 8 == 0, Cout % 32 == 0, maps of at least
// 6x6 (4x4 maps would fill a quarter of an 8x8 output quarter: the direct kernels are better there), fp32 math, no LeakyReLU,
// statistics groups = whole images or one group, no forced split.
bool g6d_wino_eligible(const G6dConv& d) {
  const bool on = g6d_knob(G6D_KNOB_CONV_WINO) != 0, on16 = g6d_knob(G6D_KNOB_CONV_WINO16) != 0;
  if (!on) return false;
  if (d.math_mode != 0) {     // 16-bit kernel: host-rounded 16-bit filters, chunks of 16 channels, 64-channel blocks
    if (!on16 || !d.weight_wino16 || (d.Cin & 15) || (d.Cout & 63) || !g6d_aligned16(d.weight_wino16)) return false;
  } else if (!d.weight_wino) return false;
  const bool k2 = d.kd == 1 && d.Di == 1 && d.pd == 0, k3 = d.kd == 3 && d.pd == 1;
  if (!(k2 || k3) || d.kh != 3 || d.kw != 3 || d.ph != 1 || d.pw != 1 || d.sd != 1 || d.sh != 1 || d.sw != 1) return false;
  if ((d.Cin & 7) || (d.Cout & 31) || d.Hi < 6 || d.Wi < 6 || d.out_act > 1 || d.split_k > 1) return false;
  if (d.mul && (!k2 || !d.in_scale)) return false;
  if ((d.in_image_mod > 0 || d.mul_group_images > 0) && !k2) return false;
  if (d.stats && d.stat_rows_per_group > 0 && d.stat_rows_per_group % (d.Do * d.Ho * d.Wo)) return false;   // groups = runs of whole images
  if (d.in_scale && d.Cin > 1024) return false;                          // affine tables of the block's four quarters in LDS
  if ((d.math_mode == 0 && !g6d_aligned16(d.weight_wino)) || (d.in_scale && ((d.Cin & 3) != 0))) return false;
  if (d.math_mode != 0 && d.mul && d.kd != 1) return false;
  // Profitability (measured per layer, profiles/r02_layer_table.md): a block pays ~4 us of prologue / output transform and the
  // kernel holds a whole SIMD per wave, so layers with a short reduction (K = kd*Cin < 128: 64-channel inputs) or little total work
  // (M * K * Cout < 1.5e8: the 7-image 8x8 / 16x16 feature-net layers, the 8^3 volume layer) stay on the direct kernels.
  // (knob wino_min_work: tests send small shapes down this path with 0, which disables the rule; -1 = the built-in thresholds.)
  const double mw = g6d_knob(G6D_KNOB_WINO_MIN_WORK);
  // The 16-bit kernel competes with direct kernels that already run 16-bit MFMAs at twice the fp32 rate while its own transforms
  // stay fp32 work: measured per layer (profiles/r03_layer_table_fp16.md) it wins from K >= 192 and ~9e8 multiply-adds upwards.
  const double min_work = mw >= 0 ? mw : (d.math_mode ? 9e8 : 1.5e8);
  const double M = (double)d.N * d.Di * d.Hi * d.Wi, K = (double)d.kd * d.Cin;
  if (min_work > 0 && (K < (d.math_mode ? 192 : 128) || M * K * d.Cout < min_work)) return false;
  if ((long long)d.N * d.Di * ((d.Hi + 7) / 8) * ((d.Wi + 7) / 8) >= (1ll << 31)) return false;           // quarter list
  return (long long)(d.in_image_mod > 0 ? d.in_image_mod : d.N) * d.Di * d.Hi * d.Wi * d.ld_in < (1ll << 29);      // 2^31 bytes: the bound of the buffer loads
}

// The argument block and the prologue mode of a conv descriptor on this family (g6d_wino_launch; g6d_wino_route)
static int wino_args_of(const G6dConv& d, WinoArgs& a) {
  a.in = d.in; a.U = d.math_mode ? reinterpret_cast<const float*>(d.weight_wino16) : d.weight_wino; a.mm = d.math_mode;
  a.bias = d.bias; a.out_full = d.out; a.out_pool = nullptr;
  a.D = d.Di; a.N = d.N * d.Di; a.H = d.Hi; a.W = d.Wi; a.Cin = d.Cin; a.ld_in = d.ld_in; a.Cout = d.Cout; a.ld_full = d.ld_out;
  a.ld_pool = 0; a.relu = d.out_act == 1;
  a.mul = d.mul; a.in_scale = d.in_scale; a.in_shift = d.in_shift; a.in_relu = d.in_relu;
  a.mul_bytes = d.mul ? (unsigned)((long long)(d.mul_group_images > 0 ? (d.N + d.mul_group_images - 1) / d.mul_group_images : 1) * d.Hi * d.Wi * d.Cin * 4) : 0u;      // (< 2^31: g6d_conv_igemm)
  a.stats = d.stats; a.stats_div = d.stat_rows_per_group > 0 ? d.stat_rows_per_group / (d.Do * d.Ho * d.Wo) : 0;
  a.aff_div = d.in_affine_per_n; a.img_mod = d.in_image_mod; a.mul_div = d.mul_group_images > 0 ? d.mul_group_images * d.Di : 0;
  if (d.fin_scale)
    a.fin = G6dFin{d.fin_scale, d.fin_shift, reinterpret_cast<int*>(d.fin_counter), d.stats, 1.0 / d.fin_count, d.fin_eps, d.fin_groups * d.Cout};
  return d.mul ? 3 : (!d.in_scale ? 0 : (d.in_affine_per_n ? 2 : 1));
}

int g6d_wino_launch(const G6dConv& d, hipStream_t stream) {
  WinoArgs a = {};
  const int mode = wino_args_of(d, a);
  return wino_run(a, mode, d.kd, d.workspace, d.workspace_bytes, stream);
}

// The prologue mode and the split count g6d_wino_launch runs `d` with (no launch; splits -1: the plan refuses the layer)
void g6d_wino_route(const G6dConv& d, int* mode, int* splits) {
  WinoArgs a = {};
  *mode = wino_args_of(d, a);
  const wplan::F2Plan pl = wino_plan_of(a, *mode, d.kd, d.workspace != nullptr, d.workspace_bytes);
  *splits = pl.error ? -1 : pl.split.splits;
}
