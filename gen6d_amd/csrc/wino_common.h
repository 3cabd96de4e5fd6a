// wino_common.h — what the F(2x2,3x3) Winograd kernels of wino_conv.hip (fp32) and wino16_conv.hip (bf16 / fp16 operands) share on the
// device: the launch's argument block, the raw-patch layout in LDS, the flat quarter list's decoding and the packed two-float steps of
// the input transform; and the host function through which the launcher (wino_run, wino_conv.hip) reaches the 16-bit kernels.
#pragma once
#include "g6d_common.h"
#include "wino_plan.h"

#ifndef WINO_ABLATE
#define WINO_ABLATE 0   // profiling builds only (tools/wino_ablate.sh; results are wrong by construction): 1 = no barrier in the chunk
                        // loop, 2 = no global loads / LDS stores of the next chunk, 3 = no input transform (raw values as fragments),
                        // 4 = no fragment reads from LDS, 5 = all of them (matrix cores only), 6 = (16-bit kernels) no MFMA, 7 = no epilogue, 9 = launch + prologue only
#endif
#define WABL(n) (WINO_ABLATE == (n) || WINO_ABLATE == 5)

// Raw patch image in LDS: position (q, py, px) of quarter q at ((q*101 + py*10 + px) * 8) floats, its two 4-channel halves
// swapped when (py >> 1) is odd; filter image [ab][co][8] with the halves swapped when (co & 8) (done once on the host, the
// direct-to-LDS copy is lane-linear).  Both layouts make every ds_read_b128 of the fragment loops bank-conflict free
// (checked exhaustively over the four 16-lane service groups of the instruction; plain 12-float rows were 3-way, plain
// [co][8] rows 2-way conflicted).
#define WQ_PIX 101                         // position stride between quarters (10 x 10 used)
#define WRAW_LD 8                          // floats per raw patch position
#define WRAW_FLOATS (4 * WQ_PIX * WRAW_LD) // 3232
static_assert(WRAW_FLOATS == wplan::F2_RAW_FLOATS, "the LDS sizes of wino_plan.h count this patch");

// The argument block crosses translation units (wino_run -> wino16_launch), so its type has external linkage; the kernels take WinoArgs
// (below), the same bytes under a name private to each unit.
namespace wino {
struct Args {
  const float* in; const float* U; const float* bias; float* out_full; float* out_pool;
  int N, H, W, Cin, ld_in, Cout, ld_full, ld_pool, relu;      // N = images x depth slices (every slice is a 2-D map); = seg[0]
  int QH, QW;
  int nseg, qtotal; wplan::Seg seg[wplan::MAX_SEG];
  unsigned in_bytes;                              // extent of the input tensor(s) from `in` (< 2^31): bound of the buffer loads
  unsigned mul_bytes;                             // ... of the multiplier maps from `mul` (MODE 3)
  int splits, chunks_per_split; float* ws;       // splits > 1: tile counters + partial outputs (no bias / ReLU / pool)
  // conv-family extras (zero / null for the trunk)
  int D;                                         // depth slices per image (1 for 2-D layers); KD = 3 pads in depth
  const float* mul; const float* in_scale; const float* in_shift; int in_relu;
  int aff_div;                                   // MODE 2 / 3: image i uses affine table i / aff_div (0: one table)
  int img_mod, mul_div;                          // > 0: image i reads input image i % img_mod / multiplier map i / mul_div (G6dConv)
  double* stats; int stats_div;                  // [groups][Cout][2]; group of image i = i / stats_div (0: one group)
  G6dFin fin;                                    // fin.scale != NULL: the last block finalises the statistics
  int mm;                                        // 0: fp32 kernel; 1 / 2: the kernels of wino16_conv.hip with bf16 / fp16 operands (U holds 16-bit filters)
};
}  // namespace wino

// The 16-bit kernels (wino16_conv.hip) on a planned launch (geometry and split fields of `a` filled, `blocks` blocks of four quarters):
// the two trunk kernels (mode 0, 2-D, no statistics) or the conv-family one; kd = 1 or 3, mode as the kernels' MODE.
int wino16_launch(const wino::Args& a, int mode, int kd, long long blocks, hipStream_t stream);
// Which of them that launch runs (wino16_launch itself and g6d_wino_multi_route ask): error = the launch's refusal, or nullptr
namespace wino {
struct Pick16 { const char* error; bool trunk, two_waves; int threads; size_t lds_bytes; };
}  // namespace wino
wino::Pick16 wino16_pick(const wino::Args& a, int mode, int kd);

namespace {

typedef wplan::Seg WinoSeg;
struct WinoArgs : wino::Args {};   // (unnamed namespace: the kernels' symbols stay private to their translation unit)

typedef float f32x2w __attribute__((ext_vector_type(2)));
#define f32x2 f32x2w
__device__ __forceinline__ f32x2 lo2(const f32x4& x) { return __builtin_shufflevector(x, x, 0, 1); }
__device__ __forceinline__ f32x2 hi2(const f32x4& x) { return __builtin_shufflevector(x, x, 2, 3); }
__device__ __forceinline__ f32x4 cat2(f32x2 a, f32x2 b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3); }
// a - b on two floats in one instruction (the compiler scalarises a two-float subtraction; the packed add takes the negation as
// an operand modifier).  Register-only, consumed a whole MFMA group later.
__device__ __forceinline__ f32x2 pk_add(f32x2 a, f32x2 b) {
  f32x2 r;
  asm("v_pk_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ f32x2 pk_sub(f32x2 a, f32x2 b) {
  f32x2 r;
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// quarter q of this block -> segment geometry, image, first output row / column, validity.  The quarters (8x8 output pixels)
// of all images of all segments form one flat list, four consecutive ones per block: no block-level padding on odd quarter
// counts, and small maps (<= 8x8 pixels = one quarter per image) simply put four images into a block.
struct QGeo { int n, oy0, ox0; bool valid; int H, W, ld_in, ld_full, ld_pool, in_off, full_off, pool_off; };
__device__ __forceinline__ QGeo quarter_of(const WinoArgs& p, int q, int nq = 4) {
  const int Q = blockIdx.x * nq + q;
  int sidx = 0;
#pragma unroll
  for (int k = 1; k < wplan::MAX_SEG; ++k) sidx = (k < p.nseg && Q >= p.seg[k].qstart) ? k : sidx;
  const WinoSeg& sg = p.seg[sidx];
  QGeo g;
  g.valid = Q < p.qtotal;
  const int Ql = g.valid ? Q - sg.qstart : 0;
  const int per = sg.QH * sg.QW;
  g.n = Ql / per;
  const int r = Ql - g.n * per;
  const int qy = r / sg.QW, qx = r - qy * sg.QW;
  g.oy0 = 8 * qy; g.ox0 = 8 * qx;
  g.H = sg.H; g.W = sg.W; g.ld_in = sg.ld_in; g.ld_full = sg.ld_full; g.ld_pool = sg.ld_pool;
  g.in_off = sg.in_off; g.full_off = sg.full_off; g.pool_off = sg.pool_off;
  return g;
}

}  // namespace
