// conv16_direct.hip — direct (implicit-GEMM) 3x3 / 3x3x3 convolution on 16-bit ACTIVATIONS: the reduced-precision mode's own kernel
// family (round 6; BASELINE configs[2] "bf16" / configs[4] "fp16 MFMA convs").
//
// Replaces, in the reduced-precision mode only, the VGG trunks' 3x3 layers (reference network/pretrain_models.py:9-31,66-72; detector
// pyramid detector.py:188-197,236-241; refiner crops refiner.py:64-78) and the first convs of the refiner's 32^3 volume net
// (refiner.py:88-143).  Until round 5 that mode kept fp32 activations in HBM and LDS and rounded operands when fragments left LDS:
// its 16-bit Winograd kernels were bound by LDS WRITES of fp32 data.  Here activations are fp16 / bf16 NHWC in HBM:
//   * both operand tiles of a K step go global -> LDS by DMA (buffer_load_dwordx4 ... lds: no VGPR round trip, no ds_write, no
//     conversion), 16 bytes = 8 channels per lane; zero padding and ragged tile edges are the buffer's out-of-range zero fill;
//   * K step = 64 input channels of ONE tap (128 B per pixel row and per filter row): the LDS image [row][8 slots of 16 B] is lane-linear
//     as the DMA demands, and bank-conflict free for the ds_read_b128 fragment reads because the lane that FILLS slot s of row r fetches
//     channel group s ^ ((r >> 1) & 7) — the swizzle sits on the source address (cdna_hip_programming.md rule 21);
//   * v_mfma_f32_32x32x16_{f16,bf16}, fp32 accumulation; block = 128 output pixels x 128 output channels, 4 waves of 64 x 64 (2 x 2
//     accumulator tiles), two LDS stages of 32 KB, two blocks per CU (the second block's MFMAs cover this block's barrier / DMA waits);
//   * a tile is TH x TW pixels (TH TW = 128, TW a power of two chosen per map width) of the "tall image" [N D H rows][W columns], so 2x2
//     max-pool windows never straddle tiles and small maps pack several images into one tile;
//   * epilogue through LDS: bias, ReLU, then 16-byte stores of the full map (16-bit or fp32) and / or the 2x2 max-pooled map, and
//     optionally per-(image group, channel) sum / sum of squares in fp64 for the InstanceNorm that follows (volume net).
// K order: input-channel slice outermost, taps innermost — the nine shifted reads of a 16 KB slice hit L1 / L2.
// This file: the family's entry points and launcher.  The per-tap kernels live in conv16_tap.hip, the halo-patch kernel (fragment-major
// filters on maps it can tile: the fp32 path's trunks, selector stacks and refiner nets) in conv16w.hip, what they share in conv16_common.h.
#include "conv16_common.h"

namespace {
// What g6d_conv16_direct_route reports, filled from the parameter block the launch would carry (kernel: the plan's answer)
void c16_report(G6dConv16Route* r, const c16::Params& p, int kernel, int w_layout, int math_mode, int wm, bool half_tile, bool folded, int blocks) {
  if (!r) return;
  *r = G6dConv16Route{};
  r->kernel = kernel; r->w_layout = w_layout; r->math_mode = math_mode; r->kd = p.kd; r->wm = wm; r->half_tile = half_tile; r->folded = folded;
  r->tiles = p.ptiles; r->nN = p.nN; r->blocks = blocks;
  for (int i = 0; i < p.nseg; ++i) {
    const C16Seg& s = p.seg[i];
    if (kernel) r->seg[i] = {s.h_tile0, s.h_tw_log2, s.h_tiles_x, s.h_tpi, s.h_segh_log2, s.h_bands};
    else r->seg[i] = {s.tile0, s.tw_log2, s.tiles_x, 0, 0, 0};
  }
}

// g6d_conv16_direct_multi_ex; plan_only: validate and choose the kernel, launch nothing (g6d_conv16_direct_plan's return value; route: also
// report the choice, g6d_conv16_direct_route)
int c16_direct(const G6dConv16Seg* segs, int nseg, int Cin, const void* W16, int w_layout, float acc_scale, const float* bias, int Cout, int kd, int relu,
               int full_type, int pool_type, int math_mode, double* stats, int stat_rows_per_group, const G6dRange16* range, g6d_stream_t stream,
               bool plan_only, G6dConv16Route* route = nullptr) {
  if (!segs || nseg < 1 || nseg > 4 || !W16) { g6d_set_error("conv16_direct: 1..4 segments and filters expected"); return G6D_EINVAL; }
  if (Cin < 1 || Cout < 1 || !g6d_aligned16(W16)) { g6d_set_error("conv16_direct: bad args (Cin, Cout >= 1, 16-byte aligned filters)"); return G6D_EINVAL; }
  // w_layout 2: fragment-major filters of a 3x3x3 layer packed as the 2-D bank [Cout][9][3 Cin], channel order (dz, ci) — the pair
  // kernel folds the depth taps into its reduction (conv16w_kernel<3, ., 1, 3>)
  const bool folded = w_layout == 2;
  if (math_mode < 1 || math_mode > 3 || w_layout < 0 || w_layout > 2 || (math_mode == 3 && w_layout == 0) || (folded && (math_mode != 3 || kd != 3))) {
    g6d_set_error("conv16_direct: math_mode 1 (bf16) / 2 (fp16) / 3 (fp16 hi-lo pairs, fragment-major filters only)"); return G6D_EINVAL;
  }
  const int bk = math_mode == 3 ? 32 : C16_BK, planes = math_mode == 3 ? 2 : 1;
  // Cout = 64 (the selector's first product layer): halo-patch kernel only, filters packed as one 128-channel tile whose upper half is zero
  const bool half_tile = Cout == 64 && ((w_layout == 1 && kd == 1) || folded);      // (32-channel waves: two pixel tiles x two channel groups per block)
  if (Cin % bk || (Cout % C16_BN && !half_tile) || (kd != 1 && kd != 3)) { g6d_set_error("conv16_direct: Cin % 64 (32 for pairs), Cout % 128 (64: fragment-major 2-D layers), kd in {1,3} expected"); return G6D_EINVAL; }
  const int t16 = math_mode == 3 ? 3 : 1;                    // the 16-bit output coding of this mode
  auto type_ok = [&](int t) { return t == 0 || t == 2 || t == t16; };
  if (!type_ok(full_type) || !type_ok(pool_type) || (!full_type && !pool_type && !stats)) { g6d_set_error("conv16_direct: output types"); return G6D_EINVAL; }
  if (pool_type && kd != 1) { g6d_set_error("conv16_direct: pooling is 2-D only"); return G6D_EINVAL; }
  c16::Params p = {};
  p.nseg = nseg; p.Cin = Cin; p.Cout = Cout; p.kd = kd; p.relu = relu; p.full_type = full_type; p.pool_type = pool_type;
  p.w = static_cast<const char*>(W16); p.bias = bias; p.stats = stats; p.stat_rows_per_group = stat_rows_per_group;
  p.acc_scale = acc_scale != 0.f ? acc_scale : 1.f;
  p.ablate = (int)g6d_knob(G6D_KNOB_C16_ABLATE);
  if (range) p.rng = *range;
  const long wb = (long)(half_tile ? 128 : Cout) * 9 * kd * Cin * 2 * planes;
  if (wb >= (1L << 31)) { g6d_set_error("conv16_direct: filters beyond 2 GB"); return G6D_EINVAL; }
  p.w_bytes = (unsigned)wb;
  p.nN = Cout / C16_BN;
  int tiles = 0, D0 = segs[0].D;
  bool pertap_stats_ok = true;
  for (int i = 0; i < nseg; ++i) {
    const G6dConv16Seg& s = segs[i];
    C16Seg& o = p.seg[i];
    if (!s.in || s.N < 1 || s.D < 1 || s.H < 1 || s.W < 1 || s.ld_in < planes * Cin || s.D != D0 || (kd == 1 && s.D != 1)) { g6d_set_error("conv16_direct: bad segment"); return G6D_EINVAL; }
    const int need_full = full_type == 3 ? 2 * Cout : Cout, need_pool = pool_type == 3 ? 2 * Cout : Cout;
    if ((full_type && (!s.out_full || s.ld_full < need_full)) || (pool_type && (!s.out_pool || s.ld_pool < need_pool || (s.H & 1) || (s.W & 1)))) {
      g6d_set_error("conv16_direct: outputs missing / odd map with pooling"); return G6D_EINVAL;
    }
    if (!g6d_aligned16(s.in) || (s.ld_in & 7) || (full_type && (!g6d_aligned16(s.out_full) || (s.ld_full & 7))) || (pool_type && (!g6d_aligned16(s.out_pool) || (s.ld_pool & 7)))) {
      g6d_set_error("conv16_direct: 16-byte aligned rows expected"); return G6D_EINVAL;
    }
    // (the epilogues address an output from the tile's first pixel with 32-bit offsets: at most 32 rows of W pixels)
    if (32L * s.W * (s.ld_full > s.ld_pool ? s.ld_full : s.ld_pool) * 4 >= (1L << 32)) { g6d_set_error("conv16_direct: 32 output rows beyond 4 GB"); return G6D_EINVAL; }
    o.in = static_cast<const char*>(s.in); o.full = static_cast<char*>(s.out_full); o.pool = static_cast<char*>(s.out_pool);
    o.H = s.H; o.W = s.W; o.DH = s.D * s.H; o.rows = s.N * s.D * s.H;
    o.ld_in = s.ld_in; o.ld_full = s.ld_full; o.ld_pool = s.ld_pool;
    const int tw = c16g::pick_tw(s.W);
    int l2 = 0; while ((1 << l2) < tw) ++l2;
    o.tw_log2 = l2; o.tiles_x = (s.W + tw - 1) / tw; o.tile0 = tiles;
    const int th = C16_BM / tw;
    // (the per-tap kernels flush a tile's statistics under ONE group; the halo-patch kernel has its own rule below)
    if (stats && stat_rows_per_group > 0 && ((long)stat_rows_per_group % ((long)th * s.W) != 0)) pertap_stats_ok = false;
    tiles += o.tiles_x * ((o.rows + th - 1) / th);
    // the descriptor starts (kd == 3 ? H W : 0) + W + 1 pixels before the tensor: tap offsets are then non-negative
    const long back = ((long)(kd == 3 ? s.H * s.W : 0) + s.W + 1) * s.ld_in * 2;
    const long ext = (long)o.rows * s.W * s.ld_in * 2 + back;
    if (ext >= (1L << 31)) { g6d_set_error("conv16_direct: a segment's input beyond 2 GB"); return G6D_EINVAL; }
    o.back = (int)back; o.in_bytes = (unsigned)ext;
  }
  p.D = D0;
  p.ptiles = tiles;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // fragment-major filters, 2-D layer: the halo-patch kernel when every segment has a tiling for it (knob conv16_halo = 0: never)
  if (((w_layout == 1 && kd == 1) || folded) && g6d_knob(G6D_KNOB_CONV16_HALO) != 0) {
    const C16wAdmit a = c16w_admit(p, segs, math_mode == 3, folded);
    if (!a.ok && half_tile) { g6d_set_error("conv16_direct: Cout = 64 needs a halo tiling for every segment"); return G6D_EINVAL; }
    if (a.ok) {
      // a block = 4 waves of 128 px x 64 ch (pairs, Cout = 64: 32 ch): one pixel tile x 256 (128) channels, or two pixel tiles x 128 channels
      const int cw = (half_tile || math_mode == 3) ? 32 : 64;
      const int wm = Cout % (4 * cw) == 0 ? 1 : 2;
      p.ptiles = a.tiles;
      p.nN = Cout / (cw * (4 / wm));
      c16_report(route, p, a.per_pass ? 2 : 1, w_layout, math_mode, wm, half_tile, folded, c16::halo_grid(p, wm));
      if (plan_only) return a.per_pass ? 2 : 1;
      return c16w_launch(p, math_mode, wm, half_tile, folded, st);
    }
  }
  if (folded) { g6d_set_error("conv16_direct: depth-folded filters run on the halo-patch kernel only (planes at least one tile high, statistics groups of whole volumes)"); return G6D_EINVAL; }
  if (half_tile) { g6d_set_error("conv16_direct: Cout = 64 runs on the halo-patch kernel only (knob conv16_halo, tile shapes)"); return G6D_EINVAL; }
  if (!pertap_stats_ok) { g6d_set_error("conv16_direct: statistics groups must be whole tile rows (small maps: whole 64-pixel epilogue passes)"); return G6D_EINVAL; }
  c16_report(route, p, 0, w_layout, math_mode, 1, false, false, c16::tap_grid(p));
  if (plan_only) return 0;
  return c16tap_launch(p, w_layout, math_mode, st);
}
}  // namespace

extern "C" int g6d_conv16_direct_multi_ex(const G6dConv16Seg* segs, int nseg, int Cin, const void* W16, int w_layout, float acc_scale,
                                          const float* bias, int Cout, int kd, int relu, int full_type, int pool_type, int math_mode, double* stats,
                                          int stat_rows_per_group, const G6dRange16* range, g6d_stream_t stream) {
  return c16_direct(segs, nseg, Cin, W16, w_layout, acc_scale, bias, Cout, kd, relu, full_type, pool_type, math_mode, stats, stat_rows_per_group, range,
                    stream, false);
}

extern "C" int g6d_conv16_direct_plan(const G6dConv16Seg* segs, int nseg, int Cin, const void* W16, int w_layout, int Cout, int kd, int full_type,
                                      int pool_type, int math_mode, double* stats, int stat_rows_per_group) {
  return c16_direct(segs, nseg, Cin, W16, w_layout, 1.f, nullptr, Cout, kd, 0, full_type, pool_type, math_mode, stats, stat_rows_per_group, nullptr,
                    nullptr, true);
}

extern "C" int g6d_conv16_direct_route(const G6dConv16Seg* segs, int nseg, int Cin, const void* W16, int w_layout, int Cout, int kd, int full_type,
                                       int pool_type, int math_mode, double* stats, int stat_rows_per_group, G6dConv16Route* route) {
  if (!route) { g6d_set_error("conv16_direct_route: route expected"); return G6D_EINVAL; }
  const int rc = c16_direct(segs, nseg, Cin, W16, w_layout, 1.f, nullptr, Cout, kd, 0, full_type, pool_type, math_mode, stats, stat_rows_per_group, nullptr,
                            nullptr, true, route);
  return rc < 0 ? rc : G6D_OK;
}

extern "C" int g6d_sizeof_conv16_route(void) { return (int)sizeof(G6dConv16Route); }

extern "C" int g6d_conv16_direct_multi(const G6dConv16Seg* segs, int nseg, int Cin, const void* W16, int w_layout, float acc_scale,
                                       const float* bias, int Cout, int kd, int relu, int full_type, int pool_type, int math_mode, double* stats,
                                       int stat_rows_per_group, g6d_stream_t stream) {
  return g6d_conv16_direct_multi_ex(segs, nseg, Cin, W16, w_layout, acc_scale, bias, Cout, kd, relu, full_type, pool_type, math_mode, stats,
                                    stat_rows_per_group, nullptr, stream);
}
