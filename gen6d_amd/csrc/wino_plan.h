// wino_plan.h — the host arithmetic of a Winograd launch, once, for the F(2x2,3x3) kernels (wino_conv.hip, wino16_conv.hip) and the
// F(4x4,3x3) kernel (wino43_conv.hip): the segment record of the kernels' argument blocks, the flat quarter list, the hard size limits,
// the F(2x2) block shape, the split of the chunk list over gridDim.z and the dynamic LDS sizes.  Plain C++17 with no HIP and no project
// header: knob values and the workspace's counter constants come in as arguments (tests/wino_plan_shim.cpp builds this header with g++
// and tests/test_wino_plan_cpu.py compares every choice with the launchers' arithmetic written out in Python).
#pragma once
#include <stddef.h>

namespace wplan {

// One map size of a launch.  A launch may cover up to MAX_SEG sizes (the scales of the detector's image pyramid run the same layer):
// their quarters (8x8 output pixels) form ONE flat list, so the small scales fill the blocks the large ones leave over instead of
// being four under-filled launches.  Offsets are in floats from the launch's common base pointers.
constexpr int MAX_SEG = 4;
struct Seg { int qstart, N, H, W, QH, QW, in_off, full_off, pool_off, ld_in, ld_full, ld_pool; };

// The segment list and bases of a multi-map launch from its validated table (G6dSegTable, seg_table.h)
template <class Table>
inline void segments(const Table& t, Seg (&seg)[MAX_SEG], int& nseg, const float*& in, float*& full, float*& pool) {
  in = t.in; full = t.full; pool = t.pool; nseg = t.nseg;
  for (int k = 0; k < t.nseg; ++k) {
    const auto& g = t.seg[k];
    seg[k] = Seg{0, g.N, g.H, g.W, 0, 0, g.in_off, g.full_off, g.pool_off, g.ld_in, g.ld_full, g.ld_pool};
  }
}

// The quarter list: fills QH, QW, qstart of every segment.  n_in: the images a segment actually reads, min(N, img_cap) when img_cap > 0
// (a query batch that shares img_mod * D input images), N otherwise; in_extent: floats from the input base to the end of the last read.
struct Quarters { long long quarters, in_extent; double out_elems; long long n_in[MAX_SEG]; };
inline Quarters quarter_list(Seg* seg, int nseg, long long img_cap) {
  Quarters q = {};
  for (int k = 0; k < nseg; ++k) {
    Seg& g = seg[k];
    const long long n_in = img_cap > 0 && img_cap < g.N ? img_cap : g.N;
    const long long end = (long long)g.in_off + n_in * g.H * g.W * g.ld_in;
    if (end > q.in_extent) q.in_extent = end;
    g.QH = (g.H + 7) / 8; g.QW = (g.W + 7) / 8;
    g.qstart = (int)q.quarters;
    q.quarters += (long long)g.N * g.QH * g.QW;
    q.out_elems += (double)g.N * g.H * g.W;
    q.n_in[k] = n_in;
  }
  return q;
}

// Workspace bytes behind the tile counters (0: no split possible)
inline size_t room(bool have_workspace, size_t workspace_bytes, size_t counter_bytes) {
  return have_workspace && workspace_bytes > counter_bytes ? workspace_bytes - counter_bytes : 0;
}

// Split of the (kd, chunk) list over gridDim.z.  One block per `slot` is resident and runs a serial loop over its chunks, so a launch
// takes ceil(grid / slots) rounds of (chunks per block) steps: small grids leave CUs idle and grids just above a multiple of the slots
// pay a nearly empty last round.  Picks the split count with the smallest modelled time: rounds x block time + the hand-off (partial
// images written and read back at 2.5 TB/s chip-wide, the serial re-read of a tile's slabs by its last block); a further split must buy
// 1 - gain.  grid2: blocks x channel slices (one counter each); tile_bytes: one partial image, padded to whole tiles; all times in us.
struct SplitCost { double chunk_us, block_us, fix_us, per_us, gain; int split_max; };
struct Split { int splits, chunks_per_split; };
inline Split split_search(int nchunks, long long grid2, int slots, size_t room, int counters, double tile_bytes, double out_bytes,
                          const SplitCost& c) {
  int splits = 1;
  if (room > 0 && grid2 <= counters && c.split_max > 1 && nchunks >= 4) {
    double best = 1e30;
    for (int sp = 1; sp <= c.split_max && sp <= nchunks / 2; ++sp) {
      if ((double)sp * tile_bytes > (double)room) break;
      const int cps_ = (nchunks + sp - 1) / sp, real = (nchunks + cps_ - 1) / cps_;
      if (real != sp) continue;
      const double rounds = (double)((grid2 * sp + slots - 1) / slots);
      double t = rounds * (cps_ * c.chunk_us + c.block_us);
      if (sp > 1) t += c.fix_us + c.per_us * sp + (2 * sp + 1) * out_bytes / 2.5e6;
      if (t < best * c.gain) { best = t; splits = sp; }
    }
  }
  const int cps = (nchunks + splits - 1) / splits;
  return Split{(nchunks + cps - 1) / cps, cps};
}

// ---- dynamic LDS, in bytes.  All kernels stage the RAW 10x10 patch of a quarter at a stride of 101 positions x 8 floats.
constexpr size_t LDS_MAX = 160 * 1024;
constexpr int F2_RAW_FLOATS = 4 * 101 * 8;            // four quarters (one 8-channel plane)
constexpr int F4_NQ = 8, F4_RAWF = 28 * 64 * 4;       // F(4x4): quarters per block, floats of its raw patch region
// affine tables (scale, shift) of operand prologue `mode`: one pair, or one pair per quarter of the block (mode >= 2)
constexpr size_t affine_floats(int mode, int quarters, int Cin) { return mode == 0 ? 0 : (size_t)(mode >= 2 ? 2 * quarters : 2) * Cin; }
// wino_conv3x3_kernel<MODE, KD, NWN, NWM>: two stages of (raw patches of 2 NWM quarters, [ab][32 NWN co][8] filters, a dump row of 16
// bytes per thread), the tables and Cin floats more
constexpr size_t f2_lds_bytes(int mode, int nwn, int nwm, int Cin) {
  const size_t stage = (size_t)(nwm * F2_RAW_FLOATS / 2 + 16 * 32 * nwn * 8 + 4 * (64 * nwm * nwn));
  return (2 * stage + affine_floats(mode, 2 * nwm, Cin) + (mode == 0 ? 0 : Cin)) * sizeof(float);
}
// wino16_conv3x3_kernel<MM, 2> and wino16_conv_kernel: two stages of (two raw planes, 64-channel filters, dump row of 256 threads)
constexpr size_t w16_lds_bytes(int mode, int Cin) {
  return (2 * (size_t)(2 * F2_RAW_FLOATS + 16 * 64 * 8 + 4 * 256) + affine_floats(mode, 4, Cin)) * sizeof(float);
}
// wino16b_conv3x3_kernel: ONE raw stage, three filter stages + V, a scratch row
constexpr size_t w16b_lds_bytes() { return (size_t)(2 * F2_RAW_FLOATS + 4 * (16 * 64 * 8) + 256) * sizeof(float); }
// wino43_kernel<MODE, KD, NT> (beside 512 B of static LDS): the raw region twice, two filter half-stages of 18 positions x 16 NT
// channels, the tables
constexpr size_t f4_lds_bytes(int mode, int nt, int Cin) {
  return ((size_t)2 * F4_RAWF + 2 * (18 * 16 * nt * 8) + affine_floats(mode, F4_NQ, Cin)) * sizeof(float);
}

// Each size is the sum the launchers spelled out before this header existed, for every instantiation that is launched (the table part
// is linear in Cin: two points hold it)
#define WPLAN_F2_IS(MODE, NWN, NWM, CIN) static_assert(f2_lds_bytes(MODE, NWN, NWM, CIN) == (2 * (size_t)(2 * NWM * 101 * 8 + 16 * 32 * NWN * 8 + \
  4 * (64 * NWM * NWN)) + (MODE == 0 ? 0 : (MODE >= 2 ? 4 * NWM : 2) * CIN + CIN)) * sizeof(float), "wino_conv3x3_kernel LDS")
#define WPLAN_F2_ALL(MODE) WPLAN_F2_IS(MODE, 1, 2, 8); WPLAN_F2_IS(MODE, 1, 2, 1024); WPLAN_F2_IS(MODE, 2, 2, 8); WPLAN_F2_IS(MODE, 2, 2, 1024)
WPLAN_F2_ALL(0); WPLAN_F2_ALL(1); WPLAN_F2_ALL(2); WPLAN_F2_ALL(3); WPLAN_F2_IS(0, 4, 1, 8); WPLAN_F2_IS(0, 4, 1, 1024);
#define WPLAN_W16_IS(MODE, CIN) static_assert(w16_lds_bytes(MODE, CIN) == (2 * (size_t)(2 * (4 * 101 * 8) + 16 * 64 * 8 + 4 * 256) + \
  (MODE == 0 ? 0 : (MODE >= 2 ? 8 : 2) * CIN)) * sizeof(float), "wino16 LDS")
WPLAN_W16_IS(0, 16); WPLAN_W16_IS(1, 16); WPLAN_W16_IS(2, 16); WPLAN_W16_IS(3, 16);
WPLAN_W16_IS(0, 1024); WPLAN_W16_IS(1, 1024); WPLAN_W16_IS(2, 1024); WPLAN_W16_IS(3, 1024);
static_assert(w16b_lds_bytes() == (size_t)(2 * (4 * 101 * 8) + 4 * 16 * 64 * 8 + 256) * sizeof(float), "wino16b LDS");
#define WPLAN_F4_IS(MODE, NT, CIN) static_assert(f4_lds_bytes(MODE, NT, CIN) == ((size_t)2 * (28 * 64 * 4) + 2 * (18 * 16 * NT * 8) + \
  (MODE == 0 ? 0 : (MODE >= 2 ? 2 * 8 : 2) * CIN)) * sizeof(float) && f4_lds_bytes(MODE, NT, CIN) == (size_t)(MODE == 0 ? 0 : \
  (MODE >= 2 ? 2 * 8 : 2)) * CIN * 4 + ((size_t)2 * (28 * 64 * 4) + 2 * 18 * 16 * NT * 8) * 4, "wino43_kernel LDS")
WPLAN_F4_IS(0, 4, 8); WPLAN_F4_IS(1, 4, 8); WPLAN_F4_IS(2, 4, 8); WPLAN_F4_IS(0, 2, 8);
WPLAN_F4_IS(0, 4, 256); WPLAN_F4_IS(1, 4, 256); WPLAN_F4_IS(2, 4, 256); WPLAN_F4_IS(0, 2, 256);
#undef WPLAN_F2_IS
#undef WPLAN_F2_ALL
#undef WPLAN_W16_IS
#undef WPLAN_F4_IS

// ---- F(2x2,3x3): wino_conv3x3_kernel (fp32) and the three 16-bit kernels
// Block shape: four quarters x 64 (32) channels, or — fp32 trunk layers with Cout % 128 == 0 — two quarters x 128 channels: the same
// four waves and accumulators, half the raw patch and twice the filter tile per chunk, and the layer's input is re-read Cout / 128
// times.  wino_wide (knob; tests force both shapes): 0 = never, 2 = whenever eligible, else where the input is large against the filter
// bank (measured per layer, tools/wino_split_probe.py and BATCH=8 tools/layer_table.py with G6D_WINO_WIDE=0/1: -1.5 ... -6 % there — the
// detector's pyramid, the first layers of the crops' trunks; +1 ... 2 % where the doubled filter stream per block dominates: 16x16 and
// 8x8 maps of a few crops).  nwn = channel width of a block in 32s: 32-channel (two-wave) blocks only for channel counts that are not
// multiples of 64 — two of them share a CU, so they do not spread a small grid over more CUs; the split over the chunks does.
struct Shape { bool wide; int nq, nwn; };
inline Shape f2_shape(int wino_wide, int mm, int mode, int kd, int Cin, int Cout, long long in_extent) {
  const bool wide_on = wino_wide != 0, wide_all = wino_wide == 2;
  const bool wide = wide_on && !mm && mode == 0 && kd == 1 && (Cout & 127) == 0 && (wide_all || in_extent >= 6ll * 16 * Cin * Cout);
  return Shape{wide, wide ? 2 : 4, wide ? 4 : ((Cout & 63) ? 1 : 2)};
}

inline const char* f2_limits(long long blocks, long long in_extent) {
  if (blocks > 0x3fffffffll) return "wino_conv3x3: grid too large";
  if (in_extent * 4 >= (1ll << 31)) return "wino_conv3x3: input tensor exceeds 2^31 bytes";
  return nullptr;
}
// the 16-bit kernels' own limits (64-channel blocks only; the tables of the block's four quarters beside the stages)
inline const char* w16_limits(int Cout, int mode, int Cin) {
  if (Cout & 63) return "wino16: Cout % 64 == 0 expected";
  if (w16_lds_bytes(mode, Cin) > LDS_MAX) return "wino16: affine tables do not fit LDS";
  return nullptr;
}

// The whole launch plan: quarter list (fills seg), block shape, limits, split.  mm: 0 fp32, 1 / 2 the 16-bit kernels, whose chunk is a
// pair of 8-channel chunks at ~1.2 us against ~2.7 us; a block pays ~4 us of prologue / epilogue; 64-channel blocks hold a CU each, two
// 32-channel blocks share one.  error: nullptr, or the launch must be refused with that message (the fields behind it are then unset).
struct F2Knobs { int wide, split_max; double gain, fix_us, per_us; };       // wino_wide, wino_split_max / _gain / _fix / _per
struct F2Plan { const char* error; Quarters q; Shape shape; long long blocks, grid2; int nchunks; Split split; };
inline F2Plan f2_plan(Seg* seg, int nseg, long long img_cap, int mm, int mode, int kd, int Cin, int Cout, size_t room, int counters,
                      const F2Knobs& k) {
  F2Plan p = {};
  p.q = quarter_list(seg, nseg, img_cap);
  p.shape = f2_shape(k.wide, mm, mode, kd, Cin, Cout, p.q.in_extent);
  p.blocks = (p.q.quarters + p.shape.nq - 1) / p.shape.nq;
  if ((p.error = f2_limits(p.blocks, p.q.in_extent))) return p;
  const int nwn = p.shape.nwn;
  p.nchunks = mm ? kd * (Cin / 16) : kd * (Cin / 8);
  p.grid2 = p.blocks * (Cout / (32 * nwn));
  const double tile_bytes = (double)p.grid2 * (p.shape.wide ? 256 : 128 * nwn) * 64 * sizeof(float);
  const double out_bytes = p.q.out_elems * Cout * sizeof(float);
  p.split = split_search(p.nchunks, p.grid2, 256 * (nwn == 1 ? 2 : 1), room, counters, tile_bytes, out_bytes,
                         SplitCost{mm ? 1.2 : 2.7, 4.0, k.fix_us, k.per_us, k.gain, k.split_max});
  return p;
}

// ---- F(4x4,3x3): wino43_kernel, blocks of F4_NQ quarters x 16 nt channels
// The hard size limits of a launch, shared by the launcher (error) and g6d_wino43_eligible (fall back to another kernel): 32-bit grid,
// the 2^31-byte reach of the buffer loads on input and filter bank, the affine tables beside the stages in LDS.  nullptr = fits.
inline const char* f4_limits(long long quarters, long long in_extent_floats, int kd, int Cin, int Cout, int mode) {
  if ((quarters + F4_NQ - 1) / F4_NQ > 0x3fffffffll) return "wino43: grid too large";
  if (in_extent_floats * 4 >= (1ll << 31)) return "wino43: input tensor exceeds 2^31 bytes";
  if ((long long)kd * (Cin / 8) * 36 * Cout * 32 >= (1ll << 31)) return "wino43: filter bank exceeds 2^31 bytes";
  if (mode != 0 && f4_lds_bytes(mode, (Cout & 63) ? 2 : 4, Cin) > LDS_MAX - 512) return "wino43: affine tables do not fit LDS";
  return nullptr;
}

// One block per CU is resident and runs a serial loop of chunk_us (knob w43_chunk_us, ~2.6 us) per chunk at nt = 4, 0.55 of it at
// nt = 2, with ~6 us of prologue / epilogue
struct F4Knobs { int split_max; double gain, chunk_us; };                   // w43_split_max / _gain, w43_chunk_us
struct F4Plan { const char* error; Quarters q; int nt; long long blocks, grid2; int nchunks; Split split; };
inline F4Plan f4_plan(Seg* seg, int nseg, int mode, int kd, int Cin, int Cout, size_t room, int counters, const F4Knobs& k) {
  F4Plan p = {};
  p.q = quarter_list(seg, nseg, 0);
  p.blocks = (p.q.quarters + F4_NQ - 1) / F4_NQ;
  p.nt = (Cout & 63) ? 2 : 4;
  if ((p.error = f4_limits(p.q.quarters, p.q.in_extent, kd, Cin, Cout, mode))) return p;
  p.nchunks = kd * (Cin / 8);
  p.grid2 = p.blocks * (Cout / (16 * p.nt));
  const double tile_bytes = (double)p.grid2 * 256 * p.nt * 32 * sizeof(float);
  const double out_bytes = p.q.out_elems * Cout * sizeof(float);
  p.split = split_search(p.nchunks, p.grid2, 256, room, counters, tile_bytes, out_bytes,
                         SplitCost{p.nt == 4 ? k.chunk_us : 0.55 * k.chunk_us, 6.0, 2.0, 0.6, k.gain, k.split_max});
  return p;
}

}  // namespace wplan
