// Test infrastructure: C wrappers over gen6d_amd/csrc/wino_plan.h (the host arithmetic of the Winograd launchers), built with g++ by
// tests/test_wino_plan_cpu.py.  Segments come in as rows of 5 ints (N, H, W, in_off, ld_in); ld_full / ld_pool / the output offsets take no
// part in the plan.
#include "../gen6d_amd/csrc/wino_plan.h"
using namespace wplan;

static void fill(Seg* seg, const int* rows, int nseg) {
  for (int k = 0; k < nseg; ++k) seg[k] = Seg{0, rows[5 * k], rows[5 * k + 1], rows[5 * k + 2], 0, 0, rows[5 * k + 3], 0, 0, rows[5 * k + 4], 0, 0};
}
static void geo_out(const Seg* seg, const Quarters& q, int nseg, long long* geo) {      // per segment: qstart, QH, QW, images read
  for (int k = 0; k < nseg; ++k) { geo[4 * k] = seg[k].qstart; geo[4 * k + 1] = seg[k].QH; geo[4 * k + 2] = seg[k].QW; geo[4 * k + 3] = q.n_in[k]; }
}

extern "C" {

// knobs: wino_wide, wino_split_max; model: gain, fix, per.  out: quarters, in_extent, blocks, grid2, nchunks, splits, chunks_per_split, wide, nq, nwn
const char* wp_f2_plan(const int* rows, int nseg, long long img_cap, int mm, int mode, int kd, int Cin, int Cout, int have_ws, size_t ws_bytes,
                       size_t counter_bytes, int counters, int wide, int split_max, double gain, double fix, double per, long long* out, long long* geo) {
  Seg seg[MAX_SEG];
  fill(seg, rows, nseg);
  const F2Plan p = f2_plan(seg, nseg, img_cap, mm, mode, kd, Cin, Cout, room(have_ws != 0, ws_bytes, counter_bytes), counters,
                           F2Knobs{wide, split_max, gain, fix, per});
  const long long o[10] = {p.q.quarters, p.q.in_extent, p.blocks, p.grid2, p.nchunks, p.split.splits, p.split.chunks_per_split, p.shape.wide, p.shape.nq,
                           p.shape.nwn};
  for (int i = 0; i < 10; ++i) out[i] = o[i];
  geo_out(seg, p.q, nseg, geo);
  return p.error;
}

// out: quarters, in_extent, blocks, grid2, nchunks, splits, chunks_per_split, nt
const char* wp_f4_plan(const int* rows, int nseg, int mode, int kd, int Cin, int Cout, int have_ws, size_t ws_bytes, size_t counter_bytes, int counters,
                       int split_max, double gain, double chunk_us, long long* out, long long* geo) {
  Seg seg[MAX_SEG];
  fill(seg, rows, nseg);
  const F4Plan p = f4_plan(seg, nseg, mode, kd, Cin, Cout, room(have_ws != 0, ws_bytes, counter_bytes), counters, F4Knobs{split_max, gain, chunk_us});
  const long long o[8] = {p.q.quarters, p.q.in_extent, p.blocks, p.grid2, p.nchunks, p.split.splits, p.split.chunks_per_split, p.nt};
  for (int i = 0; i < 8; ++i) out[i] = o[i];
  geo_out(seg, p.q, nseg, geo);
  return p.error;
}

void wp_split(int nchunks, long long grid2, int slots, size_t room_bytes, int counters, double tile_bytes, double out_bytes, double chunk_us,
              double block_us, double fix_us, double per_us, double gain, int split_max, int* out) {
  const Split s = split_search(nchunks, grid2, slots, room_bytes, counters, tile_bytes, out_bytes, SplitCost{chunk_us, block_us, fix_us, per_us, gain, split_max});
  out[0] = s.splits; out[1] = s.chunks_per_split;
}

const char* wp_f4_limits(long long quarters, long long in_extent, int kd, int Cin, int Cout, int mode) { return f4_limits(quarters, in_extent, kd, Cin, Cout, mode); }
const char* wp_w16_limits(int Cout, int mode, int Cin) { return w16_limits(Cout, mode, Cin); }

// kind 0: wino_conv3x3_kernel<mode, ., a = NWN, b = NWM>; 1: the 16-bit kernels of 256 threads; 2: wino16b; 3: wino43_kernel<mode, ., a = NT>
size_t wp_lds(int kind, int mode, int a, int b, int Cin) {
  return kind == 0 ? f2_lds_bytes(mode, a, b, Cin) : kind == 1 ? w16_lds_bytes(mode, Cin) : kind == 2 ? w16b_lds_bytes() : f4_lds_bytes(mode, a, Cin);
}

// The table copy on a table of the launchers' shape (G6dSegTable, seg_table.h): rows of 9 ints N, H, W, ld_in, ld_full, ld_pool, in_off,
// full_off, pool_off -> the 12 ints of every Seg; returns nseg, or -1 if a base pointer did not arrive
int wp_segments(const int* rows, int nseg, int* out) {
  struct Row { int N, H, W, ld_in, ld_full, ld_pool, in_off, full_off, pool_off; };
  struct Table { const float* in; float* full; float* pool; int nseg; Row seg[MAX_SEG]; } t = {};
  static float base[3];
  t.in = base; t.full = base + 1; t.pool = base + 2; t.nseg = nseg;
  for (int k = 0; k < nseg; ++k) {
    const int* r = rows + 9 * k;
    t.seg[k] = Row{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8]};
  }
  Seg seg[MAX_SEG] = {};
  int n = 0; const float* in = nullptr; float* full = nullptr; float* pool = nullptr;
  segments(t, seg, n, in, full, pool);
  static_assert(sizeof(Seg) == 12 * sizeof(int), "the kernels' argument blocks embed 12 ints per segment");
  for (int k = 0; k < nseg; ++k)
    for (int i = 0; i < 12; ++i) out[12 * k + i] = reinterpret_cast<const int*>(&seg[k])[i];
  return in == base && full == base + 1 && pool == base + 2 ? n : -1;
}

}  // extern "C"
