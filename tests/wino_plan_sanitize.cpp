// Test infrastructure: a stand-alone host program that runs the launch plans of gen6d_amd/csrc/wino_plan.h (f2_plan for the F(2x2,3x3)
// kernels, f4_plan for the F(4x4,3x3) kernel) over the axes of tests/test_wino_plan_cpu.py and over extreme shapes (quarter totals near
// 2^31, ld_in far above Cin, in_off near 2^29 floats, workspaces of every size), and checks what the kernels rely on.  Meant for the
// sanitizers:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tests/wino_plan_sanitize.cpp -o wplan_san && ./wplan_san
// (tests/test_wino_plan_cpu.py builds and runs it that way).  Prints the number of plans made; exit status 1 on a broken invariant.
#include "../gen6d_amd/csrc/wino_plan.h"
#include <cstdio>
#include <initializer_list>
using namespace wplan;

static long n_plans = 0, n_refused = 0, n_bad = 0;
static const size_t COUNTER_BYTES = 16384;
static const int COUNTERS = 4096;

static void broken(const char* what, const Seg* seg, int nseg, int Cin, int Cout, int kd) {
  ++n_bad;
  std::printf("broken (%s): %d seg, N %d %dx%d, Cin %d Cout %d kd %d\n", what, nseg, seg[0].N, seg[0].H, seg[0].W, Cin, Cout, kd);
}

static void check_common(const char* what, const Seg* seg, int nseg, const Quarters& q, const Split& s, int nchunks, long long grid2, double tile_bytes,
                         size_t room_bytes, int Cin, int Cout, int kd) {
  bool ok = s.splits >= 1 && (long long)s.splits * s.chunks_per_split >= nchunks && nchunks > (long long)(s.splits - 1) * s.chunks_per_split;
  if (s.splits > 1) ok = ok && (double)s.splits * tile_bytes <= (double)room_bytes && grid2 <= COUNTERS;
  long long end = 0;
  for (int k = 0; k < nseg; ++k) {
    ok = ok && seg[k].qstart == (int)end && (k == 0 || seg[k].qstart > seg[k - 1].qstart) && seg[k].QH * 8 >= seg[k].H && seg[k].QW * 8 >= seg[k].W;
    end += (long long)seg[k].N * seg[k].QH * seg[k].QW;
  }
  ok = ok && end == q.quarters && q.in_extent * 4 < (1ll << 31);
  if (!ok) broken(what, seg, nseg, Cin, Cout, kd);
}

static void check(const Seg* in, int nseg, long long img_cap, int Cin, int Cout, int kd, size_t ws_bytes) {
  const size_t room_bytes = room(ws_bytes != 0, ws_bytes, COUNTER_BYTES);
  for (int mm = 0; mm < 3; ++mm)
    for (int mode = 0; mode < 4; ++mode)
      for (int wide = 0; wide < 3; ++wide) {
        if (mm && (Cin & 15)) continue;
        Seg seg[MAX_SEG];
        for (int k = 0; k < nseg; ++k) seg[k] = in[k];
        const F2Plan p = f2_plan(seg, nseg, img_cap, mm, mode, kd, Cin, Cout, room_bytes, COUNTERS, F2Knobs{wide, 32, 0.85, 2.0, 0.6});
        ++n_plans;
        if (p.error) { ++n_refused; continue; }
        const int nwn = p.shape.nwn;
        if (p.blocks * p.shape.nq < p.q.quarters || p.blocks > 0x3fffffffll || Cout % (32 * nwn) || (p.shape.wide && (mm || mode || kd != 1 || wide == 0)))
          broken("f2 shape", seg, nseg, Cin, Cout, kd);
        check_common("f2", seg, nseg, p.q, p.split, p.nchunks, p.grid2, (double)p.grid2 * (p.shape.wide ? 256 : 128 * nwn) * 64 * 4, room_bytes, Cin, Cout, kd);
        if (mm) (void)w16_limits(Cout, mode, Cin);
      }
  for (int mode = 0; mode < 3; ++mode) {
    Seg seg[MAX_SEG];
    for (int k = 0; k < nseg; ++k) seg[k] = in[k];
    const F4Plan p = f4_plan(seg, nseg, mode, kd, Cin, Cout, room_bytes, COUNTERS, F4Knobs{32, 0.85, 2.8});
    ++n_plans;
    if (p.error) { ++n_refused; continue; }
    if (p.blocks * F4_NQ < p.q.quarters || Cout % (16 * p.nt) || f4_lds_bytes(mode, p.nt, Cin) > LDS_MAX - 512) broken("f4 shape", seg, nseg, Cin, Cout, kd);
    check_common("f4", seg, nseg, p.q, p.split, p.nchunks, p.grid2, (double)p.grid2 * 256 * p.nt * 32 * 4, room_bytes, Cin, Cout, kd);
  }
}

int main() {
  const int sizes[] = {1, 2, 6, 7, 8, 9, 15, 16, 17, 32, 60, 120}, couts[] = {32, 64, 96, 128, 512}, kds[] = {1, 3, 9, 25};
  const size_t wss[] = {0, COUNTER_BYTES, COUNTER_BYTES + 1, (size_t)1 << 20, (size_t)96 << 20, ~(size_t)0};
  unsigned r = 12345;
  auto next = [&](unsigned n) { r = r * 1664525u + 1013904223u; return (r >> 8) % n; };
  for (int N : {1, 3, 7, 56, 448})
    for (int H : sizes)
      for (int W : sizes)
        for (int Cin : {8, 16, 64, 128, 256, 512}) {
          const int Cout = couts[next(5)], kd = kds[next(4)], nseg = 1 + (int)next(4);
          Seg seg[MAX_SEG];
          long long off = 0;
          const int ld_in = Cin + 4 * (int)next(3);
          for (int k = 0; k < nseg; ++k) {
            const int h = k ? sizes[next(12)] : H, w = k ? sizes[next(12)] : W;
            seg[k] = Seg{0, N, h, w, 0, 0, (int)(off < (1ll << 29) ? off : 1ll << 29), 0, 0, ld_in, Cout, Cout};
            off += (long long)N * h * w * ld_in;
          }
          check(seg, nseg, next(3) ? 0 : 1 + next(20), Cin, Cout, kd, wss[next(6)]);
        }
  // extremes: quarter totals near 2^31 and beyond the grid limit, rows far longer than Cin, offsets at the end of the buffer loads' reach
  const Seg big[][MAX_SEG] = {
      {{0, 0x7fffffff, 1, 1, 0, 0, 0, 0, 0, 8, 64, 64}},
      {{0, 0x7fffffff, 8, 8, 0, 0, 0, 0, 0, 8, 64, 64}, {0, 0x7fffffff, 8, 8, 0, 0, 0, 0, 0, 8, 64, 64}, {0, 0x7fffffff, 9, 9, 0, 0, 0, 0, 0, 8, 64, 64},
       {0, 0x7fffffff, 17, 17, 0, 0, 0, 0, 0, 8, 64, 64}},
      {{0, (1 << 26) - 1, 1, 1, 0, 0, 0, 0, 0, 8, 64, 64}, {0, 1, 8, 8, (1 << 29) - 520, 0, 0, 8, 64, 64}},
      {{0, 1, 32, 32, (1 << 29) - (1 << 19), 0, 0, 512, 64, 64}},
      {{0, 1, 32, 32, (1 << 29) - (1 << 19) - 4, 0, 0, 512, 64, 64}},
      {{0, 2, 6, 6, 0, 0, 0, 0, 0, 1 << 22, 64, 64}, {0, 1, 1, 1, (1 << 29) - 8, 0, 0, 1 << 22, 64, 64}},
      {{0, 1, 16384, 16384, 0, 0, 0, 0, 0, 8, 64, 64}},
      {{0, 1 << 20, 16, 16, 0, 0, 0, 0, 0, 8, 64, 64}},
  };
  const int nsegs[] = {1, 4, 2, 1, 1, 2, 1, 1};
  for (int i = 0; i < 8; ++i)
    for (int Cin : {8, 16, 1024, 4096})
      for (int Cout : {32, 64, 128, 1 << 15})
        for (int kd : {1, 3, 25})
          for (size_t ws : wss) check(big[i], nsegs[i], i & 1 ? (1ll << 40) : 0, Cin, Cout, kd, ws);
  // the split search alone, on chunk lists and grids no launch of today reaches
  for (int nchunks : {1, 3, 4, 5, 1600, 1 << 20})
    for (long long grid2 : {1ll, 4096ll, 4097ll, 1ll << 40})
      for (size_t rm : {(size_t)0, (size_t)1, (size_t)1 << 40, ~(size_t)0})
        for (int split_max : {0, 1, 2, 32, 1 << 20}) {
          const Split s = split_search(nchunks, grid2, 256, rm, COUNTERS, (double)grid2 * 65536.0, 1e9, SplitCost{2.7, 4.0, 2.0, 0.6, 0.85, split_max});
          ++n_plans;
          if (s.splits < 1 || (long long)s.splits * s.chunks_per_split < nchunks || nchunks <= (long long)(s.splits - 1) * s.chunks_per_split ||
              (s.splits > 1 && ((double)s.splits * (double)grid2 * 65536.0 > (double)rm || grid2 > COUNTERS || split_max < 2)))
            { ++n_bad; std::printf("broken: split_search(%d, %lld, %zu, %d)\n", nchunks, grid2, rm, split_max); }
        }
  std::printf("%ld plans (%ld refused), %ld broken\n", n_plans, n_refused, n_bad);
  return n_bad ? 1 : 0;
}
