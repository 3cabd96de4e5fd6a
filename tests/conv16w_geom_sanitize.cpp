// Test infrastructure: a stand-alone host program that runs the launcher's tiling choosers of gen6d_amd/csrc/conv16w_geom.h
// (c16g::halo_tiling, c16g::pick_tw) over an exhaustive set of small shapes and the extremes a launch admits (a segment's input stays
// below 2 GB: N H W < 2^24 pixels at 64 channels), and checks what the halo-patch kernel relies on.  Meant for the sanitizers:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tests/conv16w_geom_sanitize.cpp -o geom_san && ./geom_san
// (tests/test_conv16w_geom_cpu.py builds and runs it that way).  Prints the number of tilings found; exit status 1 on a broken invariant.
#include "../gen6d_amd/csrc/conv16w_geom.h"
#include <cstdio>
#include <initializer_list>
using namespace c16g;

static long n_found = 0, n_bad = 0;

static void check(int N, int H, int W) {
  for (int pairs = 0; pairs < 2; ++pairs)
    for (int in_image = 0; in_image < 2; ++in_image) {
      Tiling t = {};
      int tiles = 0;
      if (!halo_tiling(N, H, W, pairs != 0, in_image != 0, t, tiles)) continue;
      ++n_found;
      const int tw = 1 << t.h_tw_log2, th = BM / tw, segh = 1 << t.h_segh_log2;
      bool ok = tw >= 4 && tw <= 32 && tiles > 0 && t.h_P == t.h_bands * (segh + 2) * (tw + 2) && t.h_P <= 16 * NI_MAX;
      ok = ok && (t.h_tpi > 0 ? t.h_bands == 1 && segh == th && H >= th : !in_image && segh == H && t.h_bands * segh == th);
      ok = ok && (pairs ? t.h_swd == 0 && t.h_swa <= 2 : t.h_swd == 0 || t.h_swa == 0);
      // the first and the last tile decompose inside the segment
      const Tile a = tile_of(t, H, W, 0), z = tile_of(t, H, W, tiles - 1);
      ok = ok && a.g0 == 0 && a.x0 == 0 && z.x0 < W && z.g0 < (long)N * H && z.x0 + tw >= W;
      if (!ok) { ++n_bad; std::printf("broken: N %d H %d W %d pairs %d in_image %d\n", N, H, W, pairs, in_image); }
    }
}

int main() {
  for (int N : {1, 2, 5, 112, 5120})
    for (int H = 1; H <= 70; ++H)
      for (int W = 1; W <= 100; ++W) check(N, H, W);
  const int big[][3] = {{1, 1, 1 << 20}, {1, 1 << 20, 1}, {1 << 20, 1, 1}, {1 << 22, 2, 2}, {1, 4096, 4096}, {16, 352, 464}, {1 << 16, 16, 16}};
  for (const auto& s : big) check(s[0], s[1], s[2]);
  for (int W = 1; W <= 8192; ++W) {
    const int tw = pick_tw(W);
    if (tw < 4 || tw > 64 || (tw & (tw - 1))) { ++n_bad; std::printf("broken: pick_tw(%d) = %d\n", W, tw); }
  }
  std::printf("%ld tilings, %ld broken\n", n_found, n_bad);
  return n_bad ? 1 : 0;
}
