// Host build of gen6d_amd/csrc/corr_fft_plan.h for tests/test_corr_fft_plan_cpu.py (g++ -shared), and with -DCFFT_PLAN_MAIN a stand-alone
// program that walks the plan of every map up to 40 x 40 plus the detector's sizes (built with -fsanitize=address,undefined by the test).
#include "../gen6d_amd/csrc/corr_fft_plan.h"

#include <cstdio>
#include <vector>

extern "C" {
// out: T, K, V, bins, tiles, then per segment tiles_x, tiles_y, tpi, tile0; returns 0 when make_plan refuses
int p_plan(int T, int K, int nseg, const int* N, const int* H, const int* W, int* out) {
  cfft::Plan p;
  if (!cfft::make_plan(p, T, K, nseg, N, H, W)) return 0;
  out[0] = p.T; out[1] = p.K; out[2] = p.V; out[3] = p.bins; out[4] = p.tiles;
  for (int i = 0; i < nseg; ++i) {
    out[5 + 4 * i] = p.seg[i].tiles_x; out[6 + 4 * i] = p.seg[i].tiles_y; out[7 + 4 * i] = p.seg[i].tpi; out[8 + 4 * i] = p.seg[i].tile0;
  }
  return 1;
}
// out [tiles][6]: seg, n, y0, x0, window y, window x
int p_tiles(int T, int K, int nseg, const int* N, const int* H, const int* W, int* out) {
  cfft::Plan p;
  if (!cfft::make_plan(p, T, K, nseg, N, H, W)) return 0;
  for (int t = 0; t < p.tiles; ++t) {
    const cfft::Tile tl = cfft::tile_of(p, t);
    int* o = out + 6 * t;
    o[0] = tl.seg; o[1] = tl.n; o[2] = tl.y0; o[3] = tl.x0; o[4] = cfft::window_y(p, tl); o[5] = cfft::window_x(p, tl);
  }
  return 1;
}
int p_chunk(int T, int tiles_per_query, int Cin, int want) { return cfft::chunk_queries(T, tiles_per_query, Cin, want); }
long long p_spectrum_bytes(int T, long long tiles, int Cin) { return cfft::spectrum_bytes(T, tiles, Cin); }
long long p_product_bytes(int T, long long tiles, int R) { return cfft::product_bytes(T, tiles, R); }
long long p_filter_bytes(int T, int Cin, int R) { return cfft::filter_bytes(T, Cin, R); }
}

#ifdef CFFT_PLAN_MAIN
static int cover(int T, int K, int nseg, const int* N, const int* H, const int* W) {
  cfft::Plan p;
  if (!cfft::make_plan(p, T, K, nseg, N, H, W)) return 1;
  std::vector<std::vector<int>> hit(nseg);
  for (int i = 0; i < nseg; ++i) hit[i].assign((size_t)N[i] * H[i] * W[i], 0);
  for (int t = 0; t < p.tiles; ++t) {
    const cfft::Tile tl = cfft::tile_of(p, t);
    if (tl.seg < 0 || tl.seg >= nseg || tl.n < 0 || tl.n >= N[tl.seg]) return 2;
    for (int y = tl.y0; y < tl.y0 + p.V && y < H[tl.seg]; ++y)
      for (int x = tl.x0; x < tl.x0 + p.V && x < W[tl.seg]; ++x) ++hit[tl.seg][((size_t)tl.n * H[tl.seg] + y) * W[tl.seg] + x];
  }
  for (int i = 0; i < nseg; ++i)
    for (int v : hit[i]) if (v != 1) return 3;
  return 0;
}
int main() {
  for (int T : {32, 64})
    for (int H = 1; H <= 40; ++H)
      for (int W = 1; W <= 40; ++W) {
        const int N = 2;
        if (int rc = cover(T, 15, 1, &N, &H, &W)) { std::printf("T=%d %dx%d: %d\n", T, H, W, rc); return 1; }
      }
  const int N[4] = {3, 3, 3, 3}, H[4] = {88, 60, 44, 32}, W[4] = {116, 80, 60, 40};
  if (int rc = cover(32, 15, 4, N, H, W)) { std::printf("pyramid: %d\n", rc); return 1; }
  // 544 bins x 73 tiles x 1024 floats = 162.7 MB of spectrum per query: 13 queries stay below 2^31 bytes
  if (cfft::chunk_queries(32, 73, 512, 16) != 13 || cfft::chunk_queries(32, 73, 512, 8) != 8) { std::printf("chunk\n"); return 1; }
  std::printf("corr_fft_plan ok\n");
  return 0;
}
#endif
