// Test infrastructure: builds gen6d_amd/csrc/corr16_geom.h (corr16_kernel's integer geometry) for the HOST (g++) and exposes it to ctypes
// for tests/test_corr16_geom_cpu.py, whole arrays per call.  Not part of the product library.
#include "../gen6d_amd/csrc/corr16_geom.h"
using namespace corr16g;
extern "C" {
void g_consts(int* o) { o[0] = BM; o[1] = NW; o[2] = STAGE; o[3] = PIECE; o[4] = NPL; o[5] = TAP_BYTES; o[6] = RING; o[7] = LDS_BYTES; }
// pick_tile for H = 1 .. hmax, W = 1 .. wmax -> [hmax][wmax][5]: tw_log2, tiles_x, tpi, swa, swd
void g_pick_grid(int K, int hmax, int wmax, int* out) {
  for (int h = 1; h <= hmax; ++h)
    for (int w = 1; w <= wmax; ++w) {
      const Tile t = pick_tile(h, w, K);
      int* o = out + ((h - 1) * wmax + (w - 1)) * 5;
      o[0] = t.tw_log2; o[1] = t.tiles_x; o[2] = t.tpi; o[3] = t.swa; o[4] = t.swd;
    }
}
void g_patch(int tw_log2, int K, int swa, int swd, int* o) {
  const Patch g = patch_of(tw_log2, K, swa, swd);
  o[0] = g.PW; o[1] = g.P; o[2] = g.NI;
}
// tiles 0 .. n - 1 of a segment -> [n][3]: image, first row, first column
void g_origins(int tw_log2, int K, int swa, int swd, int tiles_x, int tpi, int n, int* out) {
  const Patch g = patch_of(tw_log2, K, swa, swd);
  for (int t = 0; t < n; ++t) { const Origin o = tile_origin(g, tiles_x, tpi, t); out[3 * t] = o.n; out[3 * t + 1] = o.y0; out[3 * t + 2] = o.x0; }
}
// every (piece, lane) of the tile at (y0, x0) of an H x W map -> [NPL][64][8]: prow, pcol, y, x, L, in_patch, in_map, slot_bytes
void g_pieces(int tw_log2, int K, int swa, int swd, int y0, int x0, int H, int W, int pairs, int Cin, int* out) {
  const Patch g = patch_of(tw_log2, K, swa, swd);
  const Origin og = {0, y0, x0};
  for (int k = 0; k < NPL; ++k)
    for (int lane = 0; lane < 64; ++lane) {
      const Piece pc = piece_of(g, og, k, lane);
      int* o = out + (k * 64 + lane) * 8;
      o[0] = pc.prow; o[1] = pc.pcol; o[2] = pc.y; o[3] = pc.x; o[4] = pc.L; o[5] = pc.in_patch; o[6] = in_map(pc, H, W);
      o[7] = (int)slot_bytes(pc.L, pairs != 0, Cin);
    }
}
// every (tap, lane half, tile pixel) -> [K][K][2][128]: the LDS address of fragment 0 as the kernel forms it (frag_base once, tap_addr per tap)
void g_taps(int tw_log2, int K, int swa, int swd, int stage, int* out) {
  const Patch g = patch_of(tw_log2, K, swa, swd);
  for (int r = 0; r < BM; ++r) {
    int qb, fe;
    frag_base(g, r, qb, fe);
    for (int ky = 0; ky < K; ++ky)
      for (int kx = 0; kx < K; ++kx)
        for (int h = 0; h < 2; ++h) out[((ky * K + kx) * 2 + h) * BM + r] = tap_addr(g, qb, fe, h, ky, kx, stage);
  }
}
// One computing wave's walk over nslice slices with the kernel's control flow (two filter sets ahead, steps in groups of RING, padding steps
// after the last slice): off[i] = byte offset of the i-th filter load from the filters' base, or -1 for a reload past the end;
// tap[j] = ky * K + kx of the j-th computed step.  Returns the number of loads; *ntaps = computed steps, *ntw = taps per slice.
int g_walk(int K, int wv, int nslice, long* off, int* tap, int* ntaps, int* ntw_out) {
  const int ntw = wave_taps(K, wv);
  long wp = (long)wv * TAP_BYTES;
  int wtap = wv, wleft = nslice * ntw, nl = 0, nt = 0;
  auto load = [&]() { off[nl++] = wleft > 0 ? wp : -1; --wleft; wp += filter_advance(K, wv, wtap); };
  load(); load();
  int ky0, kx0;
  first_tap(K, wv, ky0, kx0);
  int ky = ky0, kx = kx0, it = 0, c = 0;
  for (int s = 0; s < nslice * ntw; s += RING)
    for (int j = 0; j < RING; ++j) {
      const bool live = c < nslice, last = it == ntw - 1;
      load();
      if (!live) continue;
      tap[nt++] = ky * K + kx;
      next_tap(K, ky, kx);
      if (last) { ky = ky0; kx = kx0; it = 0; ++c; } else ++it;
    }
  *ntaps = nt; *ntw_out = ntw;
  return nl;
}
}
