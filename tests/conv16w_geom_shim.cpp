// Test infrastructure: builds gen6d_amd/csrc/conv16w_geom.h (the halo-patch kernel's integer geometry) for the HOST (g++) and exposes it
// to ctypes for tests/test_conv16w_geom_cpu.py, whole arrays per call.  Not part of the product library.
#include "../gen6d_amd/csrc/conv16w_geom.h"
using namespace c16g;
extern "C" {
int g_sizeof_tiling() { return (int)sizeof(Tiling); }
// a tiling as halo_tiling fills it; returns finish()'s verdict for tile indices below ntiles
int g_tiling(int tw_log2, int tiles_x, int tpi, int segh_log2, int bands, int swa, int swd, long ntiles, Tiling* out) {
  Tiling t = {};
  t.h_tw_log2 = tw_log2; t.h_tiles_x = tiles_x; t.h_tile0 = 0; t.h_tpi = tpi; t.h_segh_log2 = segh_log2; t.h_bands = bands; t.h_swa = swa; t.h_swd = swd;
  const bool ok = finish(t, ntiles);
  *out = t;
  return ok ? 1 : 0;
}
int g_patch_pixels(const Tiling* tl) { return tl->h_P; }
// the launcher's own choice for a segment of N maps of H x W: halo_tiling's verdict, the tiling it filled, and
// out8 = tw_log2, tiles_x, tpi, segh_log2, bands, swa, swd, tile count
int g_halo_tiling(int N, int H, int W, int pairs, int in_image, Tiling* tl, int* out8) {
  Tiling t = {};
  int tiles = 0;
  const bool ok = halo_tiling(N, H, W, pairs != 0, in_image != 0, t, tiles);
  *tl = t;
  out8[0] = t.h_tw_log2; out8[1] = t.h_tiles_x; out8[2] = t.h_tpi; out8[3] = t.h_segh_log2; out8[4] = t.h_bands; out8[5] = t.h_swa; out8[6] = t.h_swd;
  out8[7] = tiles;
  return ok ? 1 : 0;
}
int g_pick_tw(int W) { return pick_tw(W); }
// tiles t0 .. t0 + n - 1 -> [n][5]: g0, x0, y0, ylim, interior
void g_tiles(const Tiling* tl, int H, int W, int t0, int n, int* out) {
  for (int i = 0; i < n; ++i) {
    const Tile t = tile_of(*tl, H, W, t0 + i);
    int* o = out + 5 * i;
    o[0] = t.g0; o[1] = t.x0; o[2] = t.y0; o[3] = t.ylim; o[4] = t.interior;
  }
}
// every (piece, lane) of tile t -> [npiece][64][8]: prow, pcol, band, lr, slot, in_patch, valid, offset (as int bits)
void g_pieces(const Tiling* tl, int H, int W, int rows, int ld_in, int t, int npiece, int* out) {
  const Tile tile = tile_of(*tl, H, W, t);
  const unsigned base = tile_base(W, ld_in, tile);
  for (int ii = 0; ii < npiece; ++ii)
    for (int lane = 0; lane < 64; ++lane) {
      const Piece pc = piece_of(*tl, ii, lane);
      int* o = out + (ii * 64 + lane) * 8;
      o[0] = pc.prow; o[1] = pc.pcol; o[2] = pc.band; o[3] = pc.lr; o[4] = pc.slot; o[5] = pc.in_patch;
      o[6] = piece_valid(*tl, H, W, rows, tile, pc) ? 1 : 0;
      o[7] = (int)piece_offset(*tl, W, ld_in, base, pc);
    }
}
// tile pixels 0 .. 127 -> [128][2]: patch pixel of tap (0, 0), its patch row
void g_frag(const Tiling* tl, int* out) {
  for (int r = 0; r < BM; ++r) { out[2 * r] = frag_pixel(*tl, r); out[2 * r + 1] = frag_row(*tl, r); }
}
// the reciprocal helpers on arrays: q31 = n / d by recip31 / div31 with ok31 = recip31_ok(d, n); q16 likewise by recip16 / div16
void g_div31(const unsigned* n, const unsigned* d, int cnt, unsigned* q, int* ok) {
  for (int i = 0; i < cnt; ++i) { q[i] = div31(n[i], recip31(d[i])); ok[i] = recip31_ok(d[i], n[i]) ? 1 : 0; }
}
void g_div16(const unsigned* n, const unsigned* d, int cnt, unsigned* q) {
  for (int i = 0; i < cnt; ++i) q[i] = div16(n[i], recip16(d[i]));
}
}
