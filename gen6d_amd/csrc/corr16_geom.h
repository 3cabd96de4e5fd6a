// corr16_geom.h — the integer geometry of corr16_kernel (corr16.hip) in one place, for the device and for the host (the launcher picks its
// tiles here; tests/corr16_geom_shim.cpp builds this header with g++ and tests/test_corr16_geom_cpu.py checks it against plain formulas).
//   map size               -> tile width with its slot swizzle (pick_tile)
//   tile index             -> (image, first row, first column)
//   (piece index, lane)    -> patch row / column, map pixel, validity, logical LDS slot; slot -> byte offset inside a pixel
//   tile pixel, tap, stage -> LDS address of fragment 0 (fragment 1: that address ^ 32)
//   wave                   -> its taps of a slice, the walk over them and the advance of the running filter pointer
// A patch row is 64 B = four 16-byte slots; physical slot s of patch pixel (prow, pcol) holds logical slot s ^ swz(prow, pcol), with
// swz = ((pcol >> swa) + prow * swd) & 3.  The divisions are run-time divisions (block-uniform or once per lane, outside the tap loop).
#pragma once
#include "conv16w_geom.h"

namespace corr16g {

constexpr int BM = c16g::BM;             // pixels per tile
constexpr int NW = 11;                   // computing waves per block (+ one loader wave)
constexpr int STAGE = 42 * 1024;         // bytes of one patch stage: 672 patch rows of 64 B (K = 15, 8 x 16 tile: 660)
constexpr int PIECE = 1024;              // bytes one LDS-DMA wave instruction fills: 16 patch rows
constexpr int NPL = STAGE / PIECE;       // pieces per patch at most (42)
constexpr int TAP_BYTES = 2048;          // filters of one (slice, tap): 2 fragments x 64 lanes x 16 B
constexpr int RING = 3;                  // filter sets in flight per wave: the tap loop is unrolled by three steps
constexpr int RED_LD = 33;               // floats per pixel of a partial tile in the final reduction (four tiles at a time)
constexpr int LDS_BYTES = 2 * STAGE;     // two stages, reused by the final reduction
static_assert((STAGE / 64 + 15) / 16 <= NPL, "the largest patch pick_tile admits (STAGE / 64 rows) fits NPL pieces");
static_assert(4 * BM * RED_LD * 4 <= LDS_BYTES, "the final reduction's four partial tiles fit the two stages");

struct Tile { int tw_log2, tiles_x, tpi, swa, swd; };      // tile width (-1: none fits), tiles per map row, tiles per image, slot swizzle
// The tile width (32 .. 4, TH = BM / TW) whose (TH + K - 1) x (TW + K - 1) patch fits a stage with the least overhang, ties to the wider.
// swd = 1 only together with swa = 0: frag_base folds the swizzle's row term in BEFORE the shift by swa.
C16G_HD Tile pick_tile(int H, int W, int K) {
  double best = 1e30; int btw = 0;
  for (int tw = 32; tw >= 4; tw >>= 1) {
    const int th = BM / tw;
    if ((th + K - 1) * (tw + K - 1) > STAGE / 64) continue;
    const double waste = (double)((W + tw - 1) / tw * tw) * ((H + th - 1) / th * th) / ((double)W * H);
    if (waste < best - 1e-9) { best = waste; btw = tw; }
  }
  if (!btw) return {-1, 0, 0, 0, 0};
  int l2 = 0; while ((1 << l2) < btw) ++l2;
  const int th = BM / btw, tx = (W + btw - 1) / btw;
  return {l2, tx, tx * ((H + th - 1) / th), btw == 32 ? 2 : (btw == 16 ? 1 : 0), btw <= 8 ? 1 : 0};
}

struct Patch { int tw_log2, K, swa, swd, PW, P, NI; };     // + patch width, patch pixels, pieces that hold any of them
C16G_HD Patch patch_of(int tw_log2, int K, int swa, int swd) {
  const int PW = (1 << tw_log2) + K - 1, P = ((BM >> tw_log2) + K - 1) * PW;
  return {tw_log2, K, swa, swd, PW, P, (P + 15) >> 4};
}
struct Origin { int n, y0, x0; };                          // a tile's image and first pixel; t: tile index inside the segment
C16G_HD Origin tile_origin(const Patch& g, int tiles_x, int tpi, int t) {
  const int n = t / tpi, r = t - n * tpi, ty = r / tiles_x, tx = r - ty * tiles_x;
  return {n, ty * (BM >> g.tw_log2), tx * (1 << g.tw_log2)};
}

// lane `lane` of piece k: patch pixel 16 k + lane / 4 at map pixel (y, x), physical slot lane & 3, which holds logical slot L;
// a request is made for a pixel in the patch and in the map (anything else is left to the buffer's zero fill)
struct Piece { int prow, pcol, y, x, L; bool in_patch; };
C16G_HD Piece piece_of(const Patch& g, const Origin& o, int k, int lane) {
  const int q = k * 16 + (lane >> 2), R = g.K >> 1;
  const int prow = q / g.PW, pcol = q - prow * g.PW;
  return {prow, pcol, o.y0 - R + prow, o.x0 - R + pcol, (lane & 3) ^ (((pcol >> g.swa) + prow * g.swd) & 3), k < g.NI && q < g.P};
}
C16G_HD bool in_map(const Piece& pc, int H, int W) { return pc.y >= 0 && pc.y < H && pc.x >= 0 && pc.x < W; }
// byte offset of logical slot L inside a pixel's row — 16-bit modes: channel group L of the 32-channel slice; pairs: plane L >> 1 (Cin
// 16-bit values each), channel half L & 1 of the 16-channel slice
C16G_HD unsigned slot_bytes(int L, bool pairs, int Cin) { return pairs ? (unsigned)((L >> 1) * Cin * 2 + (L & 1) * 16) : (unsigned)(L * 16); }

// tile pixel r (row-major in the tile) -> qb: byte offset of its patch pixel for tap (0, 0); fe: its swizzle seed, column + row * swd
C16G_HD void frag_base(const Patch& g, int r, int& qb, int& fe) {
  const int py = r >> g.tw_log2, px = r & ((1 << g.tw_log2) - 1);
  qb = (py * g.PW + px) * 64; fe = px + py * g.swd;
}
// LDS address of fragment 0 of that pixel at tap (ky, kx) in `stage`, as read by lane half `fhalf`: physical slot fhalf ^ swz(py + ky,
// px + kx) (swd = 1 => swa = 0 makes ((fe + kx) >> swa) + ky * swd that swizzle); fragment 1 sits at the address ^ 32
C16G_HD int tap_addr(const Patch& g, int qb, int fe, int fhalf, int ky, int kx, int stage) {
  const int so = stage * STAGE + ky * (g.PW * 64) + kx * 64, sw = ((fe + kx) >> g.swa) + ky * g.swd;
  return qb + so + (((fhalf ^ sw) & 3) << 4);
}

// The K^2 taps of a slice are dealt to the computing waves in turn: wave wv has taps wv, wv + NW, ...
C16G_HD int wave_taps(int K, int wv) { return (K * K - wv + NW - 1) / NW; }
C16G_HD void first_tap(int K, int wv, int& ky, int& kx) { ky = wv / K; kx = wv - ky * K; }
C16G_HD void next_tap(int K, int& ky, int& kx) { kx += NW; while (kx >= K) { kx -= K; ++ky; } }
// bytes the running filter pointer moves after the load of tap wtap (updated): to the wave's next tap of the slice, or past the slice's
// end to its first tap of the next slice
C16G_HD long filter_advance(int K, int wv, int& wtap) {
  wtap += NW;
  if (wtap < K * K) return NW * TAP_BYTES;
  const long d = (long)(K * K - wtap + NW + wv) * TAP_BYTES;
  wtap = wv;
  return d;
}

}  // namespace corr16g
