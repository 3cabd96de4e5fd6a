// conv16w_geom.h — the integer geometry of the halo-patch kernel (conv16w_kernel, conv16w.hip) in one place, for the device and for the
// host (c16w_admit fills Tiling through halo_tiling; tests/conv16w_geom_shim.cpp builds this header with g++ and checks it against plain
// division and against a model of the tiling choice).
//   tile index            -> (first tall-image row, first column, first image row, rows inside the image, interior?)
//   (piece index, lane)   -> (patch row, patch column, band, row inside the band, LDS slot), validity, 32-bit buffer offset
//   tile pixel            -> patch pixel of tap (0, 0) (the fragment base)
// No run-time division: divisors that are powers of two are shifts, the others (tiles per image, tiles per row, patch width, rows per
// band) are multiplied by reciprocals the host computes once per segment and proves exact for the range they are used on.
#pragma once

#if defined(__HIPCC__)
#define C16G_HD __host__ __device__ __forceinline__
#else
#define C16G_HD inline
#endif

namespace c16g {

constexpr int BM = 128;                  // pixels per tile
constexpr int NI_MAX = 18;               // 1 KB pieces (16 patch rows of 64 B) per plane at most: 288 patch pixels

C16G_HD unsigned mulhi(unsigned a, unsigned b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (unsigned)(((unsigned long long)a * b) >> 32);
#endif
}

// n / d for a block-uniform n: m = ceil(2^31 / d) (fits 32 bits for every d >= 1), n / d = (n m) >> 31.  With m d = 2^31 + e the quotient
// is exact while n e < 2^31 (recip31_ok), which n d <= 2^31 implies.
C16G_HD unsigned recip31(unsigned d) { return (unsigned)(((1ull << 31) + d - 1) / d); }
C16G_HD bool recip31_ok(unsigned d, unsigned n_max) {
  const unsigned long long e = (unsigned long long)recip31(d) * d - (1ull << 31);
  return n_max < (1u << 31) && (unsigned long long)n_max * e < (1ull << 31);
}
C16G_HD unsigned div31(unsigned n, unsigned m) { return mulhi(n << 1, m); }

// n / d for a per-lane n < 512 and 2 <= d <= 64 (patch pixel / patch width, patch row / rows per band): m = ceil(2^16 / d) <= 2^15,
// n / d = (n m) >> 16 — a 24-bit multiply and a shift.  Exact while n e < 2^16 with e < d: 512 * 64 = 2^15.
C16G_HD unsigned recip16(unsigned d) { return (65536u + d - 1) / d; }
C16G_HD unsigned div16(unsigned n, unsigned m) { return (n * m) >> 16; }

struct Tiling {       // one segment's halo tiling (halo_tiling below); h_: halo, beside the per-tap kernels' tiling in C16Seg
  int h_tw_log2, h_tiles_x, h_tile0, h_tpi;      // tile width, tiles per row, first tile of the segment, tiles per image (0: tiles of whole small images)
  int h_segh_log2, h_bands;                // rows per band (min(H, TH): a power of two), bands per tile (TH / segh: > 1 when a tile holds several images)
  int h_swa, h_swd;                        // LDS slot swizzle: ((pcol >> swa) + prow * swd) & 3
  int h_P;                               // patch pixels: bands * (segh + 2) * (TW + 2)
  unsigned h_r_tpi, h_r_tx;                // recip31 of tpi (tpi > 0) and tiles_x
  unsigned h_r_pw, h_r_band;               // recip16 of the patch width TW + 2 and of the band height segh + 2
};

// Fills the derived fields (P, reciprocals) from tw_log2, tiles_x, tpi, segh_log2, bands; false if a reciprocal would not be exact for
// tile indices below ntiles.
C16G_HD bool finish(Tiling& t, long ntiles) {
  const int TW = 1 << t.h_tw_log2, segh = 1 << t.h_segh_log2;
  t.h_P = t.h_bands * (segh + 2) * (TW + 2);
  t.h_r_pw = recip16((unsigned)(TW + 2)); t.h_r_band = recip16((unsigned)(segh + 2));
  t.h_r_tx = recip31((unsigned)t.h_tiles_x); t.h_r_tpi = t.h_tpi > 0 ? recip31((unsigned)t.h_tpi) : 0u;
  if (ntiles >= (1L << 31)) return false;
  return recip31_ok((unsigned)t.h_tiles_x, (unsigned)ntiles) && (t.h_tpi <= 0 || recip31_ok((unsigned)t.h_tpi, (unsigned)ntiles));
}

// Tiling of one segment (N maps of H x W) for the halo-patch kernel: the tile width (32 / 16 / 8 / 4) with the least overhang; false if
// none fits (a map lower than the tile must divide it: tiles of whole images).  pairs: the fp16 pair kernel's slot swizzle (its fragment
// reads differ); in_image: only tilings whose tiles lie inside one image (depth-folded layers: N counts planes, and a tile must not span
// two).  Fills o (all but h_tile0) and the segment's tile count.
C16G_HD bool halo_tiling(int N, int H, int W, bool pairs, bool in_image, Tiling& o, int& tiles) {
  double best = 1e30;
  bool found = false;
  for (int tw = 32; tw >= 4; tw >>= 1) {
    const int th = BM / tw, tx = (W + tw - 1) / tw;
    long nt; int tpi, segh, bands;
    if (H >= th) { tpi = tx * ((H + th - 1) / th); nt = (long)N * tpi; segh = th; bands = 1; }
    else {
      if (th % H || in_image) continue;
      tpi = 0; nt = (long)tx * (((long)N * H + th - 1) / th); segh = H; bands = th / H;
    }
    if (bands * (segh + 2) * (tw + 2) > 288) continue;
    const double waste = (double)nt * BM / ((double)N * H * W);
    if (waste < best - 1e-9) {
      best = waste; found = true;
      int l2 = 0; while ((1 << l2) < tw) ++l2;
      int sl2 = 0; while ((1 << sl2) < segh) ++sl2;           // (segh = TH or a divisor of it: a power of two)
      o.h_tw_log2 = l2; o.h_tiles_x = tx; o.h_tpi = tpi; o.h_segh_log2 = sl2; o.h_bands = bands;
      tiles = (int)nt;
      // conflict-free slot swizzles found by tools/ubench/conv16_swizzle.py: ((pcol >> a) + prow * d) & (slots - 1)  (64-byte patch rows:
      // 4 slots).  The pair kernel reads 16 pixels x 4 slots per 16 lanes (16x16x32 fragments), the 16-bit modes 32 pixels x 2 slots;
      // the pair kernel relies on d = 0 and a <= 2
      if (pairs) { o.h_swa = tw >= 16 ? 1 : 0; o.h_swd = 0; }
      else { o.h_swa = tw == 32 ? 2 : (tw == 16 ? 1 : 0); o.h_swd = tw <= 8 ? 1 : 0; }
    }
  }
  // patch size and the reciprocals that replace the kernel's divisions (exact for every tile index of the segment, or no halo tiling)
  return found && finish(o, tiles);
}

// The per-tap kernels' tile width for maps W wide: the power of two in 4 .. 64 with the least column overhang, ties -> the wider tile
C16G_HD int pick_tw(int W) {
  int best = 8; double bw = 1e9;
  for (int tw = 64; tw >= 4; tw >>= 1) {
    const double waste = (double)((W + tw - 1) / tw * tw) / W;
    if (waste < bw - 1e-9) { bw = waste; best = tw; }
  }
  return best;
}

struct Tile {         // one 128-pixel tile (block-uniform)
  int g0, x0, y0, ylim;                  // first row of the tall image, first column, first row inside its image, tile rows inside the image
  int interior;                          // the whole halo patch lies inside ONE image: every patch pixel is a valid request
  int img;                               // index of the tile's image (tiles inside one image; 0 for tiles of whole small images)
};
// t: tile index inside the segment
C16G_HD Tile tile_of(const Tiling& tl, int H, int W, int t) {
  Tile o;
  const int TW = 1 << tl.h_tw_log2, TH = BM >> tl.h_tw_log2;
  if (tl.h_tpi > 0) {                                            // tiles inside one image
    const int n = (int)div31((unsigned)t, tl.h_r_tpi), r = t - n * tl.h_tpi;
    const int ty = (int)div31((unsigned)r, tl.h_r_tx), tx = r - ty * tl.h_tiles_x;
    o.y0 = ty * TH; o.x0 = tx * TW; o.g0 = n * H + o.y0; o.ylim = TH < H - o.y0 ? TH : H - o.y0;
    o.interior = o.y0 >= 1 && o.y0 + TH < H && o.x0 >= 1 && o.x0 + TW < W;
    o.img = n;
  } else {                                                     // tiles of TH / H whole images: every band touches its image's edges
    const int ty = (int)div31((unsigned)t, tl.h_r_tx), tx = t - ty * tl.h_tiles_x;
    o.y0 = 0; o.x0 = tx * TW; o.g0 = ty * TH; o.ylim = TH;
    o.interior = 0;
    o.img = 0;
  }
  return o;
}

struct Piece {        // lane `lane` of piece ii (patch pixels 16 ii + lane / 4, 16 bytes each) of one plane
  int prow, pcol, band, lr, slot;        // patch row / column, band, row inside the band's image (-1 .. segh), physical LDS slot's channel group
  int in_patch;                          // the patch pixel exists (16 ii + lane / 4 < P)
};
C16G_HD Piece piece_of(const Tiling& tl, int ii, int lane) {
  Piece o;
  const int PW = (1 << tl.h_tw_log2) + 2, bandr = (1 << tl.h_segh_log2) + 2;
  const int q = ii * 16 + (lane >> 2);
  o.prow = (int)div16((unsigned)q, tl.h_r_pw); o.pcol = q - o.prow * PW;
  o.band = (int)div16((unsigned)o.prow, tl.h_r_band); o.lr = o.prow - o.band * bandr - 1;
  o.slot = (lane & 3) ^ (((o.pcol >> tl.h_swa) + o.prow * tl.h_swd) & 3);
  o.in_patch = q < tl.h_P;
  return o;
}
// the request reads a pixel of the map (edge and banded tiles; an interior tile needs in_patch only)
C16G_HD bool piece_valid(const Tiling& tl, int H, int W, int rows, const Tile& t, const Piece& pc) {
  const int g = t.g0 + (pc.band << tl.h_segh_log2) + pc.lr, x = t.x0 + pc.pcol - 1, yimg = t.y0 + pc.lr;
  return pc.in_patch && yimg >= 0 && yimg < H && g < rows && x >= 0 && x < W;
}
// byte offset of the request from the segment's input: one block-uniform base (patch pixel (0, 0), which may lie before the tensor)
// plus the lane's part, in 32-bit arithmetic — a launch addresses less than 2^31 bytes per segment, so a valid request never wraps.
C16G_HD unsigned tile_base(int W, int ld_in, const Tile& t) { return (unsigned)(((t.g0 - 1) * W + t.x0 - 1) * ld_in * 2); }
C16G_HD unsigned piece_offset(const Tiling& tl, int W, int ld_in, unsigned base, const Piece& pc) {
  const int yrel = (pc.band << tl.h_segh_log2) + pc.lr + 1;
  return base + (unsigned)((yrel * W + pc.pcol) * ld_in * 2 + pc.slot * 16);
}
// tile pixel r (row-major in the tile) -> its patch pixel for tap (0, 0): row band * (segh + 2) + row in band, column r % TW
C16G_HD int frag_pixel(const Tiling& tl, int r) {
  const int PW = (1 << tl.h_tw_log2) + 2, bandr = (1 << tl.h_segh_log2) + 2;
  const int py = r >> tl.h_tw_log2, px = r & ((1 << tl.h_tw_log2) - 1);
  const int b = py >> tl.h_segh_log2, ly = py & ((1 << tl.h_segh_log2) - 1);
  return (b * bandr + ly) * PW + px;
}
C16G_HD int frag_row(const Tiling& tl, int r) {                // the patch row alone (the 16-bit modes' swizzle term)
  const int py = r >> tl.h_tw_log2;
  return (py >> tl.h_segh_log2) * ((1 << tl.h_segh_log2) + 2) + (py & ((1 << tl.h_segh_log2) - 1));
}

}  // namespace c16g
