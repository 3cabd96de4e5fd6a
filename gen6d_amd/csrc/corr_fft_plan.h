// corr_fft_plan.h — the integer plan of the frequency-domain correlation (corr_fft.hip) in one place, for the device and for the host (the
// launchers size their grids and buffers here; tests/corr_fft_plan_shim.cpp builds this header with g++ and tests/test_corr_fft_plan_cpu.py
// checks it against plain formulas).  Plain C++17, no HIP.
//   A K x K "same" correlation of an H x W map is cut into T x T windows (overlap-save): the window of tile (ty, tx) starts at map pixel
//   (ty V - K/2, tx V - K/2), V = T - K + 1, pixels outside the map are zero, and the circular correlation of the window with the filter
//   (zero-extended to T x T, tap (0, 0) at the window's origin) is the wanted sum at its first V x V positions: output pixels
//   (ty V .. ty V + V - 1, tx V .. tx V + V - 1), cut at the map's edge.  A real T x T window has T (T/2 + 1) Hermitian bins, bin = ky (T/2 + 1) + kx.
//   segment (N maps of H x W)    -> tiles per row, per image, first tile of the segment in the launch's flat tile list
//   tile index                   -> (segment, image, first output row, first output column)
//   tiles of a query, Cin        -> the most queries one launch may take: its spectrum X[bin][tile][2][Cin] stays below 2^31 bytes
//   tiles, Cin, references       -> bytes of the spectrum X and of the product Y[bin][tile][2][R]
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CFFT_HD __host__ __device__ inline
#else
#define CFFT_HD inline
#endif

namespace cfft {

constexpr int MAX_SEG = 4;

CFFT_HD constexpr bool valid_tk(int T, int K) { return (T == 32 || T == 64) && K >= 1 && (K & 1) && K < T; }
CFFT_HD constexpr int valid_side(int T, int K) { return T - K + 1; }          // V: outputs per window and axis
CFFT_HD constexpr int bins(int T) { return T * (T / 2 + 1); }                 // Hermitian bins of a real T x T window

struct SegPlan { int H, W, N, tiles_x, tiles_y, tpi, tile0; };                // tpi: tiles per image; tile0: the segment's first tile
struct Plan {
  int T, K, V, bins, nseg, tiles;
  SegPlan seg[MAX_SEG];
};
struct Tile { int seg, n, y0, x0; };                                          // first output pixel; the window starts K/2 before it

CFFT_HD int ceil_div(int a, int b) { return (a + b - 1) / b; }

// nseg segments of N[i] maps H[i] x W[i]; false when the arguments are out of range (or the tile count leaves 31 bits)
CFFT_HD bool make_plan(Plan& p, int T, int K, int nseg, const int* N, const int* H, const int* W) {
  if (!valid_tk(T, K) || nseg < 1 || nseg > MAX_SEG) return false;
  p.T = T; p.K = K; p.V = valid_side(T, K); p.bins = bins(T); p.nseg = nseg;
  int64_t tiles = 0;
  for (int i = 0; i < nseg; ++i) {
    if (N[i] < 1 || H[i] < 1 || W[i] < 1) return false;
    SegPlan& s = p.seg[i];
    s.H = H[i]; s.W = W[i]; s.N = N[i];
    s.tiles_x = ceil_div(W[i], p.V); s.tiles_y = ceil_div(H[i], p.V);
    s.tpi = s.tiles_x * s.tiles_y; s.tile0 = (int)tiles;
    tiles += (int64_t)s.tpi * N[i];
    if (tiles >= (1ll << 24)) return false;
  }
  p.tiles = (int)tiles;
  return true;
}

// tile t of the launch's flat list (0 <= t < p.tiles)
CFFT_HD Tile tile_of(const Plan& p, int t) {
  int si = 0;
  for (int i = 1; i < p.nseg; ++i) if (t >= p.seg[i].tile0) si = i;
  const SegPlan& s = p.seg[si];
  const int l = t - s.tile0, n = l / s.tpi, r = l - n * s.tpi, ty = r / s.tiles_x, tx = r - ty * s.tiles_x;
  return {si, n, ty * p.V, tx * p.V};
}
CFFT_HD int window_y(const Plan& p, const Tile& t) { return t.y0 - p.K / 2; }
CFFT_HD int window_x(const Plan& p, const Tile& t) { return t.x0 - p.K / 2; }

CFFT_HD int64_t spectrum_bytes(int T, int64_t tiles, int Cin) { return (int64_t)bins(T) * tiles * 2 * Cin * 4; }
CFFT_HD int64_t product_bytes(int T, int64_t tiles, int R) { return (int64_t)bins(T) * tiles * 2 * R * 4; }
CFFT_HD int64_t filter_bytes(int T, int Cin, int R) { return (int64_t)bins(T) * 2 * Cin * 2 * R * 4; }       // B'[bin][2 Cin][2 R]

// The most queries (<= want) one launch may take when a query has tiles_per_query tiles: the launch's spectrum stays below 2^31 bytes,
// the reach of the kernels' 32-bit element offsets with room to spare.  0: not even one query fits.
CFFT_HD int chunk_queries(int T, int tiles_per_query, int Cin, int want) {
  int q = want;
  while (q > 0 && spectrum_bytes(T, (int64_t)q * tiles_per_query, Cin) >= (1ll << 31)) --q;
  return q;
}

}  // namespace cfft
