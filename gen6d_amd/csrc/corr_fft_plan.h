// corr_fft_plan.h — the integer plan of the frequency-domain correlation (corr_fft.hip) in one place, for the device and for the host (the
// launchers size their grids and buffers here; tests/corr_fft_plan_shim.cpp builds this header with g++ and tests/test_corr_fft_plan_cpu.py
// checks it against plain formulas; the product kernel's block shape, stage image and ring: tests/corr_fft_gemm_plan_shim.cpp and
// tests/test_corr_fft_gemm_plan_cpu.py).  Plain C++17, no HIP.
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

// ---- the per-bin products (corrfft_gemm_kernel): Y[tile][64] = X[tile][K2] . B'[K2][64], K2 = 2 Cin, one bin per block row.
//   A block is `waves` waves of GEMM_WAVE_ROWS rows each; per K step of GEMM_KSTEP values it stages, straight into LDS in 1 KB wave
//   instructions of 64 lanes x 16 bytes, its rows of X (each wave its own: 8 pieces of 8 rows x 128 bytes) and the step's slab of B'
//   (8 pieces, shared by the block, split over the waves), into a ring of `stages` stages.
//   The X image of a wave is [row][8 slots of 16 bytes]; the slot of k-segment `seg` of row `row` is seg ^ gemm_a_swz(row), applied where
//   the piece is requested (the lane's source address) and again where the fragment is read, so the LDS destination stays lane-linear.
constexpr int GEMM_KSTEP = 32;                                  // k values per stage
constexpr int GEMM_WAVE_ROWS = 64;                              // two 32 x 32 row tiles per wave
constexpr int GEMM_COLS = 64;                                   // [re | im] x 32 references
constexpr int GEMM_PIECE = 1024;                                // bytes of one wave instruction
constexpr int GEMM_ROW_BYTES = GEMM_KSTEP * 4;                  // 128: one full line of a row per stage
constexpr int GEMM_SLOTS = GEMM_ROW_BYTES / 16;                 // 8
constexpr int GEMM_A_PIECES = GEMM_WAVE_ROWS * GEMM_ROW_BYTES / GEMM_PIECE;      // 8 per wave and stage
constexpr int GEMM_B_STAGE = GEMM_KSTEP * GEMM_COLS * 4;        // 8192 bytes of B' per stage
constexpr int GEMM_B_PIECES = GEMM_B_STAGE / GEMM_PIECE;        // 8 per block and stage
constexpr int GEMM_SMALL_M = 128;                               // up to here the two-wave block, beyond it the four-wave block
constexpr int LDS_LIMIT = 160 * 1024;

CFFT_HD constexpr int gemm_waves(int M) { return M <= GEMM_SMALL_M ? 2 : 4; }
CFFT_HD constexpr int gemm_stages(int waves) { return waves == 2 ? 2 : 2; }     // ring depth, measured (profiles/r31_corr_fft_gemm.md): 2 x 24 KB, three
                                                                                // blocks per CU; 2 x 40 KB, two blocks per CU (3 x 40 KB, one block: slower)
CFFT_HD constexpr int gemm_block_rows(int waves) { return waves * GEMM_WAVE_ROWS; }
CFFT_HD constexpr int gemm_a_stage_bytes(int waves) { return gemm_block_rows(waves) * GEMM_ROW_BYTES; }
CFFT_HD constexpr int gemm_stage_bytes(int waves) { return gemm_a_stage_bytes(waves) + GEMM_B_STAGE; }
CFFT_HD constexpr int gemm_lds_bytes(int waves) { return gemm_stages(waves) * gemm_stage_bytes(waves); }
CFFT_HD constexpr int gemm_b_pieces_per_wave(int waves) { return GEMM_B_PIECES / waves; }
// requests per wave and stage, the unit of the counted vmcnt: a wave without rows (idle) asks for its share of B' only
CFFT_HD constexpr int gemm_loads_per_stage(int waves, bool idle = false) { return (idle ? 0 : GEMM_A_PIECES) + gemm_b_pieces_per_wave(waves); }
CFFT_HD constexpr int gemm_mblocks(int M) { return (M + gemm_block_rows(gemm_waves(M)) - 1) / gemm_block_rows(gemm_waves(M)); }
// rows per block: the bin's rows spread evenly over its blocks in whole waves (292 rows: 192 + 100, not 256 + 36)
CFFT_HD constexpr int gemm_rows_per_block(int M) { return GEMM_WAVE_ROWS * ((M + gemm_mblocks(M) * GEMM_WAVE_ROWS - 1) / (gemm_mblocks(M) * GEMM_WAVE_ROWS)); }
CFFT_HD constexpr int gemm_steps(int Cin) { return 2 * Cin / GEMM_KSTEP; }
// The ring: steps 0 .. stages - 2 are requested before the loop; step t lives in stage t % stages; at the top of step t the wave waits
// until only the pieces of gemm_ahead(...) later steps are in flight (vmcnt = that x gemm_loads_per_stage), meets the barrier, and then
// requests step t + stages - 1 into the stage that step t - 1 read.
CFFT_HD constexpr int gemm_stage_of(int stages, int t) { return t % stages; }
CFFT_HD constexpr int gemm_ahead(int stages, int t, int nsteps) { return nsteps - 1 - t < stages - 2 ? nsteps - 1 - t : stages - 2; }

static_assert(GEMM_A_PIECES == 8 && GEMM_B_PIECES == 8 && GEMM_SLOTS == 8, "a piece is 8 rows x 8 slots");
static_assert(GEMM_B_PIECES % 2 == 0 && GEMM_B_PIECES % 4 == 0, "B' pieces split evenly over the waves");
static_assert(gemm_a_stage_bytes(2) + GEMM_B_STAGE == gemm_stage_bytes(2) && gemm_stage_bytes(4) == 4 * 8192 + 8192, "stage = X image + B' slab");
static_assert(gemm_lds_bytes(2) * 3 <= LDS_LIMIT && gemm_lds_bytes(4) * 2 <= LDS_LIMIT, "three small or two large blocks fit the CU's LDS");
static_assert(gemm_loads_per_stage(2) * (gemm_stages(2) - 1) < 64 && gemm_loads_per_stage(4) * (gemm_stages(4) - 1) < 64, "vmcnt has six bits");
static_assert(gemm_block_rows(gemm_waves(GEMM_SMALL_M)) >= GEMM_SMALL_M, "a small bin is one block");
static_assert(gemm_rows_per_block(292) == 192 && gemm_rows_per_block(584) == 256 && gemm_rows_per_block(73) == 128 && gemm_rows_per_block(257) == 192, "whole waves");

// block b of the grid (bins * mblocks blocks, bins % 8 == 0) -> (bin, row block): the blocks of one bin are consecutive on one XCD
CFFT_HD void gemm_block_of(int b, int mblocks, int& bin, int& mb) {
  const int xcd = b & 7, s = b >> 3;
  bin = xcd + 8 * (s / mblocks); mb = s % mblocks;
}
// wave `wave` of row block mb owns rows row0 .. min(row0 + 64, rows of the block's end, M) - 1; it is idle when that range is empty
CFFT_HD constexpr int gemm_wave_row0(int mb, int wave, int rows_per_block) { return mb * rows_per_block + wave * GEMM_WAVE_ROWS; }
CFFT_HD constexpr bool gemm_wave_idle(int mb, int wave, int rows_per_block, int M) {
  return wave * GEMM_WAVE_ROWS >= rows_per_block || gemm_wave_row0(mb, wave, rows_per_block) >= M;
}

CFFT_HD constexpr int gemm_a_swz(int row) { return (row >> 1) & (GEMM_SLOTS - 1); }
// lane `lane` of piece `piece` requests (row of the wave, k-segment) and lands at byte piece * 1024 + 16 * lane of the wave's image
CFFT_HD constexpr int gemm_a_src_row(int piece, int lane) { return piece * 8 + (lane >> 3); }
CFFT_HD constexpr int gemm_a_src_seg(int piece, int lane) { return (lane & 7) ^ gemm_a_swz(gemm_a_src_row(piece, lane)); }
// where a fragment read finds k-segment seg (k = 4 seg .. 4 seg + 3 of the stage) of the wave's row
CFFT_HD constexpr int gemm_a_lds_offset(int row, int seg) { return row * GEMM_ROW_BYTES + ((seg ^ gemm_a_swz(row)) << 4); }
// MFMA lane (r = lane & 31, h = lane >> 5) takes k = 16 h .. 16 h + 15 of the stage: segments 4 h .. 4 h + 3 of A, rows 16 h + e of B'
CFFT_HD constexpr int gemm_b_lds_offset(int k, int col) { return (k * GEMM_COLS + col) * 4; }

}  // namespace cfft
