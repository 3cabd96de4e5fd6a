// Frame ingest (gen6d_amd/ingest.py; reference prepare.py:16-42 video2image): camera-native frames -> the RGB working-resolution images
// of a batch, one launch for all frames.  The arithmetic is exact integer (include/gen6d_hip.h) and is restated in numpy
// by tests/test_ingest_cpu.py.  Measured at 2.0 - 2.4 TB/s (a third of the HBM rate, bound by byte loads and the per-tap conversion)
// and under half a percent of a tracker tick (profiles/r09_ingest_bench.md).
//
// Launch shape: the canvas is cut into 128 x 8 pixel tiles; block = one tile of one frame (flat list: blockIdx.x = frame * tiles + tile),
// 256 threads, thread = 4 consecutive pixels of one canvas row.  The 64-bit divisions of the sampling rule are done once per tile and
// canvas column / row (136 per 1024 pixels) into LDS as packed (index, step, weight) words.  A wave reads 2 canvas rows x 128 pixels: at
// rotate 0 / 180 that is whole stretches of source rows; 12 output bytes per thread go out as three dwords when the canvas rows are
// dword-aligned (W % 4 == 0).  Taps of weight 0 are not loaded (a same-size frame costs one tap per pixel), and the chroma terms of an
// NV12 sample are computed once for the taps of its 2 x 2 block (at 2:1 all four taps of a pixel share one).
// g6d_frame_ingest_mesh (second half of the file) is the same launch with a lens per frame: blocks of a frame with a mesh take their
// source coordinates from it (nodes in LDS, 64-bit integer interpolation), blocks of a frame without one run the plain tile.
// Frames of the formats after NV12 and of the full-range matrices take a block-uniform branch to the same tiles on
// frame_src.h's `Yuv` taps, in both kernels: a tick that mixes all eleven formats, with and without lenses, is one launch.
// g6d_frame_ingest_area (last part of the file) is the launch with an exact-integer area filter where a picture shrinks (§4.26); its lens
// frames that ask for it are supersampled through their mesh by a second kernel behind it (§4.28).
#include "frame_src.h"

namespace {

constexpr int TW = 128, TH = 8;

// canvas coordinate t of an axis with `tgt` picture pixels over `src` source pixels -> i0 | (i1 - i0) << 13 | weight << 14
__device__ __forceinline__ unsigned sample_word(int t, int tgt, int src) {
  long long f = (long long)((unsigned long long)(2 * t + 1) * (unsigned)src * 1024ull / (unsigned)tgt) - 1024;
  const long long hi = (long long)(src - 1) * 2048;
  f = f < 0 ? 0 : (f > hi ? hi : f);
  const unsigned i0 = (unsigned)(f >> 11), w = (unsigned)(f & 2047);
  return i0 | ((i0 + 1 < (unsigned)src ? 1u : 0u) << 13) | (w << 14);
}

// one tile of a frame by the plain rule; EXT: a frame of the formats after NV12 or of a full-range matrix (frame_src.h `extended`)
template <bool EXT>
__device__ __forceinline__ void plain_tile(const G6dFrame& f, unsigned* cw, unsigned char* __restrict__ out, int slot, int H, int W, int X0,
                                           int Y0);

__global__ void __launch_bounds__(256) frame_ingest_kernel(const G6dFrame* __restrict__ frames, unsigned char* __restrict__ out, int B, int H,
                                                           int W, float* __restrict__ K_out, int tiles_x, int tiles) {
  __shared__ unsigned cw[TW + TH];
  const int fi = blockIdx.x / tiles, tile = blockIdx.x - fi * tiles;
  const G6dFrame& f = frames[fi];
  const int slot = f.slot;
  if (slot < 0 || slot >= B) return;                      // (block-uniform)
  const int t = threadIdx.x;
  if (tile == 0 && t < 9) K_out[(size_t)9 * slot + t] = f.K[t];
  const int X0 = (tile % tiles_x) * TW, Y0 = (tile / tiles_x) * TH;
  if (extended(f)) { plain_tile<true>(f, cw, out, slot, H, W, X0, Y0); return; }   // (block-uniform) the body below stays as measured
  const int ws = f.width, hs = f.height, rot = f.rotate;
  const int ow = min(f.out_w, W), oh = min(f.out_h, H);   // an empty or negative picture leaves a black canvas
  const bool swap = rot == 90 || rot == 270;
  if (t < TW + TH) {
    unsigned v = 0;
    if (t < TW) {
      const int X = X0 + t;
      if (X < ow) v = sample_word((rot == 90 || rot == 180) ? f.out_w - 1 - X : X, f.out_w, swap ? hs : ws);
    } else {
      const int Y = Y0 + t - TW;
      if (Y < oh) v = sample_word((rot == 180 || rot == 270) ? f.out_h - 1 - Y : Y, f.out_h, swap ? ws : hs);
    }
    cw[t] = v;
  }
  __syncthreads();
  const int ry = t >> 5, X = X0 + ((t & 31) << 2), Y = Y0 + ry;
  if (Y >= H || X >= W) return;
  Src s;
  s.p0 = static_cast<const unsigned char*>(f.plane0); s.p1 = static_cast<const unsigned char*>(f.plane1);
  s.pitch0 = f.pitch0; s.pitch1 = f.pitch1;
  s.nv12 = f.format == G6D_FMT_NV12;
  s.bpp = f.format >= G6D_FMT_RGBA32 ? 4 : 3;
  s.ro = (f.format == G6D_FMT_BGR24 || f.format == G6D_FMT_BGRA32) ? 2 : 0;
  const bool m709 = f.matrix == 1;
  s.cvr = m709 ? 1880097 : 1673527; s.cug = m709 ? 223347 : 409993; s.cvg = m709 ? 558891 : 852492; s.cub = m709 ? 2214593 : 2116026;
  const unsigned rw = cw[TW + ry];
  unsigned char px[12];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int r = 0, g = 0, b = 0;
    if (X + k < ow && Y < oh) {
      const unsigned c = cw[(t & 31) * 4 + k];
      const unsigned xw = swap ? rw : c, yw = swap ? c : rw;
      const int x0 = xw & 8191, x1 = x0 + ((xw >> 13) & 1), y0 = yw & 8191, y1 = y0 + ((yw >> 13) & 1);
      const unsigned wa = xw >> 14, wb = yw >> 14;
      const unsigned w00 = (2048 - wa) * (2048 - wb), w01 = wa * (2048 - wb), w10 = (2048 - wa) * wb, w11 = wa * wb;
      int r1, g1, b1;
      unsigned ar = 1u << 21, ag = 1u << 21, ab = 1u << 21;
#define G6D_ACC(w) { ar += (w) * r1; ag += (w) * g1; ab += (w) * b1; }
      if (s.nv12) {                                       // (block-uniform) a UV sample is loaded once for the taps that share it
        const bool sx = (x1 >> 1) == (x0 >> 1), sy = (y1 >> 1) == (y0 >> 1);
        const Chroma k00 = chroma(s, x0 >> 1, y0 >> 1);
        tap_nv12(s, k00, x0, y0, r1, g1, b1); G6D_ACC(w00)
        Chroma k01 = k00;
        if (wa) { if (!sx) k01 = chroma(s, x1 >> 1, y0 >> 1); tap_nv12(s, k01, x1, y0, r1, g1, b1); G6D_ACC(w01) }
        if (wb) {
          const Chroma k10 = sy ? k00 : chroma(s, x0 >> 1, y1 >> 1);
          tap_nv12(s, k10, x0, y1, r1, g1, b1); G6D_ACC(w10)
          if (wa) {
            const Chroma k11 = sx ? k10 : (sy ? k01 : chroma(s, x1 >> 1, y1 >> 1));
            tap_nv12(s, k11, x1, y1, r1, g1, b1); G6D_ACC(w11)
          }
        }
      } else {
        tap_packed(s, x0, y0, r1, g1, b1); G6D_ACC(w00)
        if (wa) { tap_packed(s, x1, y0, r1, g1, b1); G6D_ACC(w01) }
        if (wb) { tap_packed(s, x0, y1, r1, g1, b1); G6D_ACC(w10) }
        if (wa && wb) { tap_packed(s, x1, y1, r1, g1, b1); G6D_ACC(w11) }
      }
#undef G6D_ACC
      r = ar >> 22; g = ag >> 22; b = ab >> 22;
    }
    px[3 * k] = (unsigned char)r; px[3 * k + 1] = (unsigned char)g; px[3 * k + 2] = (unsigned char)b;
  }
  unsigned char* o = out + (((size_t)slot * H + Y) * W + X) * 3;
  if (X + 4 <= W && (reinterpret_cast<uintptr_t>(o) & 3u) == 0) {
    unsigned* o32 = reinterpret_cast<unsigned*>(o);
#pragma unroll
    for (int j = 0; j < 3; ++j)
      o32[j] = (unsigned)px[4 * j] | ((unsigned)px[4 * j + 1] << 8) | ((unsigned)px[4 * j + 2] << 16) | ((unsigned)px[4 * j + 3] << 24);
  } else {
    const int nb = 3 * min(4, W - X);
#pragma unroll
    for (int j = 0; j < 12; ++j)
      if (j < nb) o[j] = px[j];
  }
}

// ---- g6d_frame_ingest_mesh: the same launch with a lens per frame (a coarse mesh of source coordinates instead of the scaling rule) ----
// frame_ingest_kernel above stays as it was measured (§4.17); the pieces of its body are restated here as functions so that the plain and
// the mesh tile of this kernel share them (pulling them out of frame_ingest_kernel changes its register allocation and schedule).

// the four taps of one pixel (weights wa, wb in 1/2048), blended per channel
__device__ __forceinline__ void gather(const Src& s, int x0, int x1, int y0, int y1, unsigned wa, unsigned wb, int& r, int& g, int& b) {
  const unsigned w00 = (2048 - wa) * (2048 - wb), w01 = wa * (2048 - wb), w10 = (2048 - wa) * wb, w11 = wa * wb;
  int r1, g1, b1;
  unsigned ar = 1u << 21, ag = 1u << 21, ab = 1u << 21;
#define G6D_ACC(w) { ar += (w) * r1; ag += (w) * g1; ab += (w) * b1; }
  if (s.nv12) {                                           // (block-uniform) a UV sample is loaded once for the taps that share it
    const bool sx = (x1 >> 1) == (x0 >> 1), sy = (y1 >> 1) == (y0 >> 1);
    const Chroma k00 = chroma(s, x0 >> 1, y0 >> 1);
    tap_nv12(s, k00, x0, y0, r1, g1, b1); G6D_ACC(w00)
    Chroma k01 = k00;
    if (wa) { if (!sx) k01 = chroma(s, x1 >> 1, y0 >> 1); tap_nv12(s, k01, x1, y0, r1, g1, b1); G6D_ACC(w01) }
    if (wb) {
      const Chroma k10 = sy ? k00 : chroma(s, x0 >> 1, y1 >> 1);
      tap_nv12(s, k10, x0, y1, r1, g1, b1); G6D_ACC(w10)
      if (wa) {
        const Chroma k11 = sx ? k10 : (sy ? k01 : chroma(s, x1 >> 1, y1 >> 1));
        tap_nv12(s, k11, x1, y1, r1, g1, b1); G6D_ACC(w11)
      }
    }
  } else {
    tap_packed(s, x0, y0, r1, g1, b1); G6D_ACC(w00)
    if (wa) { tap_packed(s, x1, y0, r1, g1, b1); G6D_ACC(w01) }
    if (wb) { tap_packed(s, x0, y1, r1, g1, b1); G6D_ACC(w10) }
    if (wa && wb) { tap_packed(s, x1, y1, r1, g1, b1); G6D_ACC(w11) }
  }
#undef G6D_ACC
  r = ar >> 22; g = ag >> 22; b = ab >> 22;
}

// the same for a frame of the extended formats: taps by frame_src.h's ext_taps (a tap of weight 0 is not loaded and counts as 0)
__device__ __forceinline__ void gather(const Yuv& s, int x0, int x1, int y0, int y1, unsigned wa, unsigned wb, int& r, int& g, int& b) {
  const unsigned w00 = (2048 - wa) * (2048 - wb), w01 = wa * (2048 - wb), w10 = (2048 - wa) * wb, w11 = wa * wb;
  Tap t00, t01, t10, t11;
  ext_taps<true>(s, x0, x1, y0, y1, wa != 0, wb != 0, t00, t01, t10, t11);
  r = ((1u << 21) + w00 * t00.r + w01 * t01.r + w10 * t10.r + w11 * t11.r) >> 22;
  g = ((1u << 21) + w00 * t00.g + w01 * t01.g + w10 * t10.g + w11 * t11.g) >> 22;
  b = ((1u << 21) + w00 * t00.b + w01 * t01.b + w10 * t10.b + w11 * t11.b) >> 22;
}
template <bool EXT> __device__ __forceinline__ auto tap_source(const G6dFrame& f) {
  if constexpr (EXT) return yuv_of(f);
  else return source_of(f);
}

// a thread's 4 pixels -> canvas row Y of image `slot` from column X on
__device__ __forceinline__ void store4(unsigned char* __restrict__ out, const unsigned char (&px)[12], int slot, int H, int W, int X, int Y) {
  unsigned char* o = out + (((size_t)slot * H + Y) * W + X) * 3;
  if (X + 4 <= W && (reinterpret_cast<uintptr_t>(o) & 3u) == 0) {
    unsigned* o32 = reinterpret_cast<unsigned*>(o);
#pragma unroll
    for (int j = 0; j < 3; ++j)
      o32[j] = (unsigned)px[4 * j] | ((unsigned)px[4 * j + 1] << 8) | ((unsigned)px[4 * j + 2] << 16) | ((unsigned)px[4 * j + 3] << 24);
  } else {
    const int nb = 3 * min(4, W - X);
#pragma unroll
    for (int j = 0; j < 12; ++j)
      if (j < nb) o[j] = px[j];
  }
}

// one tile of a frame by the plain rule (scaling + quarter turn); cw: TW + TH words of LDS
template <bool EXT>
__device__ __forceinline__ void plain_tile(const G6dFrame& f, unsigned* cw, unsigned char* __restrict__ out, int slot, int H, int W, int X0,
                                           int Y0) {
  const int t = threadIdx.x;
  const int ws = f.width, hs = f.height, rot = f.rotate;
  const int ow = min(f.out_w, W), oh = min(f.out_h, H);   // an empty or negative picture leaves a black canvas
  const bool swap = rot == 90 || rot == 270;
  if (t < TW + TH) {
    unsigned v = 0;
    if (t < TW) {
      const int X = X0 + t;
      if (X < ow) v = sample_word((rot == 90 || rot == 180) ? f.out_w - 1 - X : X, f.out_w, swap ? hs : ws);
    } else {
      const int Y = Y0 + t - TW;
      if (Y < oh) v = sample_word((rot == 180 || rot == 270) ? f.out_h - 1 - Y : Y, f.out_h, swap ? ws : hs);
    }
    cw[t] = v;
  }
  __syncthreads();
  const int ry = t >> 5, X = X0 + ((t & 31) << 2), Y = Y0 + ry;
  if (Y >= H || X >= W) return;
  const auto s = tap_source<EXT>(f);
  const unsigned rw = cw[TW + ry];
  unsigned char px[12];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int r = 0, g = 0, b = 0;
    if (X + k < ow && Y < oh) {
      const unsigned c = cw[(t & 31) * 4 + k];
      const unsigned xw = swap ? rw : c, yw = swap ? c : rw;
      const int x0 = xw & 8191, x1 = x0 + ((xw >> 13) & 1), y0 = yw & 8191, y1 = y0 + ((yw >> 13) & 1);
      gather(s, x0, x1, y0, y1, xw >> 14, yw >> 14, r, g, b);
    }
    px[3 * k] = (unsigned char)r; px[3 * k + 1] = (unsigned char)g; px[3 * k + 2] = (unsigned char)b;
  }
  store4(out, px, slot, H, W, X, Y);
}

constexpr int MESH_NX = TW / 2 + 1, MESH_NY = TH / 2 + 1;  // a tile's nodes at the finest step, 2

// v = (g - j) * m0 + j * m1 of one node column (x and y parts), 64-bit: |m| <= 2^30, g <= 16
struct Col { long long x, y; };
__device__ __forceinline__ Col column(const int2* nd, int at, int below, int g, int j) {
  const int2 m0 = nd[at], m1 = nd[at + below];
  return Col{(long long)(g - j) * m0.x + (long long)j * m1.x, (long long)(g - j) * m0.y + (long long)j * m1.y};
}

// one tile of a lens frame.  The canvas coordinates are those AFTER the quarter turn (the host undid it when it built the mesh), so there
// is no rotation here.  nd: MESH_NX * MESH_NY nodes of LDS
template <bool EXT>
__device__ __forceinline__ void mesh_tile(const G6dFrame& f, const G6dMesh& m, int2* nd, unsigned char* __restrict__ out, int slot, int H, int W,
                                          int X0, int Y0) {
  const int t = threadIdx.x;
  const int lg = min(max(m.step_log2, 1), 4), g = 1 << lg, sh = 2 * lg + 5;
  const int tnx = (TW >> lg) + 1, tny = max(TH >> lg, 1) + 1;   // nodes of this tile (a tile lies inside one row of cells at step 16)
  const int c0 = X0 >> lg, r0 = Y0 >> lg;
  for (int k = t; k < tnx * tny; k += 256) {              // columns / rows past the mesh's edge are read only by pixels outside the picture
    const int r = k / tnx, c = k - r * tnx;
    const int* p = m.nodes + 2 * ((size_t)max(min(r0 + r, m.ny - 1), 0) * m.nx + max(min(c0 + c, m.nx - 1), 0));
    nd[k] = make_int2(p[0], p[1]);
  }
  __syncthreads();
  const int ry = t >> 5, X = X0 + ((t & 31) << 2), Y = Y0 + ry;
  if (Y >= H || X >= W) return;
  const int ws = f.width, hs = f.height;
  const int ow = min(f.out_w, W), oh = min(f.out_h, H);
  const auto s = tap_source<EXT>(f);
  // a thread's 4 pixels lie in one cell (two at step 2): the node columns they use, blended down the cell once
  const int j = Y & (g - 1), at = ((Y >> lg) - r0) * tnx + (X >> lg) - c0;
  const Col q0 = column(nd, at, tnx, g, j), q1 = column(nd, at + 1, tnx, g, j);
  const Col q2 = lg == 1 ? column(nd, at + 2, tnx, g, j) : q1;
  const long long half = 1ll << (sh - 1);
  const int xhi = (ws - 1) * 2048, yhi = (hs - 1) * 2048;
  unsigned char px[12];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int r = 0, gr = 0, b = 0;
    if (X + k < ow && Y < oh) {
      const bool second = lg == 1 && k >= 2;
      const Col& l = second ? q1 : q0;
      const Col& h = second ? q2 : q1;
      const int i = (X + k) & (g - 1);
      int fx = (int)(((g - i) * l.x + i * h.x + half) >> sh), fy = (int)(((g - i) * l.y + i * h.y + half) >> sh);
      if (fx >= -1024 && fx <= xhi + 1024 && fy >= -1024 && fy <= yhi + 1024) {   // else: the constant border, black
        fx = min(max(fx, 0), xhi); fy = min(max(fy, 0), yhi);
        const int x0 = fx >> 11, y0 = fy >> 11;
        gather(s, x0, min(x0 + 1, ws - 1), y0, min(y0 + 1, hs - 1), fx & 2047, fy & 2047, r, gr, b);
      }
    }
    px[3 * k] = (unsigned char)r; px[3 * k + 1] = (unsigned char)gr; px[3 * k + 2] = (unsigned char)b;
  }
  store4(out, px, slot, H, W, X, Y);
}

__global__ void __launch_bounds__(256) frame_ingest_lens_kernel(const G6dFrame* __restrict__ frames, const G6dMesh* __restrict__ meshes,
                                                                unsigned char* __restrict__ out, int B, int H, int W,
                                                                float* __restrict__ K_out, int tiles_x, int tiles) {
  __shared__ unsigned cw[TW + TH];
  __shared__ int2 nd[MESH_NX * MESH_NY];
  const int fi = blockIdx.x / tiles, tile = blockIdx.x - fi * tiles;
  const G6dFrame& f = frames[fi];
  const int slot = f.slot;
  if (slot < 0 || slot >= B) return;                      // (block-uniform)
  if (tile == 0 && threadIdx.x < 9) K_out[(size_t)9 * slot + threadIdx.x] = f.K[threadIdx.x];
  const int X0 = (tile % tiles_x) * TW, Y0 = (tile / tiles_x) * TH;
  const G6dMesh& m = meshes[fi];
  if (extended(f)) {                                             // (block-uniform, as every branch here)
    if (m.nodes) mesh_tile<true>(f, m, nd, out, slot, H, W, X0, Y0);
    else plain_tile<true>(f, cw, out, slot, H, W, X0, Y0);
  } else if (m.nodes) mesh_tile<false>(f, m, nd, out, slot, H, W, X0, Y0);
  else plain_tile<false>(f, cw, out, slot, H, W, X0, Y0);
}

// ---- g6d_frame_ingest_area: the same launch with an area filter on every axis that shrinks (include/gen6d_hip.h) ----
// The two kernels above stay as they were measured.  Same tiles, same flat block list; what differs is the thread's work.  A canvas pixel
// of a shrinking axis owns the source stretch [t S, (t+1) S) / T, so the footprints of neighbouring pixels are disjoint but for the source
// pixel a boundary cuts: a per-thread loop over the footprint reads every source byte once (twice at such a boundary, from the same
// block or its tile neighbour) and converts it there, and a horizontal pass staged in LDS would have nothing left to share.  What decides
// the speed is which lanes sit side by side: thread = one canvas COLUMN of the tile (4 of its 8 rows), so the 64 lanes of a wave walk 64
// neighbouring footprints of one canvas row and each of their loads covers one contiguous stretch of a source row (at 4:1, 256 bytes of a
// luma plane).  The 3-byte results go through LDS and leave as dwords, as the plain tile's do.  A turned frame (90 / 270) reads columns,
// as it does in the plain tile.  The descriptors (first index, first weight, count) of the tile's 128 columns and 8 rows are built
// once per tile with 32-bit divisions (t S < 2^26); the tap loops divide nothing.  Cost grows with the footprint: one thread sums
// (S / T)^2 taps per pixel, which is the work there is for the ratios the ingest is meant for and slow for a thumbnail of a huge frame.

// canvas coordinate t of an axis with `tgt` picture pixels over `src` source pixels -> (i0 | w0 << 13, count): the taps i0 .. i0 + count - 1;
// the first weighs w0, every later one min(step, what is left of D), step = tgt and D = src where the axis shrinks, else 2048 and 2048
__device__ __forceinline__ uint2 area_word(int t, int tgt, int src) {
  if (src <= tgt) {                                       // no shrink: the plain rule's two taps (2048 - a, a), one when a == 0
    const unsigned v = sample_word(t, tgt, src), a = v >> 14;
    return make_uint2((v & 8191u) | ((2048u - a) << 13), a ? 2u : 1u);
  }
  const unsigned lo = (unsigned)t * (unsigned)src;        // t < tgt < src <= 8192: below 2^26
  const unsigned i0 = lo / (unsigned)tgt, i1 = (lo + (unsigned)src - 1u) / (unsigned)tgt;
  return make_uint2(i0 | (((i0 + 1u) * (unsigned)tgt - lo) << 13), i1 - i0 + 1u);   // (i0 + 1) tgt <= lo + tgt < lo + src: the min of the rule
}

// floor((2 sigma + D) / (2 D)) with d2 = 2 D <= 2^27 and sigma <= 255 D: the quotient is at most 255, so a float estimate (relative error
// below 2^-21, absolute below 2^-13) is the floor or one beside it, and one exact 64-bit remainder settles which
__device__ __forceinline__ int area_round(unsigned long long sigma, unsigned d2, float inv) {
  const unsigned long long n = 2ull * sigma + (d2 >> 1);
  int q = (int)((float)n * inv);
  const long long r = (long long)n - (long long)q * (long long)d2;
  if (r < 0) --q;
  else if (r >= (long long)d2) ++q;
  return q;
}

// KIND: 0 packed RGB, 1 NV12 under matrix 0 / 1 (both on `Src`), 2 the 8-bit YUV layouts on `Yuv`, 3 P010, 4 GRAY8
template <int KIND, typename S>
__device__ __forceinline__ void area_sum(const S& s, uint2 xd, uint2 yd, unsigned xstep, unsigned xD, unsigned ystep, unsigned yD,
                                         unsigned long long& R, unsigned long long& G, unsigned long long& Bl) {
  const int x0 = xd.x & 8191, y0 = yd.x & 8191, nx = (int)xd.y, ny = (int)yd.y;
  const unsigned xw0 = xd.x >> 13;
  unsigned wy = yd.x >> 13, ly = yD - wy;
  R = G = Bl = 0;
  for (int j = 0; j < ny; ++j) {
    const int y = y0 + j;
    unsigned rr = 0, gg = 0, bb = 0, wx = xw0, lx = xD - xw0;   // a row's sums: at most 255 * 2^13
    int r1, g1, b1;
    if constexpr (KIND == 1) {                            // a UV sample is loaded and converted once for the taps of a row that share it
      int cx = -1;
      Chroma k;
      for (int i = 0; i < nx; ++i) {
        const int x = x0 + i;
        if ((x >> 1) != cx) { cx = x >> 1; k = chroma(s, cx, y >> 1); }
        tap_nv12(s, k, x, y, r1, g1, b1);
        rr += wx * r1; gg += wx * g1; bb += wx * b1;
        wx = min(xstep, lx); lx -= wx;
      }
    } else if constexpr (KIND == 2 || KIND == 3) {
      using T = typename std::conditional<KIND == 3, long long, int>::type;
      int cx = -1;
      Kc<T> k;
      for (int i = 0; i < nx; ++i) {
        const int x = x0 + i;
        if ((x >> 1) != cx) { cx = x >> 1; k = yuv_chroma<T>(s, cx, y >> s.csy); }
        yuv_tap<T>(s, k, x, y, r1, g1, b1);
        rr += wx * r1; gg += wx * g1; bb += wx * b1;
        wx = min(xstep, lx); lx -= wx;
      }
    } else {
      for (int i = 0; i < nx; ++i) {
        if constexpr (KIND == 0) tap_packed(s, x0 + i, y, r1, g1, b1);
        else { const Tap t = gray_tap(s, x0 + i, y); r1 = t.r; g1 = t.g; b1 = t.b; }
        rr += wx * r1; gg += wx * g1; bb += wx * b1;
        wx = min(xstep, lx); lx -= wx;
      }
    }
    R += (unsigned long long)wy * rr; G += (unsigned long long)wy * gg; Bl += (unsigned long long)wy * bb;   // at most 255 * 2^26
    wy = min(ystep, ly); ly -= wy;
  }
}

// one tile of a frame by the area rule; aw: TW + TH descriptors, stage: the tile's TW x TH x 3 result bytes (LDS both)
template <int KIND, typename S>
__device__ __forceinline__ void area_tile(const G6dFrame& f, const S& s, uint2* aw, unsigned* stage, unsigned char* __restrict__ out, int slot,
                                          int H, int W, int X0, int Y0) {
  const int t = threadIdx.x;
  const int rot = f.rotate;
  const int ow = min(f.out_w, W), oh = min(f.out_h, H);   // an empty or negative picture leaves a black canvas
  const bool swap = rot == 90 || rot == 270;
  const int csrc = swap ? f.height : f.width, rsrc = swap ? f.width : f.height;   // the source extent a canvas column / row index runs over
  if (t < TW + TH) {
    uint2 v = make_uint2(0u, 0u);
    if (t < TW) {
      const int X = X0 + t;
      if (X < ow) v = area_word((rot == 90 || rot == 180) ? f.out_w - 1 - X : X, f.out_w, csrc);
    } else {
      const int Y = Y0 + t - TW;
      if (Y < oh) v = area_word((rot == 180 || rot == 270) ? f.out_h - 1 - Y : Y, f.out_h, rsrc);
    }
    aw[t] = v;
  }
  __syncthreads();
  const bool cshrink = csrc > f.out_w, rshrink = rsrc > f.out_h;
  const unsigned cstep = cshrink ? (unsigned)f.out_w : 2048u, cD = cshrink ? (unsigned)csrc : 2048u;
  const unsigned rstep = rshrink ? (unsigned)f.out_h : 2048u, rD = rshrink ? (unsigned)rsrc : 2048u;
  const unsigned d2 = 2u * cD * rD;                       // 2 D <= 2^27
  const float inv = 1.f / (float)d2;
  const int col = t & (TW - 1), X = X0 + col;
  unsigned char* st = reinterpret_cast<unsigned char*>(stage);
  const uint2 c = aw[col];
#pragma unroll 1
  for (int ry = t >> 7; ry < TH; ry += 2) {
    int r = 0, g = 0, b = 0;
    if (X < ow && Y0 + ry < oh) {
      const uint2 rw = aw[TW + ry];
      unsigned long long sr, sg, sb;
      if (swap) area_sum<KIND>(s, rw, c, rstep, rD, cstep, cD, sr, sg, sb);
      else area_sum<KIND>(s, c, rw, cstep, cD, rstep, rD, sr, sg, sb);
      r = area_round(sr, d2, inv); g = area_round(sg, d2, inv); b = area_round(sb, d2, inv);
    }
    unsigned char* p = st + (ry * TW + col) * 3;
    p[0] = (unsigned char)r; p[1] = (unsigned char)g; p[2] = (unsigned char)b;
  }
  __syncthreads();
  // the tile's rows leave as dwords where the canvas row is dword-aligned (3 TW bytes of a row = 96 dwords), as bytes elsewhere
  const int nb = 3 * min(TW, W - X0);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int idx = t + 256 * j, ry = idx / 96, b0 = 4 * (idx - ry * 96), Y = Y0 + ry;
    if (Y >= H || b0 >= nb) continue;
    unsigned char* o = out + (((size_t)slot * H + Y) * W + X0) * 3 + b0;
    const unsigned v = stage[idx];
    if (b0 + 4 <= nb && (reinterpret_cast<uintptr_t>(o) & 3u) == 0) *reinterpret_cast<unsigned*>(o) = v;
    else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (b0 + e < nb) o[e] = (unsigned char)(v >> (8 * e));
    }
  }
}

// ---- lens frames of g6d_frame_ingest_area: n x n sub-samples per canvas pixel through the mesh (header) ----
// The mesh tile's launch shape (thread = 4 consecutive pixels of a canvas row, store4) with a loop over the pixel's sub-samples around
// its body.  A pixel's sub-samples lie within half a canvas pixel of its centre, so those of a pixel on a cell's first column / row fall
// into the cell before it: the tile's node array has one more column at the left and one more row at the top than mesh_tile's.
// 60 VGPRs, no scratch, 3168 bytes of LDS; 0.50 ms for 32 1080p NV12 frames at n = 2 and 4.3 ms for 32 2160p frames at n = 4
// (profiles/r33_lens_area.md): 4 n^2 taps per pixel, each converted where it is read.

constexpr int MESHA_NX = TW / 2 + 2, MESHA_NY = TH / 2 + 2;   // a tile's nodes at the finest step, 2

// (TWINS of the two `gather` above: the same taps and weights, the sum neither rounded nor shifted.  A change of the blend goes into both;
// tests/test_ingest_lens_area_gpu.py holds them together: samples_log2 = 0 through mesh_tile against the restatement of this rule)
__device__ __forceinline__ void gather_sum(const Src& s, int x0, int x1, int y0, int y1, unsigned wa, unsigned wb, unsigned& ar, unsigned& ag,
                                           unsigned& ab) {
  const unsigned w00 = (2048 - wa) * (2048 - wb), w01 = wa * (2048 - wb), w10 = (2048 - wa) * wb, w11 = wa * wb;
  int r1, g1, b1;
  ar = ag = ab = 0;
#define G6D_ACC(w) { ar += (w) * r1; ag += (w) * g1; ab += (w) * b1; }
  if (s.nv12) {                                           // (block-uniform) a UV sample is loaded once for the taps that share it
    const bool sx = (x1 >> 1) == (x0 >> 1), sy = (y1 >> 1) == (y0 >> 1);
    const Chroma k00 = chroma(s, x0 >> 1, y0 >> 1);
    tap_nv12(s, k00, x0, y0, r1, g1, b1); G6D_ACC(w00)
    Chroma k01 = k00;
    if (wa) { if (!sx) k01 = chroma(s, x1 >> 1, y0 >> 1); tap_nv12(s, k01, x1, y0, r1, g1, b1); G6D_ACC(w01) }
    if (wb) {
      const Chroma k10 = sy ? k00 : chroma(s, x0 >> 1, y1 >> 1);
      tap_nv12(s, k10, x0, y1, r1, g1, b1); G6D_ACC(w10)
      if (wa) {
        const Chroma k11 = sx ? k10 : (sy ? k01 : chroma(s, x1 >> 1, y1 >> 1));
        tap_nv12(s, k11, x1, y1, r1, g1, b1); G6D_ACC(w11)
      }
    }
  } else {
    tap_packed(s, x0, y0, r1, g1, b1); G6D_ACC(w00)
    if (wa) { tap_packed(s, x1, y0, r1, g1, b1); G6D_ACC(w01) }
    if (wb) { tap_packed(s, x0, y1, r1, g1, b1); G6D_ACC(w10) }
    if (wa && wb) { tap_packed(s, x1, y1, r1, g1, b1); G6D_ACC(w11) }
  }
#undef G6D_ACC
}
// the extended formats: frame_src.h's yuv_taps (a chroma sample loaded once for the taps that share it, a tap of weight 0 not loaded) with
// every tap summed as it arrives.  What is kept of a chroma sample is (d, e), not its three products (yuv_chroma's Kc, 64-bit for P010):
// the products are formed again at each tap, which costs multiplies and saves the registers that decide how many waves the plain tiles
// of this launch run with
struct De { int d, e; };
template <typename T> __device__ __forceinline__ De yuv_de(const Yuv& s, int cx, int cy) {
  constexpr int mid = sizeof(T) == 8 ? 512 : 128;
  const size_t o = (size_t)cy * s.cpitch + (size_t)cx * s.cstep;
  return De{sample<T>(s.pu + o) - mid, sample<T>(s.pv + o) - mid};
}
template <typename T> __device__ __forceinline__ void yuv_tap_de(const Yuv& s, De q, int x, int y, int& r, int& g, int& b) {   // yuv_chroma's terms
  constexpr T rnd = sizeof(T) == 8 ? (T)1 << 21 : (T)1 << 19;
  const T d = q.d, e = q.e;
  yuv_tap<T>(s, Kc<T>{s.cvr * e + rnd, -s.cug * d - s.cvg * e + rnd, s.cub * d + rnd}, x, y, r, g, b);
}
template <typename T>
__device__ __forceinline__ void yuv_gather_sum(const Yuv& s, int x0, int x1, int y0, int y1, unsigned wa, unsigned wb, unsigned& ar,
                                               unsigned& ag, unsigned& ab) {
  int r1, g1, b1;
  ar = ag = ab = 0;
#define G6D_ACC(w) { const unsigned w_ = (w); ar += w_ * r1; ag += w_ * g1; ab += w_ * b1; }
  const bool sx = (x1 >> 1) == (x0 >> 1), sy = (y1 >> s.csy) == (y0 >> s.csy);
  De k0 = yuv_de<T>(s, x0 >> 1, y0 >> s.csy), k1 = k0;    // the chroma of the row's x0 tap and of its x1 tap
  yuv_tap_de<T>(s, k0, x0, y0, r1, g1, b1); G6D_ACC((2048 - wa) * (2048 - wb))
  if (wa) { if (!sx) k1 = yuv_de<T>(s, x1 >> 1, y0 >> s.csy); yuv_tap_de<T>(s, k1, x1, y0, r1, g1, b1); G6D_ACC(wa * (2048 - wb)) }
  if (wb) {
    if (!sy) k0 = yuv_de<T>(s, x0 >> 1, y1 >> s.csy);
    yuv_tap_de<T>(s, k0, x0, y1, r1, g1, b1); G6D_ACC((2048 - wa) * wb)
    if (wa) {
      if (sx) k1 = k0;
      else if (!sy) k1 = yuv_de<T>(s, x1 >> 1, y1 >> s.csy);
      yuv_tap_de<T>(s, k1, x1, y1, r1, g1, b1); G6D_ACC(wa * wb)
    }
  }
#undef G6D_ACC
}
__device__ __forceinline__ void gather_sum(const Yuv& s, int x0, int x1, int y0, int y1, unsigned wa, unsigned wb, unsigned& ar, unsigned& ag,
                                           unsigned& ab) {
  if (s.kind == 0) yuv_gather_sum<int>(s, x0, x1, y0, y1, wa, wb, ar, ag, ab);                   // (block-uniform)
  else if (s.kind == 1) yuv_gather_sum<long long>(s, x0, x1, y0, y1, wa, wb, ar, ag, ab);
  else {
    const unsigned v = (2048 - wa) * (2048 - wb) * gray_tap(s, x0, y0).r + (wa ? wa * (2048 - wb) * gray_tap(s, x1, y0).r : 0u) +
                       (wb ? (2048 - wa) * wb * gray_tap(s, x0, y1).r : 0u) + (wa && wb ? wa * wb * gray_tap(s, x1, y1).r : 0u);
    ar = ag = ab = v;
  }
}

// one tile of a lens frame with 2^L x 2^L sub-samples per pixel, L = 1..3.  nd: MESHA_NX * MESHA_NY nodes of LDS.  Positions are in units
// of 1 / (2n) canvas pixel (U, V of the header), a cell is G = 2 n g of them wide.  The header's upper clamp of the cell index (nx - 2) is
// not computed: inside the picture nx >= ceil(out_w / g) + 1 keeps the index below it, and the LDS index depends on the position alone.
template <bool EXT>
__device__ __forceinline__ void mesh_area_tile(const G6dFrame& f, const G6dMesh& m, int L, int2* nd, unsigned char* __restrict__ out, int slot,
                                               int H, int W, int X0, int Y0) {
  const int t = threadIdx.x;
  const int lg = min(max(m.step_log2, 1), 4), n = 1 << L, lG = 1 + L + lg, G = 1 << lG, sh = 2 * lG + 5;
  const int tnx = (TW >> lg) + 2, tny = max(TH >> lg, 1) + 2;   // mesh_tile's nodes and the column / row before them
  const int c0 = (X0 >> lg) - 1, r0 = (Y0 >> lg) - 1;           // -1 at the picture's edge: loaded as a copy of 0 and not used (cells clamp at 0)
  for (int k = t; k < tnx * tny; k += 256) {              // columns / rows past the mesh's edge are read only by pixels outside the picture
    const int r = k / tnx, c = k - r * tnx;
    const int* p = m.nodes + 2 * ((size_t)max(min(r0 + r, m.ny - 1), 0) * m.nx + max(min(c0 + c, m.nx - 1), 0));
    nd[k] = make_int2(p[0], p[1]);
  }
  __syncthreads();
  const int ry = t >> 5, X = X0 + ((t & 31) << 2), Y = Y0 + ry;
  if (Y >= H || X >= W) return;
  const int ws = f.width, hs = f.height;
  const int ow = min(f.out_w, W), oh = min(f.out_h, H);
  const auto s = tap_source<EXT>(f);
  const long long half = 1ll << (sh - 1);
  const int xhi = (ws - 1) * 2048, yhi = (hs - 1) * 2048;
  const int fs = 22 + 2 * L;
  // One pixel at a time, its sums in 6 registers (sums for 4 pixels at once cost 24 and the kernel half the waves the plain tiles of this
  // launch run with); the loop is not unrolled, so its 3 bytes go into the thread's 12 by shifts, not by an index
  unsigned o0 = 0, o1 = 0, o2 = 0;
#pragma unroll 1
  for (int kk = 0; kk < 4; ++kk) {
    const int P = X + kk;
    if (P >= ow || Y >= oh) break;                        // the rest of the 4 lies outside the picture: 0
    unsigned long long sr = 0, sg = 0, sb = 0;            // sums of A: below 2^37
#pragma unroll 1
    for (int q = 0; q < n * n; ++q) {                     // sub-sample (k, l) = (q mod n, q / n): one loop, one counter
      // r: the pixel's cell row or, on that cell's first row and for l < n / 2, the one above; j < 0 at the top edge.  Columns likewise
      const int V = 2 * n * Y + 2 * (q >> L) + 1 - n, r = max(V >> lG, 0), j = V - (r << lG);
      const int U = 2 * n * P + 2 * (q & (n - 1)) + 1 - n, c = max(U >> lG, 0), i = U - (c << lG);
      // the four nodes of the cell straight from LDS: each term of S is one 32 x 32 -> 64-bit multiply-add (|weight| < 2^18), where node
      // columns blended once per sub-row are 64-bit factors, and 12 registers that stay live across the taps
      const int2* row = nd + (r - r0) * tnx - c0;
      const int2 m00 = row[c], m01 = row[c + 1], m10 = row[c + tnx], m11 = row[c + tnx + 1];
      const int w00 = (G - i) * (G - j), w01 = i * (G - j), w10 = (G - i) * j, w11 = i * j;
      int fx = (int)(((long long)w00 * m00.x + (long long)w01 * m01.x + (long long)w10 * m10.x + (long long)w11 * m11.x + half) >> sh);
      int fy = (int)(((long long)w00 * m00.y + (long long)w01 * m01.y + (long long)w10 * m10.y + (long long)w11 * m11.y + half) >> sh);
      if (fx >= -1024 && fx <= xhi + 1024 && fy >= -1024 && fy <= yhi + 1024) {   // else: the constant border, A = 0
        fx = min(max(fx, 0), xhi); fy = min(max(fy, 0), yhi);
        const int x0 = fx >> 11, y0 = fy >> 11;
        unsigned ar, ag, ab;
        gather_sum(s, x0, min(x0 + 1, ws - 1), y0, min(y0 + 1, hs - 1), fx & 2047, fy & 2047, ar, ag, ab);
        sr += ar; sg += ag; sb += ab;
      }
    }
    const unsigned long long rnd = 1ull << (fs - 1);
    const unsigned v = (unsigned)((sr + rnd) >> fs) | ((unsigned)((sg + rnd) >> fs) << 8) | ((unsigned)((sb + rnd) >> fs) << 16);
    o0 |= kk == 0 ? v : (kk == 1 ? v << 24 : 0u);
    o1 |= kk == 1 ? v >> 8 : (kk == 2 ? v << 16 : 0u);
    o2 |= kk == 2 ? v >> 16 : (kk == 3 ? v << 8 : 0u);
  }
  unsigned char px[12];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    px[e] = (unsigned char)(o0 >> (8 * e)); px[4 + e] = (unsigned char)(o1 >> (8 * e)); px[8 + e] = (unsigned char)(o2 >> (8 * e));
  }
  store4(out, px, slot, H, W, X, Y);
}

__global__ void __launch_bounds__(256) frame_ingest_area_kernel(const G6dFrame* __restrict__ frames, const G6dMesh* __restrict__ meshes,
                                                                unsigned char* __restrict__ out, int B, int H, int W,
                                                                float* __restrict__ K_out, int tiles_x, int tiles) {
  __shared__ uint2 aw[TW + TH];
  __shared__ unsigned stage[TW * TH * 3 / 4];
  __shared__ int2 nd[MESH_NX * MESH_NY];
  const int fi = blockIdx.x / tiles, tile = blockIdx.x - fi * tiles;
  const G6dFrame& f = frames[fi];
  const int slot = f.slot;
  if (slot < 0 || slot >= B) return;                      // (block-uniform, as every branch below)
  if (tile == 0 && threadIdx.x < 9) K_out[(size_t)9 * slot + threadIdx.x] = f.K[threadIdx.x];
  const int X0 = (tile % tiles_x) * TW, Y0 = (tile / tiles_x) * TH;
  if (meshes && meshes[fi].nodes) {                       // a lens frame: samples_log2 = 0 is the mesh rule itself (header, consequence 1);
    if (meshes[fi].samples_log2 > 0) return;              // more samples: frame_ingest_lens_area_kernel's frame
    if (extended(f)) mesh_tile<true>(f, meshes[fi], nd, out, slot, H, W, X0, Y0);
    else mesh_tile<false>(f, meshes[fi], nd, out, slot, H, W, X0, Y0);
    return;
  }
  if (extended(f)) {
    const Yuv s = yuv_of(f);
    if (s.kind == 0) area_tile<2>(f, s, aw, stage, out, slot, H, W, X0, Y0);
    else if (s.kind == 1) area_tile<3>(f, s, aw, stage, out, slot, H, W, X0, Y0);
    else area_tile<4>(f, s, aw, stage, out, slot, H, W, X0, Y0);
  } else {
    const Src s = source_of(f);
    if (s.nv12) area_tile<1>(f, s, aw, stage, out, slot, H, W, X0, Y0);
    else area_tile<0>(f, s, aw, stage, out, slot, H, W, X0, Y0);
  }
}

// The lens frames of a g6d_frame_ingest_area call that ask for more than one sample, in a launch of their own behind
// frame_ingest_area_kernel's (same grid; every other block leaves at once).  As a branch of that kernel the tile made its plain tiles 16 to
// 23 % slower at unchanged register and LDS figures (profiles/r33_lens_area.md), so that kernel keeps the code it was measured with.
__global__ void __launch_bounds__(256) frame_ingest_lens_area_kernel(const G6dFrame* __restrict__ frames, const G6dMesh* __restrict__ meshes,
                                                                     unsigned char* __restrict__ out, int B, int H, int W, int tiles_x,
                                                                     int tiles) {
  __shared__ int2 nd[MESHA_NX * MESHA_NY];
  const int fi = blockIdx.x / tiles, tile = blockIdx.x - fi * tiles;
  const G6dMesh& m = meshes[fi];
  if (!m.nodes || m.samples_log2 <= 0) return;            // (block-uniform, as every branch below) frame_ingest_area_kernel's frame
  const G6dFrame& f = frames[fi];
  const int slot = f.slot;
  if (slot < 0 || slot >= B) return;                      // (K_out[slot] is written by frame_ingest_area_kernel, for every frame)
  const int X0 = (tile % tiles_x) * TW, Y0 = (tile / tiles_x) * TH, L = min(m.samples_log2, 3);
  if (extended(f)) mesh_area_tile<true>(f, m, L, nd, out, slot, H, W, X0, Y0);
  else mesh_area_tile<false>(f, m, L, nd, out, slot, H, W, X0, Y0);
}

}  // namespace

extern "C" int g6d_sizeof_frame_desc(void) { return (int)sizeof(G6dFrame); }

extern "C" int g6d_frame_ingest(const G6dFrame* frames, int n, uint8_t* out, int B, int H, int W, float* K_out, g6d_stream_t stream) {
  if (!frames || n < 0 || !out || !K_out || B < 1 || H < 1 || W < 1) {
    g6d_set_error("frame_ingest: bad args (null table / out / K_out, n < 0 or a non-positive canvas)"); return G6D_EINVAL;
  }
  if (n == 0) return G6D_OK;
  const long long tiles_ll = (((long long)W + TW - 1) / TW) * (((long long)H + TH - 1) / TH);      // (in 64 bits: the product of two ints)
  if ((long long)W + TW - 1 > 0x7fffffffLL || (long long)H + TH - 1 > 0x7fffffffLL || tiles_ll * n > 0x7fffffffLL) { g6d_set_error("frame_ingest: too many tiles for one launch"); return G6D_EINVAL; }
  const int tiles_x = (W + TW - 1) / TW, tiles = (int)tiles_ll;
  hipLaunchKernelGGL(frame_ingest_kernel, dim3((unsigned)(tiles * n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), frames, out, B, H,
                     W, K_out, tiles_x, tiles);
  return g6d_check_launch("frame_ingest");
}

extern "C" int g6d_sizeof_mesh_desc(void) { return (int)sizeof(G6dMesh); }

extern "C" int g6d_frame_ingest_mesh(const G6dFrame* frames, const G6dMesh* meshes, int n, uint8_t* out, int B, int H, int W, float* K_out,
                                     g6d_stream_t stream) {
  if (!frames || !meshes || n < 0 || !out || !K_out || B < 1 || H < 1 || W < 1) {
    g6d_set_error("frame_ingest_mesh: bad args (null table / meshes / out / K_out, n < 0 or a non-positive canvas)"); return G6D_EINVAL;
  }
  if (n == 0) return G6D_OK;
  const long long tiles_ll = (((long long)W + TW - 1) / TW) * (((long long)H + TH - 1) / TH);      // (in 64 bits: the product of two ints)
  if ((long long)W + TW - 1 > 0x7fffffffLL || (long long)H + TH - 1 > 0x7fffffffLL || tiles_ll * n > 0x7fffffffLL) { g6d_set_error("frame_ingest_mesh: too many tiles for one launch"); return G6D_EINVAL; }
  const int tiles_x = (W + TW - 1) / TW, tiles = (int)tiles_ll;
  hipLaunchKernelGGL(frame_ingest_lens_kernel, dim3((unsigned)(tiles * n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), frames,
                     meshes, out, B, H, W, K_out, tiles_x, tiles);
  return g6d_check_launch("frame_ingest_mesh");
}

extern "C" int g6d_frame_ingest_area(const G6dFrame* frames, const G6dMesh* meshes, int n, uint8_t* out, int B, int H, int W, float* K_out,
                                     g6d_stream_t stream) {
  if (!frames || n < 0 || !out || !K_out || B < 1 || H < 1 || W < 1) {
    g6d_set_error("frame_ingest_area: bad args (null table / out / K_out, n < 0 or a non-positive canvas)"); return G6D_EINVAL;
  }
  if (n == 0) return G6D_OK;
  const long long tiles_ll = (((long long)W + TW - 1) / TW) * (((long long)H + TH - 1) / TH);      // (in 64 bits: the product of two ints)
  if ((long long)W + TW - 1 > 0x7fffffffLL || (long long)H + TH - 1 > 0x7fffffffLL || tiles_ll * n > 0x7fffffffLL) { g6d_set_error("frame_ingest_area: too many tiles for one launch"); return G6D_EINVAL; }
  const int tiles_x = (W + TW - 1) / TW, tiles = (int)tiles_ll;
  hipLaunchKernelGGL(frame_ingest_area_kernel, dim3((unsigned)(tiles * n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), frames,
                     meshes, out, B, H, W, K_out, tiles_x, tiles);
  const int rc = g6d_check_launch("frame_ingest_area");
  if (rc != G6D_OK || !meshes) return rc;
  // the lens frames with samples_log2 > 0 (which frames those are is known on the device only: the mesh table lives there)
  hipLaunchKernelGGL(frame_ingest_lens_area_kernel, dim3((unsigned)(tiles * n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), frames,
                     meshes, out, B, H, W, tiles_x, tiles);
  return g6d_check_launch("frame_ingest_area");
}
