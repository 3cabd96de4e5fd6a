// conv16_common.h — what the direct 16-bit convolution's three kernels share: the launch's parameter block, the epilogue pass through an
// fp32 LDS tile and the statistics flushes (device code), and the host functions through which the launcher (conv16_direct.hip) reaches
// the per-tap kernels (conv16_tap.hip) and the halo-patch kernel (conv16w.hip).
#pragma once
#include "g6d_common.h"
#include "conv16w_geom.h"
#include "pair16.h"
#include <type_traits>

// The parameter block crosses translation units (launcher -> c16w_admit, c16w_launch, c16tap_launch), so its type has external linkage;
// the kernels take C16Params (below), the same bytes under a name private to each unit.
namespace c16 {
struct Seg : c16g::Tiling {        // (the base: the halo-patch kernel's own tiling of the same segment, the h_* fields)
  const char* in; char* full; char* pool;
  int H, W, DH;            // map height / width, rows per image group (D * H)
  int rows;                // N * D * H rows of the tall image
  int ld_in, ld_full, ld_pool;
  int tw_log2, tiles_x, tile0;
  unsigned in_bytes;       // extent of the input buffer as the descriptor sees it (incl. the back-shift)
  int back;                // bytes the descriptor base lies BEFORE the tensor (offset of tap (0,0,0) from the centre, negated)
};
struct Params {
  Seg seg[4];
  int nseg, Cin, Cout, kd, D, relu, full_type, pool_type;   // *_type: 0 none, 1 = 16-bit (the operand type), 2 = fp32
  const char* w; unsigned w_bytes; const float* bias;
  int ptiles, nN;
  double* stats; int stat_rows_per_group;                    // optional: [groups][Cout][2]
  float acc_scale;                                           // y = acc * acc_scale + bias (the filters may carry a power-of-two scale)
  int ablate;                                                // knob c16_ablate (timing experiments)
  G6dRange16 rng;                                            // pair exponents / range record (zero: unscaled, not recorded)
};
// The grids of the two launches (blocks of 256 threads; whole groups of 8 tile blocks per channel block), in one copy for the launch and
// for g6d_conv16_direct_route: the halo-patch kernel on blocks of wm pixel tiles, the per-tap kernels on single tiles
inline int halo_grid(const Params& p, int wm) { return ((p.ptiles + wm - 1) / wm + 7) / 8 * 8 * p.nN; }
inline int tap_grid(const Params& p) { return (p.ptiles + 7) / 8 * 8 * p.nN; }
}  // namespace c16

// The per-tap kernels (conv16_tap.hip): chooses the instantiation for (w_layout, math_mode) and launches it on p.ptiles tiles.
int c16tap_launch(const c16::Params& p, int w_layout, int math_mode, hipStream_t stream);
// The halo-patch kernel (conv16w.hip).  c16w_admit fills the halo tiling (the h_* fields) of every segment of p and applies the
// statistics-group rule; ok: every segment has a tiling the kernel can run, per_pass: some tile holds several statistics groups
// (c16w_stats_per_pass), tiles: the launch's tile count.  folded: a depth-folded 3x3x3 layer (w_layout 2), whose planes are the images of the tiling.
struct C16wAdmit { bool ok, per_pass; int tiles; };
C16wAdmit c16w_admit(c16::Params& p, const G6dConv16Seg* segs, bool pairs, bool folded);
// launches conv16w_kernel for blocks of wm pixel tiles on p.ptiles tiles and p.nN channel blocks
int c16w_launch(const c16::Params& p, int math_mode, int wm, bool half_tile, bool folded, hipStream_t stream);

namespace {

constexpr int C16_BM = 128, C16_BN = 128, C16_BK = 64;
constexpr int C16_EP_LD = 68;                                  // floats per pixel row of the epilogue tile (64 channels + 4: conflict-free b128 reads)

typedef c16::Seg C16Seg;
struct C16Params : c16::Params {};   // (unnamed namespace: the kernels' symbols stay private to their translation unit)

// Epilogue, one PASS = one fp32 LDS tile ep[NPX px][68] of 64 output channels (already holding acc * acc_scale + bias (+ ReLU) of tile
// pixels px0 .. px0 + NPX - 1, the NT threads synchronised): 16-byte stores of the full map and / or the 2x2 max-pooled map, optional
// per-(group, channel) statistics.  NPX is a multiple of two tile rows (pool windows stay inside a pass).
// Output element types (full_type / pool_type): 1 = the 16-bit type T, 2 = fp32, 3 = fp16 hi / lo PAIR [pixel][2][Cout] (hi = rn16(v),
// lo = rn16(v - hi): the input format of the MM = 3 kernels; ld counts 16-bit elements and holds both planes).
// NT = threads that share the pass (256: the whole block, NPX = 128; 64: one wave, tid = lane, no block-wide synchronisation inside).
// FT / PT / ST >= 0: full_type / pool_type / (statistics on) known at compile time — the halo-patch kernel picks the variant of its
// launch with one block-uniform branch; -1: read from p.
// Addresses: one block-uniform 64-bit base per output (the tile's first pixel) + a 32-bit lane part (the launcher bounds a tile's extent
// in an output to 2^32 bytes); a pixel (py, px) of the tile is stored iff py < yl and px < xl, two block-uniform limits.
// wst (NT = 64): the lane's fp64 sums of the wave's passes, see c16_stats_flush.
template <int MM, int NT, int NPX, int CH = 64, int FT = -1, int PT = -1, int ST = -1>
__device__ __forceinline__ void c16_epilogue_pass(const C16Params& p, const C16Seg& sg, const float* ep, double* red, int tid, int cbase, int g0, int x0,
                                                  int tw_log2, int ylim, int px0, unsigned& amax, double (&wst)[2]) {
  typedef typename C16T<MM>::T T;
  typedef typename C16T<MM>::V V8;
  static_assert(NT == 64 || (NPX == 128 && CH == 64), "the block-wide form handles whole tiles of 64 channels");
  constexpr int C8 = CH / 8, C4 = CH / 4;                                           // 16-byte items per pixel: 16-bit / fp32 output
  const int full_type = FT >= 0 ? FT : p.full_type, pool_type = PT >= 0 ? PT : p.pool_type;
  const bool stats_on = ST >= 0 ? ST != 0 : p.stats != nullptr;
  const int TW = 1 << tw_log2, W = sg.W;
  const int py0 = px0 >> tw_log2;                                                   // first tile row of the pass
  const int yl = min(ylim, sg.rows - g0), xl = W - x0;
  auto inside = [&](int lp, unsigned& pix) {                                        // lp: pixel of the pass = row of ep; pix: its index from the tile's first pixel
    const int px = px0 + lp, py = px >> tw_log2, xx = px & (TW - 1);
    pix = (unsigned)(py * W + xx);
    return py < yl && xx < xl;
  };
  // pair outputs hold split16(v * 2^-eo); amax: max bits(|v|) of the stored unscaled values, recorded by the caller once per wave
  // after its last pass (G6dRange16).  The two pair branches below restate c16_pair_split (pair16.h, the definition) in their own order.
  const bool pairs = full_type == 3 || pool_type == 3;
  const int eo = pairs ? g6d_exp_out(p.rng) : 0;
  if (full_type == 1) {
    char* fb = sg.full + (((long)g0 * W + x0) * sg.ld_full + cbase) * 2;
#pragma unroll
    for (int j = 0; j < NPX * C8 / NT; ++j) {
      const int lp = tid / C8 + (NT / C8) * j, ch = (tid % C8) * 8;
      unsigned pix;
      if (inside(lp, pix)) {
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(ep + lp * C16_EP_LD + ch), v1 = *reinterpret_cast<const f32x4*>(ep + lp * C16_EP_LD + ch + 4);
        V8 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) { o[e] = (T)v0[e]; o[4 + e] = (T)v1[e]; }
        *reinterpret_cast<V8*>(fb + (pix * (unsigned)sg.ld_full + ch) * 2u) = o;
      }
    }
  } else if (full_type == 3) {
    char* fb = sg.full + (((long)g0 * W + x0) * sg.ld_full + cbase) * 2;
#pragma unroll
    for (int j = 0; j < NPX * C8 / NT; ++j) {
      const int lp = tid / C8 + (NT / C8) * j, ch = (tid % C8) * 8;
      unsigned pix;
      if (inside(lp, pix)) {
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(ep + lp * C16_EP_LD + ch), v1 = *reinterpret_cast<const f32x4*>(ep + lp * C16_EP_LD + ch + 4);
        V8 hi, lo;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          amax = max(amax, max(g6d_abs_bits(v0[e]), g6d_abs_bits(v1[e])));
          const float u0 = ldexpf(v0[e], -eo), u1 = ldexpf(v1[e], -eo);
          hi[e] = (T)u0; lo[e] = (T)(u0 - (float)hi[e]);
          hi[4 + e] = (T)u1; lo[4 + e] = (T)(u1 - (float)hi[4 + e]);
        }
        char* o = fb + (pix * (unsigned)sg.ld_full + ch) * 2u;
        *reinterpret_cast<V8*>(o) = hi;
        *reinterpret_cast<V8*>(o + p.Cout * 2) = lo;
      }
    }
  } else if (full_type == 2) {
    char* fb = sg.full + (((long)g0 * W + x0) * sg.ld_full + cbase) * 4;
#pragma unroll
    for (int j = 0; j < NPX * C4 / NT; ++j) {
      const int lp = tid / C4 + (NT / C4) * j, ch = (tid % C4) * 4;
      unsigned pix;
      if (inside(lp, pix))
        *reinterpret_cast<f32x4*>(fb + (pix * (unsigned)sg.ld_full + ch) * 4u) = *reinterpret_cast<const f32x4*>(ep + lp * C16_EP_LD + ch);
    }
  }
  if (pool_type) {
    // pooled maps have even H and W and tiles start on even rows and columns: pooled pixel (g0 / 2 + qy, x0 / 2 + qx) is stored iff the
    // window's first pixel is
    const int W2 = W >> 1;
    const long pb = ((long)(g0 >> 1) * W2 + (x0 >> 1)) * sg.ld_pool + cbase;
    auto pooled = [&](auto per_c) {
      constexpr int per = decltype(per_c)::value, chunks = CH / per;               // channels per item, items per pooled pixel (powers of two)
      static_assert((NPX / 4) * chunks % NT == 0, "whole rounds of items");
#pragma unroll
      for (int j = 0; j < (NPX / 4) * chunks / NT; ++j) {
        const int it = tid + NT * j, pp = it / chunks, ch = (it % chunks) * per;
        const int pry = pp >> (tw_log2 - 1), prx = pp & ((TW >> 1) - 1);
        const int r00 = ((2 * pry) << tw_log2) + 2 * prx;
        if (py0 + 2 * pry < yl && 2 * prx < xl) {
          float m[8];
#pragma unroll
          for (int e = 0; e < 8; e += 4) {
            if (e < per) {
              const f32x4 q0 = *reinterpret_cast<const f32x4*>(ep + r00 * C16_EP_LD + ch + e), q1 = *reinterpret_cast<const f32x4*>(ep + (r00 + 1) * C16_EP_LD + ch + e);
              const f32x4 q2 = *reinterpret_cast<const f32x4*>(ep + (r00 + TW) * C16_EP_LD + ch + e), q3 = *reinterpret_cast<const f32x4*>(ep + (r00 + TW + 1) * C16_EP_LD + ch + e);
#pragma unroll
              for (int u = 0; u < 4; ++u) m[e + u] = fmaxf(fmaxf(q0[u], q1[u]), fmaxf(q2[u], q3[u]));
            }
          }
          const unsigned o = (unsigned)(((py0 >> 1) + pry) * W2 + prx) * (unsigned)sg.ld_pool + ch;
          if constexpr (per == 4) {
            f32x4 ov = {m[0], m[1], m[2], m[3]};
            *reinterpret_cast<f32x4*>(sg.pool + pb * 4 + o * 4u) = ov;
          } else if (pool_type == 1) {
            V8 ov;
#pragma unroll
            for (int e = 0; e < 8; ++e) ov[e] = (T)m[e];
            *reinterpret_cast<V8*>(sg.pool + pb * 2 + o * 2u) = ov;
          } else {
            V8 hi, lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              amax = max(amax, g6d_abs_bits(m[e]));
              const float u = ldexpf(m[e], -eo);
              hi[e] = (T)u; lo[e] = (T)(u - (float)hi[e]);
            }
            char* d = sg.pool + pb * 2 + o * 2u;
            *reinterpret_cast<V8*>(d) = hi;
            *reinterpret_cast<V8*>(d + p.Cout * 2) = lo;
          }
        }
      }
    };
    if (pool_type == 2) pooled(std::integral_constant<int, 4>{});
    else pooled(std::integral_constant<int, 8>{});
  }
  if (stats_on) {
    // per-(group, channel) sum / sum of squares of the fp32 results of the tile's VALID pixels (a tile never straddles groups):
    // fp32 partial sums of 32 pixels each, in pixel order, combined in fp64
    auto sum32 = [&](int lp0, int c, float& s1, float& s2) {
      s1 = 0.f; s2 = 0.f;
      // (block-uniform) every pixel of the pass is valid: no test per pixel
      if (py0 + (NPX >> tw_log2) <= yl && TW <= xl) {
#pragma unroll 8
        for (int lp = lp0; lp < lp0 + 32; ++lp) { const float v = ep[lp * C16_EP_LD + c]; s1 += v; s2 += v * v; }
      } else {
        for (int lp = lp0; lp < lp0 + 32; ++lp) {
          unsigned pix;
          if (inside(lp, pix)) { const float v = ep[lp * C16_EP_LD + c]; s1 += v; s2 += v * v; }
        }
      }
    };
    if constexpr (NT == 256) {
      const int grp = p.stat_rows_per_group > 0 ? (int)(((long)g0 * W) / p.stat_rows_per_group) : 0;
      const int c = tid & 63, q = tid >> 6;
      float s1, s2;
      sum32(32 * q, c, s1, s2);
      red[(q * 64 + c) * 2] = (double)s1; red[(q * 64 + c) * 2 + 1] = (double)s2;
      __syncthreads();
      if (tid < 128) {
        const int cc = tid >> 1, w = tid & 1;
        const double v = red[(0 * 64 + cc) * 2 + w] + red[(1 * 64 + cc) * 2 + w] + red[(2 * 64 + cc) * 2 + w] + red[(3 * 64 + cc) * 2 + w];
        atomicAdd(p.stats + ((long)grp * p.Cout + cbase + cc) * 2 + w, v);
      }
    } else {
      // one wave: lane = channel lane % CH of pixel group lane / CH (CH = 32: the two halves of the pass, every lane at work)
      constexpr int PPG = NPX * CH / 64;                                            // pixels per group
#pragma unroll
      for (int q = 0; q < PPG / 32; ++q) {
        float s1, s2;
        sum32(PPG * (tid / CH) + 32 * q, tid % CH, s1, s2);
        wst[0] += (double)s1; wst[1] += (double)s2;
      }
    }
  }
}

// The wave-private statistics after a wave's last pass: the pixel groups of a channel are added across lanes, then ONE pair of fp64
// atomics per (wave, channel).  (Every lane takes part: no early return before it.)
template <int CH>
__device__ __forceinline__ void c16_stats_flush(const C16Params& p, const C16Seg& sg, int lane, int cbase, int g0, double (&wst)[2]) {
  static_assert(CH == 32 || CH == 64, "one or two pixel groups per channel");
  if constexpr (CH == 32) { wst[0] += __shfl_xor(wst[0], 32); wst[1] += __shfl_xor(wst[1], 32); }
  const unsigned grp = p.stat_rows_per_group > 0 ? (unsigned)(g0 * sg.W) / (unsigned)p.stat_rows_per_group : 0u;   // (pixels of a segment < 2^31)
  if (lane < CH) {
    double* d = p.stats + ((long)grp * p.Cout + cbase + lane) * 2;
    atomicAdd(d, wst[0]);
    atomicAdd(d + 1, wst[1]);
  }
}

// A banded tile (several small images per tile, conv16w_kernel) may span several statistics groups; the launcher then admits only
// groups of whole epilogue passes, and the wave-private sums are flushed after EVERY pass under the pass's own group (g = the pass's
// first row of the tall image; a pass past the last image holds no valid pixel and flushes nothing) and start again from zero.
template <int CH>
__device__ __forceinline__ void c16_stats_flush_pass(const C16Params& p, const C16Seg& sg, int lane, int cbase, int g, double (&wst)[2]) {
  if (g < sg.rows) c16_stats_flush<CH>(p, sg, lane, cbase, g, wst);      // (block-uniform: every lane takes part)
  wst[0] = 0.0; wst[1] = 0.0;
}
// (block-uniform) the tile of TH rows x W columns holds more than one statistics group (c16w_admit's per_pass, conv16w.hip, mirrors it)
__device__ __forceinline__ bool c16w_stats_per_pass(const C16Params& p, const C16Seg& sg, int tw_log2) {
  return p.stats != nullptr && p.stat_rows_per_group > 0 && p.stat_rows_per_group < (C16_BM >> tw_log2) * sg.W;
}

}  // namespace
