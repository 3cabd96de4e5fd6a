// conv16_direct.hip — direct (implicit-GEMM) 3x3 / 3x3x3 convolution on 16-bit ACTIVATIONS: the reduced-precision mode's own kernel
// family (round 6; BASELINE configs[2] "bf16" / configs[4] "fp16 MFMA convs").
//
// Replaces, in the reduced-precision mode only, the VGG trunks' 3x3 layers (reference network/pretrain_models.py:9-31,66-72; detector
// pyramid detector.py:188-197,236-241; refiner crops refiner.py:64-78) and the first convs of the refiner's 32^3 volume net
// (refiner.py:88-143).  Until round 5 that mode kept fp32 activations in HBM and LDS and rounded operands when fragments left LDS:
// its 16-bit Winograd kernels were bound by LDS WRITES of fp32 data.  Here activations are fp16 / bf16 NHWC in HBM:
//   * both operand tiles of a K step go global -> LDS by DMA (buffer_load_dwordx4 ... lds: no VGPR round trip, no ds_write, no
//     conversion), 16 bytes = 8 channels per lane; zero padding and ragged tile edges are the buffer's out-of-range zero fill;
//   * K step = 64 input channels of ONE tap (128 B per pixel row and per filter row): the LDS image [row][8 slots of 16 B] is lane-linear
//     as the DMA demands, and bank-conflict free for the ds_read_b128 fragment reads because the lane that FILLS slot s of row r fetches
//     channel group s ^ ((r >> 1) & 7) — the swizzle sits on the source address (cdna_hip_programming.md rule 21);
//   * v_mfma_f32_32x32x16_{f16,bf16}, fp32 accumulation; block = 128 output pixels x 128 output channels, 4 waves of 64 x 64 (2 x 2
//     accumulator tiles), two LDS stages of 32 KB, two blocks per CU (the second block's MFMAs cover this block's barrier / DMA waits);
//   * a tile is TH x TW pixels (TH TW = 128, TW a power of two chosen per map width) of the "tall image" [N D H rows][W columns], so 2x2
//     max-pool windows never straddle tiles and small maps pack several images into one tile;
//   * epilogue through LDS: bias, ReLU, then 16-byte stores of the full map (16-bit or fp32) and / or the 2x2 max-pooled map, and
//     optionally per-(image group, channel) sum / sum of squares in fp64 for the InstanceNorm that follows (volume net).
// K order: input-channel slice outermost, taps innermost — the nine shifted reads of a 16 KB slice hit L1 / L2.
#include "g6d_common.h"
#include "conv16w_geom.h"
#include "pair16.h"
#include <type_traits>

namespace {

constexpr int C16_BM = 128, C16_BN = 128, C16_BK = 64;
constexpr int C16_STAGE = (C16_BM + C16_BN) * C16_BK * 2;      // 32 KB
constexpr int C16_LDS = 2 * C16_STAGE;                         // 64 KB
constexpr int C16_EP_LD = 68;                                  // floats per pixel row of the epilogue tile (64 channels + 4: conflict-free b128 reads)

struct C16Seg : c16g::Tiling {     // (the base: the halo-patch kernel's own tiling of the same segment, the h_* fields)
  const char* in; char* full; char* pool;
  int H, W, DH;            // map height / width, rows per image group (D * H)
  int rows;                // N * D * H rows of the tall image
  int ld_in, ld_full, ld_pool;
  int tw_log2, tiles_x, tile0;
  unsigned in_bytes;       // extent of the input buffer as the descriptor sees it (incl. the back-shift)
  int back;                // bytes the descriptor base lies BEFORE the tensor (offset of tap (0,0,0) from the centre, negated)
};
struct C16Params {
  C16Seg seg[4];
  int nseg, Cin, Cout, kd, D, relu, full_type, pool_type;   // *_type: 0 none, 1 = 16-bit (the operand type), 2 = fp32
  const char* w; unsigned w_bytes; const float* bias;
  int ptiles, nN;
  double* stats; int stat_rows_per_group;                    // optional: [groups][Cout][2]
  float acc_scale;                                           // y = acc * acc_scale + bias (the filters may carry a power-of-two scale)
  int ablate;                                                // knob c16_ablate (timing experiments)
  G6dRange16 rng;                                            // pair exponents / range record (zero: unscaled, not recorded)
};

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
// (block-uniform) the tile of TH rows x W columns holds more than one statistics group
__device__ __forceinline__ bool c16w_stats_per_pass(const C16Params& p, const C16Seg& sg, int tw_log2) {
  return p.stats != nullptr && p.stat_rows_per_group > 0 && p.stat_rows_per_group < (C16_BM >> tw_log2) * sg.W;
}

// Epilogue of the per-tap kernels: two passes of 64 channels through ONE fp32 LDS tile.
template <int MM, typename WriteTile>
__device__ __forceinline__ void c16_epilogue(const C16Params& p, const C16Seg& sg, char* lds, int tid, int nt, int g0, int x0, int tw_log2, int ylim,
                                             WriteTile write_tile) {
  // write_tile(h, ep, cbase): the waves that own channels [cbase, cbase + 64) of the block store acc * acc_scale + bias (+ ReLU) of the
  // tile's 128 pixels into ep[pixel * C16_EP_LD + channel - cbase];  ylim: tile rows below it lie inside the image
  float* ep = reinterpret_cast<float*>(lds);
  double* red = reinterpret_cast<double*>(lds + C16_BM * C16_EP_LD * 4);       // [4 quarters][64 ch][2] statistics partials
  unsigned amax = 0;
  double wst[2] = {0.0, 0.0};                                                   // (the wave-private form's)
#pragma unroll 1
  for (int h = 0; h < 2; ++h) {
    const int cbase = nt * C16_BN + 64 * h;
    write_tile(h, ep, cbase);
    __syncthreads();
    c16_epilogue_pass<MM, 256, 128>(p, sg, ep, red, tid, cbase, g0, x0, tw_log2, ylim, 0, amax, wst);
    __syncthreads();
  }
  if (p.full_type == 3 || p.pool_type == 3) g6d_range_record(p.rng, amax);
}

// The 2 x 2 wave layout of conv16_kernel / conv16r_kernel: wave (wm, wn) holds pixels 64 wm .. + 63 x channels 64 wn .. + 63.
__device__ __forceinline__ void c16_write22(const C16Params& p, const f32x16 (&acc)[2][2], int lane, int wv, int h, float* ep, int cbase) {
  const int wm = wv >> 1, wn = wv & 1;
  if (wn != h) return;
  const float as = ldexpf(p.acc_scale, g6d_exp_in(p.rng));     // pair input held as x * 2^-e_in
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt2 = 0; nt2 < 2; ++nt2) {
      const float bv = p.bias ? p.bias[cbase + 32 * nt2 + (lane & 31)] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int px = 64 * wm + 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        float v = fmaf(acc[mt][nt2][r], as, bv);
        if (p.relu) v = fmaxf(v, 0.f);
        ep[px * C16_EP_LD + 32 * nt2 + (lane & 31)] = v;
      }
    }
}

template <int MM>
__global__ __launch_bounds__(256, 2) void conv16_kernel(const C16Params p) {
  typedef typename C16T<MM>::V V8;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // block id -> (pixel tile, channel tile): the nN channel tiles of a pixel tile run back to back on ONE XCD (ids = xcd mod 8)
  const int xcd = blockIdx.x & 7, jj = blockIdx.x >> 3;
  const int nt = jj % p.nN, ptile = (jj / p.nN) * 8 + xcd;
  if (ptile >= p.ptiles) return;
  int si = 0;
#pragma unroll
  for (int i = 1; i < 4; ++i) if (i < p.nseg && ptile >= p.seg[i].tile0) si = i;
  const C16Seg& sg = p.seg[si];
  const int t = ptile - sg.tile0;
  const int tw_log2 = sg.tw_log2, TW = 1 << tw_log2;
  const int tx = t % sg.tiles_x, ty = t / sg.tiles_x;
  const int g0 = ty * (C16_BM >> tw_log2), x0 = tx * TW;
  const int H = sg.H, W = sg.W, D = p.D;
  const int ntaps = 9 * p.kd;

  // ---- geometry of the four A rows this lane fills per K step: byte offset of the (shifted-back) centre pixel + tap validity mask
  unsigned a_off[4], a_mask[4], b_off[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = 32 * wv + 8 * i + (lane >> 3);
    const int slot = (lane & 7) ^ ((r >> 1) & 7);
    const int g = g0 + (r >> tw_log2), x = x0 + (r & (TW - 1));
    unsigned m = 0;
    if (g < sg.rows && x < W) {
      const int y = g % H, z = (g / H) % D;
      unsigned my = (y > 0 ? 1u : 0u) | 2u | (y < H - 1 ? 4u : 0u);            // ky = 0,1,2 valid
      unsigned mx = (x > 0 ? 1u : 0u) | 2u | (x < W - 1 ? 4u : 0u);
      unsigned m9 = 0;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) if (my >> ky & 1) m9 |= mx << (3 * ky);
      if (p.kd == 3) {
        if (z > 0) m |= m9;
        m |= m9 << 9;
        if (z < D - 1) m |= m9 << 18;
      } else m = m9;
    }
    a_mask[i] = m;
    a_off[i] = (unsigned)(((long)g * W + x) * sg.ld_in * 2) + slot * 16;
    b_off[i] = (unsigned)((long)(nt * C16_BN + r) * ntaps * p.Cin * 2) + slot * 16;
  }
  const __amdgpu_buffer_rsrc_t rs_in = c16_rsrc(sg.in - sg.back, sg.in_bytes);
  const __amdgpu_buffer_rsrc_t rs_w = c16_rsrc(p.w, p.w_bytes);
  typedef __attribute__((address_space(3))) void* lds_ptr;

  const int nchunk = p.Cin / C16_BK, nk = nchunk * ntaps;
  // K-step state (scalar): tap = (kz, ky, kx), channel chunk
  auto issue = [&](int k, int stage) {
    const int c = k / ntaps, tap = k - c * ntaps;
    const int kz = tap / 9, r9 = tap - 9 * kz, ky = r9 / 3, kx = r9 - 3 * ky;
    const unsigned a_k = (unsigned)(((kz * H + ky) * W + kx) * sg.ld_in * 2 + c * (C16_BK * 2));
    const unsigned b_k = (unsigned)((tap * p.Cin + c * C16_BK) * 2);
    char* sa = lds + stage * C16_STAGE + (32 * wv) * 128;
    char* sb = sa + C16_BM * 128;
    if (!((p.ablate & 1) && k > 1)) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned vo = (a_mask[i] >> tap & 1u) ? a_off[i] + a_k : C16_OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_in, (lds_ptr)(sa + i * 1024), 16, vo, 0, 0, 0);
      }
    }
    if (!((p.ablate & 2) && k > 1)) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_ptr)(sb + i * 1024), 16, b_off[i] + b_k, 0, 0, 0);
    }
  };

  const int wm = wv >> 1, wn = wv & 1;
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  // fragment read offsets: row = tile row (lane & 31), logical slot 2 ks + (lane >> 5) -> physical slot ^ ((row >> 1) & 7)
  const int frow = lane & 31, fhalf = lane >> 5, fsw = (frow >> 1) & 7;
  const int a_rd = (64 * wm + frow) * 128, b_rd = C16_BM * 128 + (64 * wn + frow) * 128;

  issue(0, 0);
  for (int k = 0; k < nk; ++k) {
    const int stage = k & 1;
    if (k + 1 < nk) {
      issue(k + 1, stage ^ 1);
      if (p.ablate) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    const char* st = lds + stage * C16_STAGE;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int sl = ((2 * ks + fhalf) ^ fsw) * 16;
      V8 a0 = *reinterpret_cast<const V8*>(st + a_rd + sl);
      V8 a1 = *reinterpret_cast<const V8*>(st + a_rd + 32 * 128 + sl);
      V8 b0 = *reinterpret_cast<const V8*>(st + b_rd + sl);
      V8 b1 = *reinterpret_cast<const V8*>(st + b_rd + 32 * 128 + sl);
      if constexpr (MM == 1) {
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
      } else {
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                       // every wave has read this stage: the next iteration may refill it
  }

  c16_epilogue<MM>(p, sg, lds, tid, nt, g0, x0, tw_log2, C16_BM >> tw_log2,
                   [&](int h, float* ep, int cbase) { c16_write22(p, acc, lane, wv, h, ep, cbase); });
}


// ---------------------------------------------------------------------------------------------------------------------------------
// conv16r_kernel: the same tile with the FILTER operand kept out of LDS.  Measured on the kernel above: a wave spends as long issuing
// its 8 LDS-DMA pieces per K step (~100 cycles each beside MFMAs) as in its 16 MFMAs.  The filters are therefore packed on the host in
// FRAGMENT order — [channel tile][K step][ks][plane][32-channel group j][lane][8 values]: one coalesced 1 KB run per wave instruction,
// L2-resident — and go straight into registers one K step ahead (plain global loads: ~6 cycles of issue); only the activation tile
// takes the DMA path (4 pieces per wave and step), LDS holds 16 KB per stage, and the fragment loop reads LDS for A only.
//   MM = 1 / 2  bf16 / fp16 operands, K step = 64 channels of one tap
//   MM = 3      fp32-class arithmetic on the fp16 matrix cores: every operand is a PAIR of fp16 values (hi = rn16(x), lo = rn16(x - hi);
//               gfx950's MFMA keeps fp16 subnormals, tools/ubench/mfma_f16_denorm.hip), activations [pixel][2][C] (hi plane, lo plane),
//               acc += a_hi b_hi + a_hi b_lo + a_lo b_hi (the dropped lo x lo term is 2^-22 relative): 3 MFMAs of 32 cycles per 16 channels
//               against 8 x 64 cycles on the fp32 matrix cores.  K step = 32 channels (two planes of 64-byte rows: the same 16 KB stage).
template <int MM> struct C16R {
  static constexpr int BK = MM == 3 ? 32 : 64, NP = MM == 3 ? 2 : 1, KS = BK / 16, ROWB = BK * 2, SL = ROWB / 16;
  static constexpr int STAGE = NP * C16_BM * ROWB;            // 16 KB
  static constexpr int RPI = 1024 / ROWB;                     // rows one DMA wave-instruction fills (8 / 16)
};

template <int MM, int NSTAGE>
__global__ __launch_bounds__(256, 2) void conv16r_kernel(const C16Params p) {
  typedef typename C16T3<MM>::V V8;
  typedef C16R<MM> R;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int xcd = blockIdx.x & 7, jj = blockIdx.x >> 3;
  const int nt = jj % p.nN, ptile = (jj / p.nN) * 8 + xcd;
  if (ptile >= p.ptiles) return;
  int si = 0;
#pragma unroll
  for (int i = 1; i < 4; ++i) if (i < p.nseg && ptile >= p.seg[i].tile0) si = i;
  const C16Seg& sg = p.seg[si];
  const int t = ptile - sg.tile0;
  const int tw_log2 = sg.tw_log2, TW = 1 << tw_log2;
  const int tx = t % sg.tiles_x, ty = t / sg.tiles_x;
  const int g0 = ty * (C16_BM >> tw_log2), x0 = tx * TW;
  const int H = sg.H, W = sg.W, D = p.D;
  const int ntaps = 9 * p.kd;

  // ---- A rows this lane fills: instruction i of wave wv covers plane i / (4 / NP), rows 32 wv + RPI (i % (4 / NP)) + lane / SL
  constexpr int NR = 4 / R::NP;                                // distinct rows per lane (4 / 2)
  unsigned a_off[NR], a_mask[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int r = 32 * wv + R::RPI * i + lane / R::SL;
    const int sw = R::SL == 8 ? (r >> 1) & 7 : (r >> 2) & 3;
    const int slot = (lane & (R::SL - 1)) ^ sw;
    const int g = g0 + (r >> tw_log2), x = x0 + (r & (TW - 1));
    unsigned m = 0;
    if (g < sg.rows && x < W) {
      const int y = g % H, z = (g / H) % D;
      unsigned my = (y > 0 ? 1u : 0u) | 2u | (y < H - 1 ? 4u : 0u);
      unsigned mx = (x > 0 ? 1u : 0u) | 2u | (x < W - 1 ? 4u : 0u);
      unsigned m9 = 0;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) if (my >> ky & 1) m9 |= mx << (3 * ky);
      if (p.kd == 3) {
        if (z > 0) m |= m9;
        m |= m9 << 9;
        if (z < D - 1) m |= m9 << 18;
      } else m = m9;
    }
    a_mask[i] = m;
    a_off[i] = (unsigned)(((long)g * W + x) * sg.ld_in * 2) + slot * 16;
  }
  const __amdgpu_buffer_rsrc_t rs_in = c16_rsrc(sg.in - sg.back, sg.in_bytes);
  typedef __attribute__((address_space(3))) void* lds_ptr;
  const int nchunk = p.Cin / R::BK, nk = nchunk * ntaps;
  const int plane_bytes = p.Cin * 2;                            // MM = 3: the lo plane of a pixel follows its hi plane

  auto issue_a = [&](int k, int stage) {
    const int c = k / ntaps, tap = k - c * ntaps;
    const int kz = tap / 9, r9 = tap - 9 * kz, ky = r9 / 3, kx = r9 - 3 * ky;
    const unsigned a_k = (unsigned)(((kz * H + ky) * W + kx) * sg.ld_in * 2 + c * (R::BK * 2));
    char* sa = lds + stage * R::STAGE;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ri = i % NR, pl = i / NR;
      const unsigned vo = (a_mask[ri] >> tap & 1u) ? a_off[ri] + a_k + pl * plane_bytes : C16_OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_in, (lds_ptr)(sa + pl * (C16_BM * R::ROWB) + (32 * wv + R::RPI * ri) * R::ROWB), 16, vo, 0, 0, 0);
    }
  };
  // ---- B fragments of K step k: [ks][plane][t] 16 bytes per lane, one coalesced 1 KB run per wave instruction.  Hand-issued loads:
  // beside LDS-DMA requests hipcc waits vmcnt(0) for any load it tracks (the whole pipeline drained every other step, ISA checked), so
  // these are invisible to its wait-count pass and retired by the counted s_waitcnt at the end of the step that requested them.
  const int wm = wv >> 1, wn = wv & 1;
  constexpr int NB = R::KS * R::NP * 2;                        // 8
  constexpr int STEP_B = R::KS * R::NP * 4 * 1024;             // bytes of one K step of one channel tile
  const char* wtile = p.w + (long)nt * nk * STEP_B;             // (uniform)
  const unsigned b_voff = (2 * wn) * 1024 + lane * 16;
  auto load_b = [&](int k, V8 (&b)[NB]) {
    const char* ws = wtile + (long)k * STEP_B;
#pragma unroll
    for (int q = 0; q < R::KS * R::NP; ++q) {
      const char* wq = ws + q * 4096;
      asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(b[2 * q]) : "v"(b_voff), "s"(wq) : "memory");
      asm volatile("global_load_dwordx4 %0, %1, %2 offset:1024" : "=v"(b[2 * q + 1]) : "v"(b_voff), "s"(wq) : "memory");
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  const int frow = lane & 31, fhalf = lane >> 5;
  const int fsw = R::SL == 8 ? (frow >> 1) & 7 : (frow >> 2) & 3;
  const int a_rd = (64 * wm + frow) * R::ROWB;

  auto compute = [&](int stage, const V8 (&b)[NB]) {
    const char* st = lds + stage * R::STAGE;
#pragma unroll
    for (int ks = 0; ks < R::KS; ++ks) {
      const int sl = ((2 * ks + fhalf) ^ fsw) * 16;
      V8 a[R::NP][2];
#pragma unroll
      for (int pl = 0; pl < R::NP; ++pl) {
        a[pl][0] = *reinterpret_cast<const V8*>(st + pl * (C16_BM * R::ROWB) + a_rd + sl);
        a[pl][1] = *reinterpret_cast<const V8*>(st + pl * (C16_BM * R::ROWB) + a_rd + 32 * R::ROWB + sl);
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int n2 = 0; n2 < 2; ++n2) {
          acc[mt][n2] = c16_mfma<MM>(a[0][mt], b[(ks * R::NP) * 2 + n2], acc[mt][n2]);
          if constexpr (MM == 3) {
            acc[mt][n2] = c16_mfma<MM>(a[0][mt], b[(ks * R::NP + 1) * 2 + n2], acc[mt][n2]);      // hi x lo
            acc[mt][n2] = c16_mfma<MM>(a[1][mt], b[(ks * R::NP) * 2 + n2], acc[mt][n2]);          // lo x hi
          }
        }
    }
  };

  // ---- K loop, three LDS stages, ONE barrier per step.  Step k: request B(k+1) and the DMA of step k+2 (into the stage step k-1 read:
  // every wave passed the barrier that ended it), compute step k, then retire B(k+1) and DMA(k+1) with a counted wait that leaves only
  // this step's four DMA pieces in flight (requests return in order), and meet at the barrier — which both frees stage k % 3 and
  // publishes everybody's DMA(k+1).
  static_assert(NSTAGE == 3, "the stage arithmetic below assumes three stages");
  V8 b0[NB], b1[NB];
  load_b(0, b0);
  issue_a(0, 0);
  if (nk > 1) { issue_a(1, 1); asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); }
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  int stage = 0;
  auto step = [&](int k, const V8 (&bc)[NB], V8 (&bn)[NB]) {
    if (k + 1 < nk && !((p.ablate & 2) && k > 1)) load_b(k + 1, bn);
    const int s2 = stage >= 1 ? stage - 1 : 2;               // (stage + 2) % 3
    if (k + 2 < nk && !((p.ablate & 1) && k > 1)) issue_a(k + 2, s2);
    compute(stage, bc);
    if (k + 2 < nk && !p.ablate) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    stage = stage == 2 ? 0 : stage + 1;
  };
#pragma unroll 1
  for (int k = 0; k < nk; k += 2) {
    step(k, b0, b1);
    if (k + 1 < nk) step(k + 1, b1, b0);
  }
  c16_epilogue<MM == 3 ? 2 : MM>(p, sg, lds, tid, nt, g0, x0, tw_log2, C16_BM >> tw_log2,
                                 [&](int h, float* ep, int cbase) { c16_write22(p, acc, lane, wv, h, ep, cbase); });
}


// ---------------------------------------------------------------------------------------------------------------------------------
// conv16w_kernel: the HALO-PATCH kernel (2-D layers).  Measured on the two kernels above (tools/conv16_ablate.py): without the
// activation requests they run 15 % faster, without the filter requests 14 %, without both 38 % — a step's 32-48 KB of vector-memory
// traffic and two barriers per 16 MFMAs hold them at a third of the MFMA rate.  Here
//   * the activations of a 32-channel slice are staged ONCE per slice as the tile's halo patch — (TH + 2) x (TW + 2) pixels (tiles of
//     several small images: one band of H + 2 rows per image, so that zero padding between images stays zero) — and all nine taps read
//     shifted windows of it: ~1.4 KB of activation traffic per tap instead of 8, ONE barrier per slice (between barriers the waves run
//     free: the patch is read-only and the filters are private);
//   * a wave owns 128 pixels x 64 output channels (4 x 2 accumulator tiles): an activation fragment read from LDS feeds two MFMAs and
//     a filter fragment four — 64 B/clk/CU of ds_read_b128 and 32 B/clk/CU of filter loads at the full MFMA rate (LDS delivers 256,
//     L2 ~56).  A block is four waves: WM pixel tiles x (4 / WM) channel groups — 128 px x 256 ch, or 2 tiles x 128 ch for Cout = 128;
//   * filters: fragment-major, straight into registers TWO taps ahead (ring of three sets, hand-issued loads and counted waits);
//   * a patch row holds 64 B (4 slots of 16 B), lane-linear for the DMA, the slot swizzled by (patch row, column) so that the shifted
//     ds_read_b128 fragment reads of every tap are bank-conflict free (tools/ubench/conv16_swizzle.py); a fragment address is
//     row base | swizzled slot, and the second 16-channel half of the slice is that address ^ 32: one VALU per read;
//   * the nine taps are unrolled (tap offsets are immediates); the epilogue is PRIVATE to a wave (its own fp32 LDS tile, no block
//     barrier): blocks and waves drift apart freely, one block's epilogue runs beside its neighbours' MFMAs.
//   MM = 1 / 2: bf16 / fp16, a wave owns 128 px x 64 ch.  MM = 3: fp16 hi / lo pairs (see conv16r_kernel), two planes per patch, three
//   MFMAs per product; a wave owns 128 px x 32 ch (64 accumulator registers: with the two-plane fragment and filter sets a 64-channel
//   wave needs > 256 registers = one block per CU, every prologue and epilogue exposed).  Two blocks per CU in every mode.  The pair
//   path runs on v_mfma_f32_16x16x32_f16 (8 x 2 accumulators of 16 x 16): at two waves per SIMD the chip holds a higher clock on that
//   shape than on 32x32x16 at equal cycles per FLOP (tools/ubench/mfma16_peak.hip) — its own fragment scheme and slot swizzle below.
// timing experiments only (WRONG results), a compile-time switch (make FLAGS_conv16_direct=-DC16W_ABLATE=n): after the first slice, bit 0 = no
// patch requests, bit 1 = no filter requests, bit 2 = no fragment reads
#ifndef C16W_ABLATE
#define C16W_ABLATE 0
#endif
template <int MM> struct C16W {
  static constexpr int NP = MM == 3 ? 2 : 1, KS = 2, NI_MAX = 18;             // planes, 16-channel groups per slice, DMA pieces per plane at most
  static constexpr int PLANE = NI_MAX * 1024;                                   // 288 patch rows of 64 B
  static constexpr int NT2 = MM == 3 ? 1 : 2;                                   // 32-channel accumulator tiles per wave (a wave = 128 px x 32 NT2 ch)
  static constexpr int NBL = KS * NP * NT2;                                     // filter loads per tap and wave
  static constexpr int NPX = 64;                                                // pixels per epilogue pass
  static constexpr int EPW = NPX * C16_EP_LD * 4;                               // a wave's epilogue tile
};

struct C16Geom {      // one 128-pixel tile of the halo tiling (block-uniform: scalar registers): its segment, position, pieces per plane
  int si, ni;
  c16g::Tile t;
};
__device__ __forceinline__ C16Geom c16w_geom(const C16Params& p, int ptile) {
  C16Geom o;
  int si = 0;
#pragma unroll
  for (int i = 1; i < 4; ++i) if (i < p.nseg && ptile >= p.seg[i].h_tile0) si = i;
  const C16Seg& sg = p.seg[si];
  o.si = si; o.ni = (sg.h_P + 15) >> 4;
  o.t = c16g::tile_of(sg, sg.H, sg.W, ptile - sg.h_tile0);
  return o;
}

// s_waitcnt vmcnt(BASE + n) for a wave-uniform run-time n in [0, HI] (the instruction takes an immediate only): a compare chain
template <int BASE, int HI>
__device__ __forceinline__ void c16_wait_vm(int n) {
  if constexpr (HI == 0) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(BASE) : "memory");
  } else {
    if (n >= HI) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(BASE + HI) : "memory");
    else c16_wait_vm<BASE, HI - 1>(n);
  }
}

// KD = 3 (pairs only): a 3x3x3 layer with its DEPTH TAPS FOLDED INTO THE REDUCTION.  The map is the tall image of N D planes of H x W, a
// tile lies inside one plane (the launcher admits only such tilings), and the filters are packed as a 2-D bank of 3 Cin channels in the
// order (dz, ci): slice c of the K loop is channel slice c % (Cin / 32) of depth tap dz = c / (Cin / 32), and its patch is the SAME halo
// patch one plane down or up — the piece offsets move by (dz - 1) H W pixels, LDS holds what it holds for a 2-D layer.  Where plane
// z + dz - 1 lies outside the volume (the plane after z = D - 1 is plane 0 of the NEXT volume: padding, not data) the slice contributes
// zero: its pieces are requested out of range, so that the DMA overwrites the stage with zeros (the pieces zeroed once and never
// requested — in-plane halo outside the map — stay zero for every slice).  Slices are ordered by dz, so a block whose tiles ALL lie in
// plane 0 (D - 1) simply starts its loop after the dz = 0 slices (ends it before the dz = 2 slices) and walks the filters from there.
template <int MM, int WM, int NT2 = C16W<MM>::NT2, int KD = 1>
__global__ __launch_bounds__(256, 2) void conv16w_kernel(const C16Params p) {
  typedef typename C16T3<MM>::V V8;
  typedef C16W<MM> R;
  static_assert(KD == 1 || (KD == 3 && MM == 3), "depth taps fold into the pair kernel's reduction only");
  constexpr int WN = 4 / WM, NP = R::NP, KS = R::KS, NBL = KS * NP * NT2, CW = 32 * NT2;   // (NT2 = 1 in a 16-bit mode: 32-channel waves for Cout = 64)
  constexpr bool SINGLE = MM == 3 && WM == 2;                  // one patch stage instead of two (see the slice hand-over below)
  constexpr int TILE_B = NP * R::PLANE, STAGE = WM * TILE_B;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  // block id -> (tile group, channel block): the channel blocks of a tile group run back to back on ONE XCD (ids = xcd mod 8)
  const int xcd = blockIdx.x & 7, jj = blockIdx.x >> 3;
  const int cb = jj % p.nN, tg = (jj / p.nN) * 8 + xcd;
  if (tg * WM >= p.ptiles) return;
  const int wm = wv / WN, wn = wv % WN;
  const int nchunk = KD == 1 ? p.Cin >> 5 : 3 * (p.Cin >> 5);
  typedef __attribute__((address_space(3))) void* lds_ptr;

  // ---- the patch pieces this lane requests per slice: tile tl, pieces ii = wv + 4 j of its ni pieces per plane (rows 16 ii + lane / 4),
  // the same piece of every plane (the lo plane of a pixel follows its hi plane: one offset serves both).  The geometry
  // (conv16w_geom.h) is computed once per tile; an INTERIOR tile — its whole patch inside one image — needs no validity test.
  // A piece none of whose lanes lies inside the map (halo pixels outside the image) is not requested: its LDS rows are zeroed here,
  // once, in both stages (the geometry is the same for every slice).
  constexpr int NPJ = (R::NI_MAX + 3) / 4;                     // pieces per wave, tile and plane at most
  unsigned poff[WM][NPJ], pmask[WM];
  C16Geom gms[WM];
#pragma unroll
  for (int tl = 0; tl < WM; ++tl) {
    gms[tl] = c16w_geom(p, min(tg * WM + tl, p.ptiles - 1));
    const C16Geom& gm = gms[tl];
    const C16Seg& sg = p.seg[gm.si];
    const unsigned base = c16g::tile_base(sg.W, sg.ld_in, gm.t);
    unsigned pm = 0;
    if (gm.t.interior) {
#pragma unroll
      for (int j = 0; j < NPJ; ++j) {
        const c16g::Piece pc = c16g::piece_of(sg, wv + 4 * j, lane);
        poff[tl][j] = pc.in_patch ? c16g::piece_offset(sg, sg.W, sg.ld_in, base, pc) : C16_OOB;     // (the tail of the last piece)
        if (wv + 4 * j < gm.ni) pm |= 1u << j;
      }
    } else {
#pragma unroll
      for (int j = 0; j < NPJ; ++j) {
        const int ii = wv + 4 * j;
        const c16g::Piece pc = c16g::piece_of(sg, ii, lane);
        const bool ok = c16g::piece_valid(sg, sg.H, sg.W, sg.rows, gm.t, pc);
        poff[tl][j] = ok ? c16g::piece_offset(sg, sg.W, sg.ld_in, base, pc) : C16_OOB;
        if (ii < gm.ni) {
          if (__builtin_amdgcn_ballot_w64(ok) != 0) pm |= 1u << j;
          else {
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) {
              char* dst = lds + tl * TILE_B + pl * R::PLANE + ii * 1024 + lane * 16;
              *reinterpret_cast<f32x4*>(dst) = z;
              if constexpr (!SINGLE) *reinterpret_cast<f32x4*>(dst + STAGE) = z;
            }
          }
        }
      }
    }
    pmask[tl] = __builtin_amdgcn_readfirstlane(pm);
  }
  // KD = 3: the plane of each tile inside its volume, and the slices [c_lo, c_hi) the block walks (all of them unless every tile of the
  // block lies in the first / last plane)
  int c_lo_ = 0, c_hi_ = nchunk;
  [[maybe_unused]] int zt[WM];
  [[maybe_unused]] const int ncs = p.Cin >> 5;
  if constexpr (KD == 3) {
    bool first = true, last = true;
#pragma unroll
    for (int tl = 0; tl < WM; ++tl) {
      zt[tl] = (int)((unsigned)gms[tl].t.img % (unsigned)p.D);
      first = first && zt[tl] == 0; last = last && zt[tl] == p.D - 1;
    }
    c_lo_ = first ? ncs : 0; c_hi_ = last ? 2 * ncs : 3 * ncs;
  }
  const int c_lo = c_lo_, c_hi = c_hi_;
  const unsigned plane_b = (unsigned)(p.Cin * 2);
  auto issue_patch = [&](int c, int stage) {
    if (c >= c_hi) return;                                             // (no request past the last slice: the waits count 0 pieces there)
    [[maybe_unused]] int dz = 1;
    unsigned ck;
    if constexpr (KD == 3) { dz = (c >= ncs ? 1 : 0) + (c >= 2 * ncs ? 1 : 0); ck = (unsigned)((c - dz * ncs) * 64); }
    else ck = (unsigned)(c * 64);
#pragma unroll
    for (int tl = 0; tl < WM; ++tl) {
      const C16Seg& sg = p.seg[gms[tl].si];
      const __amdgpu_buffer_rsrc_t rs_in = c16_rsrc(sg.in, sg.in_bytes - sg.back);
      unsigned ckt = ck;
      bool pad = false;
      if constexpr (KD == 3) {
        ckt = ck + (unsigned)((dz - 1) * (sg.H * sg.W * sg.ld_in * 2));    // the same patch one plane down / up (wraps to the true offset)
        pad = (unsigned)(zt[tl] + dz - 1) >= (unsigned)p.D;                // ... which lies outside the volume: zeros
      }
#pragma unroll
      for (int j = 0; j < NPJ; ++j) {
        if (pmask[tl] >> j & 1) {
          const unsigned vo = (poff[tl][j] == C16_OOB || pad) ? C16_OOB : poff[tl][j] + ckt;      // (C16_OOB + a plane stays beyond the buffer)
#pragma unroll
          for (int pl = 0; pl < NP; ++pl)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_in, (lds_ptr)(lds + stage * STAGE + tl * TILE_B + pl * R::PLANE + (wv + 4 * j) * 1024), 16,
                                                     vo + pl * plane_b, 0, 0, 0);
        }
      }
    }
  };
  // this wave's tile (fragment geometry, epilogue)
  const C16Geom gm = WM == 1 ? gms[0] : gms[wm ? WM - 1 : 0];
  const C16Seg& sgw = p.seg[gm.si];
  const int f_tw_log2 = sgw.h_tw_log2, f_PW = (1 << f_tw_log2) + 2;

  // ---- filter fragments of (slice c, tap t): KS x NP x 2 pieces of 16 bytes per lane of THIS wave's 64 channels, hand-issued (see
  // conv16r_kernel).  Packed K steps hold 64 channels (pairs: 32): slice c is half (c & 1) of packed step (c >> 1) * 9 + t.
  const int chan0 = (cb * WN + wn) * CW;
  const int nkp = (MM == 3 ? nchunk : nchunk >> 1) * 9;
  const char* wtile = p.w + (long)(chan0 >> 7) * nkp * 16384;
  unsigned bvo[KS * NP];
  if constexpr (MM == 3) {
    // 16x16x32 B fragment q = n2 NP + plane: lane l needs co = 32 j + 16 n2 + (l & 15), ci = 8 (l >> 4) + e — in the packed piece
    // (ks = l >> 5, plane) the lane 32 ((l >> 4) & 1) + 16 n2 + (l & 15) of group j: four 256-byte runs of the 1 KB pieces
#pragma unroll
    for (int q = 0; q < KS * NP; ++q)
      bvo[q] = ((lane >> 5) * NP + q % NP) * 4096 + ((chan0 >> 5) & 3) * 1024 + (32 * ((lane >> 4) & 1) + 16 * (q / NP) + (lane & 15)) * 16;
  } else {
#pragma unroll
    for (int q = 0; q < KS * NP; ++q) bvo[q] = q * 4096 + ((chan0 >> 5) & 3) * 1024 + lane * 16;
  }
  // The requests walk the packed filters in step order with a running pointer: + 16 KB per tap; at a slice boundary + 16 KB for pairs,
  // and for the 16-bit modes (two 32-channel slices per packed step) + 8 KB - 8 x 16 KB into an odd slice, + 8 KB out of it.  Past the
  // last step the pointer stays on the first one (a harmless reload: the request count per step stays uniform).
  const char* wp = KD == 1 ? wtile : wtile + (long)c_lo * (9 * 16384);
  int wleft = (c_hi - c_lo) * 9;
  auto load_b = [&](int c, int t, V8 (&b)[NBL]) {                // (c, t): the step being requested — requests are issued in step order
    const unsigned long wa = (unsigned long)(wleft > 0 ? wp : wtile);
    const char* ws = reinterpret_cast<const char*>((unsigned long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)wa) |
                                                   ((unsigned long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(wa >> 32)) << 32));
#pragma unroll
    for (int q = 0; q < KS * NP; ++q) {
      asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(b[NT2 * q]) : "v"(bvo[q]), "s"(ws) : "memory");
      if constexpr (NT2 == 2) asm volatile("global_load_dwordx4 %0, %1, %2 offset:1024" : "=v"(b[NT2 * q + 1]) : "v"(bvo[q]), "s"(ws) : "memory");
    }
    --wleft;
    if (t < 8 || MM == 3) wp += 16384;
    else wp += (c & 1) ? 8192 : 8192 - 8 * 16384;
  };

  if constexpr (MM == 3) {
    // ---- pairs on v_mfma_f32_16x16x32_f16.  m-tile mt = tile pixels 16 mt + (lane & 15): the lane reads logical slot lane >> 4 (channels
    // 8 (lane >> 4) .. + 7 of the slice) of the pixel's patch row in each plane, so one read per (m-tile, plane) covers the whole slice and
    // feeds one MFMA per (16-channel n-tile, term).  The pair tilings have swd = 0 and swa <= 2 (c16_halo_tiling): the slot swizzle
    // (column >> swa) & 3 of tap column kx is then the same for the eight m-tiles (their columns differ by multiples of 16) — xs[kx],
    // the logical slot folded in — and a fragment address is qb[mt] + the tap's offset: one VALU per two reads (hi and lo plane).
    int qb[8], xs[3];
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) qb[mt] = c16g::frag_pixel(sgw, 16 * mt + (lane & 15)) * 64 + wm * TILE_B;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) xs[kx] = ((lane >> 4) ^ ((((lane & 15 & ((1 << f_tw_log2) - 1)) + kx) >> sgw.h_swa) & 3)) << 4;
    const int PW64 = f_PW * 64;
    auto tap_off = [&](int t, int stg) { return xs[t % 3] + (stg * STAGE + (t / 3) * PW64 + (t % 3) * 64); };
    auto read_pair = [&](int mp, int off, V8 (&a)[2][NP]) {      // the fragments of m-tiles 2 mp, 2 mp + 1
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int addr = qb[2 * mp + i] + off;
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) a[i][pl] = *reinterpret_cast<const V8*>(lds + pl * R::PLANE + addr);
      }
    };
    f32x4 acc[8][2];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[a][b][r] = 0.f;
    // the 12 MFMAs of an m-tile pair: b[n2 NP + plane], terms hi x hi, hi x lo, lo x hi; four independent accumulators between two
    // dependent MFMAs
    auto mfmas = [&](int mp, const V8 (&a)[2][NP], const V8 (&b)[NBL]) {
#pragma unroll
      for (int term = 0; term < 3; ++term) {
        const int pa = term == 2 ? 1 : 0, pb = term == 1 ? 1 : 0;
#pragma unroll
        for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
          for (int i = 0; i < 2; ++i)
            acc[2 * mp + i][n2] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i][pa], b[n2 * NP + pb], acc[2 * mp + i][n2], 0, 0, 0);
      }
    };

    // ---- K loop as in the 16-bit modes below (filter ring, counted waits, one barrier per slice).  A ROLLING set of three m-tile pairs'
    // fragments: pair g = 4 tap + (pair of the tap) sits in fa[g % 3]; right after its MFMAs have issued, the same registers receive
    // pair g + 3 — consumed 24 MFMAs later.  The first three pairs of a slice are read after its barrier.
    V8 bs[3][NBL];
    V8 fa[3][2][NP];
    issue_patch(c_lo, 0);
    load_b(0, 0, bs[0]);
    load_b(0, 1, bs[1]);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // (lgkmcnt: the zeroed halo pieces)
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int mp = 0; mp < 3; ++mp) read_pair(mp, tap_off(0, 0), fa[mp]);
    int stage = 0;
#pragma unroll 1
    for (int c = c_lo; c < ((C16W_ABLATE & 8) ? 0 : c_hi); ++c) {      // (ablation bit 3: no K loop at all — what a block costs outside it)
      // (opaque to the optimiser: it would otherwise hoist the per-(tap, m-tile) addresses out of the slice loop and spill them)
#pragma unroll
      for (int mt = 0; mt < 8; ++mt) asm volatile("" : "+v"(qb[mt]));
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) asm volatile("" : "+v"(xs[kx]));
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int t2 = (t + 2) % 9, c2 = c + (t + 2) / 9;
        if (!((C16W_ABLATE & 2) && c > 0)) load_b(c2, t2, bs[(t + 2) % 3]);
        if (t == 0 && !SINGLE && !((C16W_ABLATE & 1) && c > 0)) issue_patch(c + 1, stage ^ 1);
        if (C16W_ABLATE) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NBL) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        const int off = tap_off(t, stage), noff = tap_off(t < 8 ? t + 1 : 0, stage);
#pragma unroll
        for (int mp = 0; mp < 4; ++mp) {
          const int g = 4 * t + mp, gn = g + 3;                       // (36 pairs per slice)
          mfmas(mp, fa[g % 3], bs[t % 3]);
          if (gn < 36 && !((C16W_ABLATE & 4) && c > 0)) read_pair(gn % 4, gn / 4 == t ? off : noff, fa[g % 3]);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (t == 8) {
          asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // (vmcnt: this wave's pieces of the next patch, see below)
          __builtin_amdgcn_s_barrier();                          // every wave has read this patch and received its share of the next
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (SINGLE) {
            // one LDS stage (the two-tile form: two stages would be 147 KB = one block per CU): the next patch is requested only now,
            // into the stage everybody has just left; the other block of the CU computes while it arrives
            issue_patch(c + 1, 0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
          } else stage ^= 1;
          if (c + 1 < c_hi) {
#pragma unroll
            for (int mp = 0; mp < 3; ++mp) read_pair(mp, tap_off(0, stage), fa[mp]);
          }
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // the look-ahead filter requests past the end have landed
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);

    // ---- epilogue, private to the wave (as in the 16-bit modes): the 16 x 16 accumulator holds pixel 4 (lane >> 4) + r of its m-tile and
    // channel lane & 15 of its n-tile
    if (tg * WM + wm >= p.ptiles) return;                         // (the odd tile of the last group)
    const C16Seg& sg = p.seg[gm.si];
    float* ep = reinterpret_cast<float*>(lds + wv * R::EPW);
    float bv[2];
#pragma unroll
    for (int n2 = 0; n2 < 2; ++n2) bv[n2] = p.bias ? p.bias[chan0 + 16 * n2 + (lane & 15)] : 0.f;
    constexpr int MTP = R::NPX / 16;                              // m-tiles per pass
    const float as = ldexpf(p.acc_scale, g6d_exp_in(p.rng));     // pair input held as x * 2^-e_in
    unsigned amax = 0;
    double wst[2] = {0.0, 0.0};
    // the passes, specialised on the launch's output format (full_type, pool_type, statistics: -1 = read from p in the pass) and on where
    // the statistics are flushed (spc: 0 = once per tile by the caller, 1 = after every pass under the pass's own group, -1 = per_pass)
    const bool per_pass = c16w_stats_per_pass(p, sg, f_tw_log2);
    auto passes = [&](auto ftc, auto ptc, auto stc, auto spc) {
#pragma unroll
      for (int ps = 0; ps < 8 / MTP; ++ps) {
#pragma unroll
        for (int m = 0; m < MTP; ++m)
#pragma unroll
          for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int px = 16 * m + 4 * (lane >> 4) + r;
              float v = fmaf(acc[ps * MTP + m][n2][r], as, bv[n2]);
              if (p.relu) v = fmaxf(v, 0.f);
              ep[px * C16_EP_LD + 16 * n2 + (lane & 15)] = v;
            }
        c16_epilogue_pass<2, 64, R::NPX, CW, decltype(ftc)::value, decltype(ptc)::value, decltype(stc)::value>(
            p, sg, ep, nullptr, lane, chan0, gm.t.g0, gm.t.x0, f_tw_log2, gm.t.ylim, ps * R::NPX, amax, wst);
        if (decltype(spc)::value > 0 || (decltype(spc)::value < 0 && per_pass))
          c16_stats_flush_pass<CW>(p, sg, lane, chan0, gm.t.g0 + ((ps * R::NPX) >> f_tw_log2), wst);
      }
    };
    typedef std::integral_constant<int, -1> any_;
    typedef std::integral_constant<int, 0> c0_;
    typedef std::integral_constant<int, 1> c1_;
    // the trunks' forms (pair outputs, no statistics) and the selector's (fp32 map and statistics); anything else: the general form
    // (and the feature net's 8 x 8 maps: the same with one statistics group per pass)
    if (!p.stats && p.full_type == 3 && p.pool_type == 0) passes(std::integral_constant<int, 3>{}, c0_{}, c0_{}, c0_{});
    else if (!p.stats && p.full_type == 0 && p.pool_type == 3) passes(c0_{}, std::integral_constant<int, 3>{}, c0_{}, c0_{});
    else if (!p.stats && p.full_type == 3 && p.pool_type == 3) passes(std::integral_constant<int, 3>{}, std::integral_constant<int, 3>{}, c0_{}, c0_{});
    else if (p.stats && p.full_type == 2 && p.pool_type == 0 && !per_pass) passes(std::integral_constant<int, 2>{}, c0_{}, c1_{}, c0_{});
    else if (p.stats && p.full_type == 2 && p.pool_type == 0) passes(std::integral_constant<int, 2>{}, c0_{}, c1_{}, c1_{});
    else passes(any_{}, any_{}, any_{}, any_{});
    if (p.stats && !per_pass) c16_stats_flush<CW>(p, sg, lane, chan0, gm.t.g0, wst);
    g6d_range_record(p.rng, amax);
  } else {
    // ---- fragment geometry of this wave's tile: m-tile mt = tile pixels 32 mt + (lane & 31) -> patch row of tap (0, 0)
    const int fhalf = lane >> 5;
    // slot swizzle of patch (row, column): ((column >> swa) + row * swd) & 3, and swd != 0 only with swa == 0 (c16_halo_tiling): with
    // fe = column + row * swd (swa == 0) or column (swd == 0) the swizzle of tap (ky, kx) is ((fe + kx) >> swa) + ky * swd
    int qb[4], fe[4];
    const int PW64 = f_PW * 64, swa = sgw.h_swa, swd = sgw.h_swd;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int r = 32 * mt + (lane & 31);
      qb[mt] = c16g::frag_pixel(sgw, r) * 64 + wm * TILE_B; fe[mt] = (r & ((1 << f_tw_log2) - 1)) + c16g::frag_row(sgw, r) * swd;
    }
    auto tap_addr = [&](int ky, int kx, int stage, int (&tb)[4]) {
      const int so = stage * STAGE + (ky * PW64 + kx * 64);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int sw = ((fe[mt] + kx) >> swa) + ky * swd;
        tb[mt] = qb[mt] + so + (((fhalf ^ sw) & 3) << 4);
      }
    };
    auto frag_read = [&](int addr, V8 (&a)[NP]) {
#pragma unroll
      for (int pl = 0; pl < NP; ++pl) a[pl] = *reinterpret_cast<const V8*>(lds + pl * R::PLANE + addr);
    };
    f32x16 acc[4][NT2];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < NT2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    // the MFMAs of one m-tile and one 16-channel group: b[ks * NT2 + n2]
    auto mfmas = [&](int mt, const V8 (&a)[NP], const V8 (&b)[NBL], int ks) {
#pragma unroll
      for (int n2 = 0; n2 < NT2; ++n2) acc[mt][n2] = c16_mfma<MM>(a[0], b[ks * NT2 + n2], acc[mt][n2]);
    };

    // ---- K loop: slices outermost (one patch, one barrier each), the nine taps unrolled inside.  FILTER loads return in order among
    // themselves, so before the MFMAs of step (c, t) vmcnt(2 NBL) — the two younger filter sets — proves B(c, t) has arrived.  LDS-DMA
    // requests are NOT ordered against them (measured on corr16_kernel: a counted wait that budgeted the younger patch pieces let MFMAs
    // start on filters still in flight once the filters missed L2 — the DMA of L2-resident activations overtakes them): the wait therefore
    // never budgets for DMA pieces (while some are in flight it is merely stricter than needed), and the wave's own pieces of the next
    // patch are drained with vmcnt(0) before the slice's barrier.
    // ONE set of activation fragments, replaced m-tile by m-tile: right after the MFMAs of (m-tile, 16-channel group) have issued, the
    // same registers receive the m-tile's fragment of the NEXT group (the other half of the slice, or the next tap) — consumed eight
    // MFMAs later.
    V8 bs[3][NBL];
    V8 fa[4][NP];
    int tb[4], ntb[4];
    issue_patch(0, 0);
    load_b(0, 0, bs[0]);
    load_b(0, 1, bs[1]);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // (lgkmcnt: the zeroed halo pieces)
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    tap_addr(0, 0, 0, tb);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) frag_read(tb[mt], fa[mt]);
    int stage = 0;
#pragma unroll 1
    for (int c = 0; c < ((C16W_ABLATE & 8) ? 0 : nchunk); ++c) {      // (ablation bit 3: no K loop at all — what a block costs outside it)
      // (opaque to the optimiser: it would otherwise hoist the 36 per-(tap, m-tile) swizzle terms out of the slice loop and spill them)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) asm volatile("" : "+v"(fe[mt]), "+v"(qb[mt]));
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int t2 = (t + 2) % 9, c2 = c + (t + 2) / 9;
        if (!((C16W_ABLATE & 2) && c > 0)) load_b(c2, t2, bs[(t + 2) % 3]);
        if (t == 0 && !((C16W_ABLATE & 1) && c > 0)) issue_patch(c + 1, stage ^ 1);
        if (C16W_ABLATE) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NBL) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (t < 8) tap_addr((t + 1) / 3, (t + 1) % 3, stage, ntb);
        else tap_addr(0, 0, stage ^ 1, ntb);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
          mfmas(mt, fa[mt], bs[t % 3], 0);
          if (!((C16W_ABLATE & 4) && c > 0)) frag_read(tb[mt] ^ 32, fa[mt]);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
          mfmas(mt, fa[mt], bs[t % 3], 1);
          if (t < 8 && !((C16W_ABLATE & 4) && c > 0)) frag_read(ntb[mt], fa[mt]);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) tb[mt] = ntb[mt];
        if (t == 8) {
          asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // (vmcnt: this wave's pieces of the next patch, see above)
          __builtin_amdgcn_s_barrier();                          // every wave has read this patch and received its share of the next
          __builtin_amdgcn_sched_barrier(0);
          stage ^= 1;
          if (c + 1 < nchunk) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) frag_read(tb[mt], fa[mt]);
          }
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // the look-ahead filter requests past the end have landed
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);

    // ---- epilogue, private to the wave: its 128 px x 64 ch go through its own fp32 LDS tile in passes of NPX pixels
    if (tg * WM + wm >= p.ptiles) return;                         // (the odd tile of the last group)
    const C16Seg& sg = p.seg[gm.si];
    float* ep = reinterpret_cast<float*>(lds + wv * R::EPW);
    float bv[NT2];
#pragma unroll
    for (int n2 = 0; n2 < NT2; ++n2) bv[n2] = p.bias ? p.bias[chan0 + 32 * n2 + (lane & 31)] : 0.f;
    constexpr int MTP = R::NPX / 32;                              // m-tiles per pass
    const float as = ldexpf(p.acc_scale, g6d_exp_in(p.rng));     // pair input held as x * 2^-e_in
    unsigned amax = 0;
    double wst[2] = {0.0, 0.0};
    const bool per_pass = c16w_stats_per_pass(p, sg, f_tw_log2);
    auto passes = [&](auto ftc, auto ptc, auto stc) {              // (specialised on the output format as in the pair branch)
#pragma unroll
      for (int ps = 0; ps < 4 / MTP; ++ps) {
#pragma unroll
        for (int m = 0; m < MTP; ++m)
#pragma unroll
          for (int n2 = 0; n2 < NT2; ++n2)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int px = 32 * m + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
              float v = fmaf(acc[ps * MTP + m][n2][r], as, bv[n2]);
              if (p.relu) v = fmaxf(v, 0.f);
              ep[px * C16_EP_LD + 32 * n2 + (lane & 31)] = v;
            }
        c16_epilogue_pass<MM, 64, R::NPX, CW, decltype(ftc)::value, decltype(ptc)::value, decltype(stc)::value>(
            p, sg, ep, nullptr, lane, chan0, gm.t.g0, gm.t.x0, f_tw_log2, gm.t.ylim, ps * R::NPX, amax, wst);
        if (decltype(stc)::value != 0 && per_pass)                   // (statistics run on the general form only)
          c16_stats_flush_pass<CW>(p, sg, lane, chan0, gm.t.g0 + ((ps * R::NPX) >> f_tw_log2), wst);
      }
    };
    typedef std::integral_constant<int, -1> any_;
    typedef std::integral_constant<int, 0> c0_;
    typedef std::integral_constant<int, 1> c1_;
    if (!p.stats && p.full_type == 1 && p.pool_type == 0) passes(c1_{}, c0_{}, c0_{});
    else if (!p.stats && p.full_type == 0 && p.pool_type == 1) passes(c0_{}, c1_{}, c0_{});
    else if (!p.stats && p.full_type == 1 && p.pool_type == 1) passes(c1_{}, c1_{}, c0_{});
    else passes(any_{}, any_{}, any_{});
    if (p.stats && !per_pass) c16_stats_flush<CW>(p, sg, lane, chan0, gm.t.g0, wst);
    if (p.full_type == 3 || p.pool_type == 3) g6d_range_record(p.rng, amax);
  }
}

// Tiling of one segment for the halo-patch kernel: the tile width (32 / 16 / 8 / 4) with the least overhang; false if none fits
// (a map lower than the tile must divide it: tiles of whole images).  pairs: the fp16 pair kernel's slot swizzle (its fragment reads differ);
// in_image: only tilings whose tiles lie inside one image (depth-folded layers: s.N counts planes, and a tile must not span two)
bool c16_halo_tiling(const G6dConv16Seg& s, C16Seg& o, int& tiles, bool pairs, bool in_image = false) {
  double best = 1e30;
  bool found = false;
  for (int tw = 32; tw >= 4; tw >>= 1) {
    const int th = C16_BM / tw, tx = (s.W + tw - 1) / tw;
    long nt; int tpi, segh, bands;
    if (s.H >= th) { tpi = tx * ((s.H + th - 1) / th); nt = (long)s.N * tpi; segh = th; bands = 1; }
    else {
      if (th % s.H || in_image) continue;
      tpi = 0; nt = (long)tx * (((long)s.N * s.H + th - 1) / th); segh = s.H; bands = th / s.H;
    }
    if (bands * (segh + 2) * (tw + 2) > 288) continue;
    const double waste = (double)nt * C16_BM / ((double)s.N * s.H * s.W);
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
  return found && c16g::finish(o, tiles);
}

int c16_pick_tw(int W, int pool) {
  // tile width (power of two, 4..64; even for pooling) with the least column overhang, ties -> the wider tile
  int best = 8; double bw = 1e9;
  for (int tw = 64; tw >= (pool ? 4 : 4); tw >>= 1) {
    const double waste = (double)((W + tw - 1) / tw * tw) / W;
    if (waste < bw - 1e-9) { bw = waste; best = tw; }
  }
  return best;
}

}  // namespace

namespace {
// g6d_conv16_direct_multi_ex; plan_only: validate and choose the kernel, launch nothing (g6d_conv16_direct_plan's return value)
int c16_direct(const G6dConv16Seg* segs, int nseg, int Cin, const void* W16, int w_layout, float acc_scale, const float* bias, int Cout, int kd, int relu,
               int full_type, int pool_type, int math_mode, double* stats, int stat_rows_per_group, const G6dRange16* range, g6d_stream_t stream,
               bool plan_only) {
  if (!segs || nseg < 1 || nseg > 4 || !W16) { g6d_set_error("conv16_direct: 1..4 segments and filters expected"); return G6D_EINVAL; }
  // w_layout 2: fragment-major filters of a 3x3x3 layer packed as the 2-D bank [Cout][9][3 Cin], channel order (dz, ci) — the pair
  // kernel folds the depth taps into its reduction (conv16w_kernel<3, ., 1, 3>)
  const bool folded = w_layout == 2;
  if (math_mode < 1 || math_mode > 3 || w_layout < 0 || w_layout > 2 || (math_mode == 3 && w_layout == 0) || (folded && (math_mode != 3 || kd != 3))) {
    g6d_set_error("conv16_direct: math_mode 1 (bf16) / 2 (fp16) / 3 (fp16 hi-lo pairs, fragment-major filters only)"); return G6D_EINVAL;
  }
  const int bk = math_mode == 3 ? 32 : C16_BK, planes = math_mode == 3 ? 2 : 1;
  // Cout = 64 (the selector's first product layer): halo-patch kernel only, filters packed as one 128-channel tile whose upper half is zero
  const bool half_tile = Cout == 64 && ((w_layout == 1 && kd == 1) || folded);      // (32-channel waves: two pixel tiles x two channel groups per block)
  if (Cin % bk || (Cout % C16_BN && !half_tile) || (kd != 1 && kd != 3)) { g6d_set_error("conv16_direct: Cin % 64 (32 for pairs), Cout % 128 (64: fragment-major 2-D layers), kd in {1,3} expected"); return G6D_EINVAL; }
  const int t16 = math_mode == 3 ? 3 : 1;                    // the 16-bit output coding of this mode
  auto type_ok = [&](int t) { return t == 0 || t == 2 || t == t16; };
  if (!type_ok(full_type) || !type_ok(pool_type) || (!full_type && !pool_type && !stats)) { g6d_set_error("conv16_direct: output types"); return G6D_EINVAL; }
  if (pool_type && kd != 1) { g6d_set_error("conv16_direct: pooling is 2-D only"); return G6D_EINVAL; }
  C16Params p = {};
  p.nseg = nseg; p.Cin = Cin; p.Cout = Cout; p.kd = kd; p.relu = relu; p.full_type = full_type; p.pool_type = pool_type;
  p.w = static_cast<const char*>(W16); p.bias = bias; p.stats = stats; p.stat_rows_per_group = stat_rows_per_group;
  p.acc_scale = acc_scale != 0.f ? acc_scale : 1.f;
  p.ablate = (int)g6d_knob(G6D_KNOB_C16_ABLATE);
  if (range) p.rng = *range;
  const long wb = (long)(half_tile ? 128 : Cout) * 9 * kd * Cin * 2 * planes;
  if (wb >= (1L << 31)) { g6d_set_error("conv16_direct: filters beyond 2 GB"); return G6D_EINVAL; }
  p.w_bytes = (unsigned)wb;
  p.nN = Cout / C16_BN;
  int tiles = 0, D0 = segs[0].D;
  bool pertap_stats_ok = true;
  for (int i = 0; i < nseg; ++i) {
    const G6dConv16Seg& s = segs[i];
    C16Seg& o = p.seg[i];
    if (!s.in || s.N < 1 || s.D < 1 || s.H < 1 || s.W < 1 || s.ld_in < planes * Cin || s.D != D0 || (kd == 1 && s.D != 1)) { g6d_set_error("conv16_direct: bad segment"); return G6D_EINVAL; }
    const int need_full = full_type == 3 ? 2 * Cout : Cout, need_pool = pool_type == 3 ? 2 * Cout : Cout;
    if ((full_type && (!s.out_full || s.ld_full < need_full)) || (pool_type && (!s.out_pool || s.ld_pool < need_pool || (s.H & 1) || (s.W & 1)))) {
      g6d_set_error("conv16_direct: outputs missing / odd map with pooling"); return G6D_EINVAL;
    }
    if (!g6d_aligned16(s.in) || (s.ld_in & 7) || (full_type && (!g6d_aligned16(s.out_full) || (s.ld_full & 7))) || (pool_type && (!g6d_aligned16(s.out_pool) || (s.ld_pool & 7)))) {
      g6d_set_error("conv16_direct: 16-byte aligned rows expected"); return G6D_EINVAL;
    }
    // (the epilogues address an output from the tile's first pixel with 32-bit offsets: at most 32 rows of W pixels)
    if (32L * s.W * (s.ld_full > s.ld_pool ? s.ld_full : s.ld_pool) * 4 >= (1L << 32)) { g6d_set_error("conv16_direct: 32 output rows beyond 4 GB"); return G6D_EINVAL; }
    o.in = static_cast<const char*>(s.in); o.full = static_cast<char*>(s.out_full); o.pool = static_cast<char*>(s.out_pool);
    o.H = s.H; o.W = s.W; o.DH = s.D * s.H; o.rows = s.N * s.D * s.H;
    o.ld_in = s.ld_in; o.ld_full = s.ld_full; o.ld_pool = s.ld_pool;
    const int tw = c16_pick_tw(s.W, pool_type != 0);
    int l2 = 0; while ((1 << l2) < tw) ++l2;
    o.tw_log2 = l2; o.tiles_x = (s.W + tw - 1) / tw; o.tile0 = tiles;
    const int th = C16_BM / tw;
    // (the per-tap kernels flush a tile's statistics under ONE group; the halo-patch kernel has its own rule below)
    if (stats && stat_rows_per_group > 0 && ((long)stat_rows_per_group % ((long)th * s.W) != 0)) pertap_stats_ok = false;
    tiles += o.tiles_x * ((o.rows + th - 1) / th);
    // the descriptor starts (kd == 3 ? H W : 0) + W + 1 pixels before the tensor: tap offsets are then non-negative
    const long back = ((long)(kd == 3 ? s.H * s.W : 0) + s.W + 1) * s.ld_in * 2;
    const long ext = (long)o.rows * s.W * s.ld_in * 2 + back;
    if (ext >= (1L << 31)) { g6d_set_error("conv16_direct: a segment's input beyond 2 GB"); return G6D_EINVAL; }
    o.back = (int)back; o.in_bytes = (unsigned)ext;
  }
  p.D = D0;
  p.ptiles = tiles;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // fragment-major filters, 2-D layer: the halo-patch kernel when every segment has a tiling for it (knob conv16_halo = 0: never)
  if (((w_layout == 1 && kd == 1) || folded) && g6d_knob(G6D_KNOB_CONV16_HALO) != 0) {
    bool ok = true, per_pass = false;
    int htiles = 0;
    for (int i = 0; i < nseg && ok; ++i) {
      int nt_ = 0;
      if (folded) {
        // the planes of the volumes are the images of the tiling; statistics groups are whole volumes (a tile lies inside one plane)
        G6dConv16Seg planes_ = segs[i];
        planes_.N = segs[i].N * segs[i].D; planes_.D = 1;
        ok = (long)segs[i].N * segs[i].D < (1L << 31) && c16_halo_tiling(planes_, p.seg[i], nt_, true, true);
        p.seg[i].h_tile0 = htiles; htiles += nt_;
        if (stats && stat_rows_per_group > 0 && ok) ok = stat_rows_per_group % ((long)segs[i].D * segs[i].H * segs[i].W) == 0;
        continue;
      }
      ok = c16_halo_tiling(segs[i], p.seg[i], nt_, math_mode == 3);
      p.seg[i].h_tile0 = htiles; htiles += nt_;
      if (stats && stat_rows_per_group > 0 && ok) {
        const C16Seg& o = p.seg[i];
        const int th = C16_BM >> o.h_tw_log2;
        // groups are whole images.  In-image tiles then lie inside one group; a banded tile (whole small images) does when the group is
        // whole tiles, or else spans groups of whole epilogue passes (flushed per pass).  A group smaller than a pass, or not aligned to
        // one, has no place to be summed: no halo tiling, and the per-tap kernels reject it too
        const long tile_px = (long)th * segs[i].W, pass_px = (long)(C16W<3>::NPX >> o.h_tw_log2) * segs[i].W;
        static_assert(C16W<1>::NPX == C16W<3>::NPX && C16W<2>::NPX == C16W<3>::NPX, "one pass size in every mode");
        ok = (stat_rows_per_group % (segs[i].H * segs[i].W) == 0) &&
             (o.h_tpi > 0 || stat_rows_per_group % tile_px == 0 || (stat_rows_per_group < tile_px && stat_rows_per_group % pass_px == 0));
        per_pass = per_pass || (ok && stat_rows_per_group < tile_px);       // (what c16w_stats_per_pass finds in the kernel)
      }
    }
    if (!ok && half_tile) { g6d_set_error("conv16_direct: Cout = 64 needs a halo tiling for every segment"); return G6D_EINVAL; }
    if (ok) {
      // a block = 4 waves of 128 px x 64 ch (pairs: 32 ch): one pixel tile x 256 (128) channels, or two pixel tiles x 128 channels
      const int cw = half_tile ? 32 : 32 * (math_mode == 3 ? C16W<3>::NT2 : C16W<2>::NT2);
      const int wm = Cout % (4 * cw) == 0 ? 1 : 2;
      p.ptiles = htiles;
      p.nN = Cout / (cw * (4 / wm));
      if (plan_only) return per_pass ? 2 : 1;
      const int hblocks = ((htiles + wm - 1) / wm + 7) / 8 * 8 * p.nN;
      auto launch = [&](auto kern, int main_lds, int ep_lds) {
        const int bytes = main_lds > ep_lds ? main_lds : ep_lds;
        g6d_allow_lds(reinterpret_cast<const void*>(kern), bytes);
        hipLaunchKernelGGL(kern, dim3(hblocks), dim3(256), bytes, st, p);
      };
#define C16W_LAUNCH(MM_, WM_) launch(&conv16w_kernel<MM_, WM_>, ((MM_ == 3 && WM_ == 2) ? 1 : 2) * WM_ * C16W<MM_>::NP * C16W<MM_>::PLANE, 4 * C16W<MM_>::EPW)
      if (half_tile && math_mode != 3) {
        if (math_mode == 1) launch(&conv16w_kernel<1, 2, 1>, 2 * 2 * C16W<1>::PLANE, 4 * C16W<1>::EPW);
        else launch(&conv16w_kernel<2, 2, 1>, 2 * 2 * C16W<2>::PLANE, 4 * C16W<2>::EPW);
      }
      else if (folded) {
        if (wm == 1) launch(&conv16w_kernel<3, 1, 1, 3>, 2 * C16W<3>::NP * C16W<3>::PLANE, 4 * C16W<3>::EPW);
        else launch(&conv16w_kernel<3, 2, 1, 3>, 2 * C16W<3>::NP * C16W<3>::PLANE, 4 * C16W<3>::EPW);      // (one stage of two tiles)
      }
      else if (math_mode == 1) { if (wm == 1) C16W_LAUNCH(1, 1); else C16W_LAUNCH(1, 2); }
      else if (math_mode == 2) { if (wm == 1) C16W_LAUNCH(2, 1); else C16W_LAUNCH(2, 2); }
      else { if (wm == 1) C16W_LAUNCH(3, 1); else C16W_LAUNCH(3, 2); }   // (two tiles per block: Cout = 64)
#undef C16W_LAUNCH
      return g6d_check_launch("conv16w_direct");
    }
  }
  if (folded) { g6d_set_error("conv16_direct: depth-folded filters run on the halo-patch kernel only (planes at least one tile high, statistics groups of whole volumes)"); return G6D_EINVAL; }
  if (half_tile) { g6d_set_error("conv16_direct: Cout = 64 runs on the halo-patch kernel only (knob conv16_halo, tile shapes)"); return G6D_EINVAL; }
  if (!pertap_stats_ok) { g6d_set_error("conv16_direct: statistics groups must be whole tile rows (small maps: whole 64-pixel epilogue passes)"); return G6D_EINVAL; }
  if (plan_only) return 0;
  const int blocks = (tiles + 7) / 8 * 8 * p.nN;
  if (w_layout == 0) {
    if (math_mode == 1) {
      g6d_allow_lds(reinterpret_cast<const void*>(&conv16_kernel<1>), C16_LDS);
      hipLaunchKernelGGL(conv16_kernel<1>, dim3(blocks), dim3(256), C16_LDS, st, p);
    } else {
      g6d_allow_lds(reinterpret_cast<const void*>(&conv16_kernel<2>), C16_LDS);
      hipLaunchKernelGGL(conv16_kernel<2>, dim3(blocks), dim3(256), C16_LDS, st, p);
    }
    return g6d_check_launch("conv16_direct");
  }
  constexpr int NST = 3, LDSR = NST * 16384;                   // three 16 KB stages (>= the epilogue's 38.9 KB tile)
  if (math_mode == 1) {
    g6d_allow_lds(reinterpret_cast<const void*>(&conv16r_kernel<1, NST>), LDSR);
    hipLaunchKernelGGL((conv16r_kernel<1, NST>), dim3(blocks), dim3(256), LDSR, st, p);
  } else if (math_mode == 2) {
    g6d_allow_lds(reinterpret_cast<const void*>(&conv16r_kernel<2, NST>), LDSR);
    hipLaunchKernelGGL((conv16r_kernel<2, NST>), dim3(blocks), dim3(256), LDSR, st, p);
  } else {
    g6d_allow_lds(reinterpret_cast<const void*>(&conv16r_kernel<3, NST>), LDSR);
    hipLaunchKernelGGL((conv16r_kernel<3, NST>), dim3(blocks), dim3(256), LDSR, st, p);
  }
  return g6d_check_launch("conv16r_direct");
}
}  // namespace

extern "C" int g6d_conv16_direct_multi_ex(const G6dConv16Seg* segs, int nseg, int Cin, const void* W16, int w_layout, float acc_scale,
                                          const float* bias, int Cout, int kd, int relu, int full_type, int pool_type, int math_mode, double* stats,
                                          int stat_rows_per_group, const G6dRange16* range, g6d_stream_t stream) {
  return c16_direct(segs, nseg, Cin, W16, w_layout, acc_scale, bias, Cout, kd, relu, full_type, pool_type, math_mode, stats, stat_rows_per_group, range,
                    stream, false);
}

extern "C" int g6d_conv16_direct_plan(const G6dConv16Seg* segs, int nseg, int Cin, const void* W16, int w_layout, int Cout, int kd, int full_type,
                                      int pool_type, int math_mode, double* stats, int stat_rows_per_group) {
  return c16_direct(segs, nseg, Cin, W16, w_layout, 1.f, nullptr, Cout, kd, 0, full_type, pool_type, math_mode, stats, stat_rows_per_group, nullptr,
                    nullptr, true);
}

extern "C" int g6d_conv16_direct_multi(const G6dConv16Seg* segs, int nseg, int Cin, const void* W16, int w_layout, float acc_scale,
                                       const float* bias, int Cout, int kd, int relu, int full_type, int pool_type, int math_mode, double* stats,
                                       int stat_rows_per_group, g6d_stream_t stream) {
  return g6d_conv16_direct_multi_ex(segs, nseg, Cin, W16, w_layout, acc_scale, bias, Cout, kd, relu, full_type, pool_type, math_mode, stats,
                                    stat_rows_per_group, nullptr, stream);
}
