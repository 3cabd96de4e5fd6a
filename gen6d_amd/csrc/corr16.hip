// corr16.hip — corr16_kernel: the detector's K x K correlation (K = 15, 7; reference network/detector.py:188-197,222-224: the query's
// feature map correlated with the 32 reference-centre features) on 16-bit activations — the halo-patch scheme of conv16w_kernel
// (conv16w.hip) with K^2 taps per patch.  Cout = 32 (the reference views), so a 128-pixel tile has ONE wave's worth of output
// channels: the block's NW = 11 computing waves (three per SIMD with the loader, 150 registers each) split the TAPS of every slice (wave w:
// taps w, w + NW, ...), each accumulates its partial 128 px x 32 ch sums over all slices, and the partials are added through LDS at the
// end.  One more wave requests the patches (see inside).  Every index below comes from corr16_geom.h, which the host tests.
//   * patch: (TH + K - 1) x (TW + K - 1) rows of 64 B, double-buffered (2 x 42 KB); a row holds TWO fragments at addr and addr ^ 32: the
//     two 16-channel groups of a 32-channel slice (MM = 1 / 2), or the hi and lo plane of a 16-channel slice (MM = 3: fp16 pairs,
//     fp32-class results) — the same LDS geometry, addressing and filter traffic in both arithmetics;
//   * filters: [slice][tap][2 fragments][64 lanes][8 values] (host: ops.corr16_pack), 2 KB per (slice, tap), straight into registers two
//     of the wave's taps ahead; a slice's K^2 x 2 KB are read by one wave each;
//   * per tap a wave issues 8 (MM = 3: 12) MFMAs, 8 ds_read_b128 (one fragment set, replaced m-tile by m-tile) and ~24 address VALUs.
#include "g6d_common.h"
#include "corr16_geom.h"
#include "pair16.h"

namespace {
namespace cg = corr16g;

struct Corr16Seg {
  const char* in; float* out;
  int H, W, rows, ld_in, ld_out;
  int tw_log2, tiles_x, tpi, tile0, swa, swd;                // cg::Tile and the segment's first tile
  unsigned in_bytes;
};
struct Corr16Params {
  Corr16Seg seg[4];
  int nseg, Cin, K, ptiles, nslice;
  const char* w;
  float acc_scale;
  G6dRange16 rng;                                            // slot_in: the input map's exponent
};

template <int MM>
__global__ __launch_bounds__(64 * (cg::NW + 1), 1) void corr16_kernel(const Corr16Params p) {
  constexpr int NW = cg::NW, NPL = cg::NPL;
  typedef typename C16T3<MM>::V V8;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ptile = blockIdx.x;
  int si = 0;
#pragma unroll
  for (int i = 1; i < 4; ++i) if (i < p.nseg && ptile >= p.seg[i].tile0) si = i;
  const Corr16Seg& sg = p.seg[si];
  const int tw_log2 = sg.tw_log2, K = p.K;
  const cg::Patch pt = cg::patch_of(tw_log2, K, sg.swa, sg.swd);
  const cg::Origin og = cg::tile_origin(pt, sg.tiles_x, sg.tpi, ptile - sg.tile0);
  const int nslice = p.nslice;
  typedef __attribute__((address_space(3))) void* lds_ptr;
  f32x16 acc[4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

  if (wv == NW) {
    // ---- THE LOADER WAVE.  LDS-DMA requests are not ordered against ordinary loads (a counted wait that budgeted a patch's pieces beside
    // the filter loads let MFMAs start on filters still in flight, once the filters missed L2: wrong tiles at random), and they share
    // the one vmcnt counter of their wave: the patches are therefore requested by a wave of their own, which does nothing else — its
    // vmcnt(0) before every barrier is exact — and the eleven computing waves count filter loads only.
    // piece k: patch pixels 16 k + lane / 4; physical slot lane & 3 holds the piece's logical slot L (cg::piece_of, cg::slot_bytes)
    unsigned poff[NPL];
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      const cg::Piece pc = cg::piece_of(pt, og, k, lane);
      const long px = ((long)og.n * sg.H + pc.y) * sg.W + pc.x;
      poff[k] = pc.in_patch && cg::in_map(pc, sg.H, sg.W) ? (unsigned)(px * sg.ld_in * 2) + cg::slot_bytes(pc.L, MM == 3, p.Cin) : C16_OOB;
    }
    const __amdgpu_buffer_rsrc_t rs_in = c16_rsrc(sg.in, sg.in_bytes);
    auto issue_patch = [&](int c, int stage) {
      const unsigned ck = (unsigned)(c * (MM == 3 ? 32 : 64));
#pragma unroll
      for (int k = 0; k < NPL; ++k)
        if (k < pt.NI) {
          const unsigned vo = poff[k] == C16_OOB ? C16_OOB : poff[k] + ck;
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_in, (lds_ptr)(lds + stage * cg::STAGE + k * cg::PIECE), 16, vo, 0, 0, 0);
        }
    };
    issue_patch(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                              // patch 0 is in place
#pragma unroll 1
    for (int c = 0; c < nslice; ++c) {
      if (c + 1 < nslice) issue_patch(c + 1, (c + 1) & 1);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();                            // slice c has been read by every wave, patch c + 1 is in place
    }
  } else {
  // ---- filters: the wave's taps of every slice in order; running pointer, + NW taps per step, past the end a harmless reload
  const int ntw = cg::wave_taps(K, wv);                       // taps of this wave per slice
  const char* wp = p.w + (long)wv * cg::TAP_BYTES;
  int wtap = wv, wleft = nslice * ntw;
  const unsigned bvo = lane * 16;
  auto load_b = [&](V8 (&b)[2]) {
    const unsigned long wa = (unsigned long)(wleft > 0 ? wp : p.w);
    const char* ws = reinterpret_cast<const char*>((unsigned long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)wa) |
                                                   ((unsigned long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(wa >> 32)) << 32));
    asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(b[0]) : "v"(bvo), "s"(ws) : "memory");
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:1024" : "=v"(b[1]) : "v"(bvo), "s"(ws) : "memory");
    --wleft;
    wp += cg::filter_advance(K, wv, wtap);
  };

  // ---- fragment geometry: m-tile mt = tile pixels 32 mt + (lane & 31); patch row of tap (0, 0) = the pixel's own (row, column).
  // fe carries the swizzle's row term through the shift by swa in tap_addr: sound because swd = 1 only with swa = 0 (cg::pick_tile)
  const int fhalf = lane >> 5;
  int qb[4], fe[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) cg::frag_base(pt, 32 * mt + (lane & 31), qb[mt], fe[mt]);
  auto tap_addr = [&](int ky, int kx, int stage, int (&tb)[4]) {
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) tb[mt] = cg::tap_addr(pt, qb[mt], fe[mt], fhalf, ky, kx, stage);
  };
  V8 bs[cg::RING][2];
  V8 fa[4][2];
  int tb[4], ntb[4];
  load_b(bs[0]);
  load_b(bs[1]);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  int ky0, kx0;                                               // the wave's first tap of a slice
  cg::first_tap(K, wv, ky0, kx0);
  int ky = ky0, kx = kx0;
  tap_addr(ky, kx, 0, tb);
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    fa[mt][0] = *reinterpret_cast<const V8*>(lds + tb[mt]);
    fa[mt][1] = *reinterpret_cast<const V8*>(lds + (tb[mt] ^ 32));
  }
  int stage = 0, it = 0, c = 0;                               // tap index of the wave inside the slice, slice
  // One tap.  The filter ring runs through all slices without a break (period 3: the loop below is unrolled by three steps, slice
  // boundaries are run-time state); the filters of the wave's tap after next are requested first.  Filter loads return in order and are
  // the only requests of this wave: vmcnt(4) — the two younger sets — proves this step's filters have arrived.
  auto step = [&](const V8 (&bc)[2], V8 (&bfar)[2]) {
    const bool live = c < nslice, last = it == ntw - 1;
    load_b(bfar);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (!live) return;                                        // (padding steps after the last slice: the step count is a multiple of three)
    int nky = ky, nkx = kx;
    cg::next_tap(K, nky, nkx);
    if (last) { nky = ky0; nkx = kx0; }
    tap_addr(nky, nkx, last ? stage ^ 1 : stage, ntb);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      if constexpr (MM == 3) {
        acc[mt] = c16_mfma<MM>(fa[mt][0], bc[0], acc[mt]);      // hi x hi
        acc[mt] = c16_mfma<MM>(fa[mt][0], bc[1], acc[mt]);      // hi x lo
        acc[mt] = c16_mfma<MM>(fa[mt][1], bc[0], acc[mt]);      // lo x hi
      } else {
        acc[mt] = c16_mfma<MM>(fa[mt][0], bc[0], acc[mt]);      // channels 0..15 of the slice
        acc[mt] = c16_mfma<MM>(fa[mt][1], bc[1], acc[mt]);      // channels 16..31
      }
      if (!last) {
        fa[mt][0] = *reinterpret_cast<const V8*>(lds + ntb[mt]);
        fa[mt][1] = *reinterpret_cast<const V8*>(lds + (ntb[mt] ^ 32));
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    ky = nky; kx = nkx;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) tb[mt] = ntb[mt];
    ++it;
    if (last) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();                          // every wave has read this patch; the loader has the next one in place
      __builtin_amdgcn_sched_barrier(0);
      stage ^= 1; it = 0; ++c;
      if (c < nslice) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
          fa[mt][0] = *reinterpret_cast<const V8*>(lds + tb[mt]);
          fa[mt][1] = *reinterpret_cast<const V8*>(lds + (tb[mt] ^ 32));
        }
      }
    }
  };
  const int nsteps = nslice * ntw;
#pragma unroll 1
  for (int s_ = 0; s_ < nsteps; s_ += cg::RING) {
    asm volatile("" : "+v"(fe[0]), "+v"(fe[1]), "+v"(fe[2]), "+v"(fe[3]));
    step(bs[0], bs[2]);
    step(bs[1], bs[0]);
    step(bs[2], bs[1]);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);

  // ---- the eleven partial tiles are added through LDS, four at a time: [slot][128 px][33]
  constexpr int LD = cg::RED_LD;
  float* red = reinterpret_cast<float*>(lds);
  float sum[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) sum[e] = 0.f;
#pragma unroll 1
  for (int rd = 0; rd < (NW + 3) / 4; ++rd) {
    if (wv < NW && (wv >> 2) == rd) {
      float* mine = red + (wv & 3) * (cg::BM * LD);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) mine[(32 * mt + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * LD + (lane & 31)] = acc[mt][r];
    }
    __syncthreads();
    if (wv < 8)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int o = tid + 512 * e, px = o >> 5, ch = o & 31;
      const int ns = NW - 4 * rd < 4 ? NW - 4 * rd : 4;        // partial tiles written in this round
      for (int sl = 0; sl < ns; ++sl) sum[e] += red[sl * cg::BM * LD + px * LD + ch];
    }
    __syncthreads();
  }
  const float as = ldexpf(p.acc_scale, g6d_exp_in(p.rng));     // pair input held as x * 2^-e_in
  if (wv < 8)
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int o = tid + 512 * e, px = o >> 5, ch = o & 31;
    const int y = og.y0 + (px >> tw_log2), x = og.x0 + (px & ((1 << tw_log2) - 1));
    if (y < sg.H && x < sg.W) sg.out[(((long)og.n * sg.H + y) * sg.W + x) * sg.ld_out + ch] = sum[e] * as;
  }
}
}  // namespace

extern "C" int g6d_corr16_multi_ex(const G6dConv16Seg* segs, int nseg, int Cin, const void* W16, float acc_scale, int Cout, int k, int math_mode,
                                   const G6dRange16* range, g6d_stream_t stream) {
  if (!segs || nseg < 1 || nseg > 4 || !W16) { g6d_set_error("corr16: 1..4 segments and filters expected"); return G6D_EINVAL; }
  if (Cin < 1 || !g6d_aligned16(W16)) { g6d_set_error("corr16: bad args (Cin >= 1, 16-byte aligned filters)"); return G6D_EINVAL; }
  if (math_mode < 1 || math_mode > 3 || Cout != 32 || (k != 15 && k != 7) || Cin % 32) {
    g6d_set_error("corr16: math_mode 1 (bf16) / 2 (fp16) / 3 (fp16 pairs), Cout = 32, k in {7, 15}, Cin % 32 == 0 expected"); return G6D_EINVAL;
  }
  const int planes = math_mode == 3 ? 2 : 1;
  Corr16Params p = {};
  p.nseg = nseg; p.Cin = Cin; p.K = k; p.w = static_cast<const char*>(W16); p.acc_scale = acc_scale != 0.f ? acc_scale : 1.f;
  p.nslice = Cin / (math_mode == 3 ? 16 : 32);
  if (range) p.rng = *range;
  int tiles = 0;
  for (int i = 0; i < nseg; ++i) {
    const G6dConv16Seg& s = segs[i];
    Corr16Seg& o = p.seg[i];
    if (!s.in || !s.out_full || s.N < 1 || s.D != 1 || s.H < 1 || s.W < 1 || s.ld_in < planes * Cin || s.ld_full < Cout || (s.ld_in & 7) ||
        !g6d_aligned16(s.in) || !g6d_aligned16(s.out_full)) { g6d_set_error("corr16: bad segment"); return G6D_EINVAL; }
    const cg::Tile tl = cg::pick_tile(s.H, s.W, k);
    // (k in {7, 15} always finds a tile: tests/test_corr16_geom_cpu.py; the branch guards a future k)
    if (tl.tw_log2 < 0) { g6d_set_error("corr16: no tile shape fits"); return G6D_EINVAL; }
    o.in = static_cast<const char*>(s.in); o.out = static_cast<float*>(s.out_full);
    o.H = s.H; o.W = s.W; o.rows = s.N * s.H; o.ld_in = s.ld_in; o.ld_out = s.ld_full;
    o.tw_log2 = tl.tw_log2; o.tiles_x = tl.tiles_x; o.tpi = tl.tpi; o.tile0 = tiles; o.swa = tl.swa; o.swd = tl.swd;
    const long ext = (long)s.N * s.H * s.W * s.ld_in * 2;
    if (ext >= (1L << 31)) { g6d_set_error("corr16: a segment's input beyond 2 GB"); return G6D_EINVAL; }
    o.in_bytes = (unsigned)ext;
    tiles += s.N * o.tpi;
  }
  p.ptiles = tiles;
  hipStream_t st = static_cast<hipStream_t>(stream);
  constexpr int LDSB = cg::LDS_BYTES, NT = 64 * (cg::NW + 1);
  if (math_mode == 1) {
    g6d_allow_lds(reinterpret_cast<const void*>(&corr16_kernel<1>), LDSB);
    hipLaunchKernelGGL(corr16_kernel<1>, dim3(tiles), dim3(NT), LDSB, st, p);
  } else if (math_mode == 2) {
    g6d_allow_lds(reinterpret_cast<const void*>(&corr16_kernel<2>), LDSB);
    hipLaunchKernelGGL(corr16_kernel<2>, dim3(tiles), dim3(NT), LDSB, st, p);
  } else {
    g6d_allow_lds(reinterpret_cast<const void*>(&corr16_kernel<3>), LDSB);
    hipLaunchKernelGGL(corr16_kernel<3>, dim3(tiles), dim3(NT), LDSB, st, p);
  }
  return g6d_check_launch("corr16");
}

extern "C" int g6d_corr16_multi(const G6dConv16Seg* segs, int nseg, int Cin, const void* W16, float acc_scale, int Cout, int k, int math_mode,
                                g6d_stream_t stream) {
  return g6d_corr16_multi_ex(segs, nseg, Cin, W16, acc_scale, Cout, k, math_mode, nullptr, stream);
}
