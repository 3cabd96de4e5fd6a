// conv16w.hip — conv16w_kernel: the HALO-PATCH kernel of the direct 16-bit convolution (conv16_direct.hip: the family and its launcher;
// 2-D layers, and 3x3x3 layers with the depth taps folded).  Measured on the per-tap kernels (conv16_tap.hip, tools/conv16_ablate.py): without the
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
// timing experiments only (WRONG results), a compile-time switch (make FLAGS_conv16w=-DC16W_ABLATE=n): after the first slice, bit 0 = no
// patch requests, bit 1 = no filter requests, bit 2 = no fragment reads
#include "conv16_common.h"

#ifndef C16W_ABLATE
#define C16W_ABLATE 0
#endif

namespace {

template <int MM> struct C16W {
  static constexpr int NP = MM == 3 ? 2 : 1, KS = 2, NI_MAX = 18;             // planes, 16-channel groups per slice, DMA pieces per plane at most
  static constexpr int PLANE = NI_MAX * 1024;                                   // 288 patch rows of 64 B
  static constexpr int NT2 = MM == 3 ? 1 : 2;                                   // 32-channel accumulator tiles per wave (a wave = 128 px x 32 NT2 ch)
  static constexpr int NBL = KS * NP * NT2;                                     // filter loads per tap and wave
  static constexpr int NPX = 64;                                                // pixels per epilogue pass
  static constexpr int EPW = NPX * C16_EP_LD * 4;                               // a wave's epilogue tile
};
// LDS of conv16w_kernel<MM, WM, ., .>: the patch stages of its WM tiles, and what a block asks for — the stages, or the four waves'
// epilogue tiles where those are larger
template <int MM, int WM> struct C16WLds {
  static constexpr bool SINGLE = MM == 3 && WM == 2;                            // one patch stage instead of two (see the slice hand-over in the kernel)
  static constexpr int TILE_B = C16W<MM>::NP * C16W<MM>::PLANE, STAGE = WM * TILE_B;
  static constexpr int MAIN = (SINGLE ? 1 : 2) * STAGE, EP = 4 * C16W<MM>::EPW, BYTES = MAIN > EP ? MAIN : EP;
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
  constexpr bool SINGLE = C16WLds<MM, WM>::SINGLE;             // one patch stage instead of two (see the slice hand-over below)
  constexpr int TILE_B = C16WLds<MM, WM>::TILE_B, STAGE = C16WLds<MM, WM>::STAGE;
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
    // feeds one MFMA per (16-channel n-tile, term).  The pair tilings have swd = 0 and swa <= 2 (c16g::halo_tiling): the slot swizzle
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
    // slot swizzle of patch (row, column): ((column >> swa) + row * swd) & 3, and swd != 0 only with swa == 0 (c16g::halo_tiling): with
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

template <int MM, int WM, int NT2 = C16W<MM>::NT2, int KD = 1>
void c16w_go(const c16::Params& p, int blocks, hipStream_t st) {
  constexpr int bytes = C16WLds<MM, WM>::BYTES;
  g6d_allow_lds(reinterpret_cast<const void*>(&conv16w_kernel<MM, WM, NT2, KD>), bytes);
  hipLaunchKernelGGL((conv16w_kernel<MM, WM, NT2, KD>), dim3(blocks), dim3(256), bytes, st, C16Params{p});
}
// A block that asks for too little LDS faults on the GPU, so C16WLds::BYTES is held at compile time to the sizes the launcher spelled
// out per instantiation before the formula was one: two stages of WM tiles (pairs with WM = 2: one), or the epilogue tiles.
constexpr int c16w_max(int a, int b) { return a > b ? a : b; }
static_assert(C16WLds<1, 1>::BYTES == c16w_max(2 * 1 * C16W<1>::NP * C16W<1>::PLANE, 4 * C16W<1>::EPW) && C16WLds<1, 1>::BYTES == 69632, "conv16w_kernel<1, 1, 2, 1>");
static_assert(C16WLds<2, 1>::BYTES == c16w_max(2 * 1 * C16W<2>::NP * C16W<2>::PLANE, 4 * C16W<2>::EPW) && C16WLds<2, 1>::BYTES == 69632, "conv16w_kernel<2, 1, 2, 1>");
static_assert(C16WLds<1, 2>::BYTES == c16w_max(2 * 2 * C16W<1>::NP * C16W<1>::PLANE, 4 * C16W<1>::EPW) && C16WLds<1, 2>::BYTES == 73728, "conv16w_kernel<1, 2, 2, 1>");
static_assert(C16WLds<2, 2>::BYTES == c16w_max(2 * 2 * C16W<2>::NP * C16W<2>::PLANE, 4 * C16W<2>::EPW) && C16WLds<2, 2>::BYTES == 73728, "conv16w_kernel<2, 2, 2, 1>");
static_assert(C16WLds<1, 2>::BYTES == c16w_max(2 * 2 * C16W<1>::PLANE, 4 * C16W<1>::EPW), "conv16w_kernel<1, 2, 1, 1> (Cout = 64)");
static_assert(C16WLds<2, 2>::BYTES == c16w_max(2 * 2 * C16W<2>::PLANE, 4 * C16W<2>::EPW), "conv16w_kernel<2, 2, 1, 1> (Cout = 64)");
static_assert(C16WLds<3, 1>::BYTES == c16w_max(2 * 1 * C16W<3>::NP * C16W<3>::PLANE, 4 * C16W<3>::EPW) && C16WLds<3, 1>::BYTES == 73728, "conv16w_kernel<3, 1, 1, 1>");
static_assert(C16WLds<3, 2>::BYTES == c16w_max(1 * 2 * C16W<3>::NP * C16W<3>::PLANE, 4 * C16W<3>::EPW) && C16WLds<3, 2>::BYTES == 73728, "conv16w_kernel<3, 2, 1, 1>");
static_assert(C16WLds<3, 1>::BYTES == c16w_max(2 * C16W<3>::NP * C16W<3>::PLANE, 4 * C16W<3>::EPW), "conv16w_kernel<3, 1, 1, 3> (folded)");
static_assert(C16WLds<3, 2>::BYTES == c16w_max(2 * C16W<3>::NP * C16W<3>::PLANE, 4 * C16W<3>::EPW), "conv16w_kernel<3, 2, 1, 3> (folded: one stage of two tiles)");

}  // namespace

C16wAdmit c16w_admit(c16::Params& p, const G6dConv16Seg* segs, bool pairs, bool folded) {
  C16wAdmit a = {true, false, 0};
  const int srg = p.stat_rows_per_group;
  const bool grouped = p.stats && srg > 0;
  for (int i = 0; i < p.nseg && a.ok; ++i) {
    const G6dConv16Seg& s = segs[i];
    C16Seg& o = p.seg[i];
    int nt_ = 0;
    // folded: the planes of the volumes are the images of the tiling, and a tile lies inside one plane
    a.ok = folded ? (long)s.N * s.D < (1L << 31) && c16g::halo_tiling(s.N * s.D, s.H, s.W, true, true, o, nt_)
                  : c16g::halo_tiling(s.N, s.H, s.W, pairs, false, o, nt_);
    o.h_tile0 = a.tiles; a.tiles += nt_;
    if (!grouped || !a.ok) continue;
    if (folded) { a.ok = srg % ((long)s.D * s.H * s.W) == 0; continue; }     // statistics groups are whole volumes
    const int th = C16_BM >> o.h_tw_log2;
    // groups are whole images.  In-image tiles then lie inside one group; a banded tile (whole small images) does when the group is
    // whole tiles, or else spans groups of whole epilogue passes (flushed per pass).  A group smaller than a pass, or not aligned to
    // one, has no place to be summed: no halo tiling, and the per-tap kernels reject it too
    const long tile_px = (long)th * s.W, pass_px = (long)(C16W<3>::NPX >> o.h_tw_log2) * s.W;
    static_assert(C16W<1>::NPX == C16W<3>::NPX && C16W<2>::NPX == C16W<3>::NPX, "one pass size in every mode");
    a.ok = (srg % (s.H * s.W) == 0) && (o.h_tpi > 0 || srg % tile_px == 0 || (srg < tile_px && srg % pass_px == 0));
    a.per_pass = a.per_pass || (a.ok && srg < tile_px);                       // (what c16w_stats_per_pass finds in the kernel)
  }
  return a;
}

int c16w_launch(const c16::Params& p, int math_mode, int wm, bool half_tile, bool folded, hipStream_t stream) {
  const int blocks = c16::halo_grid(p, wm);
  if (half_tile && math_mode != 3) {                           // Cout = 64 in a 16-bit mode: 32-channel waves
    if (math_mode == 1) c16w_go<1, 2, 1>(p, blocks, stream);
    else c16w_go<2, 2, 1>(p, blocks, stream);
  } else if (folded) {
    if (wm == 1) c16w_go<3, 1, 1, 3>(p, blocks, stream);
    else c16w_go<3, 2, 1, 3>(p, blocks, stream);
  } else if (math_mode == 1) {
    if (wm == 1) c16w_go<1, 1>(p, blocks, stream); else c16w_go<1, 2>(p, blocks, stream);
  } else if (math_mode == 2) {
    if (wm == 1) c16w_go<2, 1>(p, blocks, stream); else c16w_go<2, 2>(p, blocks, stream);
  } else {
    if (wm == 1) c16w_go<3, 1>(p, blocks, stream); else c16w_go<3, 2>(p, blocks, stream);   // (two tiles per block: Cout = 64)
  }
  return g6d_check_launch("conv16w_direct");
}
