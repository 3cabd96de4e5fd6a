// The 16-bit kernels of the Winograd F(2x2,3x3) family (wino_conv.hip: the formulation, the fp32 kernel, the launcher wino_run and the
// entry points): wino16_conv3x3_kernel and wino16b_conv3x3_kernel for the trunks, wino16_conv_kernel for the conv family, their shared
// epilogue and wino16_launch, which picks among them.
//
// Reduced-precision trunk (G6dConv.math_mode semantics: 1 = bf16, 2 = fp16 operands, fp32 accumulation; opt-in speed mode, graded
// separately): the same F(2x2,3x3) formulation on v_mfma_f32_32x32x16_{bf16,f16}.  One K step of that instruction is 16 input
// channels, so a chunk is a PAIR of the fp32 kernel's 8-channel chunks:
//   raw patch  two 8-channel planes, each in the conflict-free layout of the fp32 kernel; lane half h transforms plane h (all 8 of
//              its channels: two 16-byte reads per patch position), in fp32 registers, and rounds the transformed values to the
//              operand type when they are packed into the A operand (8 values = channels 16 c + 8 h .. + 7);
//   filters    transformed and ROUNDED ON THE HOST: U16[chunk][ab][co][16] in the operand type, 32 bytes per (ab, co) row — the same
//              row size as the fp32 image, so the direct-to-LDS copy, the swizzle (halves swapped for co & 8) and the fragment read
//              (one ds_read_b128 = the 8 channels of lane half h) are unchanged, and a chunk pair fits the 32 KB filter slot;
//   MFMAs      16 per chunk (one per (a,b) position) of 8 passes instead of 2 x 64 of 16 passes: the loop is bound by the input
//              transform (~200 vector instructions) and by streaming 58 KB per chunk into LDS, not by the matrix pipe.
// Epilogue as the fp32 trunk kernel (output transform, bias, ReLU, full / pooled fp32 outputs, chunk split with in-kernel hand-off).
#include "wino_common.h"
#include <type_traits>

namespace {

__device__ __forceinline__ f32x4 ldg4(const float* __restrict__ base, int elem_off) {
  return *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(base) + ((unsigned)elem_off << 2));
}

// Epilogue shared by the 16-bit kernels (the fp32 kernel keeps its own, identical copy inline: it is scheduled by hand): output
// transform A^T D A, chunk-split hand-off, bias, ReLU, full / pooled stores, per-(group, channel) statistics and their finalisation.
template <int THREADS, int NWN>
__device__ __forceinline__ void wino_epilogue(const WinoArgs& p, f32x16 (&acc)[16], float* lds, int tid, int wm, int wn, int li, int lh, int n0) {
  const int co = n0 + wn * 32 + li;
  f32x4 Y[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float sr[2][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sr[0][j] = acc[0 + j][r] + acc[4 + j][r] + acc[8 + j][r];
      sr[1][j] = acc[4 + j][r] - acc[8 + j][r] - acc[12 + j][r];
    }
    Y[r] = f32x4{sr[0][0] + sr[0][1] + sr[0][2], sr[0][1] - sr[0][2] - sr[0][3], sr[1][0] + sr[1][1] + sr[1][2], sr[1][1] - sr[1][2] - sr[1][3]};
  }
  if (p.splits > 1) {
    constexpr int TILE = THREADS * 64;
    const int ntiles = gridDim.x * gridDim.y, tile = blockIdx.y * gridDim.x + blockIdx.x;
    float* part = p.ws + G6D_WS_COUNTERS + (size_t)tile * TILE + tid * 4;
    const size_t zstride = (size_t)ntiles * TILE;
#pragma unroll
    for (int r = 0; r < 16; ++r) g6d_store_wt(part + blockIdx.z * zstride + r * (THREADS * 4), Y[r]);
    if (!g6d_split_arrive(reinterpret_cast<int*>(p.ws) + tile, p.splits, reinterpret_cast<int*>(lds))) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) Y[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int z = 0; z < p.splits; ++z) {
      f32x4 v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] = *reinterpret_cast<const f32x4*>(part + (size_t)z * zstride + r * (THREADS * 4));
#pragma unroll
      for (int r = 0; r < 16; ++r) Y[r] += v[r];
    }
  }
  const float bv = p.bias ? p.bias[co] : 0.f;
  const bool do_relu = p.relu != 0;
  const bool do_stats = p.stats != nullptr;
  const QGeo geo[2] = {quarter_of(p, 2 * wm), quarter_of(p, 2 * wm + 1)};
  float st1[2] = {0.f, 0.f}, st2[2] = {0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const QGeo& g = geo[r >> 3];
    const int tyy = lh + 2 * ((r >> 2) & 1), txx = r & 3;
    const int n = g.n; const bool qv = g.valid;
    const int Hp = g.H >> 1, Wp = g.W >> 1;
    float y[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        y[a][b] = Y[r][2 * a + b] + bv;
        if (do_relu) y[a][b] = fmaxf(y[a][b], 0.f);
      }
    const int oy = g.oy0 + 2 * tyy, ox = g.ox0 + 2 * txx;
    if (p.out_full && qv) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
          if (oy + a < g.H && ox + b < g.W) {
            p.out_full[(size_t)g.full_off + ((size_t)(n * g.H + oy + a) * g.W + ox + b) * g.ld_full + co] = y[a][b];
            if (do_stats) { st1[r >> 3] += y[a][b]; st2[r >> 3] += y[a][b] * y[a][b]; }
          }
    }
    if (p.out_pool && qv) {
      const int py = oy >> 1, px = ox >> 1;
      if (py < Hp && px < Wp)
        p.out_pool[(size_t)g.pool_off + ((size_t)(n * Hp + py) * Wp + px) * g.ld_pool + co] = fmaxf(fmaxf(y[0][0], y[0][1]), fmaxf(y[1][0], y[1][1]));
    }
  }
  if (do_stats) {
    float* sred = lds;
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      st1[h] += __shfl_xor(st1[h], 32, 64);
      st2[h] += __shfl_xor(st2[h], 32, 64);
      if (lh == 0) {
        sred[((2 * wm + h) * 32 * NWN + wn * 32 + li) * 2] = st1[h];
        sred[((2 * wm + h) * 32 * NWN + wn * 32 + li) * 2 + 1] = st2[h];
      }
    }
    __syncthreads();
    if (tid < 32 * NWN) {
      double a1 = 0.0, a2 = 0.0;
      int cur = -1;
      for (int q = 0; q < 4; ++q) {
        const QGeo qg = quarter_of(p, q);
        if (!qg.valid) break;
        const int g = p.stats_div > 0 ? (qg.n / p.D) / p.stats_div : 0;
        if (g != cur && cur >= 0) {
          double* st = p.stats + ((size_t)cur * p.Cout + n0 + tid) * 2;
          atomicAdd(st, a1); atomicAdd(st + 1, a2); a1 = a2 = 0.0;
        }
        cur = g;
        a1 += (double)sred[(q * 32 * NWN + tid) * 2];
        a2 += (double)sred[(q * 32 * NWN + tid) * 2 + 1];
      }
      if (cur >= 0) {
        double* st = p.stats + ((size_t)cur * p.Cout + n0 + tid) * 2;
        atomicAdd(st, a1); atomicAdd(st + 1, a2);
      }
    }
    if (p.fin.scale) {
      __syncthreads();
      g6d_finalize_stats(p.fin, gridDim.x * gridDim.y, reinterpret_cast<int*>(lds));
    }
  }
}

typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
template <typename T> __device__ __forceinline__ auto a8_dummy(T a, T b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7); }
typedef __bf16 b16x4 __attribute__((ext_vector_type(4)));

template <int MM, int NWN>
__global__ void __launch_bounds__(128 * NWN, 1) wino16_conv3x3_kernel(const WinoArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int THREADS = 128 * NWN;
  constexpr int NPR = (1600 + THREADS - 1) / THREADS;         // 16-byte raw pieces per thread and chunk: 2 planes x 4 quarters x 100 x 2
  constexpr int WU_FLOATS = 16 * 32 * NWN * 8;                // [ab][co][16 x 2 bytes]
  constexpr int WSTAGE = 2 * WRAW_FLOATS + WU_FLOATS + 4 * THREADS;
  using hv4 = typename std::conditional<MM == 1, b16x4, h16x4>::type;
  using hv8 = typename std::conditional<MM == 1, bf16x8, f16x8>::type;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / NWN, wn = wave % NWN;
  const int li = lane & 31, lh = lane >> 5;
  const int n0 = blockIdx.y * (32 * NWN);
  const int nc16 = p.Cin >> 4;
  const int c_first = blockIdx.z * p.chunks_per_split;
  const int c_last = min(nc16, c_first + p.chunks_per_split) - 1;

  unsigned pboff[NPR]; int lsto[NPR];
#pragma unroll
  for (int j = 0; j < NPR; ++j) {
    const int idx = tid + THREADS * j;
    const int plane = idx / 800, r0 = idx - plane * 800;
    const int q = r0 / 200, r = r0 - q * 200, pp = r >> 1, half = r & 1;
    const int py = pp / 10, px = pp - py * 10;
    const QGeo g = quarter_of(p, q < 4 ? q : 0);
    const int iy = g.oy0 + py - 1, ix = g.ox0 + px - 1;
    const bool v = (idx < 1600) & g.valid & ((unsigned)iy < (unsigned)g.H) & ((unsigned)ix < (unsigned)g.W);
    pboff[j] = v ? (unsigned)(g.in_off + ((g.n * g.H + iy) * g.W + ix) * g.ld_in + 8 * plane + 4 * half) << 2 : 0x80000000u;
    lsto[j] = idx < 1600 ? plane * WRAW_FLOATS + (q * WQ_PIX + pp) * WRAW_LD + 4 * (half ^ ((py >> 1) & 1))
                         : 2 * WRAW_FLOATS + WU_FLOATS + 4 * tid;
  }
  const auto in_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in), 0, p.in_bytes, 0x00020000);
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  f32x4 rp[NPR];
  auto load_raw = [&](int chunk) {
#pragma unroll
    for (int j = 0; j < NPR; ++j)
      rp[j] = __builtin_bit_cast(f32x4, __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(in_rsrc, pboff[j], chunk * 64, 0)));
  };
  auto store_raw = [&](int st) {
#pragma unroll
    for (int j = 0; j < NPR; ++j)
      *reinterpret_cast<f32x4*>(__builtin_assume_aligned(lds + st * WSTAGE + lsto[j], 16)) = rp[j];
  };
  const char* ubase = reinterpret_cast<const char*>(p.U) + (size_t)n0 * 32;       // 32 bytes per (ab, co) row
  const unsigned lane16 = lane * 16;
  const unsigned lds_addr0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)lds;
  auto glds = [&](int chunk, int st, int idx) {
    const int ab = idx / NWN, h = idx % NWN;
    const char* g = ubase + (size_t)chunk * ((size_t)p.Cout * 512) + (unsigned)((ab * p.Cout + h * 32) * 32);
    const unsigned dst = __builtin_amdgcn_readfirstlane(lds_addr0 + 4u * (unsigned)(st * WSTAGE + 2 * WRAW_FLOATS + (ab * 32 * NWN + h * 32) * 8));
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane16), "s"(g), "s"(dst) : "memory");
  };
  auto load_u = [&](int chunk, int st) {
#pragma unroll
    for (int k = 0; k < 8; ++k) glds(chunk, st, wave * 8 + k);
  };
  const int tl = li & 15, ty = tl >> 2, tx = tl & 3;
  const int apos = lh * WRAW_FLOATS + ((2 * wm + (li >> 4)) * WQ_PIX + (2 * ty) * 10 + 2 * tx) * WRAW_LD;     // lane half h reads plane h
  const int bbase = 2 * WRAW_FLOATS + (wn * 32 + li) * 8 + 4 * (lh ^ ((li >> 3) & 1));
  constexpr int USTRIDE = 32 * NWN * 8;

  f32x16 acc[16];
#pragma unroll
  for (int a = 0; a < 16; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

  load_u(c_first, 0);
  load_raw(c_first);
  store_raw(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // V = B^T d B of (a,b) group `grp` on 4 channels (the fp32 kernel's transform)
  auto xform = [&](int grp, const f32x4 (&dd)[4][4], f32x4 (&vv)[4]) {
    f32x2 rl[4], rh[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 &a = dd[grp == 0 ? 0 : grp == 2 ? 2 : 1][q], &b = dd[grp == 0 ? 2 : grp == 1 ? 2 : grp == 2 ? 1 : 3][q];
      if (grp == 1) { rl[q] = pk_add(lo2(a), lo2(b)); rh[q] = pk_add(hi2(a), hi2(b)); }
      else { rl[q] = pk_sub(lo2(a), lo2(b)); rh[q] = pk_sub(hi2(a), hi2(b)); }
    }
    vv[0] = cat2(pk_sub(rl[0], rl[2]), pk_sub(rh[0], rh[2]));
    vv[1] = cat2(pk_add(rl[1], rl[2]), pk_add(rh[1], rh[2]));
    vv[2] = cat2(pk_sub(rl[2], rl[1]), pk_sub(rh[2], rh[1]));
    vv[3] = cat2(pk_sub(rl[1], rl[3]), pk_sub(rh[1], rh[3]));
  };

  for (int cc = c_first; cc <= c_last; ++cc) {
    const int c = cc - c_first;
    const float* S = lds + (c & 1) * WSTAGE;
    if (cc < c_last && !WABL(2)) {                // the copies of the next chunk first (they must be older than the loads hipcc counts)
      load_u(cc + 1, (c & 1) ^ 1);
      load_raw(cc + 1);
    }
    hv4 vh[16][2];                                // transformed patch, rounded: [a*4 + b][4-channel half of the lane's plane]
#pragma unroll
    for (int hs = 0; hs < 2; ++hs) {
      f32x4 d[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (!WABL(4) || cc == c_first) d[i][j] = *reinterpret_cast<const f32x4*>(S + apos + 4 * (hs ^ (ty & 1) ^ (i >> 1)) + (i * 10 + j) * WRAW_LD);
#pragma unroll
      for (int grp = 0; grp < 4; ++grp) {
        f32x4 v[4];
        if (WABL(3)) {
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = d[grp][q];
        } else
        xform(grp, d, v);
#pragma unroll
        for (int q = 0; q < 4; ++q) vh[grp * 4 + q][hs] = __builtin_convertvector(v[q], hv4);
      }
    }
#pragma unroll
    for (int ab = 0; ab < 16; ++ab) {
      f32x4 uraw;
      if (WABL(4)) uraw = __builtin_bit_cast(f32x4, a8_dummy(vh[ab][0], vh[ab][1])); else
      uraw = *reinterpret_cast<const f32x4*>(S + bbase + ab * USTRIDE);
      const hv8 a8 = __builtin_shufflevector(vh[ab][0], vh[ab][1], 0, 1, 2, 3, 4, 5, 6, 7);
      const hv8 b8 = __builtin_bit_cast(hv8, uraw);
      if (WINO_ABLATE == 6) { acc[ab][0] += __builtin_bit_cast(f32x4, a8)[0] * __builtin_bit_cast(f32x4, b8)[1]; continue; }
      if constexpr (MM == 1) acc[ab] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a8, b8, acc[ab], 0, 0, 0);
      else acc[ab] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a8, b8, acc[ab], 0, 0, 0);
    }
    if (cc < c_last && !WABL(2)) store_raw((c & 1) ^ 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (!WABL(1)) __syncthreads();
  }

  wino_epilogue<THREADS, NWN>(p, acc, lds, tid, wm, wn, li, lh, n0);
}

// Two waves per SIMD for the 16-bit trunk (MODE 0, 2-D, un-split launches): with one 512-register wave per SIMD the chunk of
// wino16_conv3x3_kernel costs ~8x its matrix-core time because nothing overlaps (ablation table).  Here a block is 512
// threads = 8 waves with 128 accumulator registers each: the 16 (a,b) positions of a 32-tile x 32-channel output tile are split
// over two waves (a < 2 / a >= 2), the input transform is done ONCE per tile (the 2 x 2 kernel does it in both channel waves) by
// 512 work items (tile, 4-channel group, (a,b) half) that leave the rounded V in LDS in fragment order, and the MFMA phase reads
// V and U fragments with one ds_read_b128 each.  Per chunk: requests of chunk c+2 | transform of chunk c -> V | barrier | 8 MFMAs
// per wave | raw pieces of chunk c+1 -> LDS | barrier, with the requests two chunks ahead.  LDS: one raw stage (two planes) + 3
// filter stages + V = 155 KB.
// The two partial output transforms of a tile (the transform is linear in the (a,b) accumulators) are exchanged through LDS:
// each wave finishes the 8 accumulator rows (= one quarter) it owns.
template <int MM>
__global__ void __launch_bounds__(512, 1) wino16b_conv3x3_kernel(const WinoArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int RAWS = 2 * WRAW_FLOATS;                       // floats of the raw stage (two 8-channel planes)
  constexpr int US = 16 * 64 * 8;                             // floats of a filter stage ([ab][co][16 x 2 bytes])
  constexpr int RAW0 = 0, U0 = RAWS, V0 = U0 + 3 * US, SCR = V0 + US;      // ONE raw stage, THREE filter stages, V, scratch row
  using hv4 = typename std::conditional<MM == 1, b16x4, h16x4>::type;
  using hv8 = typename std::conditional<MM == 1, bf16x8, f16x8>::type;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = blockIdx.y * 64;
  const int nc16 = p.Cin >> 4;

  // ---- raw pieces: idx = tid + 512 j < 1600 = 2 planes x 4 quarters x 100 positions x 2 halves
  unsigned pboff[4]; int lsto[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int idx = tid + 512 * j;
    const int plane = idx / 800, r0 = idx - plane * 800;
    const int q = r0 / 200, r = r0 - q * 200, pp = r >> 1, half = r & 1;
    const int py = pp / 10, px = pp - py * 10;
    const QGeo g = quarter_of(p, q < 4 ? q : 0);
    const int iy = g.oy0 + py - 1, ix = g.ox0 + px - 1;
    const bool v = (idx < 1600) & g.valid & ((unsigned)iy < (unsigned)g.H) & ((unsigned)ix < (unsigned)g.W);
    pboff[j] = v ? (unsigned)(g.in_off + ((g.n * g.H + iy) * g.W + ix) * g.ld_in + 8 * plane + 4 * half) << 2 : 0x80000000u;
    lsto[j] = idx < 1600 ? plane * WRAW_FLOATS + (q * WQ_PIX + pp) * WRAW_LD + 4 * (half ^ ((py >> 1) & 1)) : SCR - RAW0 + 4 * (tid & 63);
  }
  const auto in_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in), 0, p.in_bytes, 0x00020000);
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  // Requests run TWO chunks ahead (a chunk's work is shorter than a first-touch load: one chunk of lead left the kernel waiting on
  // memory, ablation 2): the raw pieces of chunk c+2 wait in the register set of c's parity, the filter tiles in the third stage.
  f32x4 rp[2][4];
  auto load_raw = [&](auto S, int chunk) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      rp[decltype(S)::value][j] = __builtin_bit_cast(f32x4, __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(in_rsrc, pboff[j], chunk * 64, 0)));
  };
  auto store_raw = [&](auto S) {       // (the idle pieces of the last round land in the scratch row)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<f32x4*>(__builtin_assume_aligned(lds + RAW0 + lsto[j], 16)) = rp[decltype(S)::value][j];
  };
  // ---- filter tiles: 32 pieces of 1 KB per chunk, wave w moves pieces 4w .. 4w+3
  const char* ubase = reinterpret_cast<const char*>(p.U) + (size_t)n0 * 32;
  const unsigned lane16 = lane * 16;
  const unsigned lds_addr0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)lds;
  auto load_u = [&](int chunk, int st) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int idx = wave * 4 + k, ab = idx >> 1, h = idx & 1;
      const char* g = ubase + (size_t)chunk * ((size_t)p.Cout * 512) + (unsigned)((ab * p.Cout + h * 32) * 32);
      const unsigned dst = __builtin_amdgcn_readfirstlane(lds_addr0 + 4u * (unsigned)(U0 + st * US + (ab * 64 + h * 32) * 8));
      unsigned keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(lane16), "s"(g), "s"(dst) : "memory");
    }
  };
  // ---- transform phase: wave w = (quarter qa, (a,b) half ha); lane = (tile of the quarter, 4-channel group g of the 16)
  const int qa = wave & 3, ha = wave >> 2;
  const int tl = lane & 15, ty = tl >> 2, tx = tl & 3, g4 = lane >> 4;
  const int araw = (g4 >> 1) * WRAW_FLOATS + (qa * WQ_PIX + (2 * ty) * 10 + 2 * tx) * WRAW_LD;
  const int ahalf = g4 & 1;
  // V image: [ab][tile 0..63][16 halfs]; this item's 8 bytes of row (ab, qa*16 + tl) at halfs 4*g4
  // (rows of tiles with bit 3 set carry their two 8-half groups swapped, like the filter rows: the 16-lane groups of the fragment
  // reads then cover all banks)
  const int vwr = V0 * 4 + ((8 * ha) * 64 + qa * 16 + tl) * 32 + 8 * (g4 ^ (2 * ((tl >> 3) & 1)));     // bytes from the LDS base, + ab_local * 2048
  // ---- MFMA phase: wave w = (wa = (a,b) half, wm, wn); lane = (tile / channel li, k half lh)
  const int wa = wave >> 2, wm = (wave >> 1) & 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  const int vrd = V0 * 4 + ((8 * wa) * 64 + wm * 32 + li) * 32 + 16 * (lh ^ ((li >> 3) & 1));          // bytes, + ab_local * 2048
  const int urd = (wn * 32 + li) * 8 + 4 * (lh ^ ((li >> 3) & 1)) + (8 * wa) * 512;     // floats inside a filter stage, + ab_local * 512

  f32x16 acc[8];
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

  using P0 = std::integral_constant<int, 0>; using P1 = std::integral_constant<int, 1>;
  load_u(0, 0);
  load_raw(P0{}, 0);
  store_raw(P0{});                                  // chunk 0 -> LDS (waits for its pieces)
  if (nc16 > 1) { load_u(1, 1); load_raw(P1{}, 1); }    // chunk 1: filter stage 1, register set 1
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  char* const ldsb = reinterpret_cast<char*>(lds);
  // one chunk: requests of c+2 | transform c -> V | barrier | 8 MFMAs | raw pieces of c+1 (set of c+1's parity) -> LDS | barrier
  auto chunk_step = [&](auto PAR, int c) {
    using NXT = std::integral_constant<int, decltype(PAR)::value ^ 1>;
    const float* R = lds + RAW0;
    const float* Ub = lds + U0 + (c % 3) * US;
    const bool more = c + 2 < nc16;
    if (more && !WABL(2)) {                         // the filter pieces first: they must be OLDER than the raw loads the compiler counts
      load_u(c + 2, (c + 2) % 3);
      load_raw(PAR, c + 2);                         // set of c's parity: its previous content (chunk c) went to LDS an iteration ago
    }
    // transform of the item's 4 channels: rows 0,1,2 (ha = 0: groups a = 0, 1) or 1,2,3 (ha = 1: groups a = 2, 3); the half is
    // wave-uniform: a scalar branch, no per-lane selects
    auto transform = [&](auto HA) {
      constexpr int H = decltype(HA)::value;
      f32x4 d[3][4];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int row = i + H;
          d[i][j] = *reinterpret_cast<const f32x4*>(R + araw + 4 * (ahalf ^ ((ty + (row >> 1)) & 1)) + (row * 10 + j) * WRAW_LD);
        }
#pragma unroll
      for (int gl = 0; gl < 2; ++gl) {
        // H = 0: a=0: d0 - d2, a=1: d1 + d2;   H = 1 (rows 1,2,3 in d[0..2]): a=2: d2 - d1 = d[1] - d[0], a=3: d1 - d3 = d[0] - d[2]
        f32x2 rl[4], rh[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4& x = H == 0 ? (gl == 0 ? d[0][q] : d[1][q]) : (gl == 0 ? d[1][q] : d[0][q]);
          const f32x4& y = H == 0 ? d[2][q] : (gl == 0 ? d[0][q] : d[2][q]);
          if (H == 0 && gl == 1) { rl[q] = pk_add(lo2(x), lo2(y)); rh[q] = pk_add(hi2(x), hi2(y)); }
          else { rl[q] = pk_sub(lo2(x), lo2(y)); rh[q] = pk_sub(hi2(x), hi2(y)); }
        }
        f32x4 vv[4];
        vv[0] = cat2(pk_sub(rl[0], rl[2]), pk_sub(rh[0], rh[2]));
        vv[1] = cat2(pk_add(rl[1], rl[2]), pk_add(rh[1], rh[2]));
        vv[2] = cat2(pk_sub(rl[2], rl[1]), pk_sub(rh[2], rh[1]));
        vv[3] = cat2(pk_sub(rl[1], rl[3]), pk_sub(rh[1], rh[3]));
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *reinterpret_cast<hv4*>(__builtin_assume_aligned(ldsb + vwr + (gl * 4 + q) * 2048, 8)) = __builtin_convertvector(vv[q], hv4);
      }
    };
    if (!WABL(3) || c == 0) { if (ha == 0) transform(std::integral_constant<int, 0>{}); else transform(std::integral_constant<int, 1>{}); }
    if (!WABL(1)) __syncthreads();                  // V complete; every read of the raw stage done
    hv8 a8 = {}, b8 = {};
#pragma unroll
    for (int ab = 0; ab < 8; ++ab) {
      if (!WABL(4) || (c == 0 && ab == 0)) {
        a8 = *reinterpret_cast<const hv8*>(__builtin_assume_aligned(ldsb + vrd + ab * 2048, 16));
        b8 = __builtin_bit_cast(hv8, *reinterpret_cast<const f32x4*>(Ub + urd + ab * 512));
      }
      if (WINO_ABLATE == 6) { acc[ab][0] += (float)a8[0] * (float)b8[1]; continue; }
      if constexpr (MM == 1) acc[ab] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a8, b8, acc[ab], 0, 0, 0);
      else acc[ab] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a8, b8, acc[ab], 0, 0, 0);
    }
    if (c + 1 < nc16 && !WABL(2)) {
      // chunk c+1 (requested an iteration ago) into the raw stage; everything older than the four raw loads of this iteration has
      // landed then — its filter tiles too (the compiler's own wait before the stores asks for the same)
      if (more) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      store_raw(NXT{});
    }
    if (!WABL(1)) __syncthreads();
  };
  for (int c = 0; c < nc16; c += 2) {
    chunk_step(P0{}, c);
    if (c + 1 < nc16) chunk_step(P1{}, c + 1);
  }

  // ---------------------------------------------------------------- epilogue
  // partial output transform over the wave's 8 positions: A^T = [1 1 1 0; 0 1 -1 -1] — rows a = 0,1 (wa = 0) or a = 2,3 (wa = 1)
  f32x4 Y[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float s0[4], s1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (wa == 0) { s0[j] = acc[j][r] + acc[4 + j][r]; s1[j] = acc[4 + j][r]; }
      else { s0[j] = acc[j][r]; s1[j] = -acc[j][r] - acc[4 + j][r]; }
    }
    Y[r] = f32x4{s0[0] + s0[1] + s0[2], s0[1] - s0[2] - s0[3], s1[0] + s1[1] + s1[2], s1[1] - s1[2] - s1[3]};
  }
  // the rows this wave does not own go to its slot (8 rows x 64 lanes x 16 bytes; the stages are free behind the loop's last barrier)
  f32x4* const X = reinterpret_cast<f32x4*>(lds);
#pragma unroll
  for (int rr = 0; rr < 8; ++rr) X[(wave * 8 + rr) * 64 + lane] = Y[(wa == 0 ? 8 : 0) + rr];
  __syncthreads();
  f32x4 Yo[8];
#pragma unroll
  for (int rr = 0; rr < 8; ++rr) Yo[rr] = Y[(wa == 0 ? 0 : 8) + rr] + X[((wave ^ 4) * 8 + rr) * 64 + lane];

  const int co = n0 + wn * 32 + li;
  const float bv = p.bias ? p.bias[co] : 0.f;
  const bool do_relu = p.relu != 0;
  const QGeo g = quarter_of(p, 2 * wm + wa);              // accumulator rows 8 wa .. 8 wa + 7 = the tiles of that quarter
  if (!g.valid) return;
  const int Hp = g.H >> 1, Wp = g.W >> 1, n = g.n;
#pragma unroll
  for (int rr = 0; rr < 8; ++rr) {
    const int tyy = lh + 2 * ((rr >> 2) & 1), txx = rr & 3;
    float y[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        y[a][b] = Yo[rr][2 * a + b] + bv;
        if (do_relu) y[a][b] = fmaxf(y[a][b], 0.f);
      }
    const int oy = g.oy0 + 2 * tyy, ox = g.ox0 + 2 * txx;
    if (p.out_full) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
          if (oy + a < g.H && ox + b < g.W)
            p.out_full[(size_t)g.full_off + ((size_t)(n * g.H + oy + a) * g.W + ox + b) * g.ld_full + co] = y[a][b];
    }
    if (p.out_pool) {
      const int py = oy >> 1, px = ox >> 1;
      if (py < Hp && px < Wp)
        p.out_pool[(size_t)g.pool_off + ((size_t)(n * Hp + py) * Wp + px) * g.ld_pool + co] = fmaxf(fmaxf(y[0][0], y[0][1]), fmaxf(y[1][0], y[1][1]));
    }
  }
}

// The conv family on the 16-bit kernel (G6dConv.weight_wino16, math_mode 1 / 2): the stride-1 3x3 / 3x3x3 layers of the selector, the
// refiner feature net and the volume net with the operand prologues of the fp32 kernel — MODE 0 none, 1 InstanceNorm affine(+ReLU)
// with one table, 2 one table per image group (tables of the block's four quarters in LDS), 3 query x reference multiplier + tables
// per quarter, shared input images / per-group multiplier maps of a query batch — applied in fp32 when the raw piece is written to
// LDS (zero padding stays exactly zero), KD = 3 with the depth taps folded into the reduction, statistics / finalisation epilogue.
// Same chunk (16 channels = two planes), filters and MFMA scheme as wino16_conv3x3_kernel; loads are plain (selected) global loads.
template <int MM, int MODE, int KD>
__global__ void __launch_bounds__(256, 1) wino16_conv_kernel(const WinoArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int NWN = 2, THREADS = 256, NPR = 7;
  constexpr int WU_FLOATS = 16 * 32 * NWN * 8;
  constexpr int WSTAGE = 2 * WRAW_FLOATS + WU_FLOATS + 4 * THREADS;
  constexpr int AFF0 = 2 * WSTAGE;
  using hv4 = typename std::conditional<MM == 1, b16x4, h16x4>::type;
  using hv8 = typename std::conditional<MM == 1, bf16x8, f16x8>::type;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / NWN, wn = wave % NWN;
  const int li = lane & 31, lh = lane >> 5;
  const int n0 = blockIdx.y * (32 * NWN);
  const int nc16 = p.Cin >> 4;
  const int c_first = blockIdx.z * p.chunks_per_split;
  const int c_last = min(KD * nc16, c_first + p.chunks_per_split) - 1;

  int poff[NPR], lsto[NPR], moff[MODE == 3 ? NPR : 1], aoff[MODE != 0 ? NPR : 1];
  bool pval[NPR];
  unsigned dbits = 0;
#pragma unroll
  for (int j = 0; j < NPR; ++j) {
    const int idx = tid + THREADS * j;
    const int plane = idx / 800, r0 = idx - plane * 800;
    const int q = r0 / 200, r = r0 - q * 200, pp = r >> 1, half = r & 1;
    const int py = pp / 10, px = pp - py * 10;
    const QGeo g = quarter_of(p, q < 4 ? q : 0);
    const int n = g.n;
    const int iy = g.oy0 + py - 1, ix = g.ox0 + px - 1;
    pval[j] = (idx < 1600) & g.valid & ((unsigned)iy < (unsigned)g.H) & ((unsigned)ix < (unsigned)g.W);
    const int n_in = p.img_mod > 0 ? ((n / p.D) % p.img_mod) * p.D + n % p.D : n;
    poff[j] = pval[j] ? g.in_off + ((n_in * g.H + iy) * g.W + ix) * g.ld_in + 8 * plane + 4 * half : 0;
    lsto[j] = idx < 1600 ? plane * WRAW_FLOATS + (q * WQ_PIX + pp) * WRAW_LD + 4 * (half ^ ((py >> 1) & 1))
                         : 2 * WRAW_FLOATS + WU_FLOATS + 4 * tid;
    if constexpr (MODE == 3) moff[j] = pval[j] ? (((p.mul_div > 0 ? n / p.mul_div : 0) * p.H + iy) * p.W + ix) * p.Cin + 8 * plane + 4 * half : 0;
    if constexpr (MODE != 0) aoff[j] = idx < 1600 ? (MODE >= 2 ? q * p.Cin : 0) + 8 * plane + 4 * half : 0;
    if constexpr (KD == 3) { const int dd = n % p.D; dbits |= (unsigned)(dd > 0) << (2 * j) | (unsigned)(dd < p.D - 1) << (2 * j + 1); }
  }
  const int slice = p.H * p.W * p.ld_in;
  f32x4 rp[NPR], rm[MODE == 3 ? NPR : 1];
  bool rv[NPR];
  auto load_raw = [&](int chunk) {
    const int kd = KD == 3 ? chunk / nc16 : 0, cc = KD == 3 ? chunk - kd * nc16 : chunk;
#pragma unroll
    for (int j = 0; j < NPR; ++j) {
      bool v = pval[j];
      int off = poff[j] + cc * 16;
      if constexpr (KD == 3) { v &= kd == 1 || ((dbits >> (2 * j + (kd >> 1))) & 1u) != 0; off += (kd - 1) * slice; }
      rv[j] = v;
      rp[j] = ldg4(p.in, v ? off : 0);
      if constexpr (MODE == 3) rm[j] = ldg4(p.mul, v ? moff[j] + cc * 16 : 0);
    }
  };
  auto store_raw = [&](int st, int chunk) {
    const int cc = KD == 3 ? chunk % nc16 : chunk;
#pragma unroll
    for (int j = 0; j < NPR; ++j) {
      f32x4 v = rp[j];
      if constexpr (MODE == 3) v *= rm[j];
      if constexpr (MODE != 0) {
        const f32x4 sc = *reinterpret_cast<const f32x4*>(lds + AFF0 + aoff[j] + cc * 16);
        const f32x4 sh = *reinterpret_cast<const f32x4*>(lds + AFF0 + (MODE >= 2 ? 4 : 1) * p.Cin + aoff[j] + cc * 16);
        v = v * sc + sh;
        if (p.in_relu) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
      }
      *reinterpret_cast<f32x4*>(__builtin_assume_aligned(lds + st * WSTAGE + lsto[j], 16)) = rv[j] ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  if constexpr (MODE != 0) {
    constexpr int G = MODE >= 2 ? 4 : 1;
    for (int i = tid; i < G * p.Cin; i += THREADS) {
      int g = 0;
      if constexpr (MODE >= 2) g = p.aff_div > 0 ? (quarter_of(p, i / p.Cin).n / p.D) / p.aff_div : 0;
      const int c = MODE >= 2 ? i % p.Cin : i;
      lds[AFF0 + i] = p.in_scale[g * p.Cin + c];
      lds[AFF0 + G * p.Cin + i] = p.in_shift[g * p.Cin + c];
    }
    __syncthreads();
  }
  const char* ubase = reinterpret_cast<const char*>(p.U) + (size_t)n0 * 32;
  const unsigned lane16 = lane * 16;
  const unsigned lds_addr0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)lds;
  auto glds = [&](int chunk, int st, int idx) {
    const int ab = idx / NWN, h = idx % NWN;
    const char* g = ubase + (size_t)chunk * ((size_t)p.Cout * 512) + (unsigned)((ab * p.Cout + h * 32) * 32);
    const unsigned dst = __builtin_amdgcn_readfirstlane(lds_addr0 + 4u * (unsigned)(st * WSTAGE + 2 * WRAW_FLOATS + (ab * 32 * NWN + h * 32) * 8));
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane16), "s"(g), "s"(dst) : "memory");
  };
  auto load_u = [&](int chunk, int st) {
#pragma unroll
    for (int k = 0; k < 8; ++k) glds(chunk, st, wave * 8 + k);
  };
  const int tl = li & 15, ty = tl >> 2, tx = tl & 3;
  const int apos = lh * WRAW_FLOATS + ((2 * wm + (li >> 4)) * WQ_PIX + (2 * ty) * 10 + 2 * tx) * WRAW_LD;
  const int bbase = 2 * WRAW_FLOATS + (wn * 32 + li) * 8 + 4 * (lh ^ ((li >> 3) & 1));
  constexpr int USTRIDE = 32 * NWN * 8;

  f32x16 acc[16];
#pragma unroll
  for (int a = 0; a < 16; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

  load_u(c_first, 0);
  load_raw(c_first);
  store_raw(0, c_first);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  auto xform = [&](int grp, const f32x4 (&dd)[4][4], f32x4 (&vv)[4]) {
    f32x2 rl[4], rh[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 &a = dd[grp == 0 ? 0 : grp == 2 ? 2 : 1][q], &b = dd[grp == 0 ? 2 : grp == 1 ? 2 : grp == 2 ? 1 : 3][q];
      if (grp == 1) { rl[q] = pk_add(lo2(a), lo2(b)); rh[q] = pk_add(hi2(a), hi2(b)); }
      else { rl[q] = pk_sub(lo2(a), lo2(b)); rh[q] = pk_sub(hi2(a), hi2(b)); }
    }
    vv[0] = cat2(pk_sub(rl[0], rl[2]), pk_sub(rh[0], rh[2]));
    vv[1] = cat2(pk_add(rl[1], rl[2]), pk_add(rh[1], rh[2]));
    vv[2] = cat2(pk_sub(rl[2], rl[1]), pk_sub(rh[2], rh[1]));
    vv[3] = cat2(pk_sub(rl[1], rl[3]), pk_sub(rh[1], rh[3]));
  };

  for (int cc = c_first; cc <= c_last; ++cc) {
    const int c = cc - c_first;
    const float* S = lds + (c & 1) * WSTAGE;
    if (cc < c_last) {
      load_u(cc + 1, (c & 1) ^ 1);
      load_raw(cc + 1);
    }
    hv4 vh[16][2];
#pragma unroll
    for (int hs = 0; hs < 2; ++hs) {
      f32x4 d[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          d[i][j] = *reinterpret_cast<const f32x4*>(S + apos + 4 * (hs ^ (ty & 1) ^ (i >> 1)) + (i * 10 + j) * WRAW_LD);
#pragma unroll
      for (int grp = 0; grp < 4; ++grp) {
        f32x4 v[4];
        xform(grp, d, v);
#pragma unroll
        for (int q = 0; q < 4; ++q) vh[grp * 4 + q][hs] = __builtin_convertvector(v[q], hv4);
      }
    }
#pragma unroll
    for (int ab = 0; ab < 16; ++ab) {
      const f32x4 uraw = *reinterpret_cast<const f32x4*>(S + bbase + ab * USTRIDE);
      const hv8 a8 = __builtin_shufflevector(vh[ab][0], vh[ab][1], 0, 1, 2, 3, 4, 5, 6, 7);
      const hv8 b8 = __builtin_bit_cast(hv8, uraw);
      if constexpr (MM == 1) acc[ab] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a8, b8, acc[ab], 0, 0, 0);
      else acc[ab] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a8, b8, acc[ab], 0, 0, 0);
    }
    if (cc < c_last) store_raw((c & 1) ^ 1, cc + 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  wino_epilogue<THREADS, NWN>(p, acc, lds, tid, wm, wn, li, lh, n0);
}

// ---- launch
typedef void (*Wino16Kernel)(const WinoArgs);
int w16_go(Wino16Kernel kernel, const WinoArgs& a, dim3 grid, int threads, size_t lds_bytes, hipStream_t stream) {
  g6d_allow_lds(reinterpret_cast<const void*>(kernel), (int)wplan::LDS_MAX);
  hipLaunchKernelGGL(kernel, grid, dim3(threads), lds_bytes, stream, a);
  return g6d_check_launch("wino16_conv");
}

}  // namespace

// The kernel of a planned launch (a.splits set): the trunk kernels (mode 0, 2-D, no statistics; buffer loads) — two waves per SIMD for
// un-split launches — or the conv-family one
wino::Pick16 wino16_pick(const wino::Args& a, int mode, int kd) {
  wino::Pick16 p = {};
  if ((p.error = wplan::w16_limits(a.Cout, mode, a.Cin))) return p;
  p.trunk = mode == 0 && kd == 1 && !a.stats;
  // knob wino16_2w (tests run both kernels): 0 = the one-wave-per-SIMD kernel only
  p.two_waves = p.trunk && g6d_knob(G6D_KNOB_WINO16_2W) != 0 && a.splits == 1;
  p.threads = p.two_waves ? 512 : 256;
  p.lds_bytes = p.two_waves ? wplan::w16b_lds_bytes() : wplan::w16_lds_bytes(mode, a.Cin);
  if (!p.trunk && kd == 3 && (mode & 3) == 3) p.error = "wino16: no multiplier prologue for 3x3x3";
  return p;
}

int wino16_launch(const wino::Args& args, int mode, int kd, long long blocks, hipStream_t stream) {
  const wino::Pick16 pick = wino16_pick(args, mode, kd);
  if (pick.error) { g6d_set_error(pick.error); return G6D_EINVAL; }
  const WinoArgs a{args};
  const int t = a.mm == 1 ? 0 : 1;              // operand type: bf16, fp16
  const dim3 grid((unsigned)blocks, a.Cout / 64, a.splits);
  if (pick.trunk) {
    static const Wino16Kernel one_wave[2] = {wino16_conv3x3_kernel<1, 2>, wino16_conv3x3_kernel<2, 2>};
    static const Wino16Kernel two_waves[2] = {wino16b_conv3x3_kernel<1>, wino16b_conv3x3_kernel<2>};
    return w16_go(pick.two_waves ? two_waves[t] : one_wave[t], a, grid, pick.threads, pick.lds_bytes, stream);
  }
  static const Wino16Kernel conv[2][2][4] = {   // [operand type][kd == 3][mode]
    {{wino16_conv_kernel<1, 0, 1>, wino16_conv_kernel<1, 1, 1>, wino16_conv_kernel<1, 2, 1>, wino16_conv_kernel<1, 3, 1>},
     {wino16_conv_kernel<1, 0, 3>, wino16_conv_kernel<1, 1, 3>, wino16_conv_kernel<1, 2, 3>, nullptr}},
    {{wino16_conv_kernel<2, 0, 1>, wino16_conv_kernel<2, 1, 1>, wino16_conv_kernel<2, 2, 1>, wino16_conv_kernel<2, 3, 1>},
     {wino16_conv_kernel<2, 0, 3>, wino16_conv_kernel<2, 1, 3>, wino16_conv_kernel<2, 2, 3>, nullptr}}};
  const Wino16Kernel kernel = conv[t][kd == 3][mode & 3];
  return w16_go(kernel, a, grid, pick.threads, pick.lds_bytes, stream);      // (the table's one hole: wino16_pick refused it)
}
