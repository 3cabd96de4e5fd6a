// conv16_tap.hip — the PER-TAP kernels of the direct 16-bit convolution (conv16_direct.hip: the family and its launcher): a K step is one
// tap's slice of input channels, both operand tiles through LDS (conv16_kernel, row-major filters, w_layout 0) or the activations alone
// (conv16r_kernel, fragment-major filters).  2-D and 3x3x3 layers; the maps no halo tiling fits run here.
#include "conv16_common.h"

namespace {

constexpr int C16_STAGE = (C16_BM + C16_BN) * C16_BK * 2;      // 32 KB
constexpr int C16_LDS = 2 * C16_STAGE;                         // 64 KB

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

void c16tap_go(void (*kern)(const C16Params), int lds_bytes, const c16::Params& p, hipStream_t st) {
  g6d_allow_lds(reinterpret_cast<const void*>(kern), lds_bytes);
  hipLaunchKernelGGL(kern, dim3(c16::tap_grid(p)), dim3(256), lds_bytes, st, C16Params{p});
}

}  // namespace

int c16tap_launch(const c16::Params& p, int w_layout, int math_mode, hipStream_t stream) {
  if (w_layout == 0) {
    c16tap_go(math_mode == 1 ? &conv16_kernel<1> : &conv16_kernel<2>, C16_LDS, p, stream);
    return g6d_check_launch("conv16_direct");
  }
  constexpr int NST = 3, LDSR = NST * C16R<1>::STAGE;          // three 16 KB stages (>= the epilogue's 38.9 KB tile)
  static_assert(C16R<2>::STAGE == C16R<1>::STAGE && C16R<3>::STAGE == C16R<1>::STAGE && LDSR == 3 * 16384, "one stage size in every mode");
  c16tap_go(math_mode == 1 ? &conv16r_kernel<1, NST> : math_mode == 2 ? &conv16r_kernel<2, NST> : &conv16r_kernel<3, NST>, LDSR, p, stream);
  return g6d_check_launch("conv16r_direct");
}
