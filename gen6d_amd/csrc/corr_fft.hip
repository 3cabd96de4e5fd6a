// corr_fft.hip — the detector's 15 x 15 correlation (reference network/detector.py:188-197,222-224) in the frequency domain, fp32 throughout:
// overlap-save over T x T windows (T = 32, V = 18 valid outputs per axis; corr_fft_plan.h holds every integer of the scheme).
//   corrfft_fwd_kernel    window (zero outside the map) -> its 544 Hermitian bins, X[bin][tile][2][Cin] (re plane, im plane)
//   corrfft_gemm_kernel   per bin Y'[tile][2 R] = X'[tile][2 Cin] . B'[bin][2 Cin][2 R] on v_mfma_f32_32x32x2_f32: the complex product with the
//                         conjugate filter spectrum as ONE real GEMM (rows of Xr meet [Wr | -Wi], rows of Xi meet [Wi | Wr])
//   corrfft_inv_kernel    Y[bin][tile][2][R] -> inverse real FFT / T^2, the first V x V positions to out[n][y][x][r] inside the map
// 544 * 512 * 32 * 4 real multiplications per 324 outputs = 110 k per output pixel against the direct form's 3.69 M.
// The 32-point FFT is radix 2, decimation in frequency, fully unrolled in registers; its twiddles are literals rounded from double.  Two
// real sequences ride one complex FFT wherever the data is real (two window rows; spectrum columns 0 and T/2; two output rows).
#include "g6d_common.h"
#include "corr_fft_plan.h"

namespace {

constexpr int T = 32, HB = T / 2 + 1;           // window side, Hermitian bins per row
constexpr int CG = 32;                          // channels (forward) / references (inverse) per block: the lane's low five bits
constexpr int RS = HB * 2 * CG;                 // floats per LDS row: [kx][re | im][32]
constexpr int FWD_LDS = T * RS * 4;             // 139264 bytes
constexpr int NT = 512;

struct CfftSeg { const float* in; float* out; int ld_in, ld_out; };
struct CfftParams {
  cfft::Plan plan;
  CfftSeg seg[cfft::MAX_SEG];
  int Cin;
  float* X;                                     // forward: the spectrum
  const float* Y;                               // inverse: the product
};

// cos / sin of 2 pi k / 32, k = 0 .. 16, from the nine values of the first octant pair (rounded from double)
__host__ __device__ constexpr double tw_c8(int k) {
  constexpr double c[9] = {1.0, 0.98078528040323043, 0.92387953251128674, 0.83146961230254524, 0.70710678118654752,
                           0.55557023301960218, 0.38268343236508977, 0.19509032201612825, 0.0};
  return c[k];
}
__host__ __device__ constexpr double tw_cos(int k) { return k <= 8 ? tw_c8(k) : -tw_c8(16 - k); }
__host__ __device__ constexpr double tw_sin(int k) { return k <= 8 ? tw_c8(8 - k) : tw_c8(k - 8); }
__host__ __device__ constexpr int br5(int k) { return ((k & 1) << 4) | ((k & 2) << 2) | (k & 4) | ((k & 8) >> 2) | ((k & 16) >> 4); }

// In-place forward DFT, sum_x z[x] e^{-2 pi i k x / 32}; bin k ends at position br5(k).  The inverse (unscaled) is the same routine with
// the real and imaginary arrays exchanged: fft32(im, re).
__device__ __forceinline__ void fft32(float (&re)[T], float (&im)[T]) {
#pragma unroll
  for (int h = 16; h >= 1; h >>= 1) {
#pragma unroll
    for (int b = 0; b < T; b += 2 * h) {
#pragma unroll
      for (int j = 0; j < h; ++j) {
        const int k = j * (16 / h);
        const float c = (float)tw_cos(k), s = (float)tw_sin(k);
        const float ur = re[b + j], ui = im[b + j], vr = re[b + j + h], vi = im[b + j + h];
        re[b + j] = ur + vr; im[b + j] = ui + vi;
        const float dr = ur - vr, di = ui - vi;
        if (k == 0) { re[b + j + h] = dr; im[b + j + h] = di; }
        else if (k == 8) { re[b + j + h] = di; im[b + j + h] = -dr; }
        else { re[b + j + h] = dr * c + di * s; im[b + j + h] = di * c - dr * s; }
      }
    }
  }
}

// ---- forward: block = (tile, 32 channels), thread = (g, channel): first row pair g, then spectrum column g
__global__ __launch_bounds__(NT) void corrfft_fwd_kernel(const CfftParams p) {
  extern __shared__ __attribute__((aligned(16))) float L[];
  const int tid = threadIdx.x, c = tid & (CG - 1), g = tid >> 5;
  const int tile = blockIdx.x, c0 = blockIdx.y * CG;
  const cfft::Tile t = cfft::tile_of(p.plan, tile);
  const cfft::SegPlan& sp = p.plan.seg[t.seg];
  const CfftSeg& sg = p.seg[t.seg];
  const int H = sp.H, W = sp.W, wy = cfft::window_y(p.plan, t), wx = cfft::window_x(p.plan, t);
  float re[T], im[T];
  {
    // rows 2 g and 2 g + 1 of the window as one complex sequence
    const int ya = wy + 2 * g, yb = ya + 1;
    const bool oka = ya >= 0 && ya < H, okb = yb >= 0 && yb < H;
    const float* img = sg.in + (size_t)t.n * H * W * sg.ld_in + c0 + c;
#pragma unroll
    for (int x = 0; x < T; ++x) {
      const int xx = wx + x;
      const bool okx = xx >= 0 && xx < W;
      re[x] = oka && okx ? img[((size_t)ya * W + xx) * sg.ld_in] : 0.f;
      im[x] = okb && okx ? img[((size_t)yb * W + xx) * sg.ld_in] : 0.f;
    }
  }
  fft32(re, im);
  // Z = A + i B, A and B the spectra of the two real rows: A[k] = (Z[k] + conj Z[-k]) / 2, B[k] = (Z[k] - conj Z[-k]) / 2i
  {
    float* ra = L + (2 * g) * RS + c;
    float* rb = ra + RS;
#pragma unroll
    for (int k = 0; k < HB; ++k) {
      const int a = br5(k), b = br5((T - k) & (T - 1));
      ra[k * 64] = 0.5f * (re[a] + re[b]); ra[k * 64 + 32] = 0.5f * (im[a] - im[b]);
      rb[k * 64] = 0.5f * (im[a] + im[b]); rb[k * 64 + 32] = 0.5f * (re[b] - re[a]);
    }
  }
  __syncthreads();
  // columns: thread g > 0 owns column g; thread 0 owns columns 0 and 16, both real after the row pass, as one complex sequence
  if (g == 0) {
#pragma unroll
    for (int y = 0; y < T; ++y) { re[y] = L[y * RS + c]; im[y] = L[y * RS + 16 * 64 + c]; }
  } else {
#pragma unroll
    for (int y = 0; y < T; ++y) { re[y] = L[y * RS + g * 64 + c]; im[y] = L[y * RS + g * 64 + 32 + c]; }
  }
  fft32(re, im);
  if (g == 0) {
#pragma unroll
    for (int k = 0; k < T; ++k) {
      const int a = br5(k), b = br5((T - k) & (T - 1));
      L[k * RS + c] = 0.5f * (re[a] + re[b]); L[k * RS + 32 + c] = 0.5f * (im[a] - im[b]);
      L[k * RS + 16 * 64 + c] = 0.5f * (im[a] + im[b]); L[k * RS + 16 * 64 + 32 + c] = 0.5f * (re[b] - re[a]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < T; ++k) { L[k * RS + g * 64 + c] = re[br5(k)]; L[k * RS + g * 64 + 32 + c] = im[br5(k)]; }
  }
  __syncthreads();
  // X[bin][tile][plane][c0 .. c0 + 31]: 16 bytes per lane, 128 contiguous bytes per (bin, plane)
  const size_t tiles = (size_t)p.plan.tiles;
#pragma unroll 1
  for (int i = tid; i < T * HB * 16; i += NT) {
    const int q = i & 7, pl = (i >> 3) & 1, bin = i >> 4, ky = bin / HB, kx = bin - ky * HB;
    const f32x4 v = *reinterpret_cast<const f32x4*>(L + ky * RS + kx * 64 + pl * 32 + 4 * q);
    *reinterpret_cast<f32x4*>(p.X + (((size_t)bin * tiles + tile) * 2 + pl) * p.Cin + c0 + 4 * q) = v;
  }
}

// ---- products: block = (bin, WAVES x 64 rows), wave = 64 rows x 64 columns = 4 accumulators, over a ring of STAGES LDS stages of 32 k
// each (corr_fft_plan.h holds the integers).  Per stage a wave requests its own 64 rows of X as 8 LDS-DMA pieces of 8 rows x 128 bytes
// (every 128-byte line is asked for once, whole) and its share of the stage's 8 KB of B', which the block's waves share: B' goes
// through the vector memory path once per block, not once per wave.  Lane (r = lane & 31, h = lane >> 5) then takes k = 16 h .. 16 h + 15
// of the stage for both operands: four 16-byte reads per row tile from the slot-swizzled X image, 32 single values of B' (32
// consecutive banks per half wave): the order of k inside the sum is free as long as both operands agree.
// One barrier per step: it publishes every wave's pieces of step t (each wave first retires its own with a counted vmcnt that leaves
// the later steps' requests in flight) and frees the stage that step t - 1 read, into which step t + STAGES - 1 is requested next.
// A bin's rows are spread evenly over its blocks in whole waves; a wave left without rows asks for its share of B' only.
// Rows beyond M are clamped to M - 1 in the request and never stored; the buffer descriptors end at the bin's last byte of X and B'.
// Blocks of one bin run back to back on ONE XCD (bins % 8 == 0), so B'[bin] (256 KB at Cin = 512) is fetched into one L2 once.
struct CfftGemm { const float* X; const float* B; float* Y; int M, bins, K2, mblocks, rows; };
typedef __attribute__((address_space(3))) void* cfft_lds_ptr;

template <bool V> struct CfftBool { static constexpr bool value = V; };
template <int N> __device__ __forceinline__ void cfft_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

template <int WAVES, int STAGES>
__global__ __launch_bounds__(WAVES * 64) void corrfft_gemm_kernel(const CfftGemm p) {
  extern __shared__ __attribute__((aligned(16))) char gl[];
  constexpr int ASTG = cfft::gemm_a_stage_bytes(WAVES), STG = cfft::gemm_stage_bytes(WAVES);
  constexpr int PB = cfft::gemm_b_pieces_per_wave(WAVES);
  constexpr int WIMG = cfft::GEMM_WAVE_ROWS * cfft::GEMM_ROW_BYTES;      // a wave's X image of one stage
  static_assert(STAGES == cfft::gemm_stages(WAVES) && (STAGES == 2 || STAGES == 3), "the waits below are written for rings of two and three");
  int bin, mb;
  cfft::gemm_block_of(blockIdx.x, p.mblocks, bin, mb);
  if (bin >= p.bins) return;                                   // (the whole block)
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), r = lane & 31, h = lane >> 5;
  const int m0 = cfft::gemm_wave_row0(mb, wv, p.rows), K2 = p.K2, nsteps = K2 / cfft::GEMM_KSTEP;
  const bool active = !cfft::gemm_wave_idle(mb, wv, p.rows, p.M);      // a wave without rows still stages its share of B' and meets the barriers
  const auto rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.X) + (size_t)bin * p.M * K2, 0, p.M * K2 * 4, 0x00020000);
  const auto rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.B) + (size_t)bin * K2 * cfft::GEMM_COLS, 0, K2 * cfft::GEMM_COLS * 4, 0x00020000);
  unsigned aoff[cfft::GEMM_A_PIECES];
#pragma unroll
  for (int c = 0; c < cfft::GEMM_A_PIECES; ++c)
    aoff[c] = (unsigned)min(m0 + cfft::gemm_a_src_row(c, lane), p.M - 1) * (unsigned)(K2 * 4) + 16u * cfft::gemm_a_src_seg(c, lane);
  const unsigned boff = (unsigned)(wv * PB) * cfft::GEMM_PIECE + 16u * lane;

  auto issue = [&](int t, int st, bool with_a) {
    char* sa = gl + st * STG;
    const unsigned ka = (unsigned)t * cfft::GEMM_ROW_BYTES, kb = (unsigned)t * cfft::GEMM_B_STAGE;
    if (with_a)
#pragma unroll
      for (int c = 0; c < cfft::GEMM_A_PIECES; ++c)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_a, (cfft_lds_ptr)(sa + wv * WIMG + c * cfft::GEMM_PIECE), 16, aoff[c] + ka, 0, 0, 0);
#pragma unroll
    for (int q = 0; q < PB; ++q)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_b, (cfft_lds_ptr)(sa + ASTG + (wv * PB + q) * cfft::GEMM_PIECE), 16,
                                               boff + q * cfft::GEMM_PIECE + kb, 0, 0, 0);
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][n][q] = 0.f;
  // the step's fragments: all 24 LDS reads are requested first, in the order the MFMAs use them, and the next stage's pieces behind them
  f32x4 x0[4], x1[4];
  float y0[16], y1[16];
  auto fetch = [&](int st) {
    const char* sa = gl + st * STG + wv * WIMG;
    const char* sb = gl + st * STG + ASTG + cfft::gemm_b_lds_offset(16 * h, r);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x0[j] = *reinterpret_cast<const f32x4*>(sa + cfft::gemm_a_lds_offset(r, 4 * h + j));
      x1[j] = *reinterpret_cast<const f32x4*>(sa + cfft::gemm_a_lds_offset(32 + r, 4 * h + j));
#pragma unroll
      for (int e = 4 * j; e < 4 * j + 4; ++e) {
        y0[e] = *reinterpret_cast<const float*>(sb + cfft::gemm_b_lds_offset(e, 0));
        y1[e] = *reinterpret_cast<const float*>(sb + cfft::gemm_b_lds_offset(e, 32));
      }
    }
  };
  auto mac = [&]() {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float u0 = x0[e >> 2][e & 3], u1 = x1[e >> 2][e & 3];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(u0, y0[e], acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(u0, y1[e], acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(u1, y0[e], acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(u1, y1[e], acc[1][1], 0, 0, 0);
    }
  };

#pragma unroll
  for (int t = 0; t < STAGES - 1; ++t) issue(t, t, active);    // nsteps >= 2 >= STAGES - 1 (K2 >= 64)
  // the K loop, once for a wave with rows and once for an idle wave (so that the accumulators never cross a branch)
  auto run = [&](auto act) {
    constexpr int LOADS = cfft::gemm_loads_per_stage(WAVES, !decltype(act)::value);
    int st = 0;
#pragma unroll 1
    for (int t = 0; t < nsteps; ++t) {
      // in flight here: steps t .. min(t + STAGES - 2, nsteps - 1); requests return in order, so leaving the later step's pieces retires step t's
      if (cfft::gemm_ahead(STAGES, t, nsteps) == 1) cfft_wait_vm<LOADS>(); else cfft_wait_vm<0>();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // this wave's reads of step t - 1 have returned
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      if (decltype(act)::value) { fetch(st); __builtin_amdgcn_sched_barrier(0); }
      const int sn = st == 0 ? STAGES - 1 : st - 1;            // (st + STAGES - 1) % STAGES: the stage step t - 1 read
      if (t + STAGES - 1 < nsteps) issue(t + STAGES - 1, sn, decltype(act)::value);
      __builtin_amdgcn_sched_barrier(0);
      if (decltype(act)::value) mac();
      st = st + 1 == STAGES ? 0 : st + 1;
    }
  };
  if (!active) { run(CfftBool<false>{}); return; }
  run(CfftBool<true>{});
  float* Yb = p.Y + (size_t)bin * p.M * 64 + r;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int row = m0 + 32 * i + (q & 3) + 8 * (q >> 2) + 4 * h;
      if (row < p.M) { Yb[(size_t)row * 64] = acc[i][0][q]; Yb[(size_t)row * 64 + 32] = acc[i][1][q]; }
    }
}

template <int WAVES>
void cfft_gemm_launch(const CfftGemm& p, hipStream_t stream) {
  constexpr int STAGES = cfft::gemm_stages(WAVES), LDS = cfft::gemm_lds_bytes(WAVES);
  g6d_allow_lds(reinterpret_cast<const void*>(&corrfft_gemm_kernel<WAVES, STAGES>), LDS);
  hipLaunchKernelGGL((corrfft_gemm_kernel<WAVES, STAGES>), dim3(p.bins * p.mblocks), dim3(WAVES * 64), LDS, stream, p);
}

// ---- inverse: block = tile, thread = (g, reference): first spectrum column g (thread 0: columns 0 and 16, whose inverse transforms are
// real, as one complex sequence), then output rows 2 g and 2 g + 1 (g < V / 2) as one complex sequence
constexpr int INV_ROWS = 18;                    // V at K = 15; rows kept after the column pass (V <= INV_ROWS is checked by the launcher)
constexpr int INV_LDS = INV_ROWS * RS * 4;

__global__ __launch_bounds__(NT) void corrfft_inv_kernel(const CfftParams p) {
  extern __shared__ __attribute__((aligned(16))) float L[];
  const int tid = threadIdx.x, r = tid & (CG - 1), g = tid >> 5;
  const int tile = blockIdx.x, V = p.plan.V;
  const cfft::Tile t = cfft::tile_of(p.plan, tile);
  const cfft::SegPlan& sp = p.plan.seg[t.seg];
  const CfftSeg& sg = p.seg[t.seg];
  const size_t bs = (size_t)p.plan.tiles * 64;               // floats from bin to bin
  const float* Y = p.Y + (size_t)tile * 64 + r;
  float re[T], im[T];
  if (g == 0) {
#pragma unroll
    for (int k = 0; k < T; ++k) {
      const float* y0 = Y + (size_t)(k * HB) * bs;
      const float* y16 = Y + (size_t)(k * HB + 16) * bs;
      re[k] = y0[0] - y16[32]; im[k] = y0[32] + y16[0];      // Y[., 0] + i Y[., 16]
    }
  } else {
#pragma unroll
    for (int k = 0; k < T; ++k) {
      const float* y = Y + (size_t)(k * HB + g) * bs;
      re[k] = y[0]; im[k] = y[32];
    }
  }
  fft32(im, re);                                             // inverse along y
  if (g == 0) {
#pragma unroll
    for (int y = 0; y < INV_ROWS; ++y) {
      L[y * RS + r] = re[br5(y)]; L[y * RS + 32 + r] = 0.f;
      L[y * RS + 16 * 64 + r] = im[br5(y)]; L[y * RS + 16 * 64 + 32 + r] = 0.f;
    }
  } else {
#pragma unroll
    for (int y = 0; y < INV_ROWS; ++y) { L[y * RS + g * 64 + r] = re[br5(y)]; L[y * RS + g * 64 + 32 + r] = im[br5(y)]; }
  }
  __syncthreads();
  if (2 * g >= V) return;
  // rows ya = 2 g, yb = ya + 1 (V even): Z[k] = Ga[k] + i Gb[k], with G[T - k] = conj G[k] for the half that is not stored
  const float* ga = L + (2 * g) * RS + r;
  const float* gb = ga + RS;
#pragma unroll
  for (int k = 0; k < HB; ++k) {
    const float ar = ga[k * 64], ai = ga[k * 64 + 32], br = gb[k * 64], bi = gb[k * 64 + 32];
    re[k] = ar - bi; im[k] = ai + br;
    if (k > 0 && k < T / 2) { re[T - k] = ar + bi; im[T - k] = br - ai; }
  }
  fft32(im, re);                                             // inverse along x: re = row ya, im = row yb
  const int H = sp.H, W = sp.W, ya = t.y0 + 2 * g;
  const float sc = 1.f / (T * T);
  float* o = sg.out + (size_t)t.n * H * W * sg.ld_out + r;
#pragma unroll
  for (int x = 0; x < INV_ROWS; ++x) {
    const int xx = t.x0 + x;
    if (x < V && xx < W) {
      if (ya < H) o[((size_t)ya * W + xx) * sg.ld_out] = re[br5(x)] * sc;
      if (ya + 1 < H) o[((size_t)(ya + 1) * W + xx) * sg.ld_out] = im[br5(x)] * sc;
    }
  }
}

int cfft_params(CfftParams& p, const char* what, const G6dCorrSeg* segs, int nseg, int C, int k, int Tw, bool fwd) {
  if (!segs || nseg < 1 || nseg > cfft::MAX_SEG) { g6d_set_error("corr_fft: 1..4 segments expected"); return G6D_EINVAL; }
  if (Tw != T || k != 15) { g6d_set_error("corr_fft: the kernels are built for T = 32, k = 15"); return G6D_EINVAL; }
  int N[cfft::MAX_SEG], H[cfft::MAX_SEG], W[cfft::MAX_SEG];
  for (int i = 0; i < nseg; ++i) { N[i] = segs[i].N; H[i] = segs[i].H; W[i] = segs[i].W; }
  if (!cfft::make_plan(p.plan, Tw, k, nseg, N, H, W) || p.plan.V > INV_ROWS || (p.plan.V & 1)) { g6d_set_error("corr_fft: bad map sizes"); return G6D_EINVAL; }
  for (int i = 0; i < nseg; ++i) {
    const G6dCorrSeg& s = segs[i];
    const bool ok = fwd ? (s.in && s.ld_in >= C && !(s.ld_in & 3) && g6d_aligned16(s.in)) : (s.out && s.ld_out >= C);
    if (!ok) { g6d_set_error(what); return G6D_EINVAL; }
    p.seg[i] = CfftSeg{s.in, s.out, s.ld_in, s.ld_out};
  }
  return G6D_OK;
}
}  // namespace

extern "C" int g6d_corr_fft_plan(const G6dCorrSeg* segs, int nseg, int Cin, int Cout, int k, int Tw, int64_t* out) {
  if (!segs || !out || nseg < 1 || nseg > cfft::MAX_SEG || Cin < 1 || Cout < 1) { g6d_set_error("corr_fft_plan: bad arguments"); return G6D_EINVAL; }
  int N[cfft::MAX_SEG], H[cfft::MAX_SEG], W[cfft::MAX_SEG], one[cfft::MAX_SEG];
  for (int i = 0; i < nseg; ++i) { N[i] = segs[i].N; H[i] = segs[i].H; W[i] = segs[i].W; one[i] = 1; }
  cfft::Plan p, q;
  if (!cfft::make_plan(p, Tw, k, nseg, N, H, W) || !cfft::make_plan(q, Tw, k, nseg, one, H, W)) { g6d_set_error("corr_fft_plan: bad sizes"); return G6D_EINVAL; }
  out[0] = p.tiles; out[1] = p.bins; out[2] = p.V;
  out[3] = cfft::spectrum_bytes(Tw, p.tiles, Cin); out[4] = cfft::product_bytes(Tw, p.tiles, Cout); out[5] = cfft::filter_bytes(Tw, Cin, Cout);
  out[6] = q.tiles;                                              // tiles of one query (one map per segment)
  out[7] = cfft::chunk_queries(Tw, q.tiles, Cin, 1 << 16);      // most queries per launch
  return G6D_OK;
}

extern "C" int g6d_corr_fft_fwd(const G6dCorrSeg* segs, int nseg, int Cin, int k, int Tw, float* X, g6d_stream_t stream) {
  CfftParams p = {};
  if (int rc = cfft_params(p, "corr_fft_fwd: bad segment (fp32 channels-last maps, 16-byte aligned, ld_in % 4 == 0)", segs, nseg, Cin, k, Tw, true)) return rc;
  if (!X || !g6d_aligned16(X) || Cin < CG || Cin % CG) { g6d_set_error("corr_fft_fwd: Cin % 32 == 0 and an aligned spectrum expected"); return G6D_EINVAL; }
  if (cfft::spectrum_bytes(Tw, p.plan.tiles, Cin) >= (1ll << 31)) { g6d_set_error("corr_fft_fwd: spectrum beyond 2 GB, launch fewer queries"); return G6D_ENOSPC; }
  p.Cin = Cin; p.X = X;
  g6d_allow_lds(reinterpret_cast<const void*>(&corrfft_fwd_kernel), FWD_LDS);
  hipLaunchKernelGGL(corrfft_fwd_kernel, dim3(p.plan.tiles, Cin / CG), dim3(NT), FWD_LDS, static_cast<hipStream_t>(stream), p);
  return g6d_check_launch("corr_fft_fwd");
}

extern "C" int g6d_corr_fft_gemm(const float* X, const float* B, float* Y, int tiles, int Cin, int Cout, int Tw, g6d_stream_t stream) {
  if (!X || !B || !Y || tiles < 1 || Tw != T || Cout != 32 || Cin < 32 || Cin % 32 || !g6d_aligned16(X)) {
    g6d_set_error("corr_fft_gemm: T = 32, 32 references, Cin % 32 == 0 expected"); return G6D_EINVAL;
  }
  if (cfft::spectrum_bytes(Tw, tiles, Cin) >= (1ll << 31)) { g6d_set_error("corr_fft_gemm: spectrum beyond 2 GB"); return G6D_ENOSPC; }
  if (!g6d_aligned16(B)) { g6d_set_error("corr_fft_gemm: the filter spectrum is staged in 16-byte pieces, a 16-byte aligned B' expected"); return G6D_EINVAL; }
  const CfftGemm p = {X, B, Y, tiles, cfft::bins(Tw), 2 * Cin, cfft::gemm_mblocks(tiles), cfft::gemm_rows_per_block(tiles)};
  static_assert(cfft::bins(T) % 8 == 0, "blocks of a bin stay on one XCD");
  if (cfft::gemm_waves(tiles) == 2) cfft_gemm_launch<2>(p, static_cast<hipStream_t>(stream));
  else cfft_gemm_launch<4>(p, static_cast<hipStream_t>(stream));
  return g6d_check_launch("corr_fft_gemm");
}

extern "C" int g6d_corr_fft_inv(const G6dCorrSeg* segs, int nseg, int Cout, int k, int Tw, const float* Y, g6d_stream_t stream) {
  CfftParams p = {};
  if (int rc = cfft_params(p, "corr_fft_inv: bad segment (ld_out >= 32)", segs, nseg, Cout, k, Tw, false)) return rc;
  if (!Y || Cout != CG) { g6d_set_error("corr_fft_inv: 32 references expected"); return G6D_EINVAL; }
  p.Y = Y;
  g6d_allow_lds(reinterpret_cast<const void*>(&corrfft_inv_kernel), INV_LDS);
  hipLaunchKernelGGL(corrfft_inv_kernel, dim3(p.plan.tiles), dim3(NT), INV_LDS, static_cast<hipStream_t>(stream), p);
  return g6d_check_launch("corr_fft_inv");
}
