// split16.hip — the hand-over passes into the 16-bit activation formats of the conv16_direct.hip family's kernels (conv16_tap.hip, conv16w.hip) (pair16.h: bf16 / fp16 maps and the
// fp16 hi / lo pair maps of the fp32 path): four HBM-bound elementwise kernels that write an fp32 result ONCE in the format the next conv's
// DMA loads take, and their launchers.  The three grid-stride kernels end in c16_store8; l2norm_split16_kernel keeps its paired-lane store.
#include "g6d_common.h"
#include "pair16.h"
#include <type_traits>

namespace {

// product_split_kernel: the selector's query x reference product (reference network/selector.py:183-186 — every hypothesis image is the
// reference's feature map times the query's, InstanceNorm'ed) written ONCE in the 16-bit activation format of conv16w_kernel, so that the
// first conv of every level can run on it: out[q D + d][px][plane][c] = split16((ref[d][px][c] * que[q][px][c]) * scale[q][c] + shift[q][c]).
// HBM-bound: one 16-byte (pairs: two) store per 8 channels; the reference cache (D P C floats) is re-read per query out of L2 / MALL.
template <int MM>
__global__ void __launch_bounds__(256) product_split_kernel(const float* __restrict__ ref, const float* __restrict__ que, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, char* __restrict__ out, int D, int P, int C, long total,
                                                           const G6dRange16 rng) {
  // a work item = 8 channels of one (query, pixel) for a run of PS_RUN hypotheses: the query's values and tables are loaded once per run
  // (one reference load and one / two 16-byte stores per output instead of four loads)
  constexpr int PS_RUN = 8;
  const int c8 = C >> 3, nrun = (D + PS_RUN - 1) / PS_RUN;
  const int eo = MM == 3 ? g6d_exp_out(rng) : 0;              // pairs hold split16(v * 2^-eo); amax: max bits(|v|) (G6dRange16)
  unsigned amax = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cg = (int)(i % c8);
    long r = i / c8;
    const int px = (int)(r % P); r /= P;
    const int run = (int)(r % nrun), q = (int)(r / nrun);
    const int c = cg * 8;
    const float* qp = que + ((long)q * P + px) * C + c;
    const f32x4 q0 = *reinterpret_cast<const f32x4*>(qp), q1 = *reinterpret_cast<const f32x4*>(qp + 4);
    const f32x4 s0 = *reinterpret_cast<const f32x4*>(scale + (long)q * C + c), s1 = *reinterpret_cast<const f32x4*>(scale + (long)q * C + c + 4);
    const f32x4 t0 = *reinterpret_cast<const f32x4*>(shift + (long)q * C + c), t1 = *reinterpret_cast<const f32x4*>(shift + (long)q * C + c + 4);
    const int d1 = min(D, (run + 1) * PS_RUN);
#pragma unroll 2
    for (int d = run * PS_RUN; d < d1; ++d) {
      const float* rp = ref + ((long)d * P + px) * C + c;
      const f32x4 r0 = *reinterpret_cast<const f32x4*>(rp), r1 = *reinterpret_cast<const f32x4*>(rp + 4);
      float v[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[e] = fmaf(r0[e] * q0[e], s0[e], t0[e]); v[4 + e] = fmaf(r1[e] * q1[e], s1[e], t1[e]); }
      const long row = ((long)q * D + d) * P + px;
      c16_store8<MM>(v, eo, amax, out + (row * (MM == 3 ? 2 : 1) * C + c) * 2, (long)C * 2);
    }
  }
  if constexpr (MM == 3) g6d_range_record_block<4>(rng, amax);
}

// affine_split16_kernel: y = pool2x2?(relu?(x * scale[g][c] + shift[g][c])) of an fp32 channels-last map written in the 16-bit activation
// format of conv16w_kernel (pairs on the fp32 path) — the InstanceNorm affine + ReLU (+ MaxPool) between two convs of the selector's stacks
// (reference network/selector.py:27-77), which the Winograd / implicit-GEMM kernels apply in their operand prologue and a DMA-staged
// kernel cannot.  HBM-bound elementwise pass; image n uses table n / per_n (0: one table).
template <int MM>
__global__ void __launch_bounds__(256) affine_split16_kernel(const float* __restrict__ in, int ld_in, const float* __restrict__ scale, const float* __restrict__ shift,
                                                            int per_n, int relu, int pool, int H, int W, int C, char* __restrict__ out, int ld_out,
                                                            int plane, long total, const G6dRange16 rng) {
  // out: the map's channel 0 of pixel 0 inside rows of ld_out 16-bit elements, the lo plane `plane` elements after the hi plane (dense:
  // ld_out = 2 C, plane = C; a channel slice of a wider pair map: that map's row length and channel count)
  const int c8 = C >> 3, Ho = pool ? H >> 1 : H, Wo = pool ? W >> 1 : W;
  const int eo = MM == 3 ? g6d_exp_out(rng) : 0;              // pairs hold split16(v * 2^-eo); amax: max bits(|v|) (G6dRange16)
  unsigned amax = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cg = (int)(i % c8);
    const long r = i / c8;                                     // output pixel (n Ho + y) Wo + x
    const int x = (int)(r % Wo);
    const long ny = r / Wo;
    const int y = (int)(ny % Ho);
    const long n = ny / Ho;
    const int c = cg * 8;
    const long tb = (per_n > 0 ? n / per_n : 0) * C + c;
    f32x4 s0 = {1.f, 1.f, 1.f, 1.f}, s1 = s0, t0 = {0.f, 0.f, 0.f, 0.f}, t1 = t0;
    if (scale) {
      s0 = *reinterpret_cast<const f32x4*>(scale + tb); s1 = *reinterpret_cast<const f32x4*>(scale + tb + 4);
      t0 = *reinterpret_cast<const f32x4*>(shift + tb); t1 = *reinterpret_cast<const f32x4*>(shift + tb + 4);
    }
    float v[8];
    const int np = pool ? 2 : 1;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = -3.0e38f;
    for (int dy = 0; dy < np; ++dy)
      for (int dx = 0; dx < np; ++dx) {
        const float* p_ = in + (((long)n * H + (pool ? 2 * y + dy : y)) * W + (pool ? 2 * x + dx : x)) * ld_in + c;
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(p_), a1 = *reinterpret_cast<const f32x4*>(p_ + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float u0 = fmaf(a0[e], s0[e], t0[e]), u1 = fmaf(a1[e], s1[e], t1[e]);
          if (relu) { u0 = fmaxf(u0, 0.f); u1 = fmaxf(u1, 0.f); }
          v[e] = fmaxf(v[e], u0); v[4 + e] = fmaxf(v[4 + e], u1);
        }
      }
    c16_store8<MM>(v, eo, amax, out + (r * ld_out + c) * 2, (long)plane * 2);
  }
  if constexpr (MM == 3) g6d_range_record_block<4>(rng, amax);
}

// upsample_split16_kernel: g6d_upsample_bilinear (x f, align_corners = False, the per-image InstanceNorm affine applied to the four
// neighbours: the arithmetic of upsample_bilinear_kernel, elementwise.hip) written in the 16-bit activation format — the ends of the
// feature net's 16 x 16 / 8 x 8 branches (reference network/refiner.py:72-76), which land in their channel slice of the pair `cat` map.
// out / ld_out / plane: as affine_split16_kernel.
__device__ __forceinline__ f32x4 c16_aff4(f32x4 v, f32x4 sc, f32x4 sh, bool has) {
  if (has) v = v * sc + sh;
  return v;
}
template <int MM>
__global__ void __launch_bounds__(256) upsample_split16_kernel(const float* __restrict__ in, int ld_in, const float* __restrict__ scale,
                                                              const float* __restrict__ shift, int per_n, int H, int W, int C, int f, char* __restrict__ out,
                                                              int ld_out, int plane, long total, const G6dRange16 rng) {
  const int c8 = C >> 3, Ho = H * f, Wo = W * f;
  const float rs = 1.f / (float)f;
  const int eo = MM == 3 ? g6d_exp_out(rng) : 0;
  unsigned amax = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % c8) * 8;
    const long r = i / c8;                                     // output pixel (n Ho + y) Wo + x
    const int x = (int)(r % Wo);
    const long ny = r / Wo;
    const int y = (int)(ny % Ho);
    const long n = ny / Ho;
    float sy = rs * (y + 0.5f) - 0.5f; if (sy < 0.f) sy = 0.f;
    float sx = rs * (x + 0.5f) - 0.5f; if (sx < 0.f) sx = 0.f;
    const int y0 = (int)sy, x0 = (int)sx;
    const int y1 = y0 + (y0 < H - 1), x1 = x0 + (x0 < W - 1);
    const float ly = sy - y0, lx = sx - x0, hy = 1.f - ly, hx = 1.f - lx;
    const bool has = scale != nullptr;
    const float* b = in + (size_t)n * H * W * ld_in + c;
    float v[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {                              // the fp32 kernel's item: four channels
      f32x4 sc = {1, 1, 1, 1}, sh = {0, 0, 0, 0};
      if (has) {
        const size_t o = (size_t)(per_n ? n / per_n : 0) * C + c + 4 * h;
        sc = *reinterpret_cast<const f32x4*>(scale + o); sh = *reinterpret_cast<const f32x4*>(shift + o);
      }
      const f32x4 v00 = c16_aff4(*reinterpret_cast<const f32x4*>(b + ((size_t)y0 * W + x0) * ld_in + 4 * h), sc, sh, has);
      const f32x4 v01 = c16_aff4(*reinterpret_cast<const f32x4*>(b + ((size_t)y0 * W + x1) * ld_in + 4 * h), sc, sh, has);
      const f32x4 v10 = c16_aff4(*reinterpret_cast<const f32x4*>(b + ((size_t)y1 * W + x0) * ld_in + 4 * h), sc, sh, has);
      const f32x4 v11 = c16_aff4(*reinterpret_cast<const f32x4*>(b + ((size_t)y1 * W + x1) * ld_in + 4 * h), sc, sh, has);
      const f32x4 u = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[4 * h + e] = u[e];
    }
    c16_store8<MM>(v, eo, amax, out + (r * ld_out + c) * 2, (long)plane * 2);
  }
  if constexpr (MM == 3) g6d_range_record_block<4>(rng, amax);
}

// l2norm_split16_kernel: F.normalize over the channels of an fp32 channels-last tap (the arithmetic of l2norm_rows_kernel, elementwise.hip:
// one wave per pixel, lane l sums channels 4 l .. 4 l + 3 of every 256-channel chunk, the same wave reduction) written in the 16-bit
// activation format instead of in place — the trunk's taps on their way into the feature net's first convs (reference
// network/refiner.py:69-71).  The row stays in registers between the two steps (NCH chunks of 256 channels): 4 bytes read and 4 (2)
// written per value.  16-byte stores: lanes 2 j and 2 j + 1 hold channels 8 j .. 8 j + 7 of a chunk — the even lane stores their hi
// halves, the odd lane their lo halves (16-bit modes: the even lane stores the eight values).
template <int MM, int NCH>
__global__ void __launch_bounds__(256) l2norm_split16_kernel(const float* __restrict__ x, int ld_in, int rows, char* __restrict__ out, const G6dRange16 rng) {
  typedef typename C16T3<MM>::T T;
  typedef T T4 __attribute__((ext_vector_type(4)));
  constexpr int C = 256 * NCH;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int eo = MM == 3 ? g6d_exp_out(rng) : 0;
  unsigned amax = 0;
  if (row < rows) {                                            // (wave-uniform; no return before the block-wide record)
    const float* p = x + (size_t)row * ld_in;
    f32x4 v[NCH];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      v[k] = *reinterpret_cast<const f32x4*>(p + lane * 4 + 256 * k);
      s += v[k][0] * v[k][0] + v[k][1] * v[k][1] + v[k][2] * v[k][2] + v[k][3] * v[k][3];
    }
    const float inv = 1.f / fmaxf(sqrtf(wave_sum(s)), 1e-12f);
    char* o = out + (size_t)row * (MM == 3 ? 2 * C : C) * 2;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const f32x4 u = v[k] * inv;
      T4 hi, lo;
#pragma unroll
      for (int e = 0; e < 4; ++e) { T h, l; c16_pair_split(u[e], eo, amax, h, l); hi[e] = h; lo[e] = l; }      // (16-bit modes: eo = 0, amax unused)
      // the partner lane needs: (even lane) the odd lane's hi halves, (odd lane) the even lane's lo halves
      const bool odd = lane & 1;
      uint2 mine_hi, mine_lo;
      __builtin_memcpy(&mine_hi, &hi, 8); __builtin_memcpy(&mine_lo, &lo, 8);
      const uint2 send = odd ? mine_hi : mine_lo;
      uint2 recv;
      recv.x = (unsigned)__shfl_xor((int)send.x, 1, 64); recv.y = (unsigned)__shfl_xor((int)send.y, 1, 64);
      const int c = (lane >> 1) * 8 + 256 * k;
      if (!odd) {
        const uint4 q = {mine_hi.x, mine_hi.y, recv.x, recv.y};
        *reinterpret_cast<uint4*>(o + c * 2) = q;
      } else if constexpr (MM == 3) {
        const uint4 q = {recv.x, recv.y, mine_lo.x, mine_lo.y};
        *reinterpret_cast<uint4*>(o + (C + c) * 2) = q;
      }
    }
  }
  if constexpr (MM == 3) g6d_range_record_block<4>(rng, amax);
}

// The output of a producer that may write a channel slice of wider 16-bit rows: channels [c_off, c_off + C) of rows of ld_out elements
// whose lo plane (pairs) lies `plane` elements after the hi plane.  Returns the slice's first byte, nullptr if it does not fit.
char* c16_slice_out(void* out, int C, int ld_out, int plane, int c_off, int math_mode) {
  const bool pairs = math_mode == 3;
  if (!out || !g6d_aligned16(out) || ((ld_out | plane | c_off) & 7) || c_off < 0 || ld_out < 1) return nullptr;
  if (pairs ? (plane < c_off + C || (long)plane + c_off + C > ld_out) : (c_off + C > ld_out)) return nullptr;
  return static_cast<char*>(out) + (long)c_off * 2;
}

// grid of a grid-stride pass over `total` work items: blocks of 256 threads, one item per thread up to 256 * 64 blocks
dim3 split16_grid(long total) { return dim3((unsigned)((total + 255) / 256 < 256 * 64 ? (total + 255) / 256 : 256 * 64)); }

// The launchers' common tail: launch(std::integral_constant<int, MM>, stream, range by value) for a validated math_mode (1..3).
template <typename Launch>
void split16_dispatch(int math_mode, const G6dRange16* range, g6d_stream_t stream, Launch launch) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  const G6dRange16 rng = range ? *range : G6dRange16{};
  if (math_mode == 1) launch(std::integral_constant<int, 1>{}, st, rng);
  else if (math_mode == 2) launch(std::integral_constant<int, 2>{}, st, rng);
  else launch(std::integral_constant<int, 3>{}, st, rng);
}

}  // namespace

extern "C" int g6d_product_split16_ex(const float* ref, const float* que, const float* scale, const float* shift, void* out, int qn, int D, int P,
                                      int C, int math_mode, const G6dRange16* range, g6d_stream_t stream) {
  if (!ref || !que || !scale || !shift || !out || qn < 1 || D < 1 || P < 1 || C < 8 || (C & 7) || math_mode < 1 || math_mode > 3 ||
      !g6d_aligned16(ref) || !g6d_aligned16(que) || !g6d_aligned16(scale) || !g6d_aligned16(shift) || !g6d_aligned16(out)) {
    g6d_set_error("product_split16: bad args (C % 8 == 0, 16-byte aligned pointers, math_mode 1..3)"); return G6D_EINVAL;
  }
  const long total = (long)qn * ((D + 7) / 8) * P * (C >> 3);                  // work items: runs of 8 hypotheses
  split16_dispatch(math_mode, range, stream, [&](auto mm, hipStream_t st, const G6dRange16& rng) {
    hipLaunchKernelGGL(product_split_kernel<decltype(mm)::value>, split16_grid(total), dim3(256), 0, st, ref, que, scale, shift, static_cast<char*>(out), D, P,
                       C, total, rng);
  });
  return g6d_check_launch("product_split16");
}

extern "C" int g6d_product_split16(const float* ref, const float* que, const float* scale, const float* shift, void* out, int qn, int D, int P, int C,
                                   int math_mode, g6d_stream_t stream) {
  return g6d_product_split16_ex(ref, que, scale, shift, out, qn, D, P, C, math_mode, nullptr, stream);
}

extern "C" int g6d_affine_split16_to(const float* in, int ld_in, const float* scale, const float* shift, int affine_per_n, int relu, int pool, int N, int H,
                                     int W, int C, void* out, int ld_out, int plane, int c_off, int math_mode, const G6dRange16* range,
                                     g6d_stream_t stream) {
  if (!in || !out || N < 1 || H < 1 || W < 1 || C < 8 || (C & 7) || ld_in < C || (ld_in & 3) || (scale && !shift) || affine_per_n < 0 || math_mode < 1 ||
      math_mode > 3 || (pool && ((H | W) & 1)) || !g6d_aligned16(in) || !g6d_aligned16(out) || (scale && (!g6d_aligned16(scale) || !g6d_aligned16(shift)))) {
    g6d_set_error("affine_split16: bad args (C % 8 == 0, 16-byte aligned rows, even map with pooling, math_mode 1..3)"); return G6D_EINVAL;
  }
  char* o = c16_slice_out(out, C, ld_out, plane, c_off, math_mode);
  if (!o) { g6d_set_error("affine_split16: the channel slice does not fit the output rows (multiples of 8, c_off + C <= plane, plane + c_off + C <= ld_out)"); return G6D_EINVAL; }
  const long total = (long)N * (pool ? H / 2 : H) * (pool ? W / 2 : W) * (C >> 3);
  split16_dispatch(math_mode, range, stream, [&](auto mm, hipStream_t st, const G6dRange16& rng) {
    hipLaunchKernelGGL(affine_split16_kernel<decltype(mm)::value>, split16_grid(total), dim3(256), 0, st, in, ld_in, scale, shift, affine_per_n, relu, pool, H, W,
                       C, o, ld_out, plane, total, rng);
  });
  return g6d_check_launch("affine_split16");
}

extern "C" int g6d_affine_split16_ex(const float* in, int ld_in, const float* scale, const float* shift, int affine_per_n, int relu, int pool, int N, int H,
                                     int W, int C, void* out, int math_mode, const G6dRange16* range, g6d_stream_t stream) {
  return g6d_affine_split16_to(in, ld_in, scale, shift, affine_per_n, relu, pool, N, H, W, C, out, math_mode == 3 ? 2 * C : C, C, 0, math_mode, range, stream);
}

extern "C" int g6d_upsample_bilinear_split16(const float* in, int ld_in, const float* scale, const float* shift, int affine_per_n, int N, int H, int W, int C,
                                             int factor, void* out, int ld_out, int plane, int c_off, int math_mode, const G6dRange16* range,
                                             g6d_stream_t stream) {
  if (!in || !out || N < 1 || H < 1 || W < 1 || C < 8 || (C & 7) || ld_in < C || (ld_in & 3) || (scale && !shift) || affine_per_n < 0 || factor < 1 ||
      math_mode < 1 || math_mode > 3 || !g6d_aligned16(in) || (scale && (!g6d_aligned16(scale) || !g6d_aligned16(shift)))) {
    g6d_set_error("upsample_bilinear_split16: bad args (C % 8 == 0, 16-byte aligned rows, factor >= 1, math_mode 1..3)"); return G6D_EINVAL;
  }
  if ((long)H * factor > 0x7fffffffL || (long)W * factor > 0x7fffffffL) {
    g6d_set_error("upsample_bilinear_split16: bad args (H * factor and W * factor within an int)"); return G6D_EINVAL;
  }
  char* o = c16_slice_out(out, C, ld_out, plane, c_off, math_mode);
  if (!o) { g6d_set_error("upsample_bilinear_split16: the channel slice does not fit the output rows (multiples of 8, c_off + C <= plane, plane + c_off + C <= ld_out)"); return G6D_EINVAL; }
  const long total = (long)N * H * factor * W * factor * (C >> 3);
  split16_dispatch(math_mode, range, stream, [&](auto mm, hipStream_t st, const G6dRange16& rng) {
    hipLaunchKernelGGL(upsample_split16_kernel<decltype(mm)::value>, split16_grid(total), dim3(256), 0, st, in, ld_in, scale, shift, affine_per_n, H, W, C, factor,
                       o, ld_out, plane, total, rng);
  });
  return g6d_check_launch("upsample_bilinear_split16");
}

extern "C" int g6d_l2norm_split16(const float* in, int ld_in, int rows, int C, void* out, int math_mode, const G6dRange16* range, g6d_stream_t stream) {
  if (!in || !out || rows < 1 || (C != 256 && C != 512) || ld_in < C || (ld_in & 3) || math_mode < 1 || math_mode > 3 || !g6d_aligned16(in) || !g6d_aligned16(out)) {
    g6d_set_error("l2norm_split16: bad args (C = 256 or 512, 16-byte aligned rows, math_mode 1..3)"); return G6D_EINVAL;
  }
  if (rows > 0x7fffffff - 3) { g6d_set_error("l2norm_split16: bad args (rows + 3 within an int)"); return G6D_EINVAL; }
  const dim3 grid((rows + 3) / 4);
  char* o = static_cast<char*>(out);
  split16_dispatch(math_mode, range, stream, [&](auto mm, hipStream_t st, const G6dRange16& rng) {
    constexpr int MM = decltype(mm)::value;
    if (C == 256) hipLaunchKernelGGL((l2norm_split16_kernel<MM, 1>), grid, dim3(256), 0, st, in, ld_in, rows, o, rng);
    else hipLaunchKernelGGL((l2norm_split16_kernel<MM, 2>), grid, dim3(256), 0, st, in, ld_in, rows, o, rng);
  });
  return g6d_check_launch("l2norm_split16");
}

extern "C" int g6d_affine_split16(const float* in, int ld_in, const float* scale, const float* shift, int affine_per_n, int relu, int pool, int N, int H, int W,
                                  int C, void* out, int math_mode, g6d_stream_t stream) {
  return g6d_affine_split16_ex(in, ld_in, scale, shift, affine_per_n, relu, pool, N, H, W, C, out, math_mode, nullptr, stream);
}
