// Micro-benchmark: the rate a bare stream of v_mfma_f32_32x32x16_f16 sustains on the whole chip (every CU, 1 or 2 waves per SIMD, NACC
// independent accumulators, milliseconds long so that the clock settles under the load), timed with HIP events.
// Second part: the fp16 hi / lo pair product of conv16w_kernel (MM = 3) on the two MFMA shapes at the same work per wave — a 128 px x 32 ch
// tile (4 x 1 accumulators of 32 x 32, or 8 x 2 of 16 x 16), one "tap" = 32 input channels = 24 MFMAs 32x32x16 or 48 MFMAs 16x16x32,
// terms hi x hi, hi x lo, lo x hi — with the A fragments in registers or re-read from LDS by ds_read_b128 (16 reads per tap in both
// shapes, one m-tile's registers refilled right after its MFMAs issue, as in the kernel).  The two shapes alternate in one process.
//   hipcc -O3 --offload-arch=gfx950 tools/ubench/mfma16_peak.hip -o tools/ubench/mfma16_peak.bin && tools/ubench/mfma16_peak.bin
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <algorithm>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <int NACC, int WPS, int RANDOM>
__global__ void __launch_bounds__(256, WPS) k(float* out, int iters) {
  f32x16 acc[NACC];
  for (int a = 0; a < NACC; ++a) for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
  f16x8 x[4], y[2];
  unsigned h = threadIdx.x * 2654435761u + blockIdx.x * 40503u + 12345u;
  auto rnd = [&]() { h = h * 1664525u + 1013904223u; return RANDOM ? (_Float16)(((int)(h >> 9) & 0xffff) * (1.0f / 32768.0f) - 1.0f) : (_Float16)(1.0f + (h >> 30)); };
  for (int i = 0; i < 4; ++i) for (int e = 0; e < 8; ++e) x[i][e] = rnd();
  for (int i = 0; i < 2; ++i) for (int e = 0; e < 8; ++e) y[i][e] = rnd();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const int a = m % NACC;
      acc[a] = __builtin_amdgcn_mfma_f32_32x32x16_f16(x[(m >> 1) & 3], y[m & 1], acc[a], 0, 0, 0);
    }
  }
  float s = 0.f;
  for (int a = 0; a < NACC; ++a) for (int r = 0; r < 16; ++r) s += acc[a][r];
  out[blockIdx.x * 256 + threadIdx.x] = s;
}

template <int NACC, int WPS, int RANDOM> void run(float* out, int cus) {
  const int iters = 40000, blocks = cus * WPS;
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  hipLaunchKernelGGL((k<NACC, WPS, RANDOM>), dim3(blocks), dim3(256), 0, 0, out, 1000);
  hipDeviceSynchronize();
  hipEventRecord(e0);
  hipLaunchKernelGGL((k<NACC, WPS, RANDOM>), dim3(blocks), dim3(256), 0, 0, out, iters);
  hipEventRecord(e1); hipDeviceSynchronize();
  float ms; hipEventElapsedTime(&ms, e0, e1);
  const double flops = 2.0 * 32 * 32 * 16 * 16.0 * iters * 4 * blocks;
  const double cyc_at_24 = ms * 1e-3 * 2.4e9 / (16.0 * iters * WPS);
  printf("%s operands, accumulators %d, waves/SIMD %d: %.2f ms, %.0f TFLOP/s, %.1f cycles per MFMA and SIMD at 2.4 GHz\n", RANDOM ? "random" : "small-integer", NACC, WPS, ms, flops / ms * 1e-9, cyc_at_24);
}

// ---- the pair product on both shapes.  S16 = 0: v_mfma_f32_32x32x16_f16, 4 m-tiles x 2 channel halves = 8 groups of (2 planes, 3 MFMAs);
// S16 = 1: v_mfma_f32_16x16x32_f16, 8 m-tiles of (2 planes, 2 n-tiles x 3 MFMAs).  PAIR = 0: every operand random in [-1, 1); PAIR = 1:
// hi = fp16(x), lo = fp16(x - hi) of random fp32 x.  LDS = 1: a group's two A fragments are re-read from LDS (conflict-free, 1 KB per
// wave-instruction, the address alternating between two copies per tap) right after its MFMAs issue.
constexpr int PAIR_LDS = 32 * 1024;
template <int S16, int WPS, int PAIR, int LDS>
__global__ void __launch_bounds__(256, WPS) kp(const f16x8* src, float* out, int iters) {
  __shared__ __attribute__((aligned(16))) char lds[PAIR_LDS];
  const int lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < PAIR_LDS / 16; i += 256) reinterpret_cast<f16x8*>(lds)[i] = src[i];
  __syncthreads();
  unsigned h = threadIdx.x * 2654435761u + blockIdx.x * 40503u + 777u;
  auto rf = [&]() { h = h * 1664525u + 1013904223u; return (float)(int)(h >> 8) * (1.0f / 8388608.0f) - 1.0f; };
  auto operand = [&](f16x8& hi, f16x8& lo) {
    for (int e = 0; e < 8; ++e) {
      if (PAIR) { const float x = rf(); hi[e] = (_Float16)x; lo[e] = (_Float16)(x - (float)hi[e]); }
      else { hi[e] = (_Float16)rf(); lo[e] = (_Float16)rf(); }
    }
  };
  f16x8 a[8][2], b[2][2];                                      // A: group x plane; B: (S16 = 0: channel half, S16 = 1: n-tile) x plane
  for (int g = 0; g < 8; ++g) operand(a[g][0], a[g][1]);
  for (int j = 0; j < 2; ++j) operand(b[j][0], b[j][1]);
  f32x16 acc32[4];
  f32x4 acc16[8][2];
  for (int m = 0; m < 4; ++m) for (int r = 0; r < 16; ++r) acc32[m][r] = 0.f;
  for (int m = 0; m < 8; ++m) for (int n = 0; n < 2; ++n) for (int r = 0; r < 4; ++r) acc16[m][n][r] = 0.f;
  for (int it = 0; it < iters; ++it) {
    const int cp = ((it + 1) & 1) * 16384;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      if constexpr (S16 == 0) {
        const int mt = g & 3, hf = g >> 2;
        acc32[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[g][0], b[hf][0], acc32[mt], 0, 0, 0);
        acc32[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[g][0], b[hf][1], acc32[mt], 0, 0, 0);
        acc32[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[g][1], b[hf][0], acc32[mt], 0, 0, 0);
      } else {
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          acc16[g][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[g][0], b[n][0], acc16[g][n], 0, 0, 0);
          acc16[g][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[g][0], b[n][1], acc16[g][n], 0, 0, 0);
          acc16[g][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[g][1], b[n][0], acc16[g][n], 0, 0, 0);
        }
      }
      if constexpr (LDS) {
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) a[g][pl] = *reinterpret_cast<const f16x8*>(lds + cp + pl * 8192 + g * 1024 + lane * 16);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  float s = 0.f;
  for (int m = 0; m < 4; ++m) for (int r = 0; r < 16; ++r) s += acc32[m][r];
  for (int m = 0; m < 8; ++m) for (int n = 0; n < 2; ++n) for (int r = 0; r < 4; ++r) s += acc16[m][n][r];
  out[blockIdx.x * 256 + threadIdx.x] = s;
}

template <int S16, int WPS, int PAIR, int LDS> double run_pair(const f16x8* src, float* out, int cus, double* cyc) {
  const int iters = 20000, blocks = cus * WPS;
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  hipLaunchKernelGGL((kp<S16, WPS, PAIR, LDS>), dim3(blocks), dim3(256), 0, 0, src, out, 2000);
  hipDeviceSynchronize();
  hipEventRecord(e0);
  hipLaunchKernelGGL((kp<S16, WPS, PAIR, LDS>), dim3(blocks), dim3(256), 0, 0, src, out, iters);
  hipEventRecord(e1); hipDeviceSynchronize();
  float ms; hipEventElapsedTime(&ms, e0, e1);
  hipEventDestroy(e0); hipEventDestroy(e1);
  const double flops = 2.0 * 128 * 32 * 32 * 3.0 * iters * 4 * blocks;          // 128 px x 32 ch x 32 K x 3 terms per tap and wave
  *cyc = ms * 1e-3 * 2.4e9 / ((S16 ? 48.0 : 24.0) * iters * WPS);
  return flops / ms * 1e-9;
}

template <int WPS, int PAIR, int LDS> void row_pair(const f16x8* src, float* out, int cus) {
  constexpr int REP = 5;
  double t32[REP], t16[REP], c32[REP], c16[REP];
  for (int r = 0; r < REP; ++r) {
    t32[r] = run_pair<0, WPS, PAIR, LDS>(src, out, cus, &c32[r]);
    t16[r] = run_pair<1, WPS, PAIR, LDS>(src, out, cus, &c16[r]);
  }
  double q[REP];
  for (int r = 0; r < REP; ++r) q[r] = t16[r] / t32[r];
  auto med = [](double* v) { double w[REP]; std::copy(v, v + REP, w); std::sort(w, w + REP); return w[REP / 2]; };
  auto lo = [](double* v) { return *std::min_element(v, v + REP); };
  auto hi = [](double* v) { return *std::max_element(v, v + REP); };
  printf("| %s | %s | %d | %.0f (%.0f-%.0f) | %.1f | %.0f (%.0f-%.0f) | %.1f | %.3f (%.3f-%.3f) |\n", PAIR ? "pair-like" : "random", LDS ? "LDS" : "registers", WPS,
         med(t32), lo(t32), hi(t32), med(c32), med(t16), lo(t16), hi(t16), med(c16), med(q), lo(q), hi(q));
}

int main() {
  hipDeviceProp_t pr; hipGetDeviceProperties(&pr, 0);
  const int cus = pr.multiProcessorCount;
  printf("%s, %d CUs, clock %d kHz\n", pr.name, cus, pr.clockRate);
  float* out; hipMalloc(&out, 4 << 20);
  run<8, 1, 0>(out, cus); run<8, 2, 0>(out, cus); run<8, 1, 1>(out, cus); run<8, 2, 1>(out, cus); run<8, 2, 1>(out, cus); run<8, 2, 0>(out, cus);

  // LDS contents: pair-like fragments (hi plane, lo plane) of random fp32 values
  f16x8 hsrc[PAIR_LDS / 16];
  unsigned h = 99991u;
  for (int i = 0; i < PAIR_LDS / 16; ++i)
    for (int e = 0; e < 8; ++e) {
      h = h * 1664525u + 1013904223u;
      const float x = (float)(int)(h >> 8) * (1.0f / 8388608.0f) - 1.0f;
      const _Float16 hv = (_Float16)x;
      hsrc[i][e] = ((i * 16) & 8192) ? (_Float16)(x - (float)hv) : hv;
    }
  f16x8* src; hipMalloc(&src, PAIR_LDS); hipMemcpy(src, hsrc, PAIR_LDS, hipMemcpyHostToDevice);
  printf("\nfp16 pair product, 128 px x 32 ch per wave, one tap = 32 input channels x 3 terms; TFLOP/s median (min-max) of 5 alternated runs\n");
  printf("| operands | A fragments | waves/SIMD | 32x32x16 TFLOP/s | cyc/MFMA @2.4 | 16x16x32 TFLOP/s | cyc/MFMA @2.4 | 16x16x32 / 32x32x16 |\n");
  printf("|---|---|---|---|---|---|---|---|\n");
  row_pair<1, 0, 0>(src, out, cus); row_pair<2, 0, 0>(src, out, cus);
  row_pair<1, 1, 0>(src, out, cus); row_pair<2, 1, 0>(src, out, cus);
  row_pair<1, 0, 1>(src, out, cus); row_pair<2, 0, 1>(src, out, cus);
  row_pair<1, 1, 1>(src, out, cus); row_pair<2, 1, 1>(src, out, cus);
  hipFree(src); hipFree(out);
  return 0;
}
