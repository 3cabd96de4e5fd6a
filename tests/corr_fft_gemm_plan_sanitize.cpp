// A stand-alone program (no Python in the process) that walks the product kernel's part of gen6d_amd/csrc/corr_fft_plan.h over the same
// axes as tests/test_corr_fft_gemm_plan_cpu.py: M = 1 .. 600, Cin = 32 .. 512 in steps of 32.  The test builds it with
// -fsanitize=address,undefined and expects "0 broken".
#include "corr_fft_gemm_plan_shim.cpp"

#include <cstdio>

int main() {
  int broken = 0, walked = 0;
  const int bins = cfft::bins(32);
  for (int M = 1; M <= 600; ++M) {
    int shape[10];
    g_shape(M, shape);
    std::vector<int> hit((size_t)bins * M, 0), clamp((size_t)bins * M, 0);
    const int rc = g_cover(M, bins, hit.data(), clamp.data());
    bool ok = rc == 0 && shape[5] <= cfft::LDS_LIMIT && shape[8] <= shape[2] && shape[8] % cfft::GEMM_WAVE_ROWS == 0 && shape[3] * shape[8] >= M &&
              (shape[3] - 1) * shape[8] < M;
    int live = 0;                                                    // waves with rows, per bin
    for (int mb = 0; mb < shape[3]; ++mb)
      for (int wv = 0; wv < shape[0]; ++wv) live += !cfft::gemm_wave_idle(mb, wv, shape[8], M);
    ok = ok && live == (M + cfft::GEMM_WAVE_ROWS - 1) / cfft::GEMM_WAVE_ROWS;
    long long asked = 0;
    for (size_t i = 0; i < hit.size(); ++i) { ok = ok && hit[i] == 1; asked += clamp[i]; }
    ok = ok && asked == (long long)bins * live * cfft::GEMM_A_PIECES * 64;
    if (!ok) { std::printf("M = %d: cover %d\n", M, rc); ++broken; }
    ++walked;
  }
  for (int waves : {2, 4}) {
    if (int rc = g_stage_image(waves)) { std::printf("stage image of %d waves: rule %d\n", waves, rc); ++broken; }
    for (int Cin = 32; Cin <= 512; Cin += 32) {
      int peak = 0;
      const int rc = g_ring(waves, g_steps(Cin), &peak);
      if (rc || peak > cfft::gemm_stages(waves) - 1) { std::printf("ring of %d waves, Cin = %d: rule %d, peak %d\n", waves, Cin, rc, peak); ++broken; }
      ++walked;
    }
  }
  int extra[2];
  if (g_conflicts(extra) || extra[0] || extra[1]) { std::printf("fragment reads: %d + %d extra LDS cycles\n", extra[0], extra[1]); ++broken; }
  std::printf("corr_fft gemm plan: %d cases, %d broken\n", walked, broken);
  return broken ? 1 : 0;
}
