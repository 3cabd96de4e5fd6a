// Track health of the multi-stream tracker (gen6d_amd/tracking.py HealthPolicy): the state machine that tells a stream
// that still follows its object from one that lost it, run on the device between the launches of a tick so that no host round trip sits
// between a frame's refinement and its commit.  Latency-class kernels: one thread per slot (a wave serves 64 slots), float64 arithmetic
// on the float32 tables as in track_commit; the arithmetic lives in pose_algebra.h, which also builds for the host
// (tests/track_health_shim.cpp).  Per-stream tables beside pose_table: health [S][4] int32 = (status, bad, vbad, flags) and
// measures [S][12] float32.  Within one launch no two slots name the same stream, so every table row has one writer.
#include "g6d_common.h"
#include "pose_algebra.h"

namespace {

using namespace pa;

__device__ __forceinline__ M3 ld_m3(const float* p) { M3 r; for (int i = 0; i < 9; ++i) r.m[i] = p[i]; return r; }
__device__ __forceinline__ P34 ld_p34(const float* p) { P34 r; for (int i = 0; i < 12; ++i) r.m[i] = p[i]; return r; }

// Before the gather: a LOST stream, or one whose table row is not finite, is parked like an unused slot.
__global__ void __launch_bounds__(64) track_gate_kernel(const float* __restrict__ pose_table, int* __restrict__ health,
                                                        const int* __restrict__ slot_stream, int* __restrict__ slot_eff, int batch) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= batch) return;
  const int s = slot_stream[b];
  int eff = -1;
  if (s >= 0) {
    int* row = health + (size_t)4 * s;
    if (row[0] != TH_LOST) {
      if (pose_finite(ld_p34(pose_table + (size_t)12 * s))) eff = s;
      else { row[0] = TH_LOST; row[3] = THF_NONFINITE; }
    }
  }
  slot_eff[b] = eff;
}

// After the refinement, before the commit: gates, state update, and the slot maps of the commit and of the emit.
__global__ void __launch_bounds__(64) track_health_kernel(const float* __restrict__ pose_prev, const float* __restrict__ pose_new,
                                                          const float* __restrict__ Ks, const int* __restrict__ pic, int W, int H,
                                                          const int* __restrict__ slot_eff, int reset, const float* __restrict__ center,
                                                          double diameter, int patience, HealthGates g, int* __restrict__ health,
                                                          float* __restrict__ measures, int* __restrict__ slot_commit,
                                                          int* __restrict__ slot_draw, int batch) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= batch) return;
  const int s = slot_eff[b];
  int commit = -1, draw = -1;
  if (s >= 0) {
    const double w = pic ? (double)pic[2 * b] : (double)W, h = pic ? (double)pic[2 * b + 1] : (double)H;
    const V3 c{center[0], center[1], center[2]};
    const P34 cur = ld_p34(pose_new + 12 * b);
    const M3 K = ld_m3(Ks + 9 * b);
    double m[7];
    int f;
    if (reset) {
      f = health_gates(nullptr, cur, K, w, h, c, diameter, g, m);
    } else {
      const P34 prev = ld_p34(pose_prev + 12 * b);
      f = health_gates(&prev, cur, K, w, h, c, diameter, g, m);
    }
    int* hrow = health + (size_t)4 * s;
    int row[4] = {hrow[0], hrow[1], hrow[2], hrow[3]};
    bool cm, dr;
    health_update(f, reset != 0, patience, row, cm, dr);
    for (int i = 0; i < 4; ++i) hrow[i] = row[i];
    float* mrow = measures + (size_t)12 * s;
    for (int i = 0; i < 7; ++i) mrow[i] = (float)m[i];
    if (cm) commit = s;
    if (dr) draw = s;
  }
  slot_commit[b] = commit;
  slot_draw[b] = draw;
}

// The detector's check of the slots committed in this tick, against the stream's committed raw pose.
__global__ void __launch_bounds__(64) track_verify_kernel(const float* __restrict__ det, const float* __restrict__ pose_table,
                                                          const float* __restrict__ Ks, const int* __restrict__ slot_commit,
                                                          const float* __restrict__ center, double diameter, double ref_px,
                                                          double max_shift, double max_log2_scale, int patience, int* __restrict__ health,
                                                          float* __restrict__ measures, int batch) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= batch) return;
  const int s = slot_commit[b];
  if (s < 0) return;
  double m[2];
  const int f = verify_gates(det[5 * b], det[5 * b + 1], det[5 * b + 2], ld_p34(pose_table + (size_t)12 * s), ld_m3(Ks + 9 * b),
                             V3{center[0], center[1], center[2]}, diameter, ref_px, max_shift, max_log2_scale, m);
  int* hrow = health + (size_t)4 * s;
  int row[4] = {hrow[0], hrow[1], hrow[2], hrow[3]};
  verify_update(f, patience, row);
  for (int i = 0; i < 4; ++i) hrow[i] = row[i];
  measures[(size_t)12 * s + 7] = (float)m[0];
  measures[(size_t)12 * s + 8] = (float)m[1];
}

}  // namespace

#define HEALTH_STREAM(s) reinterpret_cast<hipStream_t>(s)

extern "C" int g6d_track_gate(const float* pose_table, int32_t* health, const int* slot_stream, int* slot_eff, int batch,
                              g6d_stream_t stream) {
  if (!pose_table || !health || !slot_stream || !slot_eff || batch < 1) { g6d_set_error("track_gate: bad args"); return G6D_EINVAL; }
  if (batch > 0x7fffffff - 63) { g6d_set_error("track_gate: bad args (batch + 63 within an int)"); return G6D_EINVAL; }
  hipLaunchKernelGGL(track_gate_kernel, dim3((batch + 63) / 64), dim3(64), 0, HEALTH_STREAM(stream), pose_table, health, slot_stream,
                     slot_eff, batch);
  return g6d_check_launch("track_gate");
}

extern "C" int g6d_track_health(const float* pose_prev, const float* pose_new, const float* K, const int32_t* pic, int W, int H,
                                const int* slot_eff, int reset, const float* center, double diameter, int patience, double min_px,
                                double max_px, double margin, double max_rot_deg, double max_shift, double max_log2_scale,
                                int32_t* health, float* measures, int* slot_commit, int* slot_draw, int batch, g6d_stream_t stream) {
  if ((!pose_prev && !reset) || !pose_new || !K || (!pic && (W < 1 || H < 1)) || !slot_eff || !center || !(diameter > 0) ||
      patience < 1 || !health || !measures || !slot_commit || !slot_draw || batch < 1) {
    g6d_set_error("track_health: bad args (pose_prev unless reset, pic or W, H >= 1, diameter > 0, patience >= 1)"); return G6D_EINVAL;
  }
  const pa::HealthGates g{min_px, max_px, margin, max_rot_deg, max_shift, max_log2_scale};
  if (batch > 0x7fffffff - 63) { g6d_set_error("track_health: bad args (batch + 63 within an int)"); return G6D_EINVAL; }
  hipLaunchKernelGGL(track_health_kernel, dim3((batch + 63) / 64), dim3(64), 0, HEALTH_STREAM(stream), pose_prev, pose_new, K, pic, W, H,
                     slot_eff, reset ? 1 : 0, center, diameter, patience, g, health, measures, slot_commit, slot_draw, batch);
  return g6d_check_launch("track_health");
}

extern "C" int g6d_track_verify(const float* det, const float* pose_table, const float* K, const int* slot_commit, const float* center,
                                double diameter, double ref_px, double verify_shift, double verify_log2_scale, int verify_patience,
                                int32_t* health, float* measures, int batch, g6d_stream_t stream) {
  if (!det || !pose_table || !K || !slot_commit || !center || !(diameter > 0) || !(ref_px > 0) || verify_patience < 1 || !health ||
      !measures || batch < 1) {
    g6d_set_error("track_verify: bad args (diameter, ref_px > 0, verify_patience >= 1)"); return G6D_EINVAL;
  }
  if (batch > 0x7fffffff - 63) { g6d_set_error("track_verify: bad args (batch + 63 within an int)"); return G6D_EINVAL; }
  hipLaunchKernelGGL(track_verify_kernel, dim3((batch + 63) / 64), dim3(64), 0, HEALTH_STREAM(stream), det, pose_table, K, slot_commit,
                     center, diameter, ref_px, verify_shift, verify_log2_scale, verify_patience, health, measures, batch);
  return g6d_check_launch("track_verify");
}
