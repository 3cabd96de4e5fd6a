// Test infrastructure: builds the track-health part of gen6d_amd/csrc/pose_algebra.h (gates, state updates) for the HOST (g++) and
// exposes it to ctypes for tests/test_track_health_cpu.py.  Not part of the product library.
#include "../gen6d_amd/csrc/pose_algebra.h"
using namespace pa;
static M3 m3(const double* p) { M3 r; for (int i = 0; i < 9; ++i) r.m[i] = p[i]; return r; }
static P34 p34(const double* p) { P34 r; for (int i = 0; i < 12; ++i) r.m[i] = p[i]; return r; }
extern "C" {
int h_finite(const double* pose) { return pose_finite(p34(pose)) ? 1 : 0; }
// prev may be NULL (an acquisition); gates = (min_px, max_px, margin, max_rot_deg, max_shift, max_log2_scale); -> flags, m[7]
int h_gates(const double* prev, const double* cur, const double* K, double w, double h, const double* c, double diameter,
            const double* gates, double* m) {
  const HealthGates g{gates[0], gates[1], gates[2], gates[3], gates[4], gates[5]};
  const V3 cc{c[0], c[1], c[2]};
  if (!prev) return health_gates(nullptr, p34(cur), m3(K), w, h, cc, diameter, g, m);
  const P34 pp = p34(prev);
  return health_gates(&pp, p34(cur), m3(K), w, h, cc, diameter, g, m);
}
// row[4] in place; out = (commit, draw)
void h_update(int f, int reset, int patience, int* row, int* out) {
  bool cm, dr;
  health_update(f, reset != 0, patience, row, cm, dr);
  out[0] = cm; out[1] = dr;
}
int h_verify(const double* det, const double* pose, const double* K, const double* c, double diameter, double ref_px, double max_shift,
             double max_log2_scale, double* m) {
  return verify_gates(det[0], det[1], det[2], p34(pose), m3(K), V3{c[0], c[1], c[2]}, diameter, ref_px, max_shift, max_log2_scale, m);
}
void h_verify_update(int f, int patience, int* row) { verify_update(f, patience, row); }
}
