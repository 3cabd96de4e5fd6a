// Test infrastructure: builds the tracking part of gen6d_amd/csrc/pose_algebra.h (box projection, weighted corner mean, PnP) for the
// HOST (g++) and exposes it to ctypes for tests/test_track_algebra_cpu.py.  Not part of the product library.
#include "../gen6d_amd/csrc/pose_algebra.h"
using namespace pa;
static M3 m3(const double* p) { M3 r; for (int i = 0; i < 9; ++i) r.m[i] = p[i]; return r; }
static P34 p34(const double* p) { P34 r; for (int i = 0; i < 12; ++i) r.m[i] = p[i]; return r; }
extern "C" {
void t_box_project(const double* box, const double* pose, const double* K, double* uv) { box_project(box, p34(pose), m3(K), uv); }
// frames [n][8][2], oldest first, pushed one by one into a ring of `num` frames as track_commit does; -> the mean over the ring [8][2]
void t_weighted(const double* frames, int n, int num, double std, double* out) {
  double ring[64 * 16];
  for (int f = 0; f + 1 < n; ++f)
    for (int k = 0; k < 16; ++k) ring[(f % num) * 16 + k] = frames[f * 16 + k];
  const int newest = (n - 1) % num;
  for (int c = 0; c < 8; ++c)
    weighted_corner(ring, num, newest, n < num ? n : num, std, c, frames[(n - 1) * 16 + 2 * c], frames[(n - 1) * 16 + 2 * c + 1],
                    out[2 * c], out[2 * c + 1]);
}
int t_pnp(const double* box, const double* uv, const double* K, const double* init, double* out) {
  P34 p;
  const int it = pnp_lm(box, uv, 0, 8, m3(K), p34(init), p, NoReduce{});
  for (int i = 0; i < 12; ++i) out[i] = p.m[i];
  return it;
}
// normal-equation sums at a pose: J^T J (upper triangle, 21), J^T r (6), error (1)
void t_pnp_sums(const double* box, const double* uv, const double* K, const double* pose, double* acc) {
  const P34 p = p34(pose);
  const V3 r = rot_log(rot_of(p));
  const double x[6] = {r.x, r.y, r.z, p.m[3], p.m[7], p.m[11]};
  pnp_sums(box, uv, 0, 8, x, m3(K), acc, NoReduce{});
}
void t_rodrigues(const double* r, double* R) { const M3 m = rodrigues(V3{r[0], r[1], r[2]}); for (int i = 0; i < 9; ++i) R[i] = m.m[i]; }
void t_rot_log(const double* R, double* r) { const V3 v = rot_log(m3(R)); r[0] = v.x; r[1] = v.y; r[2] = v.z; }
}
