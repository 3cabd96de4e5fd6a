// Pose / 2-D similarity algebra between the stages of Gen6DEstimator.predict, written once for the device kernels of
// pose_chain.hip and for the host build that tests/test_pose_chain_cpu.py checks against gen6d_amd/geometry.py and the
// golden vectors of the reference's own utils (tests/golden/geometry.npz).  float64 throughout, a few hundred flops per
// query.  Each function names the reference function whose contract it keeps.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define PA_HD __host__ __device__ __forceinline__
#else
#define PA_HD inline
#endif

namespace pa {

struct M3 { double m[9]; };     // row-major 3x3
struct P34 { double m[12]; };   // row-major [R|t]
struct V3 { double x, y, z; };

PA_HD M3 eye3() { return M3{{1, 0, 0, 0, 1, 0, 0, 0, 1}}; }
PA_HD M3 mul(const M3& a, const M3& b) {
  M3 c;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) c.m[i * 3 + j] = a.m[i * 3] * b.m[j] + a.m[i * 3 + 1] * b.m[3 + j] + a.m[i * 3 + 2] * b.m[6 + j];
  return c;
}
PA_HD M3 tr(const M3& a) { return M3{{a.m[0], a.m[3], a.m[6], a.m[1], a.m[4], a.m[7], a.m[2], a.m[5], a.m[8]}}; }
PA_HD V3 mulv(const M3& a, const V3& v) {
  return V3{a.m[0] * v.x + a.m[1] * v.y + a.m[2] * v.z, a.m[3] * v.x + a.m[4] * v.y + a.m[5] * v.z,
            a.m[6] * v.x + a.m[7] * v.y + a.m[8] * v.z};
}
PA_HD double det3(const M3& a) {
  return a.m[0] * (a.m[4] * a.m[8] - a.m[5] * a.m[7]) - a.m[1] * (a.m[3] * a.m[8] - a.m[5] * a.m[6]) +
         a.m[2] * (a.m[3] * a.m[7] - a.m[4] * a.m[6]);
}
PA_HD M3 inv3(const M3& a) {
  const double d = 1.0 / det3(a);
  M3 r;
  r.m[0] = (a.m[4] * a.m[8] - a.m[5] * a.m[7]) * d; r.m[1] = (a.m[2] * a.m[7] - a.m[1] * a.m[8]) * d; r.m[2] = (a.m[1] * a.m[5] - a.m[2] * a.m[4]) * d;
  r.m[3] = (a.m[5] * a.m[6] - a.m[3] * a.m[8]) * d; r.m[4] = (a.m[0] * a.m[8] - a.m[2] * a.m[6]) * d; r.m[5] = (a.m[2] * a.m[3] - a.m[0] * a.m[5]) * d;
  r.m[6] = (a.m[3] * a.m[7] - a.m[4] * a.m[6]) * d; r.m[7] = (a.m[1] * a.m[6] - a.m[0] * a.m[7]) * d; r.m[8] = (a.m[0] * a.m[4] - a.m[1] * a.m[3]) * d;
  return r;
}
PA_HD double norm3(const V3& v) { return sqrt(v.x * v.x + v.y * v.y + v.z * v.z); }
PA_HD V3 sub(const V3& a, const V3& b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
PA_HD V3 add(const V3& a, const V3& b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
PA_HD V3 scl(const V3& a, double s) { return V3{a.x * s, a.y * s, a.z * s}; }
PA_HD double f32(double v) { return (double)(float)v; }          // where the reference rounds to float32 on the way

PA_HD M3 rot_of(const P34& p) { return M3{{p.m[0], p.m[1], p.m[2], p.m[4], p.m[5], p.m[6], p.m[8], p.m[9], p.m[10]}}; }
PA_HD V3 trans_of(const P34& p) { return V3{p.m[3], p.m[7], p.m[11]}; }
PA_HD P34 make_pose(const M3& R, const V3& t) {
  return P34{{R.m[0], R.m[1], R.m[2], t.x, R.m[3], R.m[4], R.m[5], t.y, R.m[6], R.m[7], R.m[8], t.z}};
}
// base_utils.py:502-505
PA_HD P34 pose_inverse(const P34& p) { const M3 Rt = tr(rot_of(p)); return make_pose(Rt, scl(mulv(Rt, trans_of(p)), -1.0)); }
// base_utils.py:512-521: apply p0 first, then p1
PA_HD P34 pose_compose(const P34& p0, const P34& p1) {
  const M3 R1 = rot_of(p1);
  return make_pose(mul(R1, rot_of(p0)), add(mulv(R1, trans_of(p0)), trans_of(p1)));
}
PA_HD V3 pose_apply(const P34& p, const V3& x) { return add(mulv(rot_of(p), x), trans_of(p)); }
// base_utils.py:256-265 for one point: pixel (u, v) and depth; 0 < |depth| < 1e-4 clamped to 1e-4
PA_HD void project_point(const V3& x, const P34& p, const M3& K, double& u, double& v, double& depth) {
  const V3 c = mulv(K, pose_apply(p, x));
  double d = c.z;
  if (fabs(d) < 1e-4 && fabs(d) > 0) d = 1e-4;
  u = c.x / d; v = c.y / d; depth = d;
}
// dataset/database.py:399-410 (results are float32 in the reference)
PA_HD P34 normalize_pose(const P34& p, double scale, const V3& off) {
  const M3 R = rot_of(p);
  const V3 t = add(mulv(R, scl(off, -1.0)), scl(trans_of(p), scale));
  P34 r = make_pose(R, t);
  for (int i = 0; i < 12; ++i) r.m[i] = f32(r.m[i]);
  return r;
}
PA_HD P34 denormalize_pose(const P34& p, double scale, const V3& off) {
  const M3 R = rot_of(p);
  const V3 t = add(scl(mulv(R, off), 1.0 / scale), scl(trans_of(p), 1.0 / scale));
  P34 r = make_pose(R, t);
  for (int i = 0; i < 12; ++i) r.m[i] = f32(r.m[i]);
  return r;
}

PA_HD M3 rot_x(double a) { const double c = cos(a), s = sin(a); return M3{{1, 0, 0, 0, c, -s, 0, s, c}}; }
PA_HD M3 rot_y(double a) { const double c = cos(a), s = sin(a); return M3{{c, 0, s, 0, 1, 0, -s, 0, c}}; }
PA_HD M3 rot_z(double a) { const double c = cos(a), s = sin(a); return M3{{c, -s, 0, s, c, 0, 0, 0, 1}}; }
// base_utils.py:657-666: euler2mat(atan y,'sxyz') @ euler2mat(-atan x,'syxz')
PA_HD M3 look_at_rotation(double x, double y) { return mul(rot_x(atan2(y, 1.0)), rot_y(-atan2(x, 1.0))); }
// first angle of transforms3d.mat2euler(R, 'szyx') (pose_utils.py:96-99)
PA_HD double angle_about_z(const M3& R) {
  const double cy = sqrt(R.m[8] * R.m[8] + R.m[5] * R.m[5]);
  if (cy > 2.220446049250313e-16 * 4.0) return -atan2(R.m[1], R.m[0]);
  return atan2(R.m[3], R.m[4]);
}
// transforms3d.quaternions.quat2mat (w, x, y, z), used at pose_utils.py:239
PA_HD M3 quat2mat(double w, double x, double y, double z) {
  const double n = w * w + x * x + y * y + z * z;
  if (n < 2.220446049250313e-16) return eye3();
  const double s = 2.0 / n, X = x * s, Y = y * s, Z = z * s;
  const double wX = w * X, wY = w * Y, wZ = w * Z, xX = x * X, xY = x * Y, xZ = x * Z, yY = y * Y, yZ = y * Z, zZ = z * Z;
  return M3{{1.0 - (yY + zZ), xY - wZ, xZ + wY, xY + wZ, 1.0 - (xX + zZ), yZ - wX, xZ - wY, yZ + wX, 1.0 - (xX + yY)}};
}

// ---- 2-D similarities stored as 3x3 with last row (0,0,1)
PA_HD M3 sim2d(double scale, double angle, double ox, double oy) {
  const double c = cos(angle) * scale, s = sin(angle) * scale;
  return M3{{c, -s, ox, s, c, oy, 0, 0, 1}};
}
// transformation_crop's M (base_utils.py:646-653): centre on `position`, scale, rotate, move to the crop centre
PA_HD M3 crop_transform(double px, double py, double scale, double angle, double size) {
  M3 m = sim2d(1.0, 0.0, -px, -py);
  m = mul(sim2d(scale, 0.0, 0, 0), m);
  m = mul(sim2d(1.0, angle, 0, 0), m);
  return mul(sim2d(1.0, 0.0, size / 2, size / 2), m);
}

// pose_utils.py:55-61
PA_HD void let_me_look_at_2d(double cx, double cy, const M3& K, M3& R, double& f) {
  const double f_raw = (K.m[0] + K.m[4]) / 2;
  const double x = cx - K.m[2], y = cy - K.m[5];
  R = look_at_rotation(x / f_raw, y / f_raw);
  f = sqrt(x * x + y * y + f_raw * f_raw);
}
// pose_utils.py:51-53
PA_HD void let_me_look_at(const P34& pose, const M3& K, const V3& center, M3& R, double& f) {
  double u, v, d;
  project_point(center, pose, K, u, v, d);
  let_me_look_at_2d(u, v, K, R, f);
}
// database_utils.py:8-25 without the image warp: K_new, pose_new, pose_rect, H (source -> crop homography)
PA_HD void look_at_crop_params(const M3& K, const P34& pose, double posx, double posy, double angle, double scale, double h,
                               double w, M3& K_new, P34& pose_new, P34& pose_rect, M3& H) {
  M3 R_new; double f_new;
  let_me_look_at_2d(posx, posy, K, R_new, f_new);
  R_new = mul(rot_z(angle), R_new);
  f_new *= scale;
  K_new = M3{{f32(f_new), 0, f32(w / 2), 0, f32(f_new), f32(h / 2), 0, 0, 1}};
  H = mul(mul(K_new, R_new), inv3(K));
  M3 Rr = R_new;
  for (int i = 0; i < 9; ++i) Rr.m[i] = f32(Rr.m[i]);
  pose_rect = make_pose(Rr, V3{0, 0, 0});
  pose_new = pose_compose(pose, pose_rect);
}
// pose_utils.py:63-102 for one (reference, query) pair
PA_HD void scale_rotation_difference(const P34& ref_pose, const P34& que_pose, const M3& ref_K, const M3& que_K, const V3& center,
                                     double& scale, double& angle) {
  M3 Rr, Rq; double fr, fq;
  let_me_look_at(ref_pose, ref_K, center, Rr, fr);
  let_me_look_at(que_pose, que_K, center, Rq, fq);
  const M3 ref_rot = mul(Rr, rot_of(ref_pose)), que_rot = mul(Rq, rot_of(que_pose));
  const double ref_dist = norm3(sub(trans_of(pose_inverse(ref_pose)), center));
  const double que_dist = norm3(sub(trans_of(pose_inverse(que_pose)), center));
  scale = ref_dist / que_dist * fq / fr;
  angle = angle_about_z(mul(que_rot, tr(ref_rot)));
}

// pose_utils.py:104-111 -> :12-49: query pose from detection (position, scale) + selected view and in-plane angle
PA_HD P34 pose_from_similarity(double px, double py, double scale_r2q, double angle_r2q, const P34& ref_pose, const M3& ref_K,
                               const M3& que_K, const V3& center) {
  double rcx, rcy, rd;
  project_point(center, ref_pose, ref_K, rcx, rcy, rd);
  M3 m = sim2d(1.0, 0.0, -px, -py);
  m = mul(sim2d(1.0 / scale_r2q, 0.0, 0, 0), m);
  m = mul(sim2d(1.0, -angle_r2q, 0, 0), m);
  const M3 m_q2r = mul(sim2d(1.0, 0.0, rcx, rcy), m);
  const M3 m_r2q = inv3(m_q2r);
  const V3 ref_cam = trans_of(pose_inverse(ref_pose));
  const V3 qc = mulv(m_r2q, V3{rcx, rcy, 1.0});
  V3 qn = mulv(inv3(que_K), V3{qc.x, qc.y, 1.0});
  qn.x /= qn.z; qn.y /= qn.z;
  const double scale = sqrt(m_r2q.m[0] * m_r2q.m[4] - m_r2q.m[1] * m_r2q.m[3]);
  const double rotation = atan2(m_r2q.m[3], m_r2q.m[0]);
  const double que_f = (que_K.m[0] + que_K.m[4]) / 2, ref_f = (ref_K.m[0] + ref_K.m[4]) / 2;
  const double que_f_ = sqrt(que_f * que_f + (qn.x * qn.x + qn.y * qn.y) * que_f * que_f);
  const double que_dist = norm3(sub(ref_cam, center)) * que_f_ / ref_f / scale;
  const V3 ray{qn.x, qn.y, 1.0};
  const V3 cen3d = scl(ray, que_dist / norm3(ray));
  const M3 que_rot = mul(tr(look_at_rotation(qn.x, qn.y)), mul(rot_z(rotation), rot_of(ref_pose)));
  return make_pose(que_rot, sub(cen3d, mulv(que_rot, center)));
}

// pose_utils.py:237-244
PA_HD P34 compose_sim_pose(double scale, const double quat[4], double offx, double offy, const P34& in_pose, const V3& center) {
  const M3 rotation = quat2mat(quat[0], quat[1], quat[2], quat[3]);
  const V3 cin = pose_apply(in_pose, center);
  const V3 cque{cin.x + offx, cin.y + offy, cin.z};
  M3 A = rotation;
  for (int i = 0; i < 9; ++i) A.m[i] *= scale;
  return make_pose(A, sub(cque, mulv(A, cin)));
}
// Orthogonal polar factor U V^T of A (= the `U @ Vt` of np.linalg.svd, reflections included) and the mean singular value,
// by Newton's iteration X <- (X + X^-T) / 2: A = (U V^T)(V S V^T), so trace((U V^T)^T A) = sum(S).
PA_HD void polar3(const M3& A, M3& Q, double& mean_sv) {
  Q = A;
  for (int it = 0; it < 60; ++it) {
    const M3 Xit = tr(inv3(Q));
    double diff = 0;
    M3 N;
    for (int i = 0; i < 9; ++i) { N.m[i] = 0.5 * (Q.m[i] + Xit.m[i]); diff += fabs(N.m[i] - Q.m[i]); }
    Q = N;
    if (diff < 1e-15) break;
  }
  const M3 P = mul(tr(Q), A);
  mean_sv = (P.m[0] + P.m[4] + P.m[8]) / 3.0;
}
// pose_utils.py:217-235
PA_HD P34 pose_sim_to_pose_rigid(const P34& sim, const P34& pose_in, const M3& K_que, const M3& K_in, const V3& center) {
  const double f_que = (K_que.m[0] + K_que.m[4]) / 2, f_in = (K_in.m[0] + K_in.m[4]) / 2;
  const V3 cin = pose_apply(pose_in, center);
  M3 Q; double msv;
  polar3(rot_of(sim), Q, msv);
  const double depth_que = cin.z / msv * f_que / f_in;
  const V3 csim = pose_apply(sim, cin);
  const V3 cque = scl(csim, depth_que / csim.z);
  const M3 rotation = mul(Q, rot_of(pose_in));
  return make_pose(rotation, sub(cque, mulv(rotation, center)));
}

// ---- one refinement step, before the network (reference network/refiner.py:275-313 with the database normalised):
//      pose_in is in the DATABASE frame; (nscale, noff) = NormalizedDatabase.scale / .offset; centre 0, diameter 2.
struct RefinePrep { M3 K_warp; P34 pose_warp, pose_rect; M3 H; };
PA_HD RefinePrep refine_prepare(const P34& pose_in_db, const M3& que_K, double nscale, const V3& noff, double size, double margin) {
  const V3 center{0, 0, 0};
  const P34 in_pose = normalize_pose(pose_in_db, nscale, noff);
  M3 Rl; double new_f;
  let_me_look_at(in_pose, que_K, center, Rl, new_f);
  const double in_dist = norm3(sub(trans_of(pose_inverse(in_pose)), center));
  const double scale = size * (1 - margin) / 2.0 * in_dist / new_f;
  double px, py, pd;
  project_point(center, in_pose, que_K, px, py, pd);
  RefinePrep r;
  look_at_crop_params(que_K, in_pose, px, py, 0.0, scale, size, size, r.K_warp, r.pose_warp, r.pose_rect, r.H);
  return r;
}
// One reference view aligned with the warped query (utils/database_utils.py:54-110, rectify_rot with input pose/K)
// angle_step > 0 (round 3, reference-feature caching): the in-plane angle is snapped to multiples of angle_step (radians), so that
// the aligned crop of a view is a function of (view, bucket) only and its features can be cached across refinement steps and queries;
// *bucket receives round(angle / angle_step) (0 when angle_step <= 0).  angle_step = 0 is the reference's exact alignment.
PA_HD void align_reference(const P34& ref_pose, const M3& ref_K, const P34& pose_warp, const M3& K_warp, double size, double margin,
                           M3& K_new, P34& pose_new, M3& H, double angle_step = 0.0, int* bucket = nullptr) {
  const V3 center{0, 0, 0};
  double cx, cy, cd;
  project_point(center, ref_pose, ref_K, cx, cy, cd);
  const double dist = norm3(sub(trans_of(pose_inverse(ref_pose)), center));
  M3 Rl; double f_look;
  let_me_look_at(ref_pose, ref_K, center, Rl, f_look);
  const double scale = size * (1 - margin) / 2.0 * dist / f_look;
  double s, angle;
  scale_rotation_difference(ref_pose, pose_warp, ref_K, K_warp, center, s, angle);
  int b = 0;
  if (angle_step > 0) { b = (int)floor(angle / angle_step + 0.5); angle = b * angle_step; }
  if (bucket) *bucket = b;
  P34 rect;
  look_at_crop_params(ref_K, ref_pose, cx, cy, angle, scale, size, size, K_new, pose_new, rect, H);
}
// After the network (refiner.py:327-341): (quaternion, offset, log2 scale) -> refined pose in the database frame
PA_HD P34 refine_update(const double quat[4], double offx, double offy, double log2_scale, const RefinePrep& g, double nscale,
                        const V3& noff) {
  const V3 center{0, 0, 0};
  const P34 sim = compose_sim_pose(exp2(log2_scale), quat, offx, offy, g.pose_warp, center);
  P34 pr = pose_sim_to_pose_rigid(sim, g.pose_warp, g.K_warp, g.K_warp, center);
  pr = pose_compose(pr, pose_inverse(g.pose_rect));
  return denormalize_pose(pr, nscale, noff);
}
// cosine between camera directions seen from the (normalised) object centre (database_utils.py:27-52)
PA_HD double view_cos(const P34& a, const P34& b) {
  const V3 ca = trans_of(pose_inverse(a)), cb = trans_of(pose_inverse(b));
  return (ca.x * cb.x + ca.y * cb.y + ca.z * cb.z) / (norm3(ca) * norm3(cb));
}

// ---- tracking (reference predict.py:49-72): the object's 3-D box projected under each frame's pose, the corners averaged over the last
//      frames with Gaussian weights (weighted_pts) and a pose solved back from the averaged corners (cv2.solvePnP, SOLVEPNP_ITERATIVE)
// The 8 box corners (box[8][3], utils/draw_utils.py pts_range_to_bbox_pts order) -> pixels uv[8][2], with project_point's depth clamp
PA_HD void box_project(const double* box, const P34& p, const M3& K, double* uv) {
  for (int c = 0; c < 8; ++c) {
    double d;
    project_point(V3{box[3 * c], box[3 * c + 1], box[3 * c + 2]}, p, K, uv[2 * c], uv[2 * c + 1], d);
  }
}
// predict.py weighted_pts: the frame i steps older than the newest has weight exp(-(i/std)^2); only the last `num` frames count
PA_HD double smooth_weight(int i, double std) { const double a = i / std; return exp(-a * a); }
// One corner's weighted mean over a ring of frames: ring[k][8][2] for k < num, the newest frame at k = newest, n frames held (n <= num).
// `cur` (u, v) is the newest frame's corner (passed in registers: the caller has just projected it).
PA_HD void weighted_corner(const double* ring, int num, int newest, int n, double std, int corner, double cu, double cv, double& u,
                           double& v) {
  double su = cu, sv = cv, sw = 1.0;
  for (int i = 1; i < n; ++i) {
    const int k = (newest - i + num) % num;
    const double w = smooth_weight(i, std);
    su += w * ring[(k * 8 + corner) * 2];
    sv += w * ring[(k * 8 + corner) * 2 + 1];
    sw += w;
  }
  u = su / sw; v = sv / sw;
}

// Rodrigues vector <-> rotation matrix (cv2.Rodrigues).  exp: R = I + A [r]x + B [r]x^2, A = sin(th)/th, B = (1-cos th)/th^2
PA_HD M3 skew(const V3& a) { return M3{{0, -a.z, a.y, a.z, 0, -a.x, -a.y, a.x, 0}}; }
PA_HD M3 rodrigues(const V3& r) {
  const double th2 = r.x * r.x + r.y * r.y + r.z * r.z, th = sqrt(th2);
  double A, B;
  if (th < 1e-2) { A = 1.0 - th2 / 6.0 + th2 * th2 / 120.0; B = 0.5 - th2 / 24.0 + th2 * th2 / 720.0; }
  else { const double s = sin(0.5 * th); A = sin(th) / th; B = 2.0 * s * s / th2; }
  const M3 S = skew(r), S2 = mul(S, S);
  M3 R = eye3();
  for (int i = 0; i < 9; ++i) R.m[i] += A * S.m[i] + B * S2.m[i];
  return R;
}
// log map through the quaternion (Shepperd's choice of the largest pivot: accurate for every angle up to pi); R need not be exactly
// orthogonal (a float32 pose): the result is the rotation of the quaternion fitted to it
PA_HD V3 rot_log(const M3& R) {
  const double* m = R.m;
  const double tr = m[0] + m[4] + m[8];
  double w, x, y, z;
  if (tr >= m[0] && tr >= m[4] && tr >= m[8]) {
    const double s = 2.0 * sqrt(1.0 + tr); w = 0.25 * s; x = (m[7] - m[5]) / s; y = (m[2] - m[6]) / s; z = (m[3] - m[1]) / s;
  } else if (m[0] >= m[4] && m[0] >= m[8]) {
    const double s = 2.0 * sqrt(1.0 + m[0] - m[4] - m[8]); w = (m[7] - m[5]) / s; x = 0.25 * s; y = (m[1] + m[3]) / s; z = (m[2] + m[6]) / s;
  } else if (m[4] >= m[8]) {
    const double s = 2.0 * sqrt(1.0 + m[4] - m[0] - m[8]); w = (m[2] - m[6]) / s; x = (m[1] + m[3]) / s; y = 0.25 * s; z = (m[5] + m[7]) / s;
  } else {
    const double s = 2.0 * sqrt(1.0 + m[8] - m[0] - m[4]); w = (m[3] - m[1]) / s; x = (m[2] + m[6]) / s; y = (m[5] + m[7]) / s; z = 0.25 * s;
  }
  if (w < 0) { w = -w; x = -x; y = -y; z = -z; }
  const double n = sqrt(w * w + x * x + y * y + z * z);
  w /= n; x /= n; y /= n; z /= n;
  const double sv = sqrt(x * x + y * y + z * z);
  const double f = sv > 1e-8 ? 2.0 * atan2(sv, w) / sv : 2.0 / w;
  return V3{f * x, f * y, f * z};
}
// Right Jacobian of the Rodrigues map: R(r + d) ~ R(r) exp([Jr d]x), Jr = I - a [r]x + b [r]x^2, a = (1-cos th)/th^2, b = (th-sin th)/th^3
PA_HD M3 rodrigues_jr(const V3& r) {
  const double th2 = r.x * r.x + r.y * r.y + r.z * r.z, th = sqrt(th2);
  double a, b;
  if (th < 1e-2) { a = 0.5 - th2 / 24.0 + th2 * th2 / 720.0; b = 1.0 / 6.0 - th2 / 120.0 + th2 * th2 / 5040.0; }
  else { const double s = sin(0.5 * th); a = 2.0 * s * s / th2; b = (th - sin(th)) / (th2 * th); }
  const M3 S = skew(r), S2 = mul(S, S);
  M3 J = eye3();
  for (int i = 0; i < 9; ++i) J.m[i] += -a * S.m[i] + b * S2.m[i];
  return J;
}

// PnP of 8 corners by Levenberg-Marquardt on x = (Rodrigues vector, t): the objective of SOLVEPNP_ITERATIVE (summed squared reprojection
// error, no distortion).  Normal equations: 21 entries of J^T J (upper triangle, row-major), 6 of J^T r and the error, 28 sums.
constexpr int PNP_SUMS = 28;
constexpr int PNP_MAX_ITER = 20;           // cv2's iteration limit (calib3d cvFindExtrinsicCameraParams2)
constexpr double PNP_STEP_EPS = 1e-10;     // stop once |dx| <= eps (|x| + eps)
// Residual rows (u, v) of one corner X observed at (ou, ov) and their derivatives in x, added into acc[PNP_SUMS]
PA_HD void pnp_corner_sums(const V3& X, double ou, double ov, const M3& R, const M3& RJx, const V3& t, const M3& K, double* acc) {
  const V3 c = add(mulv(R, X), t);
  const V3 q = mulv(K, c);
  const double iz = 1.0 / q.z, u = q.x * iz, v = q.y * iz;
  const double r[2] = {u - ou, v - ov};
  // d(u, v)/dc = (K row 0 / 1 - (u, v) K row 2) / q.z; dc/dt = I, dc/dr = -R [X]x Jr = RJx
  double du[3], dv[3];
  for (int k = 0; k < 3; ++k) { du[k] = (K.m[k] - u * K.m[6 + k]) * iz; dv[k] = (K.m[3 + k] - v * K.m[6 + k]) * iz; }
  double J[2][6];
  for (int k = 0; k < 3; ++k) {
    J[0][k] = du[0] * RJx.m[k] + du[1] * RJx.m[3 + k] + du[2] * RJx.m[6 + k];
    J[1][k] = dv[0] * RJx.m[k] + dv[1] * RJx.m[3 + k] + dv[2] * RJx.m[6 + k];
    J[0][3 + k] = du[k];
    J[1][3 + k] = dv[k];
  }
  int o = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) acc[o++] += J[0][i] * J[0][j] + J[1][i] * J[1][j];
  for (int i = 0; i < 6; ++i) acc[21 + i] += J[0][i] * r[0] + J[1][i] * r[1];
  acc[27] += r[0] * r[0] + r[1] * r[1];
}
// The sums over corners [c0, c1) at x, then `reduce` (identity on the host; a cross-lane sum on the device)
template <class Reduce>
PA_HD void pnp_sums(const double* box, const double* uv, int c0, int c1, const double* x, const M3& K, double* acc, Reduce reduce) {
  const V3 r{x[0], x[1], x[2]}, t{x[3], x[4], x[5]};
  const M3 R = rodrigues(r), Jr = rodrigues_jr(r);
  for (int i = 0; i < PNP_SUMS; ++i) acc[i] = 0.0;
  for (int c = c0; c < c1; ++c) {
    const V3 X{box[3 * c], box[3 * c + 1], box[3 * c + 2]};
    const M3 RJx = mul(R, mul(skew(X), Jr));
    M3 nRJx;
    for (int i = 0; i < 9; ++i) nRJx.m[i] = -RJx.m[i];
    pnp_corner_sums(X, uv[2 * c], uv[2 * c + 1], R, nRJx, t, K, acc);
  }
  reduce(acc);
}
// (A + lam diag(A)) dx = -g by Cholesky (A = the packed upper triangle); false if a pivot is not positive
PA_HD bool pnp_solve(const double* A, double lam, const double* g, double* dx) {
  double L[6][6];
  int o = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) { L[j][i] = A[o++]; if (j == i) L[i][i] *= 1.0 + lam; }
  for (int j = 0; j < 6; ++j) {
    double d = L[j][j];
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > 0.0)) return false;
    L[j][j] = sqrt(d);
    for (int i = j + 1; i < 6; ++i) {
      double s = L[i][j];
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      L[i][j] = s / L[j][j];
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) { double s = -g[i]; for (int k = 0; k < i; ++k) s -= L[i][k] * y[k]; y[i] = s / L[i][i]; }
  for (int i = 5; i >= 0; --i) { double s = y[i]; for (int k = i + 1; k < 6; ++k) s -= L[k][i] * dx[k]; dx[i] = s / L[i][i]; }
  return true;
}
// Levenberg-Marquardt from `init` (the frame's refined pose; cv2 starts from a DLT estimate instead): Marquardt's diagonal scaling,
// lam 1e-3, /10 after a step that lowers the error, x10 otherwise, as cv2's CvLevMarq.  Every decision depends on the reduced sums
// only, so lanes that share them take the same path.  Returns the iterations run.
template <class Reduce>
PA_HD int pnp_lm(const double* box, const double* uv, int c0, int c1, const M3& K, const P34& init, P34& out, Reduce reduce) {
  const V3 r0 = rot_log(rot_of(init));
  double x[6] = {r0.x, r0.y, r0.z, init.m[3], init.m[7], init.m[11]};
  double acc[PNP_SUMS], nacc[PNP_SUMS];
  pnp_sums(box, uv, c0, c1, x, K, acc, reduce);
  double lam = 1e-3;
  int it = 0;
  while (it < PNP_MAX_ITER) {
    ++it;
    double dx[6];
    if (!pnp_solve(acc, lam, acc + 21, dx)) { lam = fmin(lam * 10.0, 1e16); continue; }
    double xn[6], nd = 0.0, nx = 0.0;
    for (int i = 0; i < 6; ++i) { xn[i] = x[i] + dx[i]; nd += dx[i] * dx[i]; }
    pnp_sums(box, uv, c0, c1, xn, K, nacc, reduce);
    if (nacc[27] < acc[27]) {
      for (int i = 0; i < 6; ++i) x[i] = xn[i];
      for (int i = 0; i < PNP_SUMS; ++i) acc[i] = nacc[i];
      lam = fmax(lam * 0.1, 1e-16);
    } else {
      lam = fmin(lam * 10.0, 1e16);
    }
    for (int i = 0; i < 6; ++i) nx += x[i] * x[i];
    if (sqrt(nd) <= PNP_STEP_EPS * (sqrt(nx) + PNP_STEP_EPS)) break;
  }
  out = make_pose(rodrigues(V3{x[0], x[1], x[2]}), V3{x[3], x[4], x[5]});
  return it;
}
struct NoReduce { PA_HD void operator()(double*) const {} };

// ---- track health (gen6d_amd/tracking.py HealthPolicy): is a refined pose a plausible continuation of its stream?
//      Every comparison is written !(x <= thr), so that a NaN fails its gate; an infinite threshold disables it.
enum { TH_NONE = 0, TH_TRACKING = 1, TH_SUSPECT = 2, TH_LOST = 3 };                                   // health[s][0]
enum { THF_NONFINITE = 1, THF_BEHIND = 2, THF_SMALL = 4, THF_LARGE = 8, THF_OUTSIDE = 16, THF_ROT = 32, THF_SHIFT = 64, THF_SCALE = 128,
       THF_VERIFY_POS = 256, THF_VERIFY_SCALE = 512, THF_FRAME_BITS = 255, THF_VERIFY_BITS = 768 };   // health[s][3]
struct HealthGates { double min_px, max_px, margin, max_rot_deg, max_shift, max_log2_scale; };
PA_HD bool pose_finite(const P34& p) {
  bool ok = true;
  for (int i = 0; i < 12; ++i) ok = ok && isfinite(p.m[i]);
  return ok;
}
// The object centre under a pose: X = R c + t, z = X.z, (u, v) = (K X).xy / z, d_px = f diameter / z with f = (K00 + K11) / 2
PA_HD void health_centre(const P34& p, const M3& K, const V3& c, double diameter, double& u, double& v, double& z, double& d_px) {
  const V3 X = pose_apply(p, c), q = mulv(K, X);
  z = X.z; u = q.x / z; v = q.y / z;
  d_px = 0.5 * (K.m[0] + K.m[4]) * diameter / z;
}
// The gates of one candidate pose -> flag bits 0..7; m[7] = (u, v, z, d_px, rot_deg, shift, log2_scale).  prev == nullptr (an
// acquisition) skips the motion gates.  The two hard failures end the evaluation: a non-finite pose leaves every measure 0, a centre
// that is not in front of the camera leaves all but z 0 (nothing past them is defined).  A previous centre that is not in front of the
// camera fails SCALE and leaves shift and log2_scale 0.
PA_HD int health_gates(const P34* prev, const P34& cur, const M3& K, double w, double h, const V3& c, double diameter,
                       const HealthGates& g, double* m) {
  for (int i = 0; i < 7; ++i) m[i] = 0.0;
  if (!pose_finite(cur)) return THF_NONFINITE;
  double u, v, z, d;
  health_centre(cur, K, c, diameter, u, v, z, d);
  m[2] = z;
  if (!(z > 0.0)) return THF_BEHIND;
  m[0] = u; m[1] = v; m[3] = d;
  int f = 0;
  if (!(d >= g.min_px)) f |= THF_SMALL;
  if (!(d <= g.max_px * fmax(w, h))) f |= THF_LARGE;
  const double mg = g.margin * d;
  if (!(u >= -mg) || !(u <= w + mg) || !(v >= -mg) || !(v <= h + mg)) f |= THF_OUTSIDE;
  if (prev) {
    double tr = 0.0;                                             // tr(R_new R_prev^T)
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) tr += cur.m[4 * i + j] * prev->m[4 * i + j];
    m[4] = acos(fmin(fmax(0.5 * (tr - 1.0), -1.0), 1.0)) * (180.0 / 3.14159265358979323846);
    if (!(m[4] <= g.max_rot_deg)) f |= THF_ROT;
    double up, vp, zp, dp;
    health_centre(*prev, K, c, diameter, up, vp, zp, dp);
    if (!(zp > 0.0)) {
      f |= THF_SCALE;
    } else {
      m[5] = hypot(u - up, v - vp) / d;
      m[6] = fabs(log2(zp / z));
      if (!(m[5] <= g.max_shift)) f |= THF_SHIFT;
      if (!(m[6] <= g.max_log2_scale)) f |= THF_SCALE;
    }
  }
  return f;
}
// State update of one evaluated frame on row = (status, bad, vbad, flags): replaces flag bits 0..7, keeps 8..9.  commit: the frame
// passed and is committed; draw: the stream is not LOST after this frame.
PA_HD void health_update(int f, bool reset, int patience, int* row, bool& commit, bool& draw) {
  int status, bad = row[1], vbad = row[2];
  if (reset) { status = f ? TH_LOST : TH_TRACKING; bad = 0; vbad = 0; }
  else if (f & (THF_NONFINITE | THF_BEHIND)) status = TH_LOST;
  else if (f) { bad += 1; status = bad >= patience ? TH_LOST : TH_SUSPECT; }
  else { bad = 0; status = TH_TRACKING; }
  row[0] = status; row[1] = bad; row[2] = vbad; row[3] = (row[3] & THF_VERIFY_BITS) | f;
  commit = f == 0; draw = status != TH_LOST;
}
// The detector's check of a committed pose: det = (x, y, reference-to-query size ratio); ref_px: the object's mean projected diameter
// in the reference views -> flag bits 8..9; m[2] = (verify_shift, verify_log2_scale)
PA_HD int verify_gates(double dx, double dy, double ds, const P34& pose, const M3& K, const V3& c, double diameter, double ref_px,
                       double max_shift, double max_log2_scale, double* m) {
  double u, v, z, d;
  health_centre(pose, K, c, diameter, u, v, z, d);
  m[0] = hypot(dx - u, dy - v) / d;
  m[1] = fabs(log2(ds * ref_px / d));
  int f = 0;
  if (!(m[0] <= max_shift)) f |= THF_VERIFY_POS;
  if (!(m[1] <= max_log2_scale)) f |= THF_VERIFY_SCALE;
  return f;
}
// ... and its state update: a failed check counts towards LOST, a passed one clears the count; bits 0..7 are kept
PA_HD void verify_update(int f, int patience, int* row) {
  if (f) { row[2] += 1; if (row[2] >= patience) row[0] = TH_LOST; }
  else row[2] = 0;
  row[3] = (row[3] & THF_FRAME_BITS) | f;
}

}  // namespace pa
