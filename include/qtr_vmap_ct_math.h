// qtr_vmap_ct_math.h — the contract of the continuous-time registration of a RAW sweep against the voxel map
// (qtr_voxel_map_register_ct, include/quatro_voxelmap_ct.h), shared by the gfx950 kernel (quatro_amd/csrc/voxelmap_ct.hip),
// its host code and the host restatement of the tests (g++), in the style of qtr_deskew_math.h: binary64 throughout,
// + - * / sqrt only, evaluated in the order written (every side compiles with -ffp-contract=off), no libm call, so host and
// device agree bit for bit.  The pose rule is qtr_deskew_math.h's, the grid and the lookup are qtr_vmap_math.h's, the terms,
// the fold, the step and the stopping rules are qtr_icp_math.h's; nothing of theirs is restated here.
//
//   unknown   E: the sensor's pose at the END of the sweep, t_end (row-major 4x4, sensor -> world).  The pose at its beginning,
//             B at t_begin < t_end, is held FIXED (the previous sweep's end).  This is LOAM's odometry model and the fixed-begin
//             form of CT-ICP: the deskew is the registration's result, not a guess made before it.
//   interval  of an iterate E: qtr_deskew_interval(t_end, t_begin, E, B), parametrised FROM THE END: iv.R = R_E, iv.c = c_E,
//             iv.dc = c_B - c_E, iv.w = Log(R_E^T R_B), iv.tau = t_end, iv.div = t_begin - t_end (negative).  A refused interval
//             (relative rotation above pi / 2) gives no point a correspondence in that iteration: the count is 0 and
//             qtr_icp_step stops with QTR_ICP_STOP_TOO_FEW.
//   point     (p, normal a, float time t), all widened to double:  u = (t - iv.tau) / iv.div  — 0 at the sweep's end, 1 at its
//             beginning;  R(u) = R_E Exp(u w) and c(u) = c_E + u dc, formed as qtr_deskew_pose forms them;
//             q = qtr_icp_transform([R(u) | c(u)], p), the lever point r = qtr_icp_transform([R(u) | c_E], p), the voxel key
//             qtr_vmap_key_of(q).
//   skipped   a point with a non-finite x, y, z or t, or a normal that fails qtr_icp_normal_ok, takes no part.  u < 0 or u > 1
//             extrapolates: the point still takes part and is counted (among the points that are not skipped).
//   terms     s = 1 - u.  Sigma, M and d = q - mu as in qtr_icp_vgicp_terms with m = R(u) (a / |a|); qtr_icp_mahal_terms is
//             called with the lever r in the place of q.  Places 0 .. 27 are multiplied by the weight N (as in
//             qtr_icp_vgicp_terms), then places 0 .. 20 by (s s), then places 21 .. 26 by s.  T_R2, T_D2, T_CNT, T_W are
//             qtr_icp_vgicp_terms'.
//   unchanged the fold shape, qtr_icp_step, qtr_icp_compose onto E (a left increment [dR dt] E), the stopping rules, the trace.
//
// The Jacobian is an approximation, first order in the sweep's own rotation.  Under a left increment (theta, dt) on E,
//   dq/d(dt) = s I                                                                   (exact),
//   dq/d(theta) = -s [c_E]x - [R_E y]x R_E (I - u Jl(u w) Jl(w)^-1) R_E^T,  y = Exp(u w) p   (Jl: the left Jacobian of SO(3)),
// because the increment also turns the relative rotation Log(R_E^T R_B) the sweep is interpolated along.  The terms use
// s [-[r]x | I] with r = R_E y + c_E, i.e. they put (1 - u) I where I - u Jl(u w) Jl(w)^-1 stands.  The gap of the two is
//   G = -u [R_E y]x R_E (I - Jl(u w) Jl(w)^-1) R_E^T,   I - Jl(u w) Jl(w)^-1 = (1 - u) [w]x / 2 + O(|w|^2),
// so with Jl(a) = I + beta [a]x + gamma [a]x^2, 0 < beta <= 1/2, 0 < gamma <= 1/6 and |Jl(w)^-1| <= 1 + |w|:
//   |G|_2 <= u |p| ((1 - u) |w| / 2 + |w|^2)   for u in [0, 1] and |w| <= 1/4   (at most |p| |w| / 8 to first order, at u = 1/2).
// Relative to the point's range |p| the gap is therefore at most u ((1 - u) |w| / 2 + |w|^2): 0.7 % of the lever at a sweep
// that turns by 3 degrees.  G vanishes at u = 0 (s = 1: the rigid Jacobian) and the whole derivative at u = 1 (s = 0).  A
// Gauss-Newton step under an approximate Jacobian moves the fixed point nowhere (the gradient's zero is that of J^T M d with the
// J used; the residual d is exact), it costs convergence rate only.
//
// The anchor: if every time equals t_end (a binary32 value), then u = 0, Exp(0) = I, s = 1, s s = 1, c(u) = c_E + 0 and r = q,
// and the call IS qtr_voxel_map_register under the same guess, bit for bit, whatever B is: x 1 + y 0 + z 0 is exact and a
// product with 1.0 changes nothing.  (An entry of E that is a NEGATIVE zero comes out of R_E Exp(0) as +0; that shows only in the
// sign of a q or term that is itself zero.  qtr_icp_compose never leaves one behind.)
#pragma once
#include "qtr_deskew_math.h"
#include "qtr_vmap_math.h"

// flags of qtr_vmap_ct_flags
#define QTR_VMAP_CT_SKIPPED 1
#define QTR_VMAP_CT_EXTRAPOLATED 2

// the interval of the iterate E (>= 12 doubles: rows 0 - 2 of a row-major 4x4) and the fixed begin pose B (likewise), from
// the end; false: refused
QM_HD bool qtr_vmap_ct_interval(double t_begin, double t_end, const double* B, const double* E, QtrDeskewInterval* iv) {
  return qtr_deskew_interval(t_end, t_begin, E, B, iv);
}

// What the census counts, from the point, its normal and its time alone: tau = t_end, div = t_begin - t_end.
QM_HD int qtr_vmap_ct_flags(double tau, double div, float px, float py, float pz, float ax, float ay, float az, float time) {
  const double t = (double)time;
  if (!qtr_icp_finite3(px, py, pz) || !qtr_deskew_finite(t) || !qtr_icp_normal_ok(ax, ay, az)) return QTR_VMAP_CT_SKIPPED;
  const double u = (t - tau) / div;
  return (u < 0.0 || u > 1.0) ? QTR_VMAP_CT_EXTRAPOLATED : 0;
}

// T[12] = [R(u) | c(u)] (rows 0 - 2 of a row-major 4x4), as qtr_deskew_pose forms it
QM_HD void qtr_vmap_ct_pose(const QtrDeskewInterval* iv, double u, double* T) {
  const double p[3] = {u * iv->w[0], u * iv->w[1], u * iv->w[2]};
  double X[9];
  qtr_deskew_exp(p, X);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c)
      T[4 * r + c] = qtr_deskew_dot3(iv->R[3 * r], X[c], iv->R[3 * r + 1], X[3 + c], iv->R[3 * r + 2], X[6 + c]);
    T[4 * r + 3] = iv->c[r] + u * iv->dc[r];
  }
}

// The source side of a match (qtr_vmap_query's counterpart): true, and T = [R(u) | c(u)], q, the lever r, s = 1 - u and the key
// of q's voxel, when the point can have a correspondence.
QM_HD bool qtr_vmap_ct_query(const QtrDeskewInterval* iv, float px, float py, float pz, float ax, float ay, float az, float time,
                             double side, double* T /* [12] */, double* q, double* r, double* s, unsigned long long* key) {
  const double t = (double)time;
  if (!qtr_icp_finite3(px, py, pz) || !qtr_deskew_finite(t) || !qtr_icp_normal_ok(ax, ay, az)) return false;
  const double u = (t - iv->tau) / iv->div;
  qtr_vmap_ct_pose(iv, u, T);
  qtr_icp_transform(T, px, py, pz, q);
  const double Tr[12] = {T[0], T[1], T[2], iv->c[0], T[4], T[5], T[6], iv->c[1], T[8], T[9], T[10], iv->c[2]};
  qtr_icp_transform(Tr, px, py, pz, r);
  *s = 1.0 - u;
  return qtr_vmap_key_of(q, side, key);
}

// the terms of one source point against the voxel q fell into: T = [R(u) | .], q, r and s from qtr_vmap_ct_query
QM_HD void qtr_vmap_ct_terms(const double* T, const double* q, const double* r, double s, float ax, float ay, float az,
                             const QtrIcpVoxel* vx, double* o /* [QTR_ICP_NT] */) {
  const double k = 1.0 - QTR_ICP_GICP_EPSILON;
  double a0 = (double)ax, a1 = (double)ay, a2 = (double)az;
  const double la = sqrt((a0 * a0 + a1 * a1) + a2 * a2);
  a0 = a0 / la;
  a1 = a1 / la;
  a2 = a2 / la;
  const double m0 = (T[0] * a0 + T[1] * a1) + T[2] * a2;
  const double m1 = (T[4] * a0 + T[5] * a1) + T[6] * a2;
  const double m2 = (T[8] * a0 + T[9] * a1) + T[10] * a2;
  const double s00 = vx->C[0] + (1.0 - k * (m0 * m0));
  const double s01 = vx->C[1] + -(k * (m0 * m1));
  const double s02 = vx->C[2] + -(k * (m0 * m2));
  const double s11 = vx->C[3] + (1.0 - k * (m1 * m1));
  const double s12 = vx->C[4] + -(k * (m1 * m2));
  const double s22 = vx->C[5] + (1.0 - k * (m2 * m2));
  const double d0 = q[0] - vx->mu[0], d1 = q[1] - vx->mu[1], dz = q[2] - vx->mu[2];
  qtr_icp_mahal_terms(s00, s01, s02, s11, s12, s22, r, d0, d1, dz, o);
  const double w = (double)vx->n;
  for (int j = 0; j <= QTR_ICP_T_R2; ++j) o[j] = w * o[j];
  const double ss = s * s;
  for (int j = 0; j < QTR_ICP_T_JTR; ++j) o[j] = ss * o[j];
  for (int j = QTR_ICP_T_JTR; j < QTR_ICP_T_R2; ++j) o[j] = s * o[j];
  o[QTR_ICP_T_D2] = (d0 * d0 + d1 * d1) + dz * dz;
  o[QTR_ICP_T_CNT] = 1.0;
  o[QTR_ICP_T_W] = w;
  o[31] = 0.0;
}

// The pose at any time t by the rule above: T12 = rows 0 - 2 of a row-major 4x4; false: the interval of (B, E) is refused
QM_HD bool qtr_vmap_ct_pose_at(double t_begin, double t_end, const double* B, const double* E, double t, double* T12) {
  QtrDeskewInterval iv;
  if (!qtr_vmap_ct_interval(t_begin, t_end, B, E, &iv)) return false;
  qtr_vmap_ct_pose(&iv, (t - iv.tau) / iv.div, T12);
  return true;
}
