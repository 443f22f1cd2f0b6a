// qtr_deskew_math.h — the contract of sweep deskew (motion compensation of a raw LiDAR sweep), shared by the gfx950 kernel
// (quatro_amd/csrc/deskew.hip), the host code that builds its knot table, and the host restatement of the tests (g++), in the
// style of qtr_icp_math.h: binary64 throughout, + - * / sqrt only, evaluated in the order written (every side compiles with
// -ffp-contract=off), no libm call, so host and device agree bit for bit.
//
//   knots     K of them, 2 <= K <= QTR_DESKEW_MAX_KNOTS: times tau_k, finite and strictly increasing, and poses T_k (rows
//             0 - 2 of a row-major 4x4: rotation R_k, translation c_k; sensor frame at tau_k -> any fixed frame).
//   interval  of a time t: j = the largest index with tau_j <= t, clamped to [0, K - 2];  s = (t - tau_j) / (tau_{j+1} - tau_j)
//             (a DIVISION by the stored difference, so t == tau_{j+1} gives s == 1 exactly).  t < tau_0 gives s < 0 on
//             interval 0 and t > tau_{K-1} gives s > 1 on the last one: both, and nothing else, are "extrapolated"
//             (s < 0 || s > 1; inside the table s never exceeds 1, rounding is monotone).
//   pose      R(t) = R_j Exp(s w_j),  c(t) = c_j + s (c_{j+1} - c_j): the rotation along the geodesic, the translation
//             linearly (LIO-SAM's deskewPoint), not the SE(3) exponential.
//   Log       w_j = Log(R_j^T R_{j+1}) through the unit quaternion with w >= 0, taken from the trace branch alone:
//             w = sqrt(1 + trace) / 2, v = (R21 - R12, R02 - R20, R10 - R01) / (4 w), (w, v) normalised.  An interval is
//             REFUSED unless  w >= QTR_DESKEW_W_MIN  (= sqrt(1/2) rounded up: a relative rotation of at most pi / 2), decided
//             on the w BEFORE the normalisation, by that comparison and no angle; a trace that is not a number fails it.
//             angle = 2 atan(|v| / w), |v| / w <= 1: three half-angle reductions x -> x / (1 + sqrt(1 + x^2)) (atan x =
//             2 atan of that), then QTR_DESKEW_ATAN_TERMS = 13 terms of the odd series in Horner form, times 8: within
//             8.7e-16 relative of the angle over (0, pi/2].  w_j = v (angle / |v|), 0 where |v| == 0.
//   Exp       Exp(p) = I + A [p]x + B [p]x^2 with A = sin(th)/th and B = (1 - cos th)/th^2 as QTR_DESKEW_EXP_TERMS = 16
//             terms each of their series in th^2 = p.p, Horner form: the truncation is below 1e-17 for th <= pi, so
//             every s in [-1, 2] on an admitted interval is covered; farther extrapolation stays deterministic and loses
//             accuracy.  Exp(0) is exactly I.
//   output    q = R_ref^T ((R(t) p + c(t)) - c_ref), (R_ref, c_ref) the pose at t_ref by the same rule (t_ref may
//             extrapolate); p = the point's float x, y, z widened, t = its float time widened; q rounded to float ONCE.
//             The fourth float is copied bit for bit.
//   skipped   a point with a non-finite x, y, z or time is copied unchanged (all four floats, bit for bit) and counted.
//   identity  knots reproduce every finite point value for value: Exp(0) = I, x 1 + y 0 + z 0 + 0 is exact.
#pragma once
#include "qtr_math.h"

#define QTR_DESKEW_MAX_KNOTS 256
#define QTR_DESKEW_W_MIN 0.70710678118654757  // the double above sqrt(1/2): w >= it <=> the interval is admitted
#define QTR_DESKEW_ATAN_TERMS 13
#define QTR_DESKEW_EXP_TERMS 16

// what qtr_deskew_table refuses (0: nothing)
#define QTR_DESKEW_OK 0
#define QTR_DESKEW_BAD_K 1         // K < 2 or K > QTR_DESKEW_MAX_KNOTS
#define QTR_DESKEW_BAD_TIME 2      // a knot time that is not finite or not above its predecessor
#define QTR_DESKEW_BAD_POSE 3      // a non-finite entry in rows 0 - 2 of a knot pose
#define QTR_DESKEW_BAD_ROTATION 4  // an interval whose relative rotation fails w >= QTR_DESKEW_W_MIN
#define QTR_DESKEW_BAD_TREF 5      // t_ref is not finite

// flags of qtr_deskew_point
#define QTR_DESKEW_SKIPPED 1
#define QTR_DESKEW_EXTRAPOLATED 2

// one interval of the knot table: 20 doubles
typedef struct QtrDeskewInterval {
  double tau;    // tau_j
  double div;    // tau_{j+1} - tau_j (> 0): the divisor of s
  double R[9];   // R_j, row-major
  double c[3];   // c_j
  double dc[3];  // c_{j+1} - c_j
  double w[3];   // Log(R_j^T R_{j+1})
} QtrDeskewInterval;

typedef struct QtrDeskewPose {
  double R[9];
  double c[3];
} QtrDeskewPose;

#define QTR_DESKEW_IV_DOUBLES 20
#define QTR_DESKEW_POSE_DOUBLES 12

QM_HD bool qtr_deskew_finite(double x) { return (x - x) == 0.0; }

QM_HD double qtr_deskew_dot3(double a0, double b0, double a1, double b1, double a2, double b2) {
  return (a0 * b0 + a1 * b1) + a2 * b2;
}

// atan(x) for 0 <= x <= ~1
QM_HD double qtr_deskew_atan(double x) {
  for (int r = 0; r < 3; ++r) x = x / (1.0 + sqrt(1.0 + x * x));
  const double z = x * x;
  double p = 1.0 / (double)(2 * (QTR_DESKEW_ATAN_TERMS - 1) + 1);
  for (int k = QTR_DESKEW_ATAN_TERMS - 2; k >= 0; --k) p = 1.0 / (double)(2 * k + 1) - z * p;
  return 8.0 * (x * p);
}

// w[3] = Log(M) of a relative rotation M (row-major); false: refused (w below QTR_DESKEW_W_MIN or not a number)
QM_HD bool qtr_deskew_log(const double* M, double* w) {
  const double tr = (M[0] + M[4]) + M[8];
  const double qw = sqrt(1.0 + tr) / 2.0;
  w[0] = w[1] = w[2] = 0.0;
  if (!(qw >= QTR_DESKEW_W_MIN)) return false;
  const double f = 4.0 * qw;
  double v0 = (M[7] - M[5]) / f, v1 = (M[2] - M[6]) / f, v2 = (M[3] - M[1]) / f;
  const double n = sqrt((qw * qw + v0 * v0) + (v1 * v1 + v2 * v2));
  const double u = qw / n;
  v0 = v0 / n;
  v1 = v1 / n;
  v2 = v2 / n;
  const double lv = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
  if (!(lv > 0.0)) return true;
  const double g = (2.0 * qtr_deskew_atan(lv / u)) / lv;
  w[0] = v0 * g;
  w[1] = v1 * g;
  w[2] = v2 * g;
  return true;
}

// E = Exp(p), row-major
QM_HD void qtr_deskew_exp(const double* p, double* E) {
  const double t2 = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
  // A = sum (-t2)^k / (2k+1)!,  2 B = sum 2 (-t2)^k / (2k+2)!: Horner from the last term, term k over term k - 1
  double A = 1.0, B = 1.0;
  for (int k = QTR_DESKEW_EXP_TERMS - 1; k >= 1; --k) {
    A = 1.0 - (t2 * (1.0 / (double)((2 * k) * (2 * k + 1)))) * A;  // (the quotient of two constants: the same double
    B = 1.0 - (t2 * (1.0 / (double)((2 * k + 1) * (2 * k + 2)))) * B;  //  wherever it is evaluated)
  }
  B = B / 2.0;
  const double x = p[0], y = p[1], z = p[2];
  // [p]x^2 = p p^T - t2 I
  E[0] = 1.0 - B * (y * y + z * z);
  E[1] = B * (x * y) - A * z;
  E[2] = B * (x * z) + A * y;
  E[3] = B * (x * y) + A * z;
  E[4] = 1.0 - B * (x * x + z * z);
  E[5] = B * (y * z) - A * x;
  E[6] = B * (x * z) - A * y;
  E[7] = B * (y * z) + A * x;
  E[8] = 1.0 - B * (x * x + y * y);
}

// the interval between two knots; false: the rotation is refused
QM_HD bool qtr_deskew_interval(double tau0, double tau1, const double* T0, const double* T1, QtrDeskewInterval* iv) {
  iv->tau = tau0;
  iv->div = tau1 - tau0;
  double M[9];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) {
      iv->R[3 * r + c] = T0[4 * r + c];
      M[3 * r + c] = qtr_deskew_dot3(T0[r], T1[c], T0[4 + r], T1[4 + c], T0[8 + r], T1[8 + c]);  // (R_0^T R_1)[r][c]
    }
    iv->c[r] = T0[4 * r + 3];
    iv->dc[r] = T1[4 * r + 3] - T0[4 * r + 3];
  }
  return qtr_deskew_log(M, iv->w);
}

// the interval index of t in a table of K - 1 intervals: binary search over tau_0 .. tau_{K-2}
QM_HD int qtr_deskew_find(const QtrDeskewInterval* tab, int K, double t) {
  int lo = 0, hi = K - 2;  // the answer lies in [lo, hi]
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].tau <= t)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// the pose at t; returns 1 where t extrapolates, else 0
QM_HD int qtr_deskew_pose(const QtrDeskewInterval* tab, int K, double t, QtrDeskewPose* P) {
  const QtrDeskewInterval* iv = tab + qtr_deskew_find(tab, K, t);
  const double s = (t - iv->tau) / iv->div;
  const double p[3] = {s * iv->w[0], s * iv->w[1], s * iv->w[2]};
  double E[9];
  qtr_deskew_exp(p, E);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c)
      P->R[3 * r + c] = qtr_deskew_dot3(iv->R[3 * r], E[c], iv->R[3 * r + 1], E[3 + c], iv->R[3 * r + 2], E[6 + c]);
    P->c[r] = iv->c[r] + s * iv->dc[r];
  }
  return (s < 0.0 || s > 1.0) ? 1 : 0;
}

// the whole table (K - 1 intervals) and the reference pose, from the caller's knots; QTR_DESKEW_OK or what is refused.
// knot_poses: K x 16 doubles, row-major 4x4 each (row 3 is not read).
QM_HD int qtr_deskew_table(const double* knot_times, const double* knot_poses, int K, double t_ref, QtrDeskewInterval* tab,
                           QtrDeskewPose* ref) {
  if (K < 2 || K > QTR_DESKEW_MAX_KNOTS) return QTR_DESKEW_BAD_K;
  for (int k = 0; k < K; ++k) {
    if (!qtr_deskew_finite(knot_times[k]) || (k > 0 && !(knot_times[k] > knot_times[k - 1]))) return QTR_DESKEW_BAD_TIME;
    for (int i = 0; i < 12; ++i)
      if (!qtr_deskew_finite(knot_poses[16 * k + i])) return QTR_DESKEW_BAD_POSE;
  }
  for (int k = 0; k + 1 < K; ++k) {
    if (!qtr_deskew_finite(knot_times[k + 1] - knot_times[k])) return QTR_DESKEW_BAD_TIME;  // (the difference overflows)
    if (!qtr_deskew_interval(knot_times[k], knot_times[k + 1], knot_poses + 16 * k, knot_poses + 16 * (k + 1), tab + k))
      return QTR_DESKEW_BAD_ROTATION;
  }
  if (!qtr_deskew_finite(t_ref)) return QTR_DESKEW_BAD_TREF;
  qtr_deskew_pose(tab, K, t_ref, ref);
  return QTR_DESKEW_OK;
}

// one finite point (x, y, z) taken at time t -> q[3], before the rounding to float; returns 1 where t extrapolates
QM_HD int qtr_deskew_point_f64(const QtrDeskewInterval* tab, int K, const QtrDeskewPose* ref, double x, double y, double z,
                               double t, double* q) {
  QtrDeskewPose P;
  const int extra = qtr_deskew_pose(tab, K, t, &P);
  double d[3];
  for (int r = 0; r < 3; ++r)
    d[r] = ((qtr_deskew_dot3(P.R[3 * r], x, P.R[3 * r + 1], y, P.R[3 * r + 2], z)) + P.c[r]) - ref->c[r];
  q[0] = qtr_deskew_dot3(ref->R[0], d[0], ref->R[3], d[1], ref->R[6], d[2]);
  q[1] = qtr_deskew_dot3(ref->R[1], d[0], ref->R[4], d[1], ref->R[7], d[2]);
  q[2] = qtr_deskew_dot3(ref->R[2], d[0], ref->R[5], d[1], ref->R[8], d[2]);
  return extra;
}

// one point: in[4] (x, y, z, fourth) and its time -> out[4]; returns QTR_DESKEW_SKIPPED, QTR_DESKEW_EXTRAPOLATED or 0.
// in and out may be the same four floats.
QM_HD int qtr_deskew_point(const QtrDeskewInterval* tab, int K, const QtrDeskewPose* ref, const float* in, float time,
                           float* out) {
  const float fx = in[0], fy = in[1], fz = in[2], fw = in[3];
  const double x = (double)fx, y = (double)fy, z = (double)fz, t = (double)time;
  if (!(qtr_deskew_finite(x) && qtr_deskew_finite(y) && qtr_deskew_finite(z) && qtr_deskew_finite(t))) {
    out[0] = fx;
    out[1] = fy;
    out[2] = fz;
    out[3] = fw;
    return QTR_DESKEW_SKIPPED;
  }
  double q[3];
  const int extra = qtr_deskew_point_f64(tab, K, ref, x, y, z, t, q);
  out[0] = (float)q[0];
  out[1] = (float)q[1];
  out[2] = (float)q[2];
  out[3] = fw;
  return extra ? QTR_DESKEW_EXTRAPOLATED : 0;
}
