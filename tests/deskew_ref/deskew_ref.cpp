// deskew_ref.cpp — host restatement of sweep deskew (quatro_amd/csrc/deskew.hip) for the tests: a loop over the points with
// include/qtr_deskew_math.h's own functions, and its pieces (arctangent, Log, Exp, pose) one by one.  Nothing of the device's
// staging, LDS table or counting is restated.
// Built by the tests with g++ -O2 -ffp-contract=off -shared -fPIC.
#include <cmath>
#include <cstring>
#include <vector>

#include "qtr_deskew_math.h"

extern "C" {

double deskew_ref_atan(double x) { return qtr_deskew_atan(x); }

// 1 and w[3] = Log(M), M row-major 3x3; 0: refused
int deskew_ref_log(const double* M, double* w) { return qtr_deskew_log(M, w) ? 1 : 0; }

void deskew_ref_exp(const double* p, double* E) { qtr_deskew_exp(p, E); }

// QTR_DESKEW_OK, T16 = the pose at t and *extrapolated; or what is refused
int deskew_ref_pose_at(const double* knot_times, const double* knot_poses, int K, double t, double* T16, int* extrapolated) {
  if (K < 2 || K > QTR_DESKEW_MAX_KNOTS) return QTR_DESKEW_BAD_K;
  std::vector<QtrDeskewInterval> tab((size_t)K - 1);
  QtrDeskewPose P;
  const int why = qtr_deskew_table(knot_times, knot_poses, K, t, tab.data(), &P);
  if (why != QTR_DESKEW_OK) return why;
  *extrapolated = qtr_deskew_pose(tab.data(), K, t, &P);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T16[4 * r + c] = P.R[3 * r + c];
    T16[4 * r + 3] = P.c[r];
  }
  T16[12] = T16[13] = T16[14] = 0.0;
  T16[15] = 1.0;
  return QTR_DESKEW_OK;
}

// the interval index and s of time t (for the interval-rule tests)
int deskew_ref_interval(const double* knot_times, const double* knot_poses, int K, double t, int* j, double* s) {
  if (K < 2 || K > QTR_DESKEW_MAX_KNOTS) return QTR_DESKEW_BAD_K;
  std::vector<QtrDeskewInterval> tab((size_t)K - 1);
  QtrDeskewPose P;
  const int why = qtr_deskew_table(knot_times, knot_poses, K, knot_times[0], tab.data(), &P);
  if (why != QTR_DESKEW_OK) return why;
  *j = qtr_deskew_find(tab.data(), K, t);
  *s = (t - tab[*j].tau) / tab[*j].div;
  return QTR_DESKEW_OK;
}

// qtr_deskew restated: out[P][4], info = {n_points, n_skipped, n_extrapolated}; QTR_DESKEW_OK or what is refused.
// out may be xyz4.
int deskew_ref_run(const float* xyz4, const float* times, int P, const double* knot_times, const double* knot_poses, int K,
                   double t_ref, float* out, int* info) {
  info[0] = info[1] = info[2] = 0;
  if (K < 2 || K > QTR_DESKEW_MAX_KNOTS) return QTR_DESKEW_BAD_K;
  std::vector<QtrDeskewInterval> tab((size_t)K - 1);
  QtrDeskewPose ref;
  const int why = qtr_deskew_table(knot_times, knot_poses, K, t_ref, tab.data(), &ref);
  if (why != QTR_DESKEW_OK) return why;
  for (int i = 0; i < P; ++i) {
    const int f = qtr_deskew_point(tab.data(), K, &ref, xyz4 + 4 * (size_t)i, times[i], out + 4 * (size_t)i);
    ++info[0];
    if (f == QTR_DESKEW_SKIPPED) ++info[1];
    if (f == QTR_DESKEW_EXTRAPOLATED) ++info[2];
  }
  return QTR_DESKEW_OK;
}

// the same points before their rounding to float: q[P][3] doubles (finite points only; a skipped point gives zeros)
int deskew_ref_run_f64(const float* xyz4, const float* times, int P, const double* knot_times, const double* knot_poses, int K,
                       double t_ref, double* q) {
  if (K < 2 || K > QTR_DESKEW_MAX_KNOTS) return QTR_DESKEW_BAD_K;
  std::vector<QtrDeskewInterval> tab((size_t)K - 1);
  QtrDeskewPose ref;
  const int why = qtr_deskew_table(knot_times, knot_poses, K, t_ref, tab.data(), &ref);
  if (why != QTR_DESKEW_OK) return why;
  for (int i = 0; i < P; ++i) {
    const float* p = xyz4 + 4 * (size_t)i;
    const double x = p[0], y = p[1], z = p[2], t = times[i];
    q[3 * (size_t)i] = q[3 * (size_t)i + 1] = q[3 * (size_t)i + 2] = 0.0;
    if (qtr_deskew_finite(x) && qtr_deskew_finite(y) && qtr_deskew_finite(z) && qtr_deskew_finite(t))
      qtr_deskew_point_f64(tab.data(), K, &ref, x, y, z, t, q + 3 * (size_t)i);
  }
  return QTR_DESKEW_OK;
}

}  // extern "C"
