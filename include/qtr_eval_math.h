// qtr_eval_math.h — the arithmetic of a registration evaluation (qtr_evaluate*: overlap, inlier RMSE, the 6x6 information
// matrix of a pose-graph edge and the point-to-plane Hessian at T), shared by the gfx950 kernel (quatro_amd/csrc/eval.hip,
// k_eval) and the host restatement of the tests (g++), in the style of qtr_icp_math.h: binary64 + - * / sqrt only, in the
// order written; both sides compile with -ffp-contract=off, so host and device agree bit for bit.
//
// Given T (row-major 4x4, maps source into target; rows 0 - 2 are used) and max_d:
//   considered source points   the finite ones (qtr_icp_finite3); each adds 1 to n_source, partner or not
//   q = qtr_icp_transform(T, p)
//   correspondence             the ICP's: nearest finite target point with qtr_icp_d2(q, t) <= max_d^2, ties to the lowest
//                              target index.  A non-finite target normal does NOT drop it (unlike ICP method 0): it only
//                              keeps it out of the plane sums
//   terms                      qtr_eval_terms: QTR_EVAL_NT doubles per source point (layout below)
//   sum                        the ICP's shape: qtr_icp_fold64 inside every 64-point wave, qtr_icp_chunk_sum per 256-point
//                              chunk, chunks in ascending order — so sum_d2 and n_corr are the numbers ONE point-to-point ICP
//                              iteration from T forms for the same set
//   qtr_eval_finish            the record from the summed terms
//
// information is Open3D's GetInformationMatrixFromPointClouds: sum G^T G with G = [ -[t]x | I ] on the TARGET point t of
// every correspondence, rotation first, then translation:
//   [[ sum (|t|^2 I - t t^T),  [sum t]x ],
//    [ [sum t]x^T,             n_corr I ]]
// hessian_plane is sum J^T J of the point-to-plane cost at T, J = [ q x n | n ] (qtr_icp_terms(0, ..)), over the
// correspondences whose target normal is finite.
#pragma once
#include "qtr_icp_math.h"

// term layout
#define QTR_EVAL_T_JTJ 0     // 21: upper triangle of sum J^T J, row-major (the places qtr_icp_terms(0, ..) gives them)
#define QTR_EVAL_T_R2 21     // sum r^2, r = (q - t) . n
#define QTR_EVAL_T_NPLANE 22 // correspondences in the plane sums
#define QTR_EVAL_T_ST 23     // 3: sum t
#define QTR_EVAL_T_STT 26    // 6: upper triangle of sum t t^T: xx xy xz yy yz zz
#define QTR_EVAL_T_D2 32     // sum d^2
#define QTR_EVAL_T_CNT 33    // correspondences
#define QTR_EVAL_T_NSRC 34   // considered source points
#define QTR_EVAL_NT 35

// what qtr_eval_finish produces (the device writes one per evaluation; the C ABI's qtr_eval_result carries the same fields)
typedef struct QtrEvalRecord {
  int valid, n_source, n_corr, n_plane;
  double overlap, sum_d2, inlier_rmse, plane_rmse;
  double information[36];
  double hessian_plane[36];
} QtrEvalRecord;

// the terms of one CONSIDERED source point.  has_corr: it found the target point t at d2 = qtr_icp_d2(q, t); has_normal:
// target normals are present and t's normal n is finite.
QM_HD void qtr_eval_terms(const double* q, int has_corr, float tx, float ty, float tz, int has_normal, float nx, float ny,
                          float nz, double d2, double* e /* [QTR_EVAL_NT] */) {
  for (int k = 0; k < QTR_EVAL_NT; ++k) e[k] = 0.0;
  e[QTR_EVAL_T_NSRC] = 1.0;
  if (!has_corr) return;
  const double t0 = (double)tx, t1 = (double)ty, t2 = (double)tz;
  e[QTR_EVAL_T_ST + 0] = t0;
  e[QTR_EVAL_T_ST + 1] = t1;
  e[QTR_EVAL_T_ST + 2] = t2;
  e[QTR_EVAL_T_STT + 0] = t0 * t0;
  e[QTR_EVAL_T_STT + 1] = t0 * t1;
  e[QTR_EVAL_T_STT + 2] = t0 * t2;
  e[QTR_EVAL_T_STT + 3] = t1 * t1;
  e[QTR_EVAL_T_STT + 4] = t1 * t2;
  e[QTR_EVAL_T_STT + 5] = t2 * t2;
  e[QTR_EVAL_T_D2] = d2;
  e[QTR_EVAL_T_CNT] = 1.0;
  if (has_normal) {
    double o[QTR_ICP_NT];
    qtr_icp_terms(0, q, tx, ty, tz, nx, ny, nz, d2, o);
    for (int k = 0; k < 21; ++k) e[QTR_EVAL_T_JTJ + k] = o[k];
    e[QTR_EVAL_T_R2] = o[QTR_ICP_T_R2];
    e[QTR_EVAL_T_NPLANE] = 1.0;
  }
}

// the record from the summed terms S.  Association of the information matrix, with s = sum t and X = sum t t^T:
//   I[0][0] = X_yy + X_zz   I[1][1] = X_xx + X_zz   I[2][2] = X_xx + X_yy     (sum |t|^2 - sum t_a^2, without the cancellation)
//   I[a][b] = -X_ab  (a != b, both < 3)
//   [s]x = [[0, -s_z, s_y], [s_z, 0, -s_x], [-s_y, s_x, 0]] in rows 0 - 2, columns 3 - 5; its transpose below the diagonal
//   I[3+a][3+a] = n_corr
// Every off-diagonal entry is written once above the diagonal and copied below it: both matrices are exactly symmetric.
QM_HD void qtr_eval_finish(const double* S /* [QTR_EVAL_NT] */, QtrEvalRecord* r) {
  const double n = S[QTR_EVAL_T_CNT], ns = S[QTR_EVAL_T_NSRC], np = S[QTR_EVAL_T_NPLANE];
  r->n_source = (int)ns;
  r->n_corr = (int)n;
  r->n_plane = (int)np;
  r->valid = n > 0.0 ? 1 : 0;
  r->overlap = ns > 0.0 ? n / ns : 0.0;
  r->sum_d2 = S[QTR_EVAL_T_D2];
  r->inlier_rmse = n > 0.0 ? sqrt(S[QTR_EVAL_T_D2] / n) : 0.0;
  r->plane_rmse = np > 0.0 ? sqrt(S[QTR_EVAL_T_R2] / np) : 0.0;
  double* I = r->information;
  for (int k = 0; k < 36; ++k) I[k] = 0.0;
  const double* X = S + QTR_EVAL_T_STT;
  const double sx = S[QTR_EVAL_T_ST + 0], sy = S[QTR_EVAL_T_ST + 1], sz = S[QTR_EVAL_T_ST + 2];
  I[0] = X[3] + X[5];
  I[7] = X[0] + X[5];
  I[14] = X[0] + X[3];
  I[1] = -X[1];
  I[2] = -X[2];
  I[8] = -X[4];
  I[4] = -sz;
  I[5] = sy;
  I[9] = sz;
  I[11] = -sx;
  I[15] = -sy;
  I[16] = sx;
  I[21] = n;
  I[28] = n;
  I[35] = n;
  double* H = r->hessian_plane;
  int k = 0;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) H[6 * a + b] = S[QTR_EVAL_T_JTJ + k++];
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < a; ++b) {
      I[6 * a + b] = I[6 * b + a];
      H[6 * a + b] = H[6 * b + a];
    }
}
