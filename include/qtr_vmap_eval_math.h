// qtr_vmap_eval_math.h — the arithmetic of evaluating a pose against the voxel map (qtr_voxel_map_evaluate*,
// include/quatro_voxelmap_eval.h: overlap, RMSE, the 6x6 information matrix of a map edge and the registration's own normal
// matrix at T), shared by the gfx950 kernels (quatro_amd/csrc/voxelmap_eval.hip) and the host restatement of the tests (g++),
// on top of qtr_vmap_math.h: binary64 + - * / sqrt only, in the order written; both sides compile with -ffp-contract=off,
// so host and device agree bit for bit.  qtr_icp_finite3, qtr_vmap_query, qtr_icp_vgicp_terms and the fold functions are
// called, not restated.
//
// Given T (row-major 4x4, maps the scan into the map's frame; rows 0 - 2 are used):
//   considered source points   the finite ones (qtr_icp_finite3); each adds 1 to n_source, matched or not
//   match                      the registration's rule, unchanged: qtr_vmap_query(T, p, a, c, q, &key) is true and the voxel of
//                              key exists (cnt > 0 and rec.n > 0).  Source normals are required.  The matched set at T is the
//                              set ONE iteration of qtr_voxel_map_register from T linearises on.
//   terms                      qtr_vmap_eval_terms: QTR_VMAP_EVAL_NT doubles per considered point (layout below); an
//                              unmatched one has only the n_source place
//   sum                        the registration's shape: qtr_icp_fold64 inside every 64-point wave, qtr_icp_chunk_sum per
//                              256-point chunk, chunks in ascending order
//   qtr_vmap_eval_finish       the record from the summed terms
//
// information is Open3D's GetInformationMatrixFromPointClouds on the voxel mean mu (binary64, not rounded to float) of every
// matched point, in qtr_eval_finish's association with t = mu: rotation first, [5][5] = n_corr.  hessian is sum w J^T M J of the
// voxelised plane-to-plane cost at T (w = the voxel's members), gradient sum w J^T M d: what qtr_icp_step solves.
//
// qtr_vmap_eval_best is host code: the winner among B records.  Only valid ones count; the largest n_corr wins, ties go to
// the smaller rmse, then to the smaller index; -1 when none is valid (B <= 0 included).  It is qtr_vmap_batch_best's rule on
// the evaluation's fields.
#ifndef QTR_VMAP_EVAL_MATH_H
#define QTR_VMAP_EVAL_MATH_H

#include "qtr_vmap_math.h"

// term layout: places 0 .. QTR_ICP_NT - 1 are qtr_icp_vgicp_terms', unchanged (21 of w J^T M J, 6 of w J^T M d, w d^T M d,
// d^2, count, w, one padding place)
#define QTR_VMAP_EVAL_T_MU (QTR_ICP_NT)          // 3: sum mu
#define QTR_VMAP_EVAL_T_MUMU (QTR_ICP_NT + 3)    // 6: upper triangle of sum mu mu^T: xx xy xz yy yz zz
#define QTR_VMAP_EVAL_T_NSRC (QTR_ICP_NT + 9)    // considered source points
#define QTR_VMAP_EVAL_NT (QTR_ICP_NT + 10)

// what qtr_vmap_eval_finish produces (the device writes one per evaluation; the C ABI's qtr_vmap_eval_result carries the
// same fields behind its status)
typedef struct QtrVmapEvalRecord {
  int valid, n_source, n_corr, reserved;
  double overlap;      // n_corr / n_source
  double sum_d2;       // sum |q - mu|^2
  double inlier_rmse;  // sqrt(sum_d2 / n_corr): the distance to the voxel means
  double sum_w;        // sum of the matched voxels' member counts
  double chi2;         // sum w d^T M d
  double rmse;         // sqrt(chi2 / sum_w): the registration's rmse at T
  double information[36];
  double hessian[36];
  double gradient[6];
} QtrVmapEvalRecord;

// the terms of one CONSIDERED source point q = T p with normal a; vx: the record of the voxel it matched, or null
QM_HD void qtr_vmap_eval_terms(const double* T, const double* q, float ax, float ay, float az, const QtrIcpVoxel* vx,
                               double* e /* [QTR_VMAP_EVAL_NT] */) {
  for (int k = 0; k < QTR_VMAP_EVAL_NT; ++k) e[k] = 0.0;
  e[QTR_VMAP_EVAL_T_NSRC] = 1.0;
  if (!vx) return;
  qtr_icp_vgicp_terms(T, q, ax, ay, az, vx, e);
  const double t0 = vx->mu[0], t1 = vx->mu[1], t2 = vx->mu[2];
  e[QTR_VMAP_EVAL_T_MU + 0] = t0;
  e[QTR_VMAP_EVAL_T_MU + 1] = t1;
  e[QTR_VMAP_EVAL_T_MU + 2] = t2;
  e[QTR_VMAP_EVAL_T_MUMU + 0] = t0 * t0;
  e[QTR_VMAP_EVAL_T_MUMU + 1] = t0 * t1;
  e[QTR_VMAP_EVAL_T_MUMU + 2] = t0 * t2;
  e[QTR_VMAP_EVAL_T_MUMU + 3] = t1 * t1;
  e[QTR_VMAP_EVAL_T_MUMU + 4] = t1 * t2;
  e[QTR_VMAP_EVAL_T_MUMU + 5] = t2 * t2;
}

// the record from the summed terms S.  information: qtr_eval_finish's association with s = sum mu and X = sum mu mu^T;
// hessian: the 21 upper entries where they stand, copied below the diagonal, so both matrices are exactly symmetric.
// Zero denominators give 0.0.
QM_HD void qtr_vmap_eval_finish(const double* S /* [QTR_VMAP_EVAL_NT] */, QtrVmapEvalRecord* r) {
  const double n = S[QTR_ICP_T_CNT], ns = S[QTR_VMAP_EVAL_T_NSRC], sw = S[QTR_ICP_T_W];
  r->n_source = (int)ns;
  r->n_corr = (int)n;
  r->valid = n > 0.0 ? 1 : 0;
  r->reserved = 0;
  r->overlap = ns > 0.0 ? n / ns : 0.0;
  r->sum_d2 = S[QTR_ICP_T_D2];
  r->inlier_rmse = n > 0.0 ? sqrt(S[QTR_ICP_T_D2] / n) : 0.0;
  r->sum_w = sw;
  r->chi2 = S[QTR_ICP_T_R2];
  r->rmse = sw > 0.0 ? sqrt(S[QTR_ICP_T_R2] / sw) : 0.0;
  double* I = r->information;
  for (int k = 0; k < 36; ++k) I[k] = 0.0;
  const double* X = S + QTR_VMAP_EVAL_T_MUMU;
  const double sx = S[QTR_VMAP_EVAL_T_MU + 0], sy = S[QTR_VMAP_EVAL_T_MU + 1], sz = S[QTR_VMAP_EVAL_T_MU + 2];
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
  double* H = r->hessian;
  int k = 0;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) H[6 * a + b] = S[k++];
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < a; ++b) {
      I[6 * a + b] = I[6 * b + a];
      H[6 * a + b] = H[6 * b + a];
    }
  for (int a = 0; a < 6; ++a) r->gradient[a] = S[QTR_ICP_T_JTR + a];
}

static inline int qtr_vmap_eval_best(const QtrVmapEvalRecord* r, int B) {
  int best = -1, i;
  for (i = 0; i < B; ++i) {
    if (!r[i].valid) continue;
    if (best < 0 || r[i].n_corr > r[best].n_corr || (r[i].n_corr == r[best].n_corr && r[i].rmse < r[best].rmse)) best = i;
  }
  return best;
}

#endif  // QTR_VMAP_EVAL_MATH_H
