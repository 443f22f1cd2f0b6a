// qtr_icp_math.h — the arithmetic of one ICP iteration, shared by the gfx950 kernel (quatro_amd/csrc/icp.hip) and the
// host restatement of the tests (g++), in the style of qtr_math.h: binary64 + - * / sqrt only, evaluated in the order
// written (both sides compile with -ffp-contract=off), so host and device agree bit for bit.
//
// One iteration, given the current transform T (row-major 4x4, maps source into target):
//   q = R p + t                       per source point, binary64 from the float32 input (qtr_icp_transform)
//   nearest target point, d^2 <= max_d^2 in binary64 (qtr_icp_d2), ties to the lowest target index
//   per-correspondence terms          qtr_icp_terms: QTR_ICP_NT doubles (zero for a point without correspondence)
//   fixed-shape sum                   qtr_icp_fold64 inside every 64-point wave, (w0 + w1) + (w2 + w3) inside every
//                                     256-point chunk, then the chunks in ascending order (qtr_icp_chunk_sum)
//   update and stopping               qtr_icp_step
//
// Plane-to-plane (method 2, Generalized ICP): every point's covariance is the plane-regularised one of
// pcl::GeneralizedIterativeClosestPoint / fast_gicp, eigenvalues (1, 1, eps) with the normal as the eps direction, which
// is a function of the unit normal alone: C = I - (1 - eps) n n^T.  eps is the constant QTR_ICP_GICP_EPSILON: it is fixed
// because qtr_icp_params may not grow (C++ callers are built against its layout).  Per correspondence p <-> b with the
// source normal a (source frame), the target normal nb and T = [R t] (qtr_icp_gicp_terms):
//   Sigma = C_b + R C_a R^T = 2 I - (1 - eps)(n n^T + m m^T),  n = nb / |nb|,  m = R (a / |a|)
//   M = Sigma^-1 by adjugate / determinant (det >= 8 eps for unit normals: no pivoting), held fixed inside the iteration
//   d = q - b,  J = [ -[q]x | I ]  (the left-multiplied increment T <- [dR dt] T of qtr_icp_compose)
//   terms: J^T M J (21), J^T M d (6), d^T M d, d^2, 1 - solved and stepped exactly like point-to-plane.
// A source point whose normal is not finite or has zero length takes no part (skipped before the search); a
// correspondence whose target normal is not finite or has zero length is dropped (qtr_icp_normal_ok).
#pragma once
#include "qtr_math.h"

#define QTR_ICP_CHUNK 256  // source points per workgroup / partial sum
#define QTR_ICP_NT 32      // terms per point (30 used, 31 by method 3; padded)

#define QTR_ICP_GICP_EPSILON 1e-3  // plane regularisation of method 2 (pcl's gicp_epsilon); fixed, see above

// term layout.  Point-to-plane: 21 upper entries of J^T J (row-major upper triangle), 6 of J^T r, sum r^2.
// Plane-to-plane: the same places with J^T M J, J^T M d, d^T M d.
// Point-to-point: sum q t^T (9, row-major: [3a+b] = q_a t_b), sum q (3), sum t (3).  Both: sum d^2, count.
#define QTR_ICP_T_JTR 21
#define QTR_ICP_T_R2 27
#define QTR_ICP_T_QT 0
#define QTR_ICP_T_SQ 9
#define QTR_ICP_T_ST 12
#define QTR_ICP_T_D2 28
#define QTR_ICP_T_CNT 29

// stop reasons (qtr_icp_result.stop_reason; the same values as include/quatro_hip.h)
#define QTR_ICP_RUNNING 0
#define QTR_ICP_STOP_MAX_ITERATIONS 1
#define QTR_ICP_STOP_TRANSFORMATION 2
#define QTR_ICP_STOP_FITNESS 3
#define QTR_ICP_STOP_TOO_FEW 4
#define QTR_ICP_STOP_DEGENERATE 5

// a pivot of the 6x6 LDL^T at or below this fraction of its own diagonal entry is a rank deficiency (a plane leaves
// three of the six directions unconstrained: their pivots are rounding noise, ~1e-16 of the diagonal)
#define QTR_ICP_PIVOT_REL 1e-12

typedef struct QtrIcpCfg {
  double max_d2;        // max_correspondence_distance^2
  double trans_eps;     // transformation_epsilon
  double fit_eps;       // euclidean_fitness_epsilon
  int max_iterations;
  int method;           // 0 point-to-plane, 1 point-to-point, 2 plane-to-plane, 3 voxelised plane-to-plane
  int min_corr;
  int pad;
} QtrIcpCfg;

typedef struct QtrIcpState {
  double T[16];         // current transform (the last good one once stopped)
  double prev_mse;      // MSE of the previous iteration's correspondences (< 0: none yet)
  double fitness;       // MSE (mean d^2) of the last evaluated correspondence set
  double rmse;          // sqrt(mean of the minimised residual^2) of that set
  int iterations;       // updates applied
  int stop;             // 1: stopped (later launches return at once)
  int reason;           // QTR_ICP_STOP_*
  int n_corr;           // correspondences of the last evaluated set
  int valid, converged;
  int pad[2];
} QtrIcpState;

QM_HD void qtr_icp_transform(const double* T, float px, float py, float pz, double* q) {
  const double x = (double)px, y = (double)py, z = (double)pz;
  q[0] = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
  q[1] = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
  q[2] = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
}

QM_HD double qtr_icp_d2(const double* q, float tx, float ty, float tz) {
  const double dx = q[0] - (double)tx, dy = q[1] - (double)ty, dz = q[2] - (double)tz;
  return (dx * dx + dy * dy) + dz * dz;
}

QM_HD bool qtr_icp_finite3(float x, float y, float z) {
  // (x - x is NaN for inf and NaN alike; no library call)
  return (x - x) == 0.0f && (y - y) == 0.0f && (z - z) == 0.0f;
}

// the terms of one correspondence q <-> (t, n); d2 = qtr_icp_d2(q, t)
QM_HD void qtr_icp_terms(int method, const double* q, float tx, float ty, float tz, float nx, float ny, float nz, double d2,
                         double* o /* [QTR_ICP_NT] */) {
  for (int k = 0; k < QTR_ICP_NT; ++k) o[k] = 0.0;
  const double t0 = (double)tx, t1 = (double)ty, t2 = (double)tz;
  if (method == 0) {
    const double n0 = (double)nx, n1 = (double)ny, n2 = (double)nz;
    const double r = ((q[0] - t0) * n0 + (q[1] - t1) * n1) + (q[2] - t2) * n2;
    double J[6];
    J[0] = q[1] * n2 - q[2] * n1;  // q x n
    J[1] = q[2] * n0 - q[0] * n2;
    J[2] = q[0] * n1 - q[1] * n0;
    J[3] = n0;
    J[4] = n1;
    J[5] = n2;
    int k = 0;
    for (int a = 0; a < 6; ++a)
      for (int b = a; b < 6; ++b) o[k++] = J[a] * J[b];
    for (int a = 0; a < 6; ++a) o[QTR_ICP_T_JTR + a] = J[a] * r;
    o[QTR_ICP_T_R2] = r * r;
  } else {
    const double t[3] = {t0, t1, t2};
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) o[QTR_ICP_T_QT + 3 * a + b] = q[a] * t[b];
    for (int a = 0; a < 3; ++a) {
      o[QTR_ICP_T_SQ + a] = q[a];
      o[QTR_ICP_T_ST + a] = t[a];
    }
  }
  o[QTR_ICP_T_D2] = d2;
  o[QTR_ICP_T_CNT] = 1.0;
}

// a normal plane-to-plane can use: finite and of non-zero length
QM_HD bool qtr_icp_normal_ok(float x, float y, float z) {
  if (!qtr_icp_finite3(x, y, z)) return false;
  const double a = (double)x, b = (double)y, c = (double)z;
  return ((a * a + b * b) + c * c) > 0.0;
}

// What plane-to-plane and its voxelised form share, from Sigma = C_b + R C_a R^T (symmetric: s00 s01 s02 s11 s12 s22), q and
// d: M = adj(Sigma) / det(Sigma), then J^T M J (21), J^T M d (6) and d^T M d into their places of o.  o[28 ..] is the caller's.
QM_HD void qtr_icp_mahal_terms(double s00, double s01, double s02, double s11, double s12, double s22, const double* q,
                               double d0, double d1, double dz, double* o /* [QTR_ICP_NT] */) {
  const double c00 = s11 * s22 - s12 * s12;
  const double c01 = s02 * s12 - s01 * s22;
  const double c02 = s01 * s12 - s02 * s11;
  const double c11 = s00 * s22 - s02 * s02;
  const double c12 = s01 * s02 - s00 * s12;
  const double c22 = s00 * s11 - s01 * s01;
  const double det = (s00 * c00 + s01 * c01) + s02 * c02;
  const double M00 = c00 / det, M01 = c01 / det, M02 = c02 / det, M11 = c11 / det, M12 = c12 / det, M22 = c22 / det;
  const double q0 = q[0], q1 = q[1], q2 = q[2];
  const double e0 = (M00 * d0 + M01 * d1) + M02 * dz;  // M d
  const double e1 = (M01 * d0 + M11 * d1) + M12 * dz;
  const double e2 = (M02 * d0 + M12 * d1) + M22 * dz;
  // B = K M
  const double B00 = q1 * M02 - q2 * M01, B01 = q1 * M12 - q2 * M11, B02 = q1 * M22 - q2 * M12;
  const double B10 = q2 * M00 - q0 * M02, B11 = q2 * M01 - q0 * M12, B12 = q2 * M02 - q0 * M22;
  const double B20 = q0 * M01 - q1 * M00, B21 = q0 * M11 - q1 * M01, B22 = q0 * M12 - q1 * M02;
  // -K M K = B K^T (symmetric; the upper triangle)
  o[0] = q1 * B02 - q2 * B01;
  o[1] = q2 * B00 - q0 * B02;
  o[2] = q0 * B01 - q1 * B00;
  o[3] = B00;
  o[4] = B01;
  o[5] = B02;
  o[6] = q2 * B10 - q0 * B12;
  o[7] = q0 * B11 - q1 * B10;
  o[8] = B10;
  o[9] = B11;
  o[10] = B12;
  o[11] = q0 * B21 - q1 * B20;
  o[12] = B20;
  o[13] = B21;
  o[14] = B22;
  o[15] = M00;
  o[16] = M01;
  o[17] = M02;
  o[18] = M11;
  o[19] = M12;
  o[20] = M22;
  o[QTR_ICP_T_JTR + 0] = q1 * e2 - q2 * e1;
  o[QTR_ICP_T_JTR + 1] = q2 * e0 - q0 * e2;
  o[QTR_ICP_T_JTR + 2] = q0 * e1 - q1 * e0;
  o[QTR_ICP_T_JTR + 3] = e0;
  o[QTR_ICP_T_JTR + 4] = e1;
  o[QTR_ICP_T_JTR + 5] = e2;
  o[QTR_ICP_T_R2] = (d0 * e0 + d1 * e1) + dz * e2;
}

// the plane-to-plane terms of one correspondence: q = T p, source normal a (source frame), target point t with normal
// nb; d2 = qtr_icp_d2(q, t).  Both normals pass qtr_icp_normal_ok.  With K = [q]x and J = [-K | I]:
//   J^T M J = [[-K M K, K M], [(K M)^T, M]],  J^T M d = (q x (M d), M d)
// B = K M is formed column by column (B[:, j] = q x M[:, j]), then -K M K = B K^T row by row (row i = q x B[i, :]).
QM_HD void qtr_icp_gicp_terms(const double* T, const double* q, float ax, float ay, float az, float tx, float ty, float tz,
                              float bx, float by, float bz, double d2, double* o /* [QTR_ICP_NT] */) {
  const double k = 1.0 - QTR_ICP_GICP_EPSILON;
  double a0 = (double)ax, a1 = (double)ay, a2 = (double)az;
  const double la = sqrt((a0 * a0 + a1 * a1) + a2 * a2);
  a0 = a0 / la;
  a1 = a1 / la;
  a2 = a2 / la;
  double n0 = (double)bx, n1 = (double)by, n2 = (double)bz;
  const double ln = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
  n0 = n0 / ln;
  n1 = n1 / ln;
  n2 = n2 / ln;
  const double m0 = (T[0] * a0 + T[1] * a1) + T[2] * a2;
  const double m1 = (T[4] * a0 + T[5] * a1) + T[6] * a2;
  const double m2 = (T[8] * a0 + T[9] * a1) + T[10] * a2;
  // Sigma (symmetric): s00 s01 s02 s11 s12 s22
  const double s00 = 2.0 - k * (n0 * n0 + m0 * m0);
  const double s01 = -(k * (n0 * n1 + m0 * m1));
  const double s02 = -(k * (n0 * n2 + m0 * m2));
  const double s11 = 2.0 - k * (n1 * n1 + m1 * m1);
  const double s12 = -(k * (n1 * n2 + m1 * m2));
  const double s22 = 2.0 - k * (n2 * n2 + m2 * m2);
  const double d0 = q[0] - (double)tx, d1 = q[1] - (double)ty, dz = q[2] - (double)tz;
  qtr_icp_mahal_terms(s00, s01, s02, s11, s12, s22, q, d0, d1, dz, o);
  o[QTR_ICP_T_D2] = d2;
  o[QTR_ICP_T_CNT] = 1.0;
  o[30] = 0.0;
  o[31] = 0.0;
}

// ---- voxelised plane-to-plane (method 3, VGICP: Koide et al., ICRA 2021) -------------------------------------------------
// The target is summarised once per call as one Gaussian per voxel and a transformed source point is matched to the voxel
// it falls into: a lookup in place of the search.
//   grid     origin o = component-wise minimum of the finite target points, side c = max_correspondence_distance exactly,
//            dims[a] = floor((max[a] - o[a]) / c) + 1, cell index floor((x - o[a]) / c) in binary64 (qtr_icp_cellf) for
//            target points and transformed source points alike.  Unlike the search's, this grid is part of the result.
//   members  of a voxel: the finite target points whose normal passes qtr_icp_normal_ok; a voxel without members does
//            not exist.
//   record   N, mu = (sum of the members' coordinates) / N, C_b = I - (1 - eps) S / N with S = sum n n^T over the members'
//            unit normals, rep = the lowest original target index among the members.  EVERY sum runs over the members in
//            ascending original target index, from 0.0 (qtr_icp_voxel_add, then qtr_icp_voxel_finish).
//   match    q = T p; no correspondence if a cell index lies outside [0, dims) (compared as double: NaN and huge values fail)
//            or the voxel does not exist; sources are not clamped and there is no distance test.
//   terms    d = q - mu, Sigma = C_b + R C_a R^T, M = Sigma^-1 (both summands have eigenvalues in [eps, 1]), weight w = N:
//            w J^T M J, w J^T M d, w d^T M d in the point-to-plane places, d^2, 1, and w in place QTR_ICP_T_W.
//   result   fitness = mean d^2, rmse = sqrt(sum w d^T M d / sum w); solve, increment and stopping rules are point-to-plane's.
#define QTR_ICP_T_W 30  // sum of the weights (method 3; one of the two padding places)

typedef struct QtrIcpVoxel {
  double mu[3];
  double C[6];  // C_b: c00 c01 c02 c11 c12 c22
  int n;        // members (0: the voxel does not exist)
  int rep;      // lowest original target index among them
} QtrIcpVoxel;

// the largest cell table of a call.  A voxel grid of more cells is refused (QTR_ERR_CAPACITY), never coarsened.
#define QTR_ICP_CELL_CAP (1 << 22)

QM_HD double qtr_icp_cellf(double x, double o, double c) { return floor((x - o) / c); }

// dims of the voxel grid over the box [o, mx] of the finite target points; returns the number of cells as a double
// (dims is meaningful only when that is <= QTR_ICP_CELL_CAP)
QM_HD double qtr_icp_voxel_dims(const double* o, const double* mx, double c, int* dims) {
  double nc = 1.0;
  for (int a = 0; a < 3; ++a) {
    const double d = qtr_icp_cellf(mx[a], o[a], c) + 1.0;
    nc = nc * d;
    dims[a] = (d >= 1.0 && d <= (double)QTR_ICP_CELL_CAP) ? (int)d : 0;
  }
  return nc;
}

// the cell of q on the voxel grid (o, c, dims): false if it lies outside
QM_HD bool qtr_icp_voxel_cell(const double* q, const double* o, double c, const int* dims, int* lin) {
  int i[3];
  for (int a = 0; a < 3; ++a) {
    const double f = qtr_icp_cellf(q[a], o[a], c);
    if (!(f >= 0.0 && f <= (double)(dims[a] - 1))) return false;  // (NaN / huge: compared as double before the cast)
    i[a] = (int)f;
  }
  *lin = i[0] + dims[0] * (i[1] + dims[1] * i[2]);
  return true;
}

// one member into the running sums acc[9] (coordinates 3, n n^T 6; zero before the first member)
QM_HD void qtr_icp_voxel_add(double* acc, float tx, float ty, float tz, float bx, float by, float bz) {
  double n0 = (double)bx, n1 = (double)by, n2 = (double)bz;
  const double ln = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
  n0 = n0 / ln;
  n1 = n1 / ln;
  n2 = n2 / ln;
  acc[0] = acc[0] + (double)tx;
  acc[1] = acc[1] + (double)ty;
  acc[2] = acc[2] + (double)tz;
  acc[3] = acc[3] + n0 * n0;
  acc[4] = acc[4] + n0 * n1;
  acc[5] = acc[5] + n0 * n2;
  acc[6] = acc[6] + n1 * n1;
  acc[7] = acc[7] + n1 * n2;
  acc[8] = acc[8] + n2 * n2;
}

QM_HD void qtr_icp_voxel_finish(const double* acc, int n, int rep, QtrIcpVoxel* vx) {
  const double k = 1.0 - QTR_ICP_GICP_EPSILON, N = (double)n;
  for (int a = 0; a < 3; ++a) vx->mu[a] = n > 0 ? acc[a] / N : 0.0;
  for (int a = 0; a < 6; ++a) vx->C[a] = 0.0;
  if (n > 0) {
    vx->C[0] = 1.0 - k * (acc[3] / N);
    vx->C[1] = -(k * (acc[4] / N));
    vx->C[2] = -(k * (acc[5] / N));
    vx->C[3] = 1.0 - k * (acc[6] / N);
    vx->C[4] = -(k * (acc[7] / N));
    vx->C[5] = 1.0 - k * (acc[8] / N);
  }
  vx->n = n;
  vx->rep = rep;
}

// the terms of one source point q = T p (normal a, source frame, qtr_icp_normal_ok) against the voxel it fell into
QM_HD void qtr_icp_vgicp_terms(const double* T, const double* q, float ax, float ay, float az, const QtrIcpVoxel* vx,
                               double* o /* [QTR_ICP_NT] */) {
  const double k = 1.0 - QTR_ICP_GICP_EPSILON;
  double a0 = (double)ax, a1 = (double)ay, a2 = (double)az;
  const double la = sqrt((a0 * a0 + a1 * a1) + a2 * a2);
  a0 = a0 / la;
  a1 = a1 / la;
  a2 = a2 / la;
  const double m0 = (T[0] * a0 + T[1] * a1) + T[2] * a2;
  const double m1 = (T[4] * a0 + T[5] * a1) + T[6] * a2;
  const double m2 = (T[8] * a0 + T[9] * a1) + T[10] * a2;
  // Sigma = C_b + (I - (1 - eps) m m^T)
  const double s00 = vx->C[0] + (1.0 - k * (m0 * m0));
  const double s01 = vx->C[1] + -(k * (m0 * m1));
  const double s02 = vx->C[2] + -(k * (m0 * m2));
  const double s11 = vx->C[3] + (1.0 - k * (m1 * m1));
  const double s12 = vx->C[4] + -(k * (m1 * m2));
  const double s22 = vx->C[5] + (1.0 - k * (m2 * m2));
  const double d0 = q[0] - vx->mu[0], d1 = q[1] - vx->mu[1], dz = q[2] - vx->mu[2];
  qtr_icp_mahal_terms(s00, s01, s02, s11, s12, s22, q, d0, d1, dz, o);
  const double w = (double)vx->n;
  for (int j = 0; j <= QTR_ICP_T_R2; ++j) o[j] = w * o[j];
  o[QTR_ICP_T_D2] = (d0 * d0 + d1 * d1) + dz * dz;
  o[QTR_ICP_T_CNT] = 1.0;
  o[QTR_ICP_T_W] = w;
  o[31] = 0.0;
}

// the in-wave fold of 64 values: for off = 32, 16, ..., 1: p[l] += p[l + off] (l < off) — what __shfl_down does
QM_HD double qtr_icp_fold64(double* p /* [64], clobbered */) {
  for (int off = 32; off >= 1; off >>= 1)
    for (int l = 0; l < off; ++l) p[l] = p[l] + p[l + off];
  return p[0];
}
QM_HD double qtr_icp_chunk_sum(const double* w /* [4] wave sums */) { return (w[0] + w[1]) + (w[2] + w[3]); }

// Solves A x = b for the symmetric 6x6 A given by its 21 upper entries (row-major upper triangle), LDL^T with a fixed
// loop order.  Returns false on a pivot that is not clearly positive (degenerate scene).
QM_HD bool qtr_icp_solve6(const double* U21, const double* b, double* x) {
  double A[6][6];
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) {
      A[i][j] = U21[k];
      A[j][i] = U21[k];
      ++k;
    }
  double L[6][6], D[6];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) L[i][j] = (i == j) ? 1.0 : 0.0;
  for (int j = 0; j < 6; ++j) {
    double d = A[j][j];
    for (int m = 0; m < j; ++m) d = d - (L[j][m] * L[j][m]) * D[m];
    if (!(d > QTR_ICP_PIVOT_REL * A[j][j])) return false;  // (also false for NaN)
    D[j] = d;
    for (int i = j + 1; i < 6; ++i) {
      double s = A[i][j];
      for (int m = 0; m < j; ++m) s = s - (L[i][m] * L[j][m]) * D[m];
      L[i][j] = s / d;
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {
    double s = b[i];
    for (int m = 0; m < i; ++m) s = s - L[i][m] * y[m];
    y[i] = s;
  }
  for (int i = 5; i >= 0; --i) {
    double s = y[i] / D[i];
    for (int m = i + 1; m < 6; ++m) s = s - L[m][i] * x[m];
    x[i] = s;
  }
  return true;
}

// rotation of the unit quaternion (1, w/2) / |(1, w/2)|: the small-angle increment without sin / cos
QM_HD void qtr_icp_rot_from_omega(const double* w, double* R /* row-major 3x3 */) {
  double q0 = 1.0, q1 = 0.5 * w[0], q2 = 0.5 * w[1], q3 = 0.5 * w[2];
  const double nq = sqrt((q0 * q0 + q1 * q1) + (q2 * q2 + q3 * q3));
  q0 = q0 / nq;
  q1 = q1 / nq;
  q2 = q2 / nq;
  q3 = q3 / nq;
  R[0] = ((q0 * q0 + q1 * q1) - q2 * q2) - q3 * q3;
  R[1] = 2.0 * (q1 * q2 - q0 * q3);
  R[2] = 2.0 * (q1 * q3 + q0 * q2);
  R[3] = 2.0 * (q1 * q2 + q0 * q3);
  R[4] = ((q0 * q0 - q1 * q1) + q2 * q2) - q3 * q3;
  R[5] = 2.0 * (q2 * q3 - q0 * q1);
  R[6] = 2.0 * (q1 * q3 - q0 * q2);
  R[7] = 2.0 * (q2 * q3 + q0 * q1);
  R[8] = ((q0 * q0 - q1 * q1) - q2 * q2) + q3 * q3;
}

// T <- [dR dt; 0 1] T
QM_HD void qtr_icp_compose(const double* dR, const double* dt, double* T) {
  double N[12];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 4; ++c) N[4 * r + c] = (dR[3 * r] * T[c] + dR[3 * r + 1] * T[4 + c]) + dR[3 * r + 2] * T[8 + c];
    N[4 * r + 3] = N[4 * r + 3] + dt[r];
  }
  for (int k = 0; k < 12; ++k) T[k] = N[k];
  T[12] = 0.0;
  T[13] = 0.0;
  T[14] = 0.0;
  T[15] = 1.0;
}

QM_HD void qtr_icp_init(QtrIcpState* st, const double* guess) {
  for (int k = 0; k < 16; ++k) st->T[k] = guess[k];
  st->prev_mse = -1.0;
  st->fitness = 1.7976931348623157e308;  // (pcl getFitnessScore without correspondences: DBL_MAX)
  st->rmse = 0.0;
  st->iterations = 0;
  st->stop = 0;
  st->reason = QTR_ICP_RUNNING;
  st->n_corr = 0;
  st->valid = 0;
  st->converged = 0;
  st->pad[0] = st->pad[1] = 0;
}

// The update of one iteration from the summed terms S: solve, compose, decide whether to stop.  trace (may be null)
// receives [T after the update (16), MSE, count] when an update was applied.
QM_HD void qtr_icp_step(const QtrIcpCfg* cfg, const double* S, QtrIcpState* st, double* trace /* [18] or null */) {
  const double n = S[QTR_ICP_T_CNT];
  st->n_corr = (int)n;
  if (n < (double)cfg->min_corr || !(n > 0.0)) {  // too few correspondences: T stays at the last good value
    if (n > 0.0) st->fitness = S[QTR_ICP_T_D2] / n;
    st->stop = 1;
    st->reason = QTR_ICP_STOP_TOO_FEW;
    st->valid = 0;
    st->converged = 0;
    return;
  }
  const double mse = S[QTR_ICP_T_D2] / n;
  st->fitness = mse;
  double dR[9], dt[3];
  if (cfg->method != 1) {  // (plane-to-plane: the same solve over J^T M J, J^T M d, d^T M d; voxelised: weighted)
    st->rmse = sqrt(S[QTR_ICP_T_R2] / (cfg->method == 3 ? S[QTR_ICP_T_W] : n));
    double b[6], x[6];
    for (int a = 0; a < 6; ++a) b[a] = -S[QTR_ICP_T_JTR + a];
    if (!qtr_icp_solve6(S, b, x)) {
      st->stop = 1;
      st->reason = QTR_ICP_STOP_DEGENERATE;
      st->valid = 0;
      st->converged = 0;
      return;
    }
    qtr_icp_rot_from_omega(x, dR);
    dt[0] = x[3];
    dt[1] = x[4];
    dt[2] = x[5];
  } else {
    st->rmse = sqrt(mse);
    double ms[3], mt[3], H[9];
    for (int a = 0; a < 3; ++a) {
      ms[a] = S[QTR_ICP_T_SQ + a] / n;
      mt[a] = S[QTR_ICP_T_ST + a] / n;
    }
    for (int a = 0; a < 3; ++a)
      for (int c = 0; c < 3; ++c) H[3 * a + c] = S[QTR_ICP_T_QT + 3 * a + c] - (S[QTR_ICP_T_SQ + a] * mt[c]);
    // a cross-covariance of rank < 2 leaves the rotation undetermined (collinear points): degenerate like a plane is
    // for point-to-plane.  H's scale: its trace of squares against the spread of the source points
    double spread = 0.0;
    for (int a = 0; a < 9; ++a) spread = spread + H[a] * H[a];
    if (!(spread > 0.0)) {
      st->stop = 1;
      st->reason = QTR_ICP_STOP_DEGENERATE;
      st->valid = 0;
      st->converged = 0;
      return;
    }
    qm_rot3_from_h(H, dR);
    for (int a = 0; a < 3; ++a) dt[a] = mt[a] - ((dR[3 * a] * ms[0] + dR[3 * a + 1] * ms[1]) + dR[3 * a + 2] * ms[2]);
  }
  qtr_icp_compose(dR, dt, st->T);
  st->iterations = st->iterations + 1;
  st->valid = 1;
  if (trace) {
    for (int k = 0; k < 16; ++k) trace[k] = st->T[k];
    trace[16] = mse;
    trace[17] = n;
  }
  // max |dT - I| over the 3x4 block
  double dmax = 0.0;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) {
      const double e = dR[3 * r + c] - (r == c ? 1.0 : 0.0);
      const double ae = e < 0 ? -e : e;
      dmax = ae > dmax ? ae : dmax;
    }
    const double ae = dt[r] < 0 ? -dt[r] : dt[r];
    dmax = ae > dmax ? ae : dmax;
  }
  const double prev = st->prev_mse;
  st->prev_mse = mse;
  if (st->iterations >= cfg->max_iterations) {
    st->reason = QTR_ICP_STOP_MAX_ITERATIONS;
  } else if (dmax <= cfg->trans_eps) {
    st->reason = QTR_ICP_STOP_TRANSFORMATION;
  } else if (prev >= 0.0) {
    const double ch = mse - prev;
    if ((ch < 0 ? -ch : ch) <= cfg->fit_eps * prev) st->reason = QTR_ICP_STOP_FITNESS;
  }
  if (st->reason != QTR_ICP_RUNNING) {
    st->stop = 1;
    st->converged = 1;
  }
}
