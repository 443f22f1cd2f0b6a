// qtr_pgo_math.h — the arithmetic of the robust pose-graph optimisation (qtr_pgo_optimize), shared by the gfx950 kernels
// (quatro_amd/csrc/pgo.hip: k_pgo_linearize, k_pgo_step) and the host restatement of the tests (g++), in the style of
// qtr_icp_math.h and qtr_eval_math.h: binary64 + - * / sqrt only (no sin, cos, acos, pow), evaluated in the order written;
// both sides compile with -ffp-contract=off, so host and device agree bit for bit.  The formulation is Open3D's
// GlobalOptimizationLevenbergMarquardt with the line process of Choi et al. 2015 (restated from its published description).
//
// Graph.  N nodes with poses X_i (row-major 4x4, keyframe i's frame -> map frame: what make_submap gives poses[i]), a
// `fixed` flag per node, E edges (s, t, Z, Omega, uncertain).  Z maps keyframe s's frame into keyframe t's frame (a
// close_loop record's T with s = the query, t = the candidate).  Omega is the 6x6 `information` of qtr_evaluate: parameters
// [omega | v], left increment in the target frame; only its upper triangle is read.
//
// Residual.  E_e = X_t^-1 (X_s Z^-1) with rigid inverses [R^T | -R^T t] (qtr_pgo_inv; the product in that association),
//   r_e = [(E21 - E12) / 2, (E02 - E20) / 2, (E10 - E01) / 2, E03, E13, E23]                        (qtr_pgo_vee).
// Z^-1 stands on the RIGHT: Omega was formed under X_t^-1 X_s = exp(xi) Z (G = [-[t]x | I] on the TARGET point, the left
// increment of qtr_icp_compose), so E_e ~ exp(xi) and r_e is that xi to first order.  Open3D forms Z^-1 X_t^-1 X_s, Z^-1 on
// the left, which measures the same error in the SOURCE frame; with an Omega built on target points that weights the wrong
// lever arms.  This is the one deliberate divergence of the residual.
//
// Jacobian.  Node increments are X_i <- [dR(delta_i) dt(delta_i)] X_i (qtr_icp_rot_from_omega, qtr_icp_compose).  r is
// linear in E, so column k of J_e = d r / d delta_s is exactly the vee of X_t^-1 G_k (X_s Z^-1) with the six generators G_k
// (k < 3: [e_k]x in the rotation block; k >= 3: e_(k-3) in the translation column), and d r / d delta_t = -J_e exactly.
// One edge contributes A_e = w_e J^T Omega J (21 upper entries, row-major upper triangle) and g_e = w_e J^T Omega r.  The
// normal matrix is the block Laplacian H = sum_e (e_s - e_t)(e_s - e_t)^T (x) A_e; no off-diagonal block is ever stored:
//   diagonal block of node i   D_i = sum of A_e over the edges incident on i              (qtr_pgo_node_gather)
//   gradient of node i         g_i = sum of +g_e (i = s) / -g_e (i = t)
//   product                    y_i = sum of +A_e (x_s - x_t) (i = s) / -(..) (i = t), then + lambda x_i   (qtr_pgo_matvec_node)
// EVERY per-node sum runs over the node's incidence list in ASCENDING EDGE INDEX (the list holds an edge once per endpoint;
// s == t is refused), starting from 0.0.
//
// Line process.  chi2_e = r^T Omega r; w_e = 1 for a certain edge, w_e = s^2 with s = mu / (mu + chi2_e) for an uncertain
// one, recomputed at every linearisation (mu = line_process_weight; mu <= 0: every w_e = 1).  The objective is
// F = sum w_e chi2_e + mu sum_uncertain (s - 1)^2 (s = sqrt(w_e), never formed by a root).  F is summed in the ICP's shape
// over 256-edge chunks: qtr_icp_fold64 per 64 edges, qtr_icp_chunk_sum, the chunks in ascending order.
//
// Levenberg-Marquardt (qtr_pgo_decide).  lambda_0 = tau max diag(H) over the free nodes (tau itself when that is not
// positive); (H + lambda I) delta = -g over the free nodes (a fixed node has delta = 0: its rows and columns are dropped);
// rho = (F - F_new) / (delta^T (lambda delta - g)); accepted when rho > 0: lambda <- lambda max(1/3, 1 - (2 rho - 1)^3)
// (the cube as two products), nu = 2; rejected: the poses are restored, lambda <- lambda nu, nu <- 2 nu.  Stops:
// QTR_PGO_STOP_MAX_ITERATIONS (trial steps evaluated), _RELATIVE (accepted with F - F_new <= rel_tol F), _STEP
// (max |delta| < step_tol: the step is not taken), _LAMBDA (lambda > QTR_PGO_LAMBDA_MAX, also where F is not finite),
// _NOTHING (no edge or no free node: nothing runs).  A connected component without a fixed node is NOT an error: lambda > 0
// keeps H + lambda I positive definite, the component keeps the gauge its initial poses gave it.
//
// Linear solve (one workgroup of QTR_PGO_THREADS threads; the order below is the kernel's).  Preconditioned conjugate
// gradients, block Jacobi: z_i = (D_i + lambda I)^-1 r_i by qtr_icp_solve6 (z_i = r_i should it refuse).  Vectors have 6 N
// entries, zero at fixed nodes.
//   x = 0, r = -g, z = M^-1 r, p = z, rz = <r, z>, rr = <r, r>, limit = pcg_tol^2 rr
//   while its < pcg_max_iterations and rr > limit:
//     q = (H + lambda I) p;  alpha = rz / <p, q>;  x[k] = x[k] + alpha p[k];  r[k] = r[k] - alpha q[k];  rr = <r, r>;  its += 1
//     if not rr > limit: stop;  z = M^-1 r;  rzn = <r, z>;  beta = rzn / rz;  rz = rzn;  p[k] = z[k] + beta p[k]
// Dot product <a, b> (qtr_pgo_dot_partial, qtr_pgo_dot_finish): thread t adds a[k] b[k] for k = t, t + 1024, ... in ascending
// order from 0.0; qtr_icp_fold64 inside each of the 16 waves; the wave sums w0 + w1 + ... + w15 from left to right.
// After the loop: u[k] = lambda x[k] - g[k] (0 at fixed nodes), denom = <x, u>, max_step = max |x[k]|, and the trial poses
// X_i <- [dR(x_i[0..3]) x_i[3..6]] X_i.
#pragma once
#include "qtr_icp_math.h"

#define QTR_PGO_THREADS 1024    // threads of the one workgroup of k_pgo_step: the stride of a dot product's partials
#define QTR_PGO_LAMBDA_MAX 1e32 // the ceiling of lambda
#define QTR_PGO_TRACE 8         // doubles per row of the iteration trace (layout: qtr_pgo_decide)

#define QTR_PGO_RUNNING 0
#define QTR_PGO_STOP_MAX_ITERATIONS 1
#define QTR_PGO_STOP_RELATIVE 2
#define QTR_PGO_STOP_STEP 3
#define QTR_PGO_STOP_LAMBDA 4
#define QTR_PGO_STOP_NOTHING 5

typedef struct QtrPgoCfg {
  double rel_tol, step_tol, tau, pcg_tol, mu;
  int max_iterations, pcg_max_iterations;
} QtrPgoCfg;

typedef struct QtrPgoState {
  double F;         // objective at the accepted poses
  double F0;        // ... and at the initial ones
  double lambda, nu;
  double denom;     // delta^T (lambda delta - g) of the last solve
  double max_step;  // max |delta| of the last solve
  int started;      // 1: the initial linearisation was taken
  int cur;          // parity of the accepted poses and of their linearisation (the trial side is 1 - cur)
  int trials;       // trial steps evaluated
  int accepted;
  int pcg_last, pcg_total;
  int stop, reason;
} QtrPgoState;

// index of (a, b) in the 21 upper entries of a symmetric 6x6, row-major upper triangle
QM_HD int qtr_pgo_u(int a, int b) { return a <= b ? (a * (11 - a)) / 2 + b : (b * (11 - b)) / 2 + a; }

// Omega[a][b] read from the upper triangle of the row-major 6x6
QM_HD double qtr_pgo_om(const double* info, int a, int b) { return a <= b ? info[6 * a + b] : info[6 * b + a]; }

// Y (3x4) = the rigid inverse of X (rows 0 - 2 of a row-major 4x4 are read)
QM_HD void qtr_pgo_inv(const double* X, double* Y /* [12] */) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Y[4 * r + c] = X[4 * c + r];
    Y[4 * r + 3] = -((X[r] * X[3] + X[4 + r] * X[7]) + X[8 + r] * X[11]);
  }
}

// C (3x4) = A B for rigid A, B (rows 0 - 2; the bottom row is 0 0 0 1)
QM_HD void qtr_pgo_mul(const double* A, const double* B, double* C /* [12] */) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) C[4 * r + c] = (A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c];
    C[4 * r + 3] = ((A[4 * r] * B[3] + A[4 * r + 1] * B[7]) + A[4 * r + 2] * B[11]) + A[4 * r + 3];
  }
}

// C (3x4) = rot(A) B for a B whose bottom row is zero (a generator times a pose): A's translation takes no part
QM_HD void qtr_pgo_rotmul(const double* A, const double* B, double* C /* [12] */) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) C[4 * r + c] = (A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c];
}

QM_HD void qtr_pgo_vee(const double* E /* [12] */, double* r /* [6] */) {
  r[0] = 0.5 * (E[9] - E[6]);
  r[1] = 0.5 * (E[2] - E[8]);
  r[2] = 0.5 * (E[4] - E[1]);
  r[3] = E[3];
  r[4] = E[7];
  r[5] = E[11];
}

// G_k P for the generator k and the 3x4 P: k < 3: e_k x every column; k >= 3: e_(k-3) in the last column
QM_HD void qtr_pgo_generator(int k, const double* P /* [12] */, double* Q /* [12] */) {
  for (int j = 0; j < 12; ++j) Q[j] = 0.0;
  if (k >= 3) {
    Q[4 * (k - 3) + 3] = 1.0;
    return;
  }
  const int a = (k + 1) % 3, b = (k + 2) % 3;  // e_k x v: row a gets -v_b, row b gets v_a
  for (int c = 0; c < 4; ++c) {
    Q[4 * a + c] = -P[4 * b + c];
    Q[4 * b + c] = P[4 * a + c];
  }
}

// r_e and (J not null) J_e, row-major 6x6: J[6 a + k] = d r_a / d delta_s[k]
QM_HD void qtr_pgo_residual(const double* Xs, const double* Xt, const double* Z, double* r /* [6] */, double* J /* [36] or null */) {
  double Zi[12], Xti[12], P[12], Em[12];
  qtr_pgo_inv(Z, Zi);
  qtr_pgo_inv(Xt, Xti);
  qtr_pgo_mul(Xs, Zi, P);
  qtr_pgo_mul(Xti, P, Em);
  qtr_pgo_vee(Em, r);
  if (!J) return;
  for (int k = 0; k < 6; ++k) {
    double Q[12], D[12], col[6];
    qtr_pgo_generator(k, P, Q);
    qtr_pgo_rotmul(Xti, Q, D);
    qtr_pgo_vee(D, col);
    for (int a = 0; a < 6; ++a) J[6 * a + k] = col[a];
  }
}

// The terms of one edge.  info: row-major 6x6, upper triangle read.  Every 6-term sum runs from index 0 to 5, left to right.
// sc: chi2, w, the edge's share of F.
QM_HD void qtr_pgo_edge_terms(const double* Xs, const double* Xt, const double* Z, const double* info, int uncertain, double mu,
                              double* A /* [21] */, double* g /* [6] */, double* sc /* [3] */) {
  double r[6], J[36], v[6], B[36];
  qtr_pgo_residual(Xs, Xt, Z, r, J);
  for (int a = 0; a < 6; ++a) {  // v = Omega r, B = Omega J
    double s = qtr_pgo_om(info, a, 0) * r[0];
    for (int b = 1; b < 6; ++b) s = s + qtr_pgo_om(info, a, b) * r[b];
    v[a] = s;
    for (int k = 0; k < 6; ++k) {
      double t = qtr_pgo_om(info, a, 0) * J[k];
      for (int b = 1; b < 6; ++b) t = t + qtr_pgo_om(info, a, b) * J[6 * b + k];
      B[6 * a + k] = t;
    }
  }
  double chi2 = r[0] * v[0];
  for (int a = 1; a < 6; ++a) chi2 = chi2 + r[a] * v[a];
  double w = 1.0, F = chi2;
  if (uncertain && mu > 0.0) {
    const double s = mu / (mu + chi2);
    w = s * s;
    F = w * chi2 + mu * ((s - 1.0) * (s - 1.0));
  }
  int n = 0;
  for (int k = 0; k < 6; ++k) {
    for (int l = k; l < 6; ++l) {
      double s = J[k] * B[l];
      for (int a = 1; a < 6; ++a) s = s + J[6 * a + k] * B[6 * a + l];
      A[n++] = w * s;
    }
    double s = J[k] * v[0];
    for (int a = 1; a < 6; ++a) s = s + J[6 * a + k] * v[a];
    g[k] = w * s;
  }
  sc[0] = chi2;
  sc[1] = w;
  sc[2] = F;
}

// D_i and g_i of node i from the edge terms EA [E][21], Eg [E][6]: off / inc are the CSR incidence lists (ascending edge
// index inside a node)
QM_HD void qtr_pgo_node_gather(int i, const int* off, const int* inc, const int* src, const double* EA, const double* Eg,
                               double* D /* [21] */, double* g /* [6] */) {
  for (int k = 0; k < 21; ++k) D[k] = 0.0;
  for (int k = 0; k < 6; ++k) g[k] = 0.0;
  for (int j = off[i]; j < off[i + 1]; ++j) {
    const int e = inc[j];
    for (int k = 0; k < 21; ++k) D[k] = D[k] + EA[(size_t)21 * e + k];
    if (src[e] == i)
      for (int k = 0; k < 6; ++k) g[k] = g[k] + Eg[(size_t)6 * e + k];
    else
      for (int k = 0; k < 6; ++k) g[k] = g[k] - Eg[(size_t)6 * e + k];
  }
}

// the largest diagonal entry of D (the caller starts from 0.0 and folds the free nodes in; a maximum has no order)
QM_HD double qtr_pgo_diag_max(const double* D /* [21] */, double m) {
  for (int a = 0; a < 6; ++a) {
    const double d = D[qtr_pgo_u(a, a)];
    m = d > m ? d : m;
  }
  return m;
}

// z = (D + lambda I)^-1 r; z = r where qtr_icp_solve6 refuses the block
QM_HD void qtr_pgo_precond(const double* D /* [21] */, double lambda, const double* r, double* z) {
  double U[21];
  for (int k = 0; k < 21; ++k) U[k] = D[k];
  for (int a = 0; a < 6; ++a) U[qtr_pgo_u(a, a)] = U[qtr_pgo_u(a, a)] + lambda;
  if (!qtr_icp_solve6(U, r, z))
    for (int a = 0; a < 6; ++a) z[a] = r[a];
}

// y_i = ((H + lambda I) x)_i for a free node i
QM_HD void qtr_pgo_matvec_node(int i, const int* off, const int* inc, const int* src, const int* dst, const double* EA,
                               double lambda, const double* x /* [6 N] */, double* y /* [6] */) {
  for (int a = 0; a < 6; ++a) y[a] = 0.0;
  for (int j = off[i]; j < off[i + 1]; ++j) {
    const int e = inc[j], s = src[e], t = dst[e];
    const double* A = EA + (size_t)21 * e;
    double d[6];
    for (int a = 0; a < 6; ++a) d[a] = x[(size_t)6 * s + a] - x[(size_t)6 * t + a];
    for (int a = 0; a < 6; ++a) {
      double v = A[qtr_pgo_u(a, 0)] * d[0];
      for (int b = 1; b < 6; ++b) v = v + A[qtr_pgo_u(a, b)] * d[b];
      y[a] = (s == i) ? y[a] + v : y[a] - v;
    }
  }
  for (int a = 0; a < 6; ++a) y[a] = y[a] + lambda * x[(size_t)6 * i + a];
}

QM_HD double qtr_pgo_dot_partial(const double* a, const double* b, int n, int t) {
  double acc = 0.0;
  for (int k = t; k < n; k += QTR_PGO_THREADS) acc = acc + a[k] * b[k];
  return acc;
}
QM_HD double qtr_pgo_dot_finish(double* part /* [QTR_PGO_THREADS], clobbered */) {
  double s = qtr_icp_fold64(part);
  for (int w = 1; w < QTR_PGO_THREADS / 64; ++w) s = s + qtr_icp_fold64(part + 64 * w);
  return s;
}

// the trial pose of a free node: Xn = [dR(x[0..3]) x[3..6]] X
QM_HD void qtr_pgo_update_node(const double* X, const double* x /* [6] */, double* Xn /* [16] */) {
  double dR[9];
  qtr_icp_rot_from_omega(x, dR);
  for (int k = 0; k < 16; ++k) Xn[k] = X[k];
  qtr_icp_compose(dR, x + 3, Xn);
}

QM_HD void qtr_pgo_init(QtrPgoState* s) {
  s->F = 0.0;
  s->F0 = 0.0;
  s->lambda = 0.0;
  s->nu = 2.0;
  s->denom = 0.0;
  s->max_step = 0.0;
  s->started = 0;
  s->cur = 0;
  s->trials = 0;
  s->accepted = 0;
  s->pcg_last = 0;
  s->pcg_total = 0;
  s->stop = 0;
  s->reason = QTR_PGO_RUNNING;
}

// What the end of a linearisation decides.  F_new, max_diag: the objective and max diag(H) at the poses just linearised (the
// trial side).  The first call takes them as the start; every later one judges the trial step.  trace (may be null) receives
// the row [F_new, lambda after, rho, accepted, PCG iterations of the step judged, F after, denom, max_step].
QM_HD void qtr_pgo_decide(const QtrPgoCfg* c, QtrPgoState* s, double F_new, double max_diag, double* trace /* [QTR_PGO_TRACE] */) {
  double rho = 0.0;
  int acc = 1;
  if (!s->started) {
    s->started = 1;
    s->F = F_new;
    s->F0 = F_new;
    s->lambda = c->tau * max_diag;
    if (!(s->lambda > 0.0)) s->lambda = c->tau;
    s->nu = 2.0;
    s->cur = 1 - s->cur;
  } else {
    s->trials = s->trials + 1;
    const double dF = s->F - F_new;
    rho = dF / s->denom;
    acc = rho > 0.0 ? 1 : 0;
    if (acc) {
      const double t = 2.0 * rho - 1.0;
      const double f = 1.0 - (t * t) * t;
      const double third = 1.0 / 3.0;
      s->lambda = s->lambda * (f > third ? f : third);
      s->nu = 2.0;
      if (dF <= c->rel_tol * s->F) s->reason = QTR_PGO_STOP_RELATIVE;
      s->F = F_new;
      s->cur = 1 - s->cur;
      s->accepted = s->accepted + 1;
    } else {
      s->lambda = s->lambda * s->nu;
      s->nu = 2.0 * s->nu;
    }
  }
  if (s->reason == QTR_PGO_RUNNING) {
    if (s->trials >= c->max_iterations)
      s->reason = QTR_PGO_STOP_MAX_ITERATIONS;
    else if (!(s->lambda <= QTR_PGO_LAMBDA_MAX))
      s->reason = QTR_PGO_STOP_LAMBDA;
  }
  if (s->reason != QTR_PGO_RUNNING) s->stop = 1;
  if (trace) {
    trace[0] = F_new;
    trace[1] = s->lambda;
    trace[2] = rho;
    trace[3] = (double)acc;
    trace[4] = (double)s->pcg_last;
    trace[5] = s->F;
    trace[6] = s->denom;
    trace[7] = s->max_step;
  }
}

// What the end of a solve records: the PCG count, denom, max_step, and the stop on a step below step_tol (the trial poses
// are then not evaluated).
QM_HD void qtr_pgo_after_solve(const QtrPgoCfg* c, QtrPgoState* s, int its, double denom, double max_step) {
  s->pcg_last = its;
  s->pcg_total = s->pcg_total + its;
  s->denom = denom;
  s->max_step = max_step;
  if (max_step < c->step_tol) {
    s->reason = QTR_PGO_STOP_STEP;
    s->stop = 1;
  }
}

// ---- the whole optimisation, serially, on the host: the order of operations the two kernels follow ---------------------
#include <stdlib.h>
#include <string.h>

// CSR incidence lists by a counting sort: off [N + 1], inc [2 E]; an edge appears in the lists of both its endpoints, and
// inside a list the edge indices ascend
static inline void qtr_pgo_incidence(int N, int E, const int* src, const int* dst, int* off, int* inc) {
  for (int i = 0; i <= N; ++i) off[i] = 0;
  for (int e = 0; e < E; ++e) {
    off[src[e] + 1] += 1;
    off[dst[e] + 1] += 1;
  }
  for (int i = 0; i < N; ++i) off[i + 1] += off[i];
  int* at = (int*)malloc(sizeof(int) * (size_t)(N > 0 ? N : 1));
  for (int i = 0; i < N; ++i) at[i] = off[i];
  for (int e = 0; e < E; ++e) {
    inc[at[src[e]]++] = e;
    inc[at[dst[e]]++] = e;
  }
  free(at);
}

static inline double qtr_pgo_dot_host(const double* a, const double* b, int n) {
  double part[QTR_PGO_THREADS];
  for (int t = 0; t < QTR_PGO_THREADS; ++t) part[t] = qtr_pgo_dot_partial(a, b, n, t);
  return qtr_pgo_dot_finish(part);
}

// F summed in the ICP's shape over the edges' shares f [E]
static inline double qtr_pgo_sum_host(const double* f, int E) {
  double acc = 0.0;
  for (int c = 0; c * QTR_ICP_CHUNK < E; ++c) {
    double w[4];
    for (int wv = 0; wv < 4; ++wv) {
      double lanes[64];
      for (int l = 0; l < 64; ++l) {
        const int e = c * QTR_ICP_CHUNK + 64 * wv + l;
        lanes[l] = e < E ? f[e] : 0.0;
      }
      w[wv] = qtr_icp_fold64(lanes);
    }
    const double cs = qtr_icp_chunk_sum(w);
    acc = c == 0 ? cs : acc + cs;
  }
  return acc;
}

// poses [16 N] in, poses_out [16 N] and weights [E] out, trace [(max_iterations + 1) QTR_PGO_TRACE] (rows written:
// 1 + st->trials), pcg_rr (may be null) [pcg_max_iterations + 1]: <r, r> before and after every iteration of the FIRST solve.
// Needs E >= 1 and a free node (the caller answers QTR_PGO_STOP_NOTHING itself).
static inline void qtr_pgo_reference(const QtrPgoCfg* cfg, int N, const double* poses, const unsigned char* fixed, int E,
                                     const int* src, const int* dst, const double* Z, const double* info,
                                     const unsigned char* uncertain, double* poses_out, double* weights, QtrPgoState* st,
                                     double* trace, double* pcg_rr) {
  const size_t n6 = (size_t)6 * N;
  int* off = (int*)malloc(sizeof(int) * (size_t)(N + 1));
  int* inc = (int*)malloc(sizeof(int) * (size_t)(2 * E));
  qtr_pgo_incidence(N, E, src, dst, off, inc);
  double* X[2] = {(double*)malloc(8 * 16 * (size_t)N), (double*)malloc(8 * 16 * (size_t)N)};
  double* EA[2] = {(double*)malloc(8 * 21 * (size_t)E), (double*)malloc(8 * 21 * (size_t)E)};
  double* Ew[2] = {(double*)malloc(8 * (size_t)E), (double*)malloc(8 * (size_t)E)};
  double* ND[2] = {(double*)malloc(8 * 21 * (size_t)N), (double*)malloc(8 * 21 * (size_t)N)};
  double* Ng[2] = {(double*)malloc(8 * n6), (double*)malloc(8 * n6)};
  double* Eg = (double*)malloc(8 * 6 * (size_t)E);
  double* Ef = (double*)malloc(8 * (size_t)E);
  double* v = (double*)malloc(8 * 5 * n6);
  double *x = v, *r = v + n6, *z = v + 2 * n6, *p = v + 3 * n6, *q = v + 4 * n6;
  memcpy(X[1], poses, 8 * 16 * (size_t)N);  // (the start is the first "trial")
  memcpy(X[0], poses, 8 * 16 * (size_t)N);
  qtr_pgo_init(st);
  for (int round = 0;; ++round) {
    // ---- k_pgo_linearize
    const int tb = 1 - st->cur;
    for (int e = 0; e < E; ++e) {
      double sc[3];
      qtr_pgo_edge_terms(X[tb] + 16 * (size_t)src[e], X[tb] + 16 * (size_t)dst[e], Z + 16 * (size_t)e, info + 36 * (size_t)e,
                         uncertain ? uncertain[e] : 0, cfg->mu, EA[tb] + 21 * (size_t)e, Eg + 6 * (size_t)e, sc);
      Ew[tb][e] = sc[1];
      Ef[e] = sc[2];
    }
    const double F_new = qtr_pgo_sum_host(Ef, E);
    double md = 0.0;
    for (int i = 0; i < N; ++i) {
      qtr_pgo_node_gather(i, off, inc, src, EA[tb], Eg, ND[tb] + 21 * (size_t)i, Ng[tb] + 6 * (size_t)i);
      if (!fixed[i]) md = qtr_pgo_diag_max(ND[tb] + 21 * (size_t)i, md);
    }
    qtr_pgo_decide(cfg, st, F_new, md, trace + (size_t)QTR_PGO_TRACE * st->trials + (st->started ? QTR_PGO_TRACE : 0));
    if (st->stop) break;
    // ---- k_pgo_step
    const int cur = st->cur;
    const double lambda = st->lambda;
    const double *A = EA[cur], *D = ND[cur], *g = Ng[cur];
    for (int i = 0; i < N; ++i)
      for (int a = 0; a < 6; ++a) {
        const size_t k = (size_t)6 * i + a;
        x[k] = 0.0;
        q[k] = 0.0;
        r[k] = fixed[i] ? 0.0 : -g[k];
      }
    for (int i = 0; i < N; ++i) {
      if (fixed[i])
        for (int a = 0; a < 6; ++a) z[6 * (size_t)i + a] = 0.0;
      else
        qtr_pgo_precond(D + 21 * (size_t)i, lambda, r + 6 * (size_t)i, z + 6 * (size_t)i);
      for (int a = 0; a < 6; ++a) p[6 * (size_t)i + a] = z[6 * (size_t)i + a];
    }
    double rz = qtr_pgo_dot_host(r, z, (int)n6), rr = qtr_pgo_dot_host(r, r, (int)n6);
    const double limit = (cfg->pcg_tol * cfg->pcg_tol) * rr;
    int its = 0;
    if (pcg_rr && round == 0) pcg_rr[0] = rr;
    while (its < cfg->pcg_max_iterations && rr > limit) {
      for (int i = 0; i < N; ++i)
        if (!fixed[i]) qtr_pgo_matvec_node(i, off, inc, src, dst, A, lambda, p, q + 6 * (size_t)i);
      const double alpha = rz / qtr_pgo_dot_host(p, q, (int)n6);
      for (size_t k = 0; k < n6; ++k) {
        x[k] = x[k] + alpha * p[k];
        r[k] = r[k] - alpha * q[k];
      }
      rr = qtr_pgo_dot_host(r, r, (int)n6);
      its += 1;
      if (pcg_rr && round == 0) pcg_rr[its] = rr;
      if (!(rr > limit)) break;
      for (int i = 0; i < N; ++i)
        if (!fixed[i]) qtr_pgo_precond(D + 21 * (size_t)i, lambda, r + 6 * (size_t)i, z + 6 * (size_t)i);
      const double rzn = qtr_pgo_dot_host(r, z, (int)n6);
      const double beta = rzn / rz;
      rz = rzn;
      for (size_t k = 0; k < n6; ++k) p[k] = z[k] + beta * p[k];
    }
    double ms = 0.0;
    for (int i = 0; i < N; ++i)
      for (int a = 0; a < 6; ++a) {
        const size_t k = (size_t)6 * i + a;
        q[k] = fixed[i] ? 0.0 : lambda * x[k] - g[k];  // (u)
        const double ax = x[k] < 0 ? -x[k] : x[k];
        ms = ax > ms ? ax : ms;
      }
    const double denom = qtr_pgo_dot_host(x, q, (int)n6);
    for (int i = 0; i < N; ++i) {
      if (fixed[i])
        memcpy(X[1 - cur] + 16 * (size_t)i, X[cur] + 16 * (size_t)i, 8 * 16);
      else
        qtr_pgo_update_node(X[cur] + 16 * (size_t)i, x + 6 * (size_t)i, X[1 - cur] + 16 * (size_t)i);
    }
    qtr_pgo_after_solve(cfg, st, its, denom, ms);
    if (st->stop) break;
  }
  memcpy(poses_out, X[st->cur], 8 * 16 * (size_t)N);
  memcpy(weights, Ew[st->cur], 8 * (size_t)E);
  for (int k = 0; k < 2; ++k) {
    free(X[k]);
    free(EA[k]);
    free(Ew[k]);
    free(ND[k]);
    free(Ng[k]);
  }
  free(Eg);
  free(Ef);
  free(v);
  free(off);
  free(inc);
}
