// pgo.hip — robust pose-graph optimisation on the device (qtr_pgo_optimize): Levenberg-Marquardt over the edges (T, Omega)
// the evaluation emits, with the line process over the uncertain ones.  The arithmetic is include/qtr_pgo_math.h; this file
// is its parallel form and follows that header's order operation for operation.
//
// Per LM iteration the host enqueues two launches:
//   k_pgo_linearize  ceil(E / 256) x 256, one thread per edge, at the TRIAL poses (side 1 - cur): r, chi2, w, J, the 21 + 6
//                    edge terms and the edge's share of F.  The last workgroup to arrive (the atomic ticket of
//                    icp_reduce_tail: nobody waits for anybody, no co-residency is assumed) adds the shares in chunk order,
//                    gathers every node's diagonal block and gradient over its incidence list, and decides
//                    (qtr_pgo_decide: it sees F and F_new): accept flips `cur`, reject leaves the accepted side alone.
//   k_pgo_step       ONE workgroup of 1024 threads: the whole PCG loop on the accepted side with __syncthreads() between
//                    phases, then denom, max |delta| and the trial poses for the next k_pgo_linearize.
// Both return at once when the state says stop.  Everything a later launch reads was written by an earlier launch, except
// the edge terms the tail of k_pgo_linearize gathers: those are ordered by the tail's fences and its ticket.
#include "common.h"
#include "../../include/qtr_pgo_math.h"

struct PgoView {
  int N, E;
  const unsigned char* fixed;  // [N]
  const unsigned char* unc;    // [E]
  const int *src, *dst;        // [E]
  const int *off, *inc;        // CSR incidence: [N + 1], [2 E]
  const double* Z;             // [E][16]
  const double* info;          // [E][36]
  double* X[2];                // poses, both sides
  double* EA[2];               // [E][21] edge blocks, both sides
  double* Ew[2];               // [E] weights
  double* Eg;                  // [E][6] edge gradients of the side being linearised (read by its own tail only)
  double* ND[2];               // [N][21] diagonal blocks
  double* Ng[2];               // [N][6] gradients
  double *vx, *vr, *vz, *vp, *vq;  // [6 N] each
  double* partials;            // [ceil(E / 256)]
  unsigned* ticket;
  QtrPgoState* st;
  double* trace;               // [max_iterations + 1][QTR_PGO_TRACE]
  QtrPgoCfg cfg;
};

__global__ __launch_bounds__(256) void k_pgo_linearize(PgoView v) {
  __shared__ double s_S[1];
  __shared__ double s_m[4];
  if (v.st->stop) return;  // (uniform: written by an earlier launch)
  const int tb = 1 - v.st->cur;
  const int tid = threadIdx.x, e = (int)blockIdx.x * 256 + tid;
  double f = 0.0;
  if (e < v.E) {
    double A[21], g[6], sc[3];
    const double* X = v.X[tb];
    qtr_pgo_edge_terms(X + (size_t)16 * v.src[e], X + (size_t)16 * v.dst[e], v.Z + (size_t)16 * e, v.info + (size_t)36 * e,
                       (int)v.unc[e], v.cfg.mu, A, g, sc);
    double* EA = v.EA[tb] + (size_t)21 * e;
#pragma unroll
    for (int k = 0; k < 21; ++k) EA[k] = A[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) v.Eg[(size_t)6 * e + k] = g[k];
    v.Ew[tb][e] = sc[1];
    f = sc[2];
  }
  if (!icp_reduce_tail<1, 1>(&f, v.partials, v.ticket, (int)blockIdx.x, (int)gridDim.x, s_S)) return;
  // the last workgroup: every edge's terms are in place (each workgroup fenced before it took its ticket)
  double m = 0.0;
  for (int i = tid; i < v.N; i += 256) {
    double D[21], g[6];
    qtr_pgo_node_gather(i, v.off, v.inc, v.src, v.EA[tb], v.Eg, D, g);
    double* ND = v.ND[tb] + (size_t)21 * i;
    for (int k = 0; k < 21; ++k) ND[k] = D[k];
    for (int k = 0; k < 6; ++k) v.Ng[tb][(size_t)6 * i + k] = g[k];
    if (!v.fixed[i]) m = qtr_pgo_diag_max(D, m);
  }
  for (int off = 32; off >= 1; off >>= 1) {
    const double o = icp_shfl_down(m, off);
    m = o > m ? o : m;
  }
  if ((tid & 63) == 0) s_m[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) m = s_m[w] > m ? s_m[w] : m;
    QtrPgoState s = *v.st;
    qtr_pgo_decide(&v.cfg, &s, s_S[0], m, v.trace + (size_t)QTR_PGO_TRACE * (s.trials + s.started));
    *v.st = s;
    __hip_atomic_store(v.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// <a, b> in the header's shape; every thread of the workgroup returns the same value.  The leading barrier orders the
// vectors' last writes before the reads and the previous call's readers of s_w before its writers.
__device__ __forceinline__ double pgo_dot(const double* a, const double* b, int n, double* s_w /* LDS [16] */) {
  __syncthreads();
  double acc = qtr_pgo_dot_partial(a, b, n, (int)threadIdx.x);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc = acc + icp_shfl_down(acc, off);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
  __syncthreads();
  double s = s_w[0];
  for (int w = 1; w < QTR_PGO_THREADS / 64; ++w) s = s + s_w[w];
  return s;
}

__global__ __launch_bounds__(QTR_PGO_THREADS) void k_pgo_step(PgoView v) {
  __shared__ double s_w[QTR_PGO_THREADS / 64];
  __shared__ double s_m[QTR_PGO_THREADS / 64];
  if (v.st->stop) return;
  const int cur = v.st->cur, tid = threadIdx.x, N = v.N, n6 = 6 * v.N;
  const double lambda = v.st->lambda;
  const double *A = v.EA[cur], *D = v.ND[cur], *g = v.Ng[cur];
  double *x = v.vx, *r = v.vr, *z = v.vz, *p = v.vp, *q = v.vq;
  for (int i = tid; i < N; i += QTR_PGO_THREADS) {
    const bool fx = v.fixed[i] != 0;
    double ri[6], zi[6];
    for (int a = 0; a < 6; ++a) {
      ri[a] = fx ? 0.0 : -g[(size_t)6 * i + a];
      zi[a] = 0.0;
    }
    if (!fx) qtr_pgo_precond(D + (size_t)21 * i, lambda, ri, zi);
    for (int a = 0; a < 6; ++a) {
      const size_t k = (size_t)6 * i + a;
      x[k] = 0.0;
      q[k] = 0.0;
      r[k] = ri[a];
      z[k] = zi[a];
      p[k] = zi[a];
    }
  }
  double rz = pgo_dot(r, z, n6, s_w), rr = pgo_dot(r, r, n6, s_w);
  const double limit = (v.cfg.pcg_tol * v.cfg.pcg_tol) * rr;
  int its = 0;
  while (its < v.cfg.pcg_max_iterations && rr > limit) {  // (uniform: every thread holds the same rr)
    __syncthreads();                                       // (p of the previous round is complete)
    for (int i = tid; i < N; i += QTR_PGO_THREADS)
      if (!v.fixed[i]) {
        double y[6];
        qtr_pgo_matvec_node(i, v.off, v.inc, v.src, v.dst, A, lambda, p, y);
        for (int a = 0; a < 6; ++a) q[(size_t)6 * i + a] = y[a];
      }
    const double alpha = rz / pgo_dot(p, q, n6, s_w);
    for (int k = tid; k < n6; k += QTR_PGO_THREADS) {
      x[k] = x[k] + alpha * p[k];
      r[k] = r[k] - alpha * q[k];
    }
    rr = pgo_dot(r, r, n6, s_w);
    its += 1;
    if (!(rr > limit)) break;
    for (int i = tid; i < N; i += QTR_PGO_THREADS)
      if (!v.fixed[i]) {
        double zi[6];
        qtr_pgo_precond(D + (size_t)21 * i, lambda, r + (size_t)6 * i, zi);
        for (int a = 0; a < 6; ++a) z[(size_t)6 * i + a] = zi[a];
      }
    const double rzn = pgo_dot(r, z, n6, s_w);
    const double beta = rzn / rz;
    rz = rzn;
    for (int k = tid; k < n6; k += QTR_PGO_THREADS) p[k] = z[k] + beta * p[k];
  }
  __syncthreads();
  double ms = 0.0;
  for (int k = tid; k < n6; k += QTR_PGO_THREADS) {
    q[k] = v.fixed[k / 6] ? 0.0 : lambda * x[k] - g[k];  // (u)
    const double ax = x[k] < 0 ? -x[k] : x[k];
    ms = ax > ms ? ax : ms;
  }
  const double denom = pgo_dot(x, q, n6, s_w);
  for (int off = 32; off >= 1; off >>= 1) {
    const double o = icp_shfl_down(ms, off);
    ms = o > ms ? o : ms;
  }
  if ((tid & 63) == 0) s_m[tid >> 6] = ms;
  const double* Xc = v.X[cur];
  double* Xn = v.X[1 - cur];
  for (int i = tid; i < N; i += QTR_PGO_THREADS) {
    double T[16];
    if (v.fixed[i]) {
      for (int k = 0; k < 16; ++k) T[k] = Xc[(size_t)16 * i + k];
    } else {
      double xi[6];
      for (int a = 0; a < 6; ++a) xi[a] = x[(size_t)6 * i + a];
      qtr_pgo_update_node(Xc + (size_t)16 * i, xi, T);
    }
    for (int k = 0; k < 16; ++k) Xn[(size_t)16 * i + k] = T[k];
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 0; w < QTR_PGO_THREADS / 64; ++w) ms = s_m[w] > ms ? s_m[w] : ms;
    QtrPgoState s = *v.st;
    qtr_pgo_after_solve(&v.cfg, &s, its, denom, ms);
    *v.st = s;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------
// The slot's optimisation arena: allocated on the first call, grown on demand with a quarter of headroom (a call returns
// only after its chain has completed, so nothing is in flight when it grows), freed with the handle.
struct PgoBufs {
  void* arena = nullptr;
  size_t arena_bytes = 0;
  QtrPgoState* pin = nullptr;    // pinned: [0] the initial state, [1] the status record read once per iteration
  const double* last_trace = nullptr;  // QTR_DBG_PGO_TRACE: the rows of the last call
  int last_rows = 0;
};

static size_t pgo_up(size_t n) { return (n + 255) & ~(size_t)255; }

static size_t pgo_arena_bytes(int N, int E, int max_iterations) {
  const size_t n = (size_t)N, e = (size_t)E;
  return pgo_up(n) + pgo_up(e) + 2 * pgo_up(e * 4) + pgo_up((n + 1) * 4) + pgo_up(2 * e * 4) + pgo_up(e * 128) + pgo_up(e * 288) +
         2 * pgo_up(n * 128) + 2 * pgo_up(e * 168) + 2 * pgo_up(e * 8) + pgo_up(e * 48) + 2 * pgo_up(n * 168) + 2 * pgo_up(n * 48) +
         5 * pgo_up(n * 48) + pgo_up((size_t)qtr_div_up(E, 256) * 8) + pgo_up(64) + pgo_up(sizeof(QtrPgoState)) +
         pgo_up(((size_t)max_iterations + 1) * QTR_PGO_TRACE * 8);
}

static hipError_t pgo_reserve(PgoBufs& P, size_t need) {
  if (!P.pin) {
    hipError_t e = hipHostMalloc((void**)&P.pin, 2 * sizeof(QtrPgoState));
    if (e != hipSuccess) return e;
  }
  if (P.arena && P.arena_bytes >= need) return hipSuccess;
  if (P.arena) (void)hipFree(P.arena);
  P.arena = nullptr;
  P.arena_bytes = 0;
  P.last_trace = nullptr;
  P.last_rows = 0;
  const size_t bytes = need + need / 4;
  hipError_t e = hipMalloc(&P.arena, bytes);
  if (e != hipSuccess) return e;
  P.arena_bytes = bytes;
  return hipSuccess;
}

static void pgo_free(PgoBufs& P) {
  if (P.arena) (void)hipFree(P.arena);
  if (P.pin) (void)hipHostFree(P.pin);
  P = PgoBufs{};
}

// the view of one call carved out of the arena (the order of pgo_arena_bytes)
static void pgo_carve(PgoBufs& P, int N, int E, int max_iterations, PgoView& v) {
  char* p = (char*)P.arena;
  auto take = [&](size_t n) {
    char* r = p;
    p += pgo_up(n);
    return r;
  };
  const size_t n = (size_t)N, e = (size_t)E;
  v.N = N;
  v.E = E;
  v.fixed = (const unsigned char*)take(n);
  v.unc = (const unsigned char*)take(e);
  v.src = (const int*)take(e * 4);
  v.dst = (const int*)take(e * 4);
  v.off = (const int*)take((n + 1) * 4);
  v.inc = (const int*)take(2 * e * 4);
  v.Z = (const double*)take(e * 128);
  v.info = (const double*)take(e * 288);
  for (int k = 0; k < 2; ++k) v.X[k] = (double*)take(n * 128);
  for (int k = 0; k < 2; ++k) v.EA[k] = (double*)take(e * 168);
  for (int k = 0; k < 2; ++k) v.Ew[k] = (double*)take(e * 8);
  v.Eg = (double*)take(e * 48);
  for (int k = 0; k < 2; ++k) v.ND[k] = (double*)take(n * 168);
  for (int k = 0; k < 2; ++k) v.Ng[k] = (double*)take(n * 48);
  v.vx = (double*)take(n * 48);
  v.vr = (double*)take(n * 48);
  v.vz = (double*)take(n * 48);
  v.vp = (double*)take(n * 48);
  v.vq = (double*)take(n * 48);
  v.partials = (double*)take((size_t)qtr_div_up(E, 256) * 8);
  v.ticket = (unsigned*)take(64);
  v.st = (QtrPgoState*)take(sizeof(QtrPgoState));
  v.trace = (double*)take(((size_t)max_iterations + 1) * QTR_PGO_TRACE * 8);
}
