// eval.hip — evaluation of a registration on the device (qtr_evaluate / _pair / _keyframes / _keyframes_batch): how much of
// the source lies on the target under T (overlap, inlier RMSE), the 6x6 information matrix of the pose-graph edge and the
// point-to-plane Hessian at T.  The arithmetic is include/qtr_eval_math.h.
//
// Per evaluation: the ICP's cell grid over the finite target points (icp_box_enqueue / icp_grid_enqueue of icp.hip: k_icp_bbox,
// k_icp_count, scan, k_icp_place, k_icp_init; built into the slot's EVALUATION arena: the ICP arena and its state are not
// touched), then ONE launch of k_eval, one workgroup per 256 source points.  Every thread transforms its point, runs the
// ICP's search (icp_nearest) and forms its QTR_EVAL_NT terms; the workgroup folds them in the ICP's shape into one partial;
// the last workgroup to finish (atomic ticket: icp_reduce_tail, d_icp_iter's; nobody waits for anybody, no co-residency is
// assumed) adds the partials in chunk order, runs qtr_eval_finish and writes the record.  An evaluation is described by an
// IcpView (st->T carries the transform, cfg.max_d2 the reach, `partials` is [nchunk][QTR_EVAL_NT], `trace` points at the
// QtrEvalRecord).
//
// The batch (qtr_evaluate_keyframes_batch) is the same chain in grouped form, blockIdx.y = pair, every pair with a grid of
// its own in the arena; a pair runs d_eval with its own chunk count, so its record is the single call's bit for bit.
#include "common.h"
#include "../../include/qtr_eval_math.h"

#define QTR_EVAL_MAX_BATCH 64
// cells per evaluation: a larger grid takes larger cells (icp_grid_of; the result does not depend on the grid's shape)
#define QTR_EVAL_CELLS (1 << 20)

__device__ __forceinline__ void d_eval(const IcpView& v, int blk, int nblk) {
  __shared__ double s_S[QTR_EVAL_NT];
  double T[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) T[k] = v.st->T[k];
  const int i = blk * QTR_ICP_CHUNK + threadIdx.x;
  double e[QTR_EVAL_NT];
#pragma unroll
  for (int k = 0; k < QTR_EVAL_NT; ++k) e[k] = 0.0;
  if (i < v.ns) {
    const float4 p = v.src[i];
    int best = -1, bat = -1;
    double bd = 0.0, q[3];
    if (qtr_icp_finite3(p.x, p.y, p.z)) {
      qtr_icp_transform(T, p.x, p.y, p.z, q);
      if (v.ncell > 0) icp_nearest(v, q, best, bat, bd);
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f), n = t;
      int plane = 0;
      if (best >= 0) {
        t = v.spts[bat];
        if (v.nrm) {
          n = v.snrm[bat];
          plane = qtr_icp_finite3(n.x, n.y, n.z) ? 1 : 0;
        }
      }
      qtr_eval_terms(q, best >= 0 ? 1 : 0, t.x, t.y, t.z, plane, n.x, n.y, n.z, bd, e);
    }
    v.corr[i] = best;
  }
  if (!icp_reduce_tail<QTR_EVAL_NT, QTR_EVAL_NT>(e, v.partials, v.ticket, blk, nblk, s_S)) return;
  if (threadIdx.x == 0) {
    qtr_eval_finish(s_S, (QtrEvalRecord*)v.trace);
    __hip_atomic_store(v.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(256) void k_eval(IcpView v) { d_eval(v, (int)blockIdx.x, (int)gridDim.x); }

__global__ __launch_bounds__(256) void k_eval_group(ViewExt<IcpView> x) {
  const IcpView& v = x.ext[blockIdx.y];  // (inline on purpose: see ViewExt)
  const int nblk = (v.ns + QTR_ICP_CHUNK - 1) / QTR_ICP_CHUNK;
  if ((int)blockIdx.x >= nblk) return;  // (before the ticket)
  d_eval(v, (int)blockIdx.x, nblk);
}

// d_icp_bbox_fold per pair and nothing else.  (k_icp_bbox_group mails every box into its slot's mailbox; a batch of
// evaluations lives on ONE slot, so its boxes stay in the arena and travel in one copy.)
__global__ __launch_bounds__(256) void k_eval_bbox_group(ViewExt<IcpView> x) {
  const IcpView& v = x.ext[blockIdx.y];  // (inline on purpose: see ViewExt)
  if ((int)blockIdx.x * 256 >= v.nt) return;
  d_icp_bbox_fold(v);
}

// ---- host side ----------------------------------------------------------------------------------------------------
// The slot's evaluation arena: allocated on the first evaluation, grown on demand (a call returns only after its chain has
// completed, so nothing is in flight when it grows), freed with the handle.
struct EvalBufs {
  void* arena = nullptr;
  size_t arena_bytes = 0;
  int* cells = nullptr;       // the pairs' counters and starts, one after the other
  size_t cell_ints = 0;
  char* pin = nullptr;        // pinned: views, initial states, boxes, records of QTR_EVAL_MAX_BATCH pairs
  IcpView* h_views = nullptr;
  QtrIcpState* h_init = nullptr;
  int* h_boxes = nullptr;     // [B][8]
  QtrEvalRecord* h_rec = nullptr;
  // fixed part of the arena
  IcpView* d_views = nullptr;
  QtrIcpState* d_init = nullptr;   // directly behind d_views: one upload
  QtrIcpState* d_state = nullptr;
  int* d_boxes = nullptr;
  unsigned* d_tickets = nullptr;   // 16 words apart
  QtrEvalRecord* d_rec = nullptr;
  char* d_var = nullptr;           // per-call part
  const int* last_corr = nullptr;  // QTR_DBG_EVAL_CORR: the first pair of the last call
  int last_ns = 0;
};

static size_t eval_fixed_bytes() {
  return qtr_up256((sizeof(IcpView) + sizeof(QtrIcpState)) * QTR_EVAL_MAX_BATCH) + qtr_up256(sizeof(QtrIcpState) * QTR_EVAL_MAX_BATCH) +
         qtr_up256(32 * QTR_EVAL_MAX_BATCH) + qtr_up256(64 * QTR_EVAL_MAX_BATCH) + qtr_up256(sizeof(QtrEvalRecord) * QTR_EVAL_MAX_BATCH);
}

static hipError_t eval_reserve(EvalBufs& E, size_t var_bytes) {
  if (!E.pin) {
    const size_t pb = qtr_up256((sizeof(IcpView) + sizeof(QtrIcpState)) * QTR_EVAL_MAX_BATCH) + qtr_up256(32 * QTR_EVAL_MAX_BATCH) +
                      qtr_up256(sizeof(QtrEvalRecord) * QTR_EVAL_MAX_BATCH);
    hipError_t e = hipHostMalloc((void**)&E.pin, pb);
    if (e != hipSuccess) return e;
    char* p = E.pin;
    E.h_views = (IcpView*)p;
    E.h_init = (QtrIcpState*)(E.h_views + QTR_EVAL_MAX_BATCH);
    p += qtr_up256((sizeof(IcpView) + sizeof(QtrIcpState)) * QTR_EVAL_MAX_BATCH);
    E.h_boxes = (int*)p;
    p += qtr_up256(32 * QTR_EVAL_MAX_BATCH);
    E.h_rec = (QtrEvalRecord*)p;
  }
  const size_t need = eval_fixed_bytes() + var_bytes;
  if (E.arena && E.arena_bytes >= need) return hipSuccess;
  if (E.arena) (void)hipFree(E.arena);
  E.arena = nullptr;
  E.arena_bytes = 0;
  E.last_corr = nullptr;
  E.last_ns = 0;
  const size_t bytes = need + need / 4;  // (headroom: a batch a little larger than the last one does not allocate again)
  hipError_t e = hipMalloc(&E.arena, bytes);
  if (e != hipSuccess) return e;
  E.arena_bytes = bytes;
  char* p = (char*)E.arena;
  E.d_views = (IcpView*)p;
  E.d_init = (QtrIcpState*)(E.d_views + QTR_EVAL_MAX_BATCH);
  p += qtr_up256((sizeof(IcpView) + sizeof(QtrIcpState)) * QTR_EVAL_MAX_BATCH);
  E.d_state = (QtrIcpState*)p;
  p += qtr_up256(sizeof(QtrIcpState) * QTR_EVAL_MAX_BATCH);
  E.d_boxes = (int*)p;
  p += qtr_up256(32 * QTR_EVAL_MAX_BATCH);
  E.d_tickets = (unsigned*)p;
  p += qtr_up256(64 * QTR_EVAL_MAX_BATCH);
  E.d_rec = (QtrEvalRecord*)p;
  p += qtr_up256(sizeof(QtrEvalRecord) * QTR_EVAL_MAX_BATCH);
  E.d_var = p;
  return hipSuccess;
}

static hipError_t eval_reserve_cells(EvalBufs& E, size_t ints) {
  if (E.cells && E.cell_ints >= ints) return hipSuccess;
  if (E.cells) (void)hipFree(E.cells);
  E.cells = nullptr;
  E.cell_ints = 0;
  size_t cap = (size_t)1 << 17;
  while (cap < ints) cap <<= 1;
  hipError_t e = hipMalloc((void**)&E.cells, cap * 4);
  if (e != hipSuccess) return e;
  E.cell_ints = cap;
  return hipSuccess;
}

static void eval_free(EvalBufs& E) {
  if (E.arena) (void)hipFree(E.arena);
  if (E.cells) (void)hipFree(E.cells);
  if (E.pin) (void)hipHostFree(E.pin);
  E = EvalBufs{};
}

static void eval_result_from(qtr_eval_result* res, const QtrEvalRecord& r) {
  res->valid = r.valid;
  res->n_source = r.n_source;
  res->n_corr = r.n_corr;
  res->n_plane = r.n_plane;
  res->overlap = r.overlap;
  res->sum_d2 = r.sum_d2;
  res->inlier_rmse = r.inlier_rmse;
  res->plane_rmse = r.plane_rmse;
  memcpy(res->information, r.information, sizeof(r.information));
  memcpy(res->hessian_plane, r.hessian_plane, sizeof(r.hessian_plane));
}
