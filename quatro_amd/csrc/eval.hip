// eval.hip — evaluation of a registration on the device (qtr_evaluate / _pair / _keyframes / _keyframes_batch): how much of
// the source lies on the target under T (overlap, inlier RMSE), the 6x6 information matrix of the pose-graph edge and the
// point-to-plane Hessian at T.  The arithmetic is include/qtr_eval_math.h.
//
// Per evaluation: the ICP's cell grid over the finite target points (k_icp_bbox / k_icp_count / scan / k_icp_place of
// icp.hip, built into the slot's EVALUATION arena: the ICP arena and its state are not touched), then ONE launch of k_eval,
// one workgroup per 256 source points.  Every thread transforms its point, runs the ICP's search (icp_nearest) and forms
// its QTR_EVAL_NT terms; the workgroup folds them in the ICP's shape into one partial; the last workgroup to finish (atomic
// ticket, as in d_icp_iter: nobody waits for anybody, no co-residency is assumed) adds the partials in chunk order, runs
// qtr_eval_finish and writes the record.  An evaluation is described by an IcpView (st->T carries the transform, cfg.max_d2
// the reach, `partials` is [nchunk][QTR_EVAL_NT], `trace` points at the QtrEvalRecord).
//
// The batch (qtr_evaluate_keyframes_batch) is the same chain in grouped form, blockIdx.y = pair, every pair with a grid of
// its own in the arena; a pair runs d_eval with its own chunk count, so its record is the single call's bit for bit.
#include "common.h"
#include "../../include/qtr_eval_math.h"

#define QTR_EVAL_MAX_BATCH 64
// cells per evaluation: a larger grid takes larger cells (icp_grid_of; the result does not depend on the grid's shape)
#define QTR_EVAL_CELLS (1 << 20)

__device__ __forceinline__ void d_eval(const IcpView& v, int blk, int nblk) {
  __shared__ double s_w[4][QTR_EVAL_NT];
  __shared__ double s_S[QTR_EVAL_NT];
  __shared__ int s_last;
  double T[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) T[k] = v.st->T[k];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = blk * QTR_ICP_CHUNK + tid;
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
  // fixed-shape sum: the shfl_down fold inside each wave (qtr_icp_fold64), then (w0 + w1) + (w2 + w3)
#pragma unroll
  for (int k = 0; k < QTR_EVAL_NT; ++k) {
    double x = e[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = x + icp_shfl_down(x, off);
    if (lane == 0) s_w[wave][k] = x;
  }
  __syncthreads();
  if (tid < QTR_EVAL_NT) {
    const double w4[4] = {s_w[0][tid], s_w[1][tid], s_w[2][tid], s_w[3][tid]};
    const double c = qtr_icp_chunk_sum(w4);
    __hip_atomic_store((unsigned long long*)(v.partials + (size_t)blk * QTR_EVAL_NT + tid),
                       (unsigned long long)__double_as_longlong(c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __threadfence();
  __syncthreads();
  if (tid == 0) {
    const unsigned done = __hip_atomic_fetch_add(v.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    s_last = (done == (unsigned)nblk - 1) ? 1 : 0;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  if (tid < QTR_EVAL_NT) {
    double acc = __longlong_as_double((long long)__hip_atomic_load((unsigned long long*)(v.partials + tid), __ATOMIC_RELAXED,
                                                                   __HIP_MEMORY_SCOPE_AGENT));
    for (int c = 1; c < nblk; ++c)
      acc = acc + __longlong_as_double((long long)__hip_atomic_load(
                      (unsigned long long*)(v.partials + (size_t)c * QTR_EVAL_NT + tid), __ATOMIC_RELAXED,
                      __HIP_MEMORY_SCOPE_AGENT));
    s_S[tid] = acc;
  }
  __syncthreads();
  if (tid == 0) {
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

// k_icp_bbox per pair, folded in LDS first.  (k_icp_bbox_group mails every box into its slot's mailbox; a batch of
// evaluations lives on ONE slot, so its boxes stay in the arena and travel in one copy.)
__global__ __launch_bounds__(256) void k_eval_bbox_group(ViewExt<IcpView> x) {
  const IcpView& v = x.ext[blockIdx.y];  // (inline on purpose: see ViewExt)
  __shared__ int s_bb[6];
  if ((int)blockIdx.x * 256 >= v.nt) return;
  if (threadIdx.x < 6) s_bb[threadIdx.x] = threadIdx.x < 3 ? 0x7fffffff : (int)0x80000000;
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < v.nt) {
    const float4 p = v.tgt[i];
    if (qtr_icp_finite3(p.x, p.y, p.z)) {
      atomicMin(s_bb + 0, icp_enc(p.x));
      atomicMin(s_bb + 1, icp_enc(p.y));
      atomicMin(s_bb + 2, icp_enc(p.z));
      atomicMax(s_bb + 3, icp_enc(p.x));
      atomicMax(s_bb + 4, icp_enc(p.y));
      atomicMax(s_bb + 5, icp_enc(p.z));
    }
  }
  __syncthreads();
  if (threadIdx.x < 3) atomicMin(v.bbox + threadIdx.x, s_bb[threadIdx.x]);
  else if (threadIdx.x < 6) atomicMax(v.bbox + threadIdx.x, s_bb[threadIdx.x]);
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

static size_t eval_up(size_t n) { return (n + 255) & ~(size_t)255; }
static size_t eval_fixed_bytes() {
  return eval_up((sizeof(IcpView) + sizeof(QtrIcpState)) * QTR_EVAL_MAX_BATCH) + eval_up(sizeof(QtrIcpState) * QTR_EVAL_MAX_BATCH) +
         eval_up(32 * QTR_EVAL_MAX_BATCH) + eval_up(64 * QTR_EVAL_MAX_BATCH) + eval_up(sizeof(QtrEvalRecord) * QTR_EVAL_MAX_BATCH);
}

static hipError_t eval_reserve(EvalBufs& E, size_t var_bytes) {
  if (!E.pin) {
    const size_t pb = eval_up((sizeof(IcpView) + sizeof(QtrIcpState)) * QTR_EVAL_MAX_BATCH) + eval_up(32 * QTR_EVAL_MAX_BATCH) +
                      eval_up(sizeof(QtrEvalRecord) * QTR_EVAL_MAX_BATCH);
    hipError_t e = hipHostMalloc((void**)&E.pin, pb);
    if (e != hipSuccess) return e;
    char* p = E.pin;
    E.h_views = (IcpView*)p;
    E.h_init = (QtrIcpState*)(E.h_views + QTR_EVAL_MAX_BATCH);
    p += eval_up((sizeof(IcpView) + sizeof(QtrIcpState)) * QTR_EVAL_MAX_BATCH);
    E.h_boxes = (int*)p;
    p += eval_up(32 * QTR_EVAL_MAX_BATCH);
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
  p += eval_up((sizeof(IcpView) + sizeof(QtrIcpState)) * QTR_EVAL_MAX_BATCH);
  E.d_state = (QtrIcpState*)p;
  p += eval_up(sizeof(QtrIcpState) * QTR_EVAL_MAX_BATCH);
  E.d_boxes = (int*)p;
  p += eval_up(32 * QTR_EVAL_MAX_BATCH);
  E.d_tickets = (unsigned*)p;
  p += eval_up(64 * QTR_EVAL_MAX_BATCH);
  E.d_rec = (QtrEvalRecord*)p;
  p += eval_up(sizeof(QtrEvalRecord) * QTR_EVAL_MAX_BATCH);
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
