// voxelmap_eval.hip — poses evaluated against the voxel map without stepping them (qtr_voxel_map_evaluate / _keyframe /
// _batch / qtr_voxel_map_eval_fetch, include/quatro_voxelmap_eval.h).  The arithmetic is include/qtr_vmap_eval_math.h: the
// registration's match rule and terms at a fixed T, the voxel means' sums beside them, the registration's sum shape, and
// qtr_vmap_eval_finish.
//
// The entry points are exports of the extension library, libquatro_ext.so (voxelmap.hip says how it is built);
// libquatro_hip.so carries this code hidden and exports none of it.
//
// A call with B items (the single entries are B = 1):
//   (copies)            host-resident clouds into the slot's evaluation arena (one copy per distinct cloud); the B views, each
//                       with its pose, and the B zeroed tickets from pinned memory, one copy
//   k_vmap_eval_group   ONE launch, grid (chunks of the largest item, B): blockIdx.y is the item, its view read from device
//                       memory (ViewExt).  A workgroup past its item's last chunk returns before it touches the ticket; the
//                       others run d_vmap_eval: d_eval's frame (eval.hip) around d_vmap_iter's lookup (voxelmap.hip) — one
//                       point per thread, one d_vmap_find, one record load, its QTR_VMAP_EVAL_NT terms, icp_reduce_tail; the
//                       last workgroup of the item to arrive runs qtr_vmap_eval_finish, writes the record and clears the ticket.
//                       (k_vmap_eval is the same body on a view in the kernel arguments, grid chunks: what a single call runs.)
//   (copy)              the B records, one copy; an item with n == 0 has no workgroup and gets the empty record on the host
// Events around upload and launch feed QTR_VMAP_EVAL_TIMES.
//
// The arena is the slot's own (Slot::veval), never its IcpBufs, EvalBufs or batch arena.  Per item it holds one view (with
// T), a ticket on a line of its own, ceil(n / QTR_ICP_CHUNK) x QTR_VMAP_EVAL_NT partial sums, the record and, with per-point
// output, n ints and 2 n doubles; behind them lie the staged host clouds.  The arena itself, the item check, the staging and
// the fetch's tail are voxelmap_group.hip, shared with the grouped registration (voxelmap_batch.hip).
// The map is only read.  No kernel waits for another workgroup, none is launched cooperatively, all stores are plain vector
// stores.
#include "../../include/quatro_voxelmap_eval.h"
#include "../../include/qtr_vmap_eval_math.h"

struct VevalView {
  const float4* src;  // [ns] points
  const float4* nrm;  // [ns] their normals, scan frame
  int ns, pad;
  double T[16];       // the pose (rows 0 - 2 read)
  double* partials;   // [nchunk][QTR_VMAP_EVAL_NT]
  unsigned* ticket;   // workgroups of this item done (reset by the last one)
  QtrVmapEvalRecord* rec;
  int* corr;          // [ns] or null: no per-point output
  double* point;      // [ns][2] with corr
};

// One workgroup (chunk `blk` of `nblk`) of one evaluation.
__device__ __forceinline__ void d_vmap_eval(const VevalView& v, const VmapView& m, int blk, int nblk) {
  __shared__ double s_S[QTR_VMAP_EVAL_NT];
  double T[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) T[k] = v.T[k];
  const int i = blk * QTR_ICP_CHUNK + threadIdx.x;
  double e[QTR_VMAP_EVAL_NT];
#pragma unroll
  for (int k = 0; k < QTR_VMAP_EVAL_NT; ++k) e[k] = 0.0;
  if (i < v.ns) {
    const float4 p = v.src[i];
    const float4 a = v.nrm[i];
    int best = -1;
    if (qtr_icp_finite3(p.x, p.y, p.z)) {
      double q[3] = {0.0, 0.0, 0.0};
      u64 key = 0;
      QtrIcpVoxel vx;
      if (qtr_vmap_query(T, p.x, p.y, p.z, a.x, a.y, a.z, m.side, q, &key)) {
        const long long s = d_vmap_find(m, key);
        if (s >= 0) {
          vx = m.rec[s];
          if (m.cnt[s] > 0 && vx.n > 0) best = 0;
        }
      }
      qtr_vmap_eval_terms(T, q, a.x, a.y, a.z, best == 0 ? &vx : nullptr, e);
    }
    if (v.corr) {
      v.corr[i] = best;
      v.point[2 * (size_t)i] = e[QTR_ICP_T_R2];
      v.point[2 * (size_t)i + 1] = e[QTR_ICP_T_W];
    }
  }
  if (!icp_reduce_tail<QTR_VMAP_EVAL_NT, QTR_VMAP_EVAL_NT>(e, v.partials, v.ticket, blk, nblk, s_S)) return;
  if (threadIdx.x == 0) {
    qtr_vmap_eval_finish(s_S, v.rec);
    __hip_atomic_store(v.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(256) void k_vmap_eval(VevalView v, VmapView m) { d_vmap_eval(v, m, (int)blockIdx.x, (int)gridDim.x); }

__global__ __launch_bounds__(256) void k_vmap_eval_group(ViewExt<VevalView> x, VmapView m) {
  const VevalView& v = x.ext[blockIdx.y];  // (inline on purpose: see ViewExt)
  const int nblk = (v.ns + QTR_ICP_CHUNK - 1) / QTR_ICP_CHUNK;
  if ((int)blockIdx.x >= nblk) return;  // (before the ticket)
  d_vmap_eval(v, m, (int)blockIdx.x, nblk);
}

// ---- host side ----------------------------------------------------------------------------------------------------
// the slot's arena (voxelmap_group.hip) and what qtr_voxel_map_eval_fetch serves of its last evaluation; pinned:
// QTR_VMAP_EVAL_MAX views with their tickets' zeros behind them, then the records' read-back
struct VmapEval : VmapArena {
  int per_point = 0;
  int n[QTR_VMAP_BATCH_MAX] = {};
  const int* corr[QTR_VMAP_BATCH_MAX] = {};
  const double* point[QTR_VMAP_BATCH_MAX] = {};
  float ms = 0.f;
};

static const size_t kVePinBack = qtr_up256(QTR_VMAP_EVAL_MAX * sizeof(VevalView)) + qtr_up256((size_t)QTR_VMAP_EVAL_MAX * 64);
static const size_t kVePinBytes = kVePinBack + qtr_up256(QTR_VMAP_EVAL_MAX * sizeof(QtrVmapEvalRecord));

static void vmap_eval_free(Slot& s) { vmap_arena_free(s.veval); }

struct VeItem : VmapGroupItem {
  size_t o_partials = 0, o_corr = 0, o_point = 0;  // offsets into the arena
};

static void vmap_eval_result_from(qtr_vmap_eval_result* res, const QtrVmapEvalRecord& r) {
  res->status = QTR_OK;
  res->valid = r.valid;
  res->n_source = r.n_source;
  res->n_corr = r.n_corr;
  res->overlap = r.overlap;
  res->sum_d2 = r.sum_d2;
  res->inlier_rmse = r.inlier_rmse;
  res->sum_w = r.sum_w;
  res->chi2 = r.chi2;
  res->rmse = r.rmse;
  memcpy(res->information, r.information, sizeof(r.information));
  memcpy(res->hessian, r.hessian, sizeof(r.hessian));
  memcpy(res->gradient, r.gradient, sizeof(r.gradient));
}

static int vmap_eval_run(qtr_handle* h, Slot& s, const qtr_voxel_map* m, const qtr_vmap_reg_item* items, int B, bool per_point,
                         VeItem* it, qtr_vmap_eval_result* results) {
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  QTR_TRY(vmap_arena_open(h, s.veval, kVePinBytes, 2));
  VmapEval& ve = *s.veval;
  const hipStream_t st = s.stream;

  // the arena's layout for this call: the views and, directly behind them, the tickets (one upload), the records, every
  // item's own arrays, then the staged clouds
  VmapCursor cur;
  const size_t o_views = cur.take((size_t)B * sizeof(VevalView));
  const size_t o_ticket = cur.take((size_t)B * 64);
  const size_t head_bytes = o_ticket + (size_t)B * 64;
  const size_t o_rec = cur.take((size_t)B * sizeof(QtrVmapEvalRecord));
  int max_chunks = 0;
  for (int i = 0; i < B; ++i) {
    const int nchunk = qtr_div_up(it[i].n, QTR_ICP_CHUNK);
    max_chunks = std::max(max_chunks, nchunk);
    it[i].o_partials = cur.take((size_t)nchunk * QTR_VMAP_EVAL_NT * 8);
    if (per_point) {
      it[i].o_corr = cur.take((size_t)it[i].n * 4);
      it[i].o_point = cur.take((size_t)it[i].n * 16);
    }
  }
  vmap_group_plan(it, B, cur);
  QTR_TRY(vmap_arena_grow(h, ve, cur.need, st));
  char* const dev = (char*)ve.dev;
  VevalView* const hv = (VevalView*)ve.pin;
  QtrVmapEvalRecord* const hrec = (QtrVmapEvalRecord*)(ve.pin + kVePinBack);
  QtrVmapEvalRecord* const drec = (QtrVmapEvalRecord*)(dev + o_rec);

  QTR_HIP_TRY(h, hipEventRecord(ve.ev[0], st));
  QTR_TRY(vmap_group_upload(h, dev, it, B, st));
  for (int i = 0; i < B; ++i) {
    VevalView v{};
    v.src = (const float4*)it[i].src;
    v.nrm = (const float4*)it[i].nrm;
    v.ns = it[i].n;
    vmap_guess(items[i].guess, v.T);
    v.partials = (double*)(dev + it[i].o_partials);
    v.ticket = (unsigned*)(dev + o_ticket + (size_t)i * 64);
    v.rec = drec + i;
    v.corr = per_point ? (int*)(dev + it[i].o_corr) : nullptr;
    v.point = per_point ? (double*)(dev + it[i].o_point) : nullptr;
    hv[i] = v;
  }
  memset(ve.pin + o_ticket, 0, (size_t)B * 64);  // (the tickets travel with the views: no launch of their own)
  QTR_HIP_TRY(h, hipMemcpyAsync(dev + o_views, ve.pin, head_bytes, hipMemcpyHostToDevice, st));
  if (max_chunks > 0) {
    if (B == 1) {
      hipLaunchKernelGGL(k_vmap_eval, dim3(max_chunks), dim3(256), 0, st, hv[0], m->v);
    } else {
      const ViewExt<VevalView> x{(const VevalView*)(dev + o_views), {0, 0, 0}};
      hipLaunchKernelGGL(k_vmap_eval_group, dim3(max_chunks, B), dim3(256), 0, st, x, m->v);
    }
    QTR_HIP_TRY(h, hipGetLastError());
  }
  QTR_HIP_TRY(h, hipEventRecord(ve.ev[1], st));
  if (max_chunks > 0)
    QTR_HIP_TRY(h, hipMemcpyAsync(hrec, drec, (size_t)B * sizeof(QtrVmapEvalRecord), hipMemcpyDeviceToHost, st));
  QTR_HIP_TRY(h, hipStreamSynchronize(st));
  for (int i = 0; i < B; ++i) {
    memset(results + i, 0, sizeof(*results));
    if (it[i].n == 0) {  // (no workgroup ran: the record of the zero sums)
      const double S[QTR_VMAP_EVAL_NT] = {};
      QtrVmapEvalRecord r;
      qtr_vmap_eval_finish(S, &r);
      vmap_eval_result_from(results + i, r);
    } else {
      vmap_eval_result_from(results + i, hrec[i]);
    }
    if (per_point) {
      ve.n[i] = it[i].n;
      ve.corr[i] = (const int*)(dev + it[i].o_corr);
      ve.point[i] = (const double*)(dev + it[i].o_point);
    }
  }
  ve.ms = 0.f;
  float ms = 0;
  if (hipEventElapsedTime(&ms, ve.ev[0], ve.ev[1]) == hipSuccess) ve.ms = ms;
  ve.per_point = per_point ? 1 : 0;
  ve.B = B;
  return QTR_OK;
}

void qtr_default_vmap_eval_params(qtr_vmap_eval_params* prm) {
  if (!prm) return;
  memset(prm, 0, sizeof(*prm));
}

int qtr_voxel_map_evaluate_batch(qtr_handle* h, int slot, const qtr_voxel_map* m, const qtr_vmap_reg_item* items, int B,
                                 const qtr_vmap_eval_params* prm, qtr_vmap_eval_result* results) {
  Slot* sp = peek_slot(h, slot);  // (nothing of the slot's own clouds, ICP, evaluation or batch state is written)
  if (!sp) return QTR_ERR_BAD_ARG;
  if (B == 0) return QTR_OK;
  if (results && B > 0)
    for (int i = 0; i < B; ++i) {
      memset(results + i, 0, sizeof(*results));
      results[i].status = QTR_ERR_NOT_RUN;
    }
  if (!items || !results || !prm) {
    snprintf(h->err, sizeof(h->err), "voxel map evaluate: %s is NULL", !items ? "items" : !results ? "results" : "prm");
    return QTR_ERR_BAD_ARG;
  }
  const int lim = prm->per_point ? QTR_VMAP_BATCH_MAX : QTR_VMAP_EVAL_MAX;
  if (B < 0 || B > lim) {
    snprintf(h->err, sizeof(h->err), "voxel map evaluate: B=%d (0 .. %d%s)", B, lim, prm->per_point ? " with per-point output" : "");
    return QTR_ERR_BAD_ARG;
  }
  std::vector<VeItem> it((size_t)B);
  QTR_TRY(vmap_check(h, m));
  QTR_TRY(vmap_group_check(h, "evaluate", "pose", "evaluate item", items, B, it.data()));
  return vmap_eval_run(h, *sp, m, items, B, prm->per_point != 0, it.data(), results);
}

int qtr_voxel_map_evaluate(qtr_handle* h, int slot, const qtr_voxel_map* m, const float* src4, const float* src_normals4, int n,
                           int mem, const double T[16], const qtr_vmap_eval_params* prm, qtr_vmap_eval_result* res) {
  if (!peek_slot(h, slot)) return QTR_ERR_BAD_ARG;
  if (res) {
    memset(res, 0, sizeof(*res));
    res->status = QTR_ERR_NOT_RUN;
  }
  if (!T || !res) {
    snprintf(h->err, sizeof(h->err), "voxel map evaluate: %s is NULL", !T ? "T" : "result");
    return QTR_ERR_BAD_ARG;
  }
  qtr_vmap_reg_item a{};
  a.src4 = src4;
  a.src_normals4 = src_normals4;
  a.n = n;
  a.mem = mem;
  memcpy(a.guess, T, sizeof(a.guess));
  return qtr_voxel_map_evaluate_batch(h, slot, m, &a, 1, prm, res);
}

int qtr_voxel_map_evaluate_keyframe(qtr_handle* h, int slot, const qtr_voxel_map* m, const qtr_keyframe* kf, const double T[16],
                                    const qtr_vmap_eval_params* prm, qtr_vmap_eval_result* res) {
  if (!peek_slot(h, slot)) return QTR_ERR_BAD_ARG;
  if (res) {
    memset(res, 0, sizeof(*res));
    res->status = QTR_ERR_NOT_RUN;
  }
  if (!T || !res) {
    snprintf(h->err, sizeof(h->err), "voxel map evaluate: %s is NULL", !T ? "T" : "result");
    return QTR_ERR_BAD_ARG;
  }
  if (!kf) {
    snprintf(h->err, sizeof(h->err), "keyframe is NULL");
    return QTR_ERR_BAD_ARG;
  }
  qtr_vmap_reg_item a{};
  a.kf = kf;
  memcpy(a.guess, T, sizeof(a.guess));
  return qtr_voxel_map_evaluate_batch(h, slot, m, &a, 1, prm, res);
}

long long qtr_voxel_map_eval_fetch(qtr_handle* h, int slot, int item, int what, void* dst, size_t bytes) {
  Slot* sp = peek_slot(h, slot);
  if (!sp || !sp->veval || sp->veval->B < 0) return -1;
  const VmapEval& ve = *sp->veval;
  if (what == QTR_VMAP_EVAL_TIMES) {
    const size_t n = sizeof(ve.ms) < bytes ? sizeof(ve.ms) : bytes;
    if (dst && n > 0) memcpy(dst, &ve.ms, n);
    return (long long)sizeof(ve.ms);
  }
  if (item < 0 || item >= ve.B || !ve.per_point) return -1;
  const void* src = nullptr;
  size_t have = 0;
  switch (what) {
    case QTR_VMAP_EVAL_CORR: src = ve.corr[item]; have = (size_t)ve.n[item] * 4; break;
    case QTR_VMAP_EVAL_POINT: src = ve.point[item]; have = (size_t)ve.n[item] * 16; break;
    default: return -1;
  }
  return vmap_group_fetch(h, *sp, src, have, dst, bytes);
}
