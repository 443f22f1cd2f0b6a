// voxelmap_batch.hip — a batch of scans and guesses registered against one voxel map in one chain of launches
// (qtr_voxel_map_register_batch / qtr_voxel_map_batch_fetch, include/quatro_voxelmap_batch.h).  The contract is
// include/qtr_vmap_batch_math.h: item i IS qtr_voxel_map_register with its cloud and guess, bit for bit.
//
// The two entry points are exports of the extension library, libquatro_ext.so (voxelmap.hip says how it is built);
// libquatro_hip.so carries this code hidden and exports none of it.
//
// A call with B items:
//   (copies)            host-resident clouds into the slot's batch arena (one copy per distinct cloud), the B views and
//                       initial states from pinned memory, one copy
//   k_vmap_init_group   one small launch: every item's state = qtr_icp_init of its guess, every ticket = 0
//   k_vmap_iter_group   max_iterations launches, grid (chunks of the largest item, B): blockIdx.y is the item, its IcpView read
//                       from device memory (ViewExt), its own chunk count where k_vmap_iter has gridDim.x.  A workgroup past its
//                       item's last chunk returns before it reads the stop flag or touches the ticket; the others run
//                       d_vmap_iter (voxelmap.hip), the body k_vmap_iter runs, so partials, fold, ticket, step and trace row
//                       are the single call's.  An item that stopped stays frozen (icp_iter_begin).
//   (host)              with QTR_ICP_BLOCK = n the B states are read back after every n launches and the loop ends once all
//                       items have stopped, as icp_loop (capi.hip) does for one; then one final read-back of the B states.
// Events around the two phases feed QTR_VMAP_BATCH_TIMES.
//
// The arena is the slot's own (Slot::vbatch), never its IcpBufs: the slot's single-call ICP state and what qtr_debug_fetch
// serves for it stay as they were.  Per item it holds one IcpView, one QtrIcpState, a ticket on a line of its own, the partial
// sums (ceil(n / QTR_ICP_CHUNK) x QTR_ICP_NT doubles), the trace (max_iterations x 18 doubles) and corr (n ints); behind
// them lie the staged host clouds.  The arena itself, the item check, the staging and the fetch's tail are voxelmap_group.hip,
// shared with the evaluation (voxelmap_eval.hip).
// The map is only read.  No kernel waits for another workgroup, none is launched cooperatively, all stores are plain vector
// stores.
#include "../../include/quatro_voxelmap_batch.h"
#include "../../include/qtr_vmap_batch_math.h"

__global__ __launch_bounds__(64) void k_vmap_init_group(ViewExt<IcpView> x, const QtrIcpState* __restrict__ init, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const IcpView& v = x.ext[b];  // (inline on purpose: see ViewExt)
  *v.st = init[b];
  *v.ticket = 0u;
}

// one iteration of every item of the group: the item's chunk count stands where k_vmap_iter has gridDim.x
__global__ __launch_bounds__(256) void k_vmap_iter_group(ViewExt<IcpView> x, VmapView m) {
  const IcpView& v = x.ext[blockIdx.y];  // (inline on purpose: see ViewExt)
  const int nblk = (v.ns + QTR_ICP_CHUNK - 1) / QTR_ICP_CHUNK;
  if ((int)blockIdx.x >= nblk) return;  // (before the stop flag and the ticket)
  d_vmap_iter(v, m, (int)blockIdx.x, nblk);
}

// ---- host side ----------------------------------------------------------------------------------------------------
enum { VB_EV_BEGIN = 0, VB_EV_LOOP, VB_EV_END, VB_EV_COUNT };
static_assert(VB_EV_COUNT <= VG_EV_MAX, "the arena's events");

// the slot's arena (voxelmap_group.hip) and what qtr_voxel_map_batch_fetch serves of its last batch; pinned:
// QTR_VMAP_BATCH_MAX views, initial states and read-back states
struct VmapBatch : VmapArena {
  int n[QTR_VMAP_BATCH_MAX] = {}, iters[QTR_VMAP_BATCH_MAX] = {};
  const double* trace[QTR_VMAP_BATCH_MAX] = {};
  const int* corr[QTR_VMAP_BATCH_MAX] = {};
  float ms[2] = {0.f, 0.f};
};

// (pinned: the views and, behind them, the initial states of a call; then the read-back states)
static const size_t kVbPinBack = qtr_up256(QTR_VMAP_BATCH_MAX * sizeof(IcpView)) + qtr_up256(QTR_VMAP_BATCH_MAX * sizeof(QtrIcpState));
static const size_t kVbPinBytes = kVbPinBack + qtr_up256(QTR_VMAP_BATCH_MAX * sizeof(QtrIcpState));

static void vmap_batch_free(Slot& s) { vmap_arena_free(s.vbatch); }

struct VbItem : VmapGroupItem {
  size_t o_partials = 0, o_trace = 0, o_corr = 0;  // offsets into the arena
};

static int vmap_batch_check(qtr_handle* h, const qtr_voxel_map* m, const qtr_vmap_reg_item* items, int B, const qtr_icp_params* prm,
                            VbItem* it) {
  QTR_TRY(vmap_check(h, m));
  QTR_TRY(check_icp_params(h, prm));
  if (prm->method != QTR_ICP_VOXEL_PLANE_TO_PLANE) {
    snprintf(h->err, sizeof(h->err), "voxel map register batch: method must be QTR_ICP_VOXEL_PLANE_TO_PLANE");
    return QTR_ERR_BAD_ARG;
  }
  return vmap_group_check(h, "register", "guess", "batch item", items, B, it);
}

static int vmap_batch_run(qtr_handle* h, Slot& s, const qtr_voxel_map* m, const qtr_vmap_reg_item* items, int B,
                          const qtr_icp_params* prm, VbItem* it, qtr_icp_result* results) {
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  QTR_TRY(vmap_arena_open(h, s.vbatch, kVbPinBytes, VB_EV_COUNT));
  VmapBatch& vb = *s.vbatch;
  const hipStream_t st = s.stream;
  const int maxit = prm->max_iterations;

  // the arena's layout for this call: the head, every item's own sections, then the staged clouds
  VmapCursor cur;
  const size_t o_views = cur.take((size_t)B * sizeof(IcpView));
  const size_t o_init = cur.take((size_t)B * sizeof(QtrIcpState));
  const size_t o_state = cur.take((size_t)B * sizeof(QtrIcpState));
  const size_t o_ticket = cur.take((size_t)B * 64);
  const size_t head_bytes = o_init + (size_t)B * sizeof(QtrIcpState);  // views and initial states: one upload
  int max_chunks = 0;
  for (int i = 0; i < B; ++i) {
    const int nchunk = qtr_div_up(it[i].n, QTR_ICP_CHUNK);
    max_chunks = std::max(max_chunks, nchunk);
    it[i].o_partials = cur.take((size_t)nchunk * QTR_ICP_NT * 8);
    it[i].o_trace = cur.take((size_t)maxit * 18 * 8);
    it[i].o_corr = cur.take((size_t)it[i].n * 4);
  }
  vmap_group_plan(it, B, cur);
  QTR_TRY(vmap_arena_grow(h, vb, cur.need, st));
  char* const dev = (char*)vb.dev;
  // (the upload's layout is this call's: the initial states follow the B views as they do in the arena)
  IcpView* const hv = (IcpView*)vb.pin;
  QtrIcpState* const hinit = (QtrIcpState*)((char*)vb.pin + o_init);
  QtrIcpState* const hback = (QtrIcpState*)((char*)vb.pin + kVbPinBack);
  QtrIcpState* const dstate = (QtrIcpState*)(dev + o_state);

  QTR_HIP_TRY(h, hipEventRecord(vb.ev[VB_EV_BEGIN], st));
  QTR_TRY(vmap_group_upload(h, dev, it, B, st));
  for (int i = 0; i < B; ++i) {
    double g[16];
    vmap_guess(items[i].guess, g);
    qtr_icp_init(&hinit[i], g);
    IcpView v{};
    icp_view_bind(v, prm, (const float4*)it[i].src, it[i].n, (const float4*)it[i].nrm, nullptr, 0, nullptr);
    v.ncell = v.dims[0] = v.dims[1] = v.dims[2] = 0;
    v.cfg.max_d2 = m->v.side * m->v.side;  // (not read: the side is the map's)
    v.st = dstate + i;
    v.ticket = (unsigned*)(dev + o_ticket + (size_t)i * 64);
    v.partials = (double*)(dev + it[i].o_partials);
    v.trace = (double*)(dev + it[i].o_trace);
    v.corr = (int*)(dev + it[i].o_corr);
    hv[i] = v;
  }
  QTR_HIP_TRY(h, hipMemcpyAsync(dev + o_views, vb.pin, head_bytes, hipMemcpyHostToDevice, st));
  const ViewExt<IcpView> x{(const IcpView*)(dev + o_views), {0, 0, 0}};
  hipLaunchKernelGGL(k_vmap_init_group, dim3(qtr_div_up(B, 64)), dim3(64), 0, st, x, (const QtrIcpState*)(dev + o_init), B);
  QTR_HIP_TRY(h, hipGetLastError());
  QTR_HIP_TRY(h, hipEventRecord(vb.ev[VB_EV_LOOP], st));
  if (max_chunks > 0) {
    const int block = h->icp_block > 0 ? h->icp_block : maxit;
    const dim3 grid(max_chunks, B);
    for (int done = 0; done < maxit;) {
      const int k_n = std::min(block, maxit - done);
      for (int k = 0; k < k_n; ++k) hipLaunchKernelGGL(k_vmap_iter_group, grid, dim3(256), 0, st, x, m->v);
      QTR_HIP_TRY(h, hipGetLastError());
      done += k_n;
      if (done >= maxit) break;
      QTR_HIP_TRY(h, hipMemcpyAsync(hback, dstate, (size_t)B * sizeof(QtrIcpState), hipMemcpyDeviceToHost, st));
      QTR_HIP_TRY(h, hipStreamSynchronize(st));
      bool all = true;
      for (int i = 0; i < B; ++i) all = all && (it[i].n == 0 || hback[i].stop);
      if (all) break;
    }
  }
  QTR_HIP_TRY(h, hipEventRecord(vb.ev[VB_EV_END], st));
  QTR_HIP_TRY(h, hipMemcpyAsync(hback, dstate, (size_t)B * sizeof(QtrIcpState), hipMemcpyDeviceToHost, st));
  QTR_HIP_TRY(h, hipStreamSynchronize(st));
  for (int i = 0; i < B; ++i) {
    qtr_icp_result* res = results + i;
    memset(res, 0, sizeof(*res));
    if (it[i].n == 0) {  // (nothing to refine: what the single call reports)
      double g[16];
      vmap_guess(items[i].guess, g);
      icp_result_empty(res, g);
    } else {
      icp_result_from(res, hback[i]);
    }
    res->status = QTR_OK;
    vb.n[i] = it[i].n;
    vb.iters[i] = it[i].n == 0 ? 0 : hback[i].iterations;
    vb.trace[i] = (const double*)(dev + it[i].o_trace);
    vb.corr[i] = (const int*)(dev + it[i].o_corr);
  }
  vb.ms[0] = vb.ms[1] = 0.f;
  float ms = 0;
  if (hipEventElapsedTime(&ms, vb.ev[VB_EV_BEGIN], vb.ev[VB_EV_LOOP]) == hipSuccess) vb.ms[0] = ms;
  if (hipEventElapsedTime(&ms, vb.ev[VB_EV_LOOP], vb.ev[VB_EV_END]) == hipSuccess) vb.ms[1] = ms;
  vb.B = B;
  return QTR_OK;
}

int qtr_voxel_map_register_batch(qtr_handle* h, int slot, const qtr_voxel_map* m, const qtr_vmap_reg_item* items, int B,
                                 const qtr_icp_params* prm, qtr_icp_result* results) {
  Slot* sp = peek_slot(h, slot);  // (nothing of the slot's own clouds or ICP state is written)
  if (!sp) return QTR_ERR_BAD_ARG;
  if (B == 0) return QTR_OK;
  if (results)
    for (int i = 0; i < B; ++i) {
      memset(results + i, 0, sizeof(*results));
      results[i].status = QTR_ERR_NOT_RUN;
    }
  if (B < 0 || B > QTR_VMAP_BATCH_MAX) {
    snprintf(h->err, sizeof(h->err), "voxel map register batch: B=%d (0 .. %d)", B, QTR_VMAP_BATCH_MAX);
    return QTR_ERR_BAD_ARG;
  }
  if (!items || !results) {
    snprintf(h->err, sizeof(h->err), "voxel map register batch: %s is NULL", !items ? "items" : "results");
    return QTR_ERR_BAD_ARG;
  }
  VbItem it[QTR_VMAP_BATCH_MAX];
  QTR_TRY(vmap_batch_check(h, m, items, B, prm, it));
  return vmap_batch_run(h, *sp, m, items, B, prm, it, results);
}

long long qtr_voxel_map_batch_fetch(qtr_handle* h, int slot, int item, int what, void* dst, size_t bytes) {
  Slot* sp = peek_slot(h, slot);
  if (!sp || !sp->vbatch || sp->vbatch->B < 0) return -1;
  const VmapBatch& vb = *sp->vbatch;
  if (what == QTR_VMAP_BATCH_TIMES) {
    const size_t n = sizeof(vb.ms) < bytes ? sizeof(vb.ms) : bytes;
    if (dst && n > 0) memcpy(dst, vb.ms, n);
    return (long long)sizeof(vb.ms);
  }
  if (item < 0 || item >= vb.B) return -1;
  const void* src = nullptr;
  size_t have = 0;
  switch (what) {
    case QTR_VMAP_BATCH_TRACE: src = vb.trace[item]; have = (size_t)vb.iters[item] * 18 * 8; break;
    case QTR_VMAP_BATCH_CORR: src = vb.corr[item]; have = (size_t)vb.n[item] * 4; break;
    default: return -1;
  }
  return vmap_group_fetch(h, *sp, src, have, dst, bytes);
}
