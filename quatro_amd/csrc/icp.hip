// icp.hip — 6-DoF ICP refinement on the device (qtr_icp / qtr_gicp / qtr_refine_pair): point-to-plane (default),
// point-to-point, plane-to-plane (Generalized ICP; its iteration is an instantiation of its own, d_icp_iter<2>) and
// voxelised plane-to-plane (VGICP, d_icp_iter<3>: the target as one record per cell of side max_correspondence_distance,
// k_icp_voxel_order / k_icp_voxel_stats after the counting sort, and a lookup in place of the search).
//
// Per call: a uniform cell grid over the finite target points (cell side >= max_correspondence_distance, so the
// nearest target within reach of any query lies in its 27 neighbouring cells), built by a counting sort into the
// handle's own ICP arena (icp_box_enqueue: k_icp_bbox; icp_grid_of on the host; icp_grid_enqueue: k_icp_count,
// exclusive_scan_i32, k_icp_place, k_icp_init — the single evaluation of eval.hip runs the same two helpers).  The FPFH
// chain's cell table is not used: its cells are the FPFH radius over the RAW scan's box and its counters must stay zero
// between registrations; the ICP table has its own counters, cleared by the call that uses them.
//
// Per iteration: ONE launch of k_icp_iter (one workgroup per 256 source points).  Every thread transforms its point
// with the current T, finds the nearest target (binary64 d^2, ties to the lowest target index, so the order inside a
// cell does not matter) and forms its terms; the terms are summed in a fixed shape (include/qtr_icp_math.h) into one
// partial per workgroup; the LAST workgroup to finish (atomic ticket) adds the partials in workgroup order
// (icp_reduce_tail, which the evaluation shares), solves, updates T and decides whether to stop.  Nobody waits for
// anybody, so no co-residency is assumed.  A launch that finds the stop flag set returns at once, so the host can enqueue
// iterations without reading anything back.  The frame around the terms is icp_iter_begin / icp_iter_finish; d_icp_iter
// and the voxel map's k_vmap_iter (voxelmap.hip) state only where their terms come from.
//
// What a method reads (target normals, source normals, a voxel grid) is asked of three predicates on the host side below;
// icp_iter_launch picks the iteration kernel, icp_view_bind fills a view, icp_result_empty is the result of a pair with
// nothing to refine.  The single-call host loop is icp_loop (capi.hip).
//
// Batched refinement (qtr_submit_batch_refine): the same kernels in grouped form, blockIdx.y = pair of the lane's group,
// the per-pair IcpViews in device memory (ViewExt).  Every pair runs the per-pair body the single-pair kernel runs
// (d_icp_*), with its own chunk count in place of gridDim.x, so its arithmetic — partials, fold, ticket, solve — is the
// single-pair call's bit for bit.  Workgroups past a pair's own end return before they take a ticket.
#include "common.h"
#include "frontend.h"
#include "../../include/qtr_icp_math.h"

struct IcpView {
  const float4* src;      // [ns] source points (x, y, z, *)
  const float4* tgt;      // [nt] target points
  const float4* nrm;      // [nt] target normals (point-to-plane, plane-to-plane) or null
  int ns, nt;
  float4* spts;           // [nt] finite target points in cell order, w = original index
  float4* snrm;           // [nt] their normals in the same order
  int* cell_cnt;          // [ncell + 1] counters (zeroed by the call)
  int* cell_start;        // [ncell + 1] exclusive scan of cell_cnt
  int* place;             // [nt][2] cell and rank in the cell of every target point (-1: not finite)
  int* bbox;              // 6 order-preserving encodings: min x, y, z, max x, y, z
  double mn[3];           // grid origin and cell side (host-computed from bbox)
  double cell;
  int dims[3];
  int ncell;
  QtrIcpCfg cfg;
  QtrIcpState* st;        // device state
  double* partials;       // [nchunk][QTR_ICP_NT]
  unsigned* ticket;       // workgroups done in the current launch (reset by the last one)
  int* corr;              // [ns] target index of every source point in the last evaluated iteration (-1: none)
  double* trace;          // [max_iterations][18] (an evaluation, eval.hip: its QtrEvalRecord)
  int* mail;              // grouped launches: device view of the slot's host mailbox (frontend.h MAIL_ICP*), else null
  const float4* src_nrm;  // [ns] source normals, source frame (plane-to-plane, voxelised or not) or null
  QtrIcpVoxel* vox;       // [nt] voxelised plane-to-plane: the record of cell c at cell_start[c] (IcpBufs: icp_reserve_vox)
  int* vord;              // [nt] ... and its scratch: every cell's places in spts in ascending original index
};

__device__ __forceinline__ int icp_enc(float f) {  // order-preserving int of a finite float (for atomicMin / Max)
  const int b = __float_as_int(f);
  return b >= 0 ? b : (b ^ 0x7fffffff);
}
static inline float icp_dec(int e) {  // (host)
  const int b = e >= 0 ? e : (e ^ 0x7fffffff);
  float f;
  memcpy(&f, &b, 4);
  return f;
}

__global__ __launch_bounds__(256) void k_icp_bbox(IcpView v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= v.nt) return;
  const float4 p = v.tgt[i];
  if (!qtr_icp_finite3(p.x, p.y, p.z)) return;
  atomicMin(v.bbox + 0, icp_enc(p.x));
  atomicMin(v.bbox + 1, icp_enc(p.y));
  atomicMin(v.bbox + 2, icp_enc(p.z));
  atomicMax(v.bbox + 3, icp_enc(p.x));
  atomicMax(v.bbox + 4, icp_enc(p.y));
  atomicMax(v.bbox + 5, icp_enc(p.z));
}

// cell index of a coordinate (binary64), the same expression on both sides of the grid
__device__ __forceinline__ double icp_cellf(double x, double mn, double cell) { return floor((x - mn) / cell); }

__device__ __forceinline__ int icp_cell_of(const IcpView& v, float4 p) {
  int c[3];
  const double x[3] = {(double)p.x, (double)p.y, (double)p.z};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double f = icp_cellf(x[a], v.mn[a], v.cell);
    c[a] = f < 0 ? 0 : (f > (double)(v.dims[a] - 1) ? v.dims[a] - 1 : (int)f);
  }
  return c[0] + v.dims[0] * (c[1] + v.dims[1] * c[2]);
}

__device__ __forceinline__ void d_icp_count(const IcpView& v, int i) {
  if (i >= v.nt) return;
  const float4 p = v.tgt[i];
  if (!qtr_icp_finite3(p.x, p.y, p.z)) {
    v.place[2 * i] = -1;
    return;
  }
  const int lin = icp_cell_of(v, p);
  v.place[2 * i] = lin;
  v.place[2 * i + 1] = atomicAdd(v.cell_cnt + lin, 1);
}

__global__ __launch_bounds__(256) void k_icp_count(IcpView v) { d_icp_count(v, blockIdx.x * blockDim.x + threadIdx.x); }

__device__ __forceinline__ void d_icp_place(const IcpView& v, int i) {
  if (i >= v.nt) return;
  const int lin = v.place[2 * i];
  if (lin < 0) return;
  const int at = v.cell_start[lin] + v.place[2 * i + 1];
  float4 p = v.tgt[i];
  p.w = __int_as_float(i);
  v.spts[at] = p;
  if (v.nrm) v.snrm[at] = v.nrm[i];
}

__global__ __launch_bounds__(256) void k_icp_place(IcpView v) { d_icp_place(v, blockIdx.x * blockDim.x + threadIdx.x); }

__global__ __launch_bounds__(256) void k_icp_init(IcpView v, QtrIcpState init) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    *v.st = init;
    *v.ticket = 0u;
  }
}

__device__ __forceinline__ double icp_shfl_down(double x, int off) { return __shfl_down(x, off, 64); }

// The nearest finite target point within reach of q on the view's cell grid: best = its index in the target cloud (-1:
// none), bat = its place in spts / snrm, bd = its binary64 d^2; ties go to the lowest target index.  Shared by the ICP
// iteration and the evaluation (eval.hip); the caller has checked v.ncell > 0 and set best = bat = -1.
__device__ __forceinline__ void icp_nearest(const IcpView& v, const double* q, int& best, int& bat, double& bd) {
  int lo[3], hi[3];
  bool any = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double f = icp_cellf(q[a], v.mn[a], v.cell);  // (NaN / huge: compared as double before any int cast)
    if (!(f >= -1.0 && f <= (double)v.dims[a])) {
      any = false;
      lo[a] = 0;
      hi[a] = -1;
    } else {
      const int c = (int)f;
      lo[a] = c - 1 < 0 ? 0 : c - 1;
      hi[a] = c + 1 > v.dims[a] - 1 ? v.dims[a] - 1 : c + 1;
    }
  }
  if (any) {
    for (int cz = lo[2]; cz <= hi[2]; ++cz)
      for (int cy = lo[1]; cy <= hi[1]; ++cy) {
        const int row = v.dims[0] * (cy + v.dims[1] * cz);
        const int s = v.cell_start[row + lo[0]], e = v.cell_start[row + hi[0] + 1];  // (cells of a row are contiguous)
        for (int j = s; j < e; ++j) {
          const float4 t = v.spts[j];
          const double d2 = qtr_icp_d2(q, t.x, t.y, t.z);
          const int idx = __float_as_int(t.w);
          if (d2 <= v.cfg.max_d2 && (best < 0 || d2 < bd || (d2 == bd && idx < best))) {
            best = idx;
            bat = j;
            bd = d2;
          }
        }
      }
  }
}

// The reduction tail d_icp_iter and d_eval (eval.hip) share, called by every thread of a workgroup (chunk `blk` of `nblk`)
// with its NT terms: the fixed-shape sum (the shfl_down fold inside each wave, qtr_icp_fold64, then (w0 + w1) + (w2 + w3))
// into the chunk's partial at partials[blk * STRIDE], a fence, the ticket.  true: this is the LAST workgroup to arrive, and
// s_S[0 .. NT) holds the partials added in chunk order; the caller resets the ticket when it is done.
template <int NT, int STRIDE>
__device__ __forceinline__ bool icp_reduce_tail(const double* x, double* partials, unsigned* ticket, int blk, int nblk,
                                                double* s_S) {
  __shared__ double s_w[4][STRIDE];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < NT; ++k) {
    double a = x[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a = a + icp_shfl_down(a, off);
    if (lane == 0) s_w[wave][k] = a;
  }
  __syncthreads();
  if (tid < NT) {
    const double w4[4] = {s_w[0][tid], s_w[1][tid], s_w[2][tid], s_w[3][tid]};
    const double c = qtr_icp_chunk_sum(w4);
    __hip_atomic_store((unsigned long long*)(partials + (size_t)blk * STRIDE + tid),
                       (unsigned long long)__double_as_longlong(c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __threadfence();
  __syncthreads();
  if (tid == 0) {
    const unsigned done = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    s_last = (done == (unsigned)nblk - 1) ? 1 : 0;
  }
  __syncthreads();
  if (!s_last) return false;
  __threadfence();
  if (tid < NT) {
    double acc = __longlong_as_double((long long)__hip_atomic_load((unsigned long long*)(partials + tid), __ATOMIC_RELAXED,
                                                                   __HIP_MEMORY_SCOPE_AGENT));
    for (int c = 1; c < nblk; ++c)
      acc = acc + __longlong_as_double((long long)__hip_atomic_load(
                      (unsigned long long*)(partials + (size_t)c * STRIDE + tid), __ATOMIC_RELAXED,
                      __HIP_MEMORY_SCOPE_AGENT));
    s_S[tid] = acc;
  }
  __syncthreads();
  return true;
}

// ---- voxelised plane-to-plane: one record per non-empty cell (include/qtr_icp_math.h), after k_icp_place ----------------
// k_icp_place orders a cell by atomic rank, which differs from run to run, and the record's sums run in ascending original
// index: d_icp_voxel_order gives every finite target point its rank by index among its cell's points (a count over the
// cell: the cells of a voxelised cloud are small) and writes its place in spts there.
__device__ __forceinline__ void d_icp_voxel_order(const IcpView& v, int i) {
  if (i >= v.nt) return;
  const int lin = v.place[2 * i];
  if (lin < 0) return;
  const int s = v.cell_start[lin], e = v.cell_start[lin + 1];
  int rank = 0;
  for (int j = s; j < e; ++j) rank += __float_as_int(v.spts[j].w) < i ? 1 : 0;
  v.vord[s + rank] = s + v.place[2 * i + 1];
}

// The thread of the point that k_icp_place put first in its cell folds the cell: its members in ascending original index
// into the record at cell_start[cell] (n = 0: no member, the voxel does not exist).
__device__ __forceinline__ void d_icp_voxel_stats(const IcpView& v, int i) {
  if (i >= v.nt) return;
  const int lin = v.place[2 * i];
  if (lin < 0 || v.place[2 * i + 1] != 0) return;
  const int s = v.cell_start[lin], e = v.cell_start[lin + 1];
  double acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = 0.0;
  int n = 0, rep = -1;
  for (int r = s; r < e; ++r) {
    const int j = v.vord[r];
    const float4 t = v.spts[j];
    const float4 b = v.snrm[j];
    if (!qtr_icp_normal_ok(b.x, b.y, b.z)) continue;
    if (n == 0) rep = __float_as_int(t.w);
    qtr_icp_voxel_add(acc, t.x, t.y, t.z, b.x, b.y, b.z);
    ++n;
  }
  QtrIcpVoxel vx;
  qtr_icp_voxel_finish(acc, n, rep, &vx);
  v.vox[s] = vx;
}

__global__ __launch_bounds__(256) void k_icp_voxel_order(IcpView v) { d_icp_voxel_order(v, blockIdx.x * blockDim.x + threadIdx.x); }
__global__ __launch_bounds__(256) void k_icp_voxel_stats(IcpView v) { d_icp_voxel_stats(v, blockIdx.x * blockDim.x + threadIdx.x); }

// The frame every iteration kernel shares (d_icp_iter below, k_vmap_iter of voxelmap.hip); a kernel states only where its
// terms come from.  icp_iter_begin: the early return on the stop flag (false: stopped), the current T, the zeroed terms.
__device__ __forceinline__ bool icp_iter_begin(const IcpView& v, double* T, double* o) {
  const QtrIcpState* st = v.st;
  if (st->stop) return false;  // (uniform: written by an earlier launch)
#pragma unroll
  for (int k = 0; k < 16; ++k) T[k] = st->T[k];
#pragma unroll
  for (int k = 0; k < QTR_ICP_NT; ++k) o[k] = 0.0;
  return true;
}

// icp_iter_finish, called by every thread of the workgroup with its terms o[0 .. NT): the reduction tail; in the last
// workgroup the padding terms, the step with its trace row, the ticket's reset.
template <int NT>
__device__ __forceinline__ void icp_iter_finish(const IcpView& v, const double* o, int blk, int nblk) {
  __shared__ double s_S[QTR_ICP_NT];
  if (!icp_reduce_tail<NT, QTR_ICP_NT>(o, v.partials, v.ticket, blk, nblk, s_S)) return;
  if (threadIdx.x == 0) {
    for (int k = NT; k < QTR_ICP_NT; ++k) s_S[k] = 0.0;  // (the padding terms)
    QtrIcpState s = *v.st;
    double* tr = (s.iterations < v.cfg.max_iterations) ? v.trace + (size_t)s.iterations * 18 : nullptr;
    qtr_icp_step(&v.cfg, s_S, &s, tr);
    *v.st = s;
    __hip_atomic_store(v.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One workgroup (chunk `blk` of `nblk`) of one iteration of one pair.  METHOD 2: the plane-to-plane body (cfg.method == 2);
// 3: its voxelised form, a lookup in place of the search (cfg.method == 3); 0: the instantiation the other two methods
// always shared.
template <int METHOD>
__device__ __forceinline__ void d_icp_iter(const IcpView& v, int blk, int nblk) {
  constexpr bool GICP = METHOD == 2, VGICP = METHOD == 3;
  double T[16], o[QTR_ICP_NT];
  if (!icp_iter_begin(v, T, o)) return;
  const int i = blk * QTR_ICP_CHUNK + threadIdx.x;
  if (i < v.ns) {
    const float4 p = v.src[i];
    int best = -1, bat = -1;
    double bd = 0.0, q[3];
    bool use = qtr_icp_finite3(p.x, p.y, p.z) && v.ncell > 0;
    if ((GICP || VGICP) && use) {  // (a source point without a usable normal is skipped before the search)
      const float4 a = v.src_nrm[i];
      use = qtr_icp_normal_ok(a.x, a.y, a.z);
    }
    if (use) {
      qtr_icp_transform(T, p.x, p.y, p.z, q);
      if (!VGICP) icp_nearest(v, q, best, bat, bd);
    }
    if (VGICP) {
      int lin = 0;
      if (use && qtr_icp_voxel_cell(q, v.mn, v.cell, v.dims, &lin)) {
        const int s = v.cell_start[lin];
        if (s < v.cell_start[lin + 1]) {
          const QtrIcpVoxel vx = v.vox[s];
          if (vx.n > 0) {
            const float4 a = v.src_nrm[i];
            best = vx.rep;
            qtr_icp_vgicp_terms(T, q, a.x, a.y, a.z, &vx, o);
          }
        }
      }
      v.corr[i] = best;
    } else if (GICP) {
      if (best >= 0) {
        const float4 n = v.snrm[bat];
        if (!qtr_icp_normal_ok(n.x, n.y, n.z)) best = -1;
      }
      v.corr[i] = best;
      if (best >= 0) {
        const float4 t = v.spts[bat];
        const float4 n = v.snrm[bat];
        const float4 a = v.src_nrm[i];
        qtr_icp_gicp_terms(T, q, a.x, a.y, a.z, t.x, t.y, t.z, n.x, n.y, n.z, bd, o);
      }
    } else {
      if (best >= 0 && v.cfg.method == 0) {
        const float4 n = v.snrm[bat];
        if (!qtr_icp_finite3(n.x, n.y, n.z)) best = -1;
      }
      v.corr[i] = best;
      if (best >= 0) {
        const float4 t = v.spts[bat];
        const float4 n = v.cfg.method == 0 ? v.snrm[bat] : make_float4(0.f, 0.f, 0.f, 0.f);
        qtr_icp_terms(v.cfg.method, q, t.x, t.y, t.z, n.x, n.y, n.z, bd, o);
      }
    }
  }
  icp_iter_finish<VGICP ? QTR_ICP_T_W + 1 : QTR_ICP_T_CNT + 1>(v, o, blk, nblk);
}

__global__ __launch_bounds__(256) void k_icp_iter(IcpView v) { d_icp_iter<0>(v, (int)blockIdx.x, (int)gridDim.x); }
__global__ __launch_bounds__(256) void k_icp_iter_gicp(IcpView v) { d_icp_iter<2>(v, (int)blockIdx.x, (int)gridDim.x); }
__global__ __launch_bounds__(256) void k_icp_iter_vgicp(IcpView v) { d_icp_iter<3>(v, (int)blockIdx.x, (int)gridDim.x); }

// ---- grouped forms (the lane's refine phase of qtr_submit_batch_refine): blockIdx.y = pair of the group ----------------
// A launch is as wide as the group's largest pair; workgroups past the pair's own end return first.

// bbox = the identity of min / max, ticket = 0 (the arena is not cleared on allocation; a single-pair call leaves its box)
__global__ __launch_bounds__(64) void k_icp_box_init_group(ViewExt<IcpView> x) {
  const IcpView& v = x.ext[blockIdx.y];  // (inline on purpose: see ViewExt)
  if (threadIdx.x < 6) v.bbox[threadIdx.x] = threadIdx.x < 3 ? 0x7fffffff : (int)0x80000000;
  if (threadIdx.x == 0) __hip_atomic_store(v.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// k_icp_bbox for the 256 target points of workgroup blockIdx.x of one pair, folded in LDS first and merged into v.bbox.
// Called by every thread of the workgroup (the caller's early return for workgroups past the pair's end is block-uniform).
__device__ __forceinline__ void d_icp_bbox_fold(const IcpView& v) {
  __shared__ int s_bb[6];
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

// d_icp_bbox_fold per pair; the pair's last workgroup (ticket) mails the box to the host
// (MAIL_ICP_BOX, then MAIL_SEQ_ICP_BOX = seqs[pair]) and leaves the ticket at zero
__global__ __launch_bounds__(256) void k_icp_bbox_group(ViewExt<IcpView> x, const int* __restrict__ seqs) {
  const IcpView& v = x.ext[blockIdx.y];  // (inline on purpose: see ViewExt)
  const int nblk = (v.nt + 255) / 256;
  if ((int)blockIdx.x >= nblk) return;
  __shared__ int s_last;
  d_icp_bbox_fold(v);
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned done = __hip_atomic_fetch_add(v.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    s_last = (done == (unsigned)nblk - 1) ? 1 : 0;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  if (threadIdx.x < 16) {
    const int seq = seqs[blockIdx.y];
    const int b = threadIdx.x < 6 ? __hip_atomic_load(v.bbox + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    mail_store_line(v.mail + MAIL_ICP_BOX, threadIdx.x, b, seq);
    __threadfence_system();
    if (threadIdx.x == 0) {
      __hip_atomic_store(v.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      v.mail[MAIL_SEQ_ICP_BOX] = seq;
    }
  }
}

// clean cell counters (what icp_device's memset does), then k_icp_init's state and ticket
__global__ __launch_bounds__(256) void k_icp_prep_group(ViewExt<IcpView> x, const QtrIcpState* __restrict__ init) {
  const IcpView& v = x.ext[blockIdx.y];  // (inline on purpose: see ViewExt)
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e <= v.ncell; e += gridDim.x * blockDim.x) v.cell_cnt[e] = 0;
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    *v.st = init[blockIdx.y];
    *v.ticket = 0u;
  }
}

__global__ __launch_bounds__(256) void k_icp_count_group(ViewExt<IcpView> x) {
  const IcpView& v = x.ext[blockIdx.y];  // (inline on purpose: see ViewExt)
  d_icp_count(v, blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ __launch_bounds__(1024) void k_icp_scan_group(ViewExt<IcpView> x) {
  const IcpView& v = x.ext[blockIdx.y];  // (inline on purpose: see ViewExt)
  d_scan_i32_copy(v.cell_cnt, v.cell_start, v.ncell);
}

__global__ __launch_bounds__(256) void k_icp_place_group(ViewExt<IcpView> x) {
  const IcpView& v = x.ext[blockIdx.y];  // (inline on purpose: see ViewExt)
  d_icp_place(v, blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ __launch_bounds__(256) void k_icp_voxel_order_group(ViewExt<IcpView> x) {
  const IcpView& v = x.ext[blockIdx.y];  // (inline on purpose: see ViewExt)
  d_icp_voxel_order(v, blockIdx.x * blockDim.x + threadIdx.x);
}
__global__ __launch_bounds__(256) void k_icp_voxel_stats_group(ViewExt<IcpView> x) {
  const IcpView& v = x.ext[blockIdx.y];  // (inline on purpose: see ViewExt)
  d_icp_voxel_stats(v, blockIdx.x * blockDim.x + threadIdx.x);
}

// one iteration of every pair of the group: the pair's chunk count stands where k_icp_iter has gridDim.x
__global__ __launch_bounds__(256) void k_icp_iter_group(ViewExt<IcpView> x) {
  const IcpView& v = x.ext[blockIdx.y];  // (inline on purpose: see ViewExt)
  const int nblk = (v.ns + QTR_ICP_CHUNK - 1) / QTR_ICP_CHUNK;
  if ((int)blockIdx.x >= nblk) return;  // (before the stop flag and the ticket)
  d_icp_iter<0>(v, (int)blockIdx.x, nblk);
}
__global__ __launch_bounds__(256) void k_icp_iter_gicp_group(ViewExt<IcpView> x) {
  const IcpView& v = x.ext[blockIdx.y];  // (inline on purpose: see ViewExt)
  const int nblk = (v.ns + QTR_ICP_CHUNK - 1) / QTR_ICP_CHUNK;
  if ((int)blockIdx.x >= nblk) return;
  d_icp_iter<2>(v, (int)blockIdx.x, nblk);
}
__global__ __launch_bounds__(256) void k_icp_iter_vgicp_group(ViewExt<IcpView> x) {
  const IcpView& v = x.ext[blockIdx.y];  // (inline on purpose: see ViewExt)
  const int nblk = (v.ns + QTR_ICP_CHUNK - 1) / QTR_ICP_CHUNK;
  if ((int)blockIdx.x >= nblk) return;
  d_icp_iter<3>(v, (int)blockIdx.x, nblk);
}

// the first QTR_ICP_MAIL_WORDS words of every pair's state into its mailbox (three tagged lines from MAIL_ICP), then
// MAIL_SEQ_ICP = seqs[pair]; one wave per pair
#define QTR_ICP_MAIL_WORDS 44  // T, prev_mse, fitness, rmse, iterations, stop, reason, n_corr, valid, converged
static_assert(offsetof(QtrIcpState, pad) == QTR_ICP_MAIL_WORDS * 4, "the mailed words end where QtrIcpState's pad begins");
static_assert(QTR_ICP_MAIL_WORDS <= 45 && MAIL_ICP + 48 <= MAIL_INTS, "three mailbox lines");
__global__ __launch_bounds__(64) void k_icp_publish_group(ViewExt<IcpView> x, const int* __restrict__ seqs) {
  const IcpView& v = x.ext[blockIdx.x];  // (inline on purpose: see ViewExt)
  const int t = threadIdx.x;
  if (t >= 48) return;  // (whole 16-lane groups stay together for the tag's shuffles)
  const int seq = seqs[blockIdx.x];
  const int w = (t >> 4) * 15 + (t & 15);  // state word carried by this lane (lane 15 of a line: the tag)
  const int val = ((t & 15) < 15 && w < QTR_ICP_MAIL_WORDS) ? ((const int*)v.st)[w] : 0;
  mail_store_line(v.mail + MAIL_ICP + 16 * (t >> 4), t & 15, val, seq);
  __threadfence_system();
  if (t == 0) v.mail[MAIL_SEQ_ICP] = seq;
}

// ---- host side ----------------------------------------------------------------------------------------------------
struct IcpBufs {
  int cap_pts = 0;        // points per cloud the arena holds
  int cap_cells = 0;
  void* arena = nullptr;  // everything but the cell table
  int* cells = nullptr;   // [2][cap_cells + 1]: counters, starts
  IcpView v{};
  QtrIcpState* h_state = nullptr;  // pinned read-back
  int* h_bbox = nullptr;
  void* vox = nullptr;    // voxelised plane-to-plane: records and order scratch (icp_reserve_vox, on the slot's first such call)
  int cap_vox = 0;        // points they hold
};

// QTR_ICP_CELL_CAP (include/qtr_icp_math.h), the largest cell table of a call: a grid of the search methods that would need
// more cells takes larger cells (still >= the correspondence distance, so the result is the same; only the candidate lists
// get longer); the voxel grid of method 3 is refused instead.
// the cell table every slot reserves for the batched refinement (qtr_submit_batch_refine), so that the lanes never allocate:
// a larger grid takes larger cells (icp_grid_of).  2^20 cells of 1 m cover a 100 m x 100 m x 100 m box.
#define QTR_ICP_BATCH_CELLS (1 << 20)

static hipError_t icp_reserve(IcpBufs& B, int cap_pts, int max_iter_cap) {
  if (B.arena && B.cap_pts >= cap_pts) return hipSuccess;
  if (B.arena) (void)hipFree(B.arena);
  if (B.h_state) (void)hipHostFree(B.h_state);
  B.arena = nullptr;
  B.h_state = nullptr;
  const size_t nchunk = (size_t)(cap_pts + QTR_ICP_CHUNK - 1) / QTR_ICP_CHUNK;
  const size_t bytes = (size_t)cap_pts * (16 + 16 + 8 + 4) + nchunk * QTR_ICP_NT * 8 + (size_t)max_iter_cap * 18 * 8 +
                       sizeof(QtrIcpState) + 4096;
  hipError_t e = hipMalloc(&B.arena, bytes);
  if (e != hipSuccess) return e;
  char* p = (char*)B.arena;
  auto take = [&](size_t n) {
    char* r = p;
    p += (n + 255) & ~(size_t)255;
    return r;
  };
  B.v.st = (QtrIcpState*)take(sizeof(QtrIcpState));
  B.v.ticket = (unsigned*)take(64);
  B.v.bbox = (int*)take(64);
  B.v.partials = (double*)take(nchunk * QTR_ICP_NT * 8);
  B.v.trace = (double*)take((size_t)max_iter_cap * 18 * 8);
  B.v.spts = (float4*)take((size_t)cap_pts * 16);
  B.v.snrm = (float4*)take((size_t)cap_pts * 16);
  B.v.place = (int*)take((size_t)cap_pts * 8);
  B.v.corr = (int*)take((size_t)cap_pts * 4);
  e = hipHostMalloc((void**)&B.h_state, sizeof(QtrIcpState) + 64);
  if (e != hipSuccess) return e;
  B.h_bbox = (int*)(B.h_state + 1);
  B.cap_pts = cap_pts;
  return hipSuccess;
}

static hipError_t icp_reserve_cells(IcpBufs& B, int ncell) {
  if (B.cells && B.cap_cells >= ncell) return hipSuccess;
  if (B.cells) (void)hipFree(B.cells);
  B.cells = nullptr;
  int cap = 1 << 16;
  while (cap < ncell) cap <<= 1;
  hipError_t e = hipMalloc((void**)&B.cells, (size_t)2 * (cap + 1) * 4 + 512);
  if (e != hipSuccess) return e;
  B.cap_cells = cap;
  return hipSuccess;
}

// the voxel records and their scratch, for clouds of cap_pts points
static hipError_t icp_reserve_vox(IcpBufs& B, int cap_pts) {
  if (B.vox && B.cap_vox >= cap_pts) return hipSuccess;
  if (B.vox) (void)hipFree(B.vox);
  B.vox = nullptr;
  B.cap_vox = 0;
  const size_t rec = ((size_t)cap_pts * sizeof(QtrIcpVoxel) + 255) & ~(size_t)255;
  const hipError_t e = hipMalloc(&B.vox, rec + (size_t)cap_pts * 4 + 256);
  if (e != hipSuccess) return e;
  B.v.vox = (QtrIcpVoxel*)B.vox;
  B.v.vord = (int*)((char*)B.vox + rec);
  B.cap_vox = cap_pts;
  return hipSuccess;
}

static void icp_free(IcpBufs& B) {
  if (B.vox) (void)hipFree(B.vox);
  if (B.arena) (void)hipFree(B.arena);
  if (B.cells) (void)hipFree(B.cells);
  if (B.h_state) (void)hipHostFree(B.h_state);
  B = IcpBufs{};
}

// What a method reads.  These three are the only place that knows: the entry points, the view binding, the grid build and
// the choice of the iteration kernel (icp_iter_launch) all ask them.
static bool icp_method_known(int method) { return method >= QTR_ICP_POINT_TO_PLANE && method <= QTR_ICP_VOXEL_PLANE_TO_PLANE; }
static bool icp_voxel_grid(int method) { return method == QTR_ICP_VOXEL_PLANE_TO_PLANE; }  // (records in place of the search)
static bool icp_reads_src_normals(int method) { return method == QTR_ICP_PLANE_TO_PLANE || icp_voxel_grid(method); }
static bool icp_reads_tgt_normals(int method) { return method == QTR_ICP_POINT_TO_PLANE || icp_reads_src_normals(method); }

static QtrIcpCfg icp_cfg_of(const qtr_icp_params* prm) {
  QtrIcpCfg c;
  c.max_d2 = prm->max_correspondence_distance * prm->max_correspondence_distance;
  c.trans_eps = prm->transformation_epsilon;
  c.fit_eps = prm->euclidean_fitness_epsilon;
  c.max_iterations = prm->max_iterations;
  c.method = prm->method;
  c.min_corr = prm->min_correspondences > 0 ? prm->min_correspondences
               : icp_reads_src_normals(prm->method) ? 4  // (pcl GICP's min_number_correspondences_)
               : icp_reads_tgt_normals(prm->method) ? 6
                                                    : 3;
  c.pad = 0;
  return c;
}

// The cell grid of a target box (6 order-preserving encodings, k_icp_bbox): cells a little larger than the correspondence
// distance (a rounding of the cell index cannot hide a point in reach); a grid of more than cap_cells cells takes larger
// ones.  Any cell >= the distance finds the same nearest neighbour (ties go to the lowest index), so the grid's shape does
// not change a result.  false: no finite target point; the view then carries the empty grid (ncell = 0), in which nothing
// is searched.
static bool icp_grid_of(IcpView& v, const int* bbox, double max_d, int cap_cells) {
  if (bbox[0] > bbox[3]) {
    v.ncell = v.dims[0] = v.dims[1] = v.dims[2] = 0;
    v.mn[0] = v.mn[1] = v.mn[2] = 0.0;
    v.cell = 1.0;
    return false;
  }
  double mx[3];
  for (int a = 0; a < 3; ++a) {
    v.mn[a] = (double)icp_dec(bbox[a]);
    mx[a] = (double)icp_dec(bbox[3 + a]);
  }
  double cell = max_d * 1.001;
  double nc = 0;
  for (;;) {
    nc = 1;
    for (int a = 0; a < 3; ++a) nc *= floor((mx[a] - v.mn[a]) / cell) + 1.0;
    if (nc <= (double)cap_cells) break;
    cell *= 1.25;
  }
  v.cell = cell;
  for (int a = 0; a < 3; ++a) v.dims[a] = (int)(floor((mx[a] - v.mn[a]) / cell) + 1.0);
  v.ncell = v.dims[0] * v.dims[1] * v.dims[2];
  return true;
}

// The voxel grid of method 3 (include/qtr_icp_math.h): origin = the box's minimum, side = the correspondence distance
// exactly.  The result depends on this grid, so it is never coarsened and every path derives it from this rule and
// QTR_ICP_CELL_CAP, not from an arena's capacity.  0: no finite target point (the empty grid, as icp_grid_of leaves it),
// 1: the view carries the grid, -1: more than QTR_ICP_CELL_CAP cells (msg names side and box).
static int icp_voxel_grid_of(IcpView& v, const int* bbox, double side, char* msg, size_t msg_len) {
  if (!icp_grid_of(v, bbox, side, QTR_ICP_CELL_CAP)) return 0;  // (its origin stays, its grid is overwritten below)
  const double mx[3] = {(double)icp_dec(bbox[3]), (double)icp_dec(bbox[4]), (double)icp_dec(bbox[5])};
  v.cell = side;
  const double nc = qtr_icp_voxel_dims(v.mn, mx, side, v.dims);
  if (!(nc <= (double)QTR_ICP_CELL_CAP)) {
    snprintf(msg, msg_len, "voxelised plane-to-plane: voxels of side %g m over a box of %g x %g x %g m are %.0f cells, more than %d",
             side, mx[0] - v.mn[0], mx[1] - v.mn[1], mx[2] - v.mn[2], nc, QTR_ICP_CELL_CAP);
    v.ncell = v.dims[0] = v.dims[1] = v.dims[2] = 0;
    return -1;
  }
  v.ncell = v.dims[0] * v.dims[1] * v.dims[2];
  return 1;
}

static void icp_result_from(qtr_icp_result* res, const QtrIcpState& st) {
  res->valid = st.valid;
  res->converged = st.converged;
  res->stop_reason = st.reason;
  res->iterations = st.iterations;
  res->n_corr = st.n_corr;
  for (int k = 0; k < 16; ++k) res->T[k] = st.T[k];
  res->fitness = st.fitness;
  res->rmse = st.rmse;
}

// what a pair with nothing to refine reports: the guess, no correspondence, reason TOO_FEW (the device state starts RUNNING)
static void icp_result_empty(qtr_icp_result* res, const double* guess) {
  QtrIcpState init;
  qtr_icp_init(&init, guess);
  init.reason = QTR_ICP_STOP_TOO_FEW;
  icp_result_from(res, init);
}

// the clouds of a refinement and the normal sets its method reads (the others: null), into a view
static void icp_view_bind(IcpView& v, const qtr_icp_params* prm, const float4* src, int ns, const float4* src_nrm,
                          const float4* tgt, int nt, const float4* tgt_nrm) {
  v.src = src;
  v.tgt = tgt;
  v.nrm = icp_reads_tgt_normals(prm->method) ? tgt_nrm : nullptr;
  v.src_nrm = icp_reads_src_normals(prm->method) ? src_nrm : nullptr;
  v.ns = ns;
  v.nt = nt;
  v.cfg = icp_cfg_of(prm);
}

// one iteration of a method: of one pair (grid = its chunks), of a group (grid = (chunks of the largest pair, pairs))
static void icp_iter_launch(int method, dim3 grid, hipStream_t st, const IcpView& v) {
  if (icp_voxel_grid(method)) hipLaunchKernelGGL(k_icp_iter_vgicp, grid, dim3(256), 0, st, v);
  else if (icp_reads_src_normals(method)) hipLaunchKernelGGL(k_icp_iter_gicp, grid, dim3(256), 0, st, v);
  else hipLaunchKernelGGL(k_icp_iter, grid, dim3(256), 0, st, v);
}
static void icp_iter_launch(int method, dim3 grid, hipStream_t st, const ViewExt<IcpView>& x) {
  if (icp_voxel_grid(method)) hipLaunchKernelGGL(k_icp_iter_vgicp_group, grid, dim3(256), 0, st, x);
  else if (icp_reads_src_normals(method)) hipLaunchKernelGGL(k_icp_iter_gicp_group, grid, dim3(256), 0, st, x);
  else hipLaunchKernelGGL(k_icp_iter_group, grid, dim3(256), 0, st, x);
}

// ---- single-pair launches (icp_device and the single evaluations, capi.hip) ----------------------------------------------
// the box of the finite target points into v.bbox; h_bbox: 6 pinned ints, which the caller reads the box back into
static hipError_t icp_box_enqueue(const IcpView& v, int* h_bbox, hipStream_t st) {
  for (int a = 0; a < 3; ++a) {
    h_bbox[a] = 0x7fffffff;
    h_bbox[3 + a] = (int)0x80000000;
  }
  const hipError_t e = hipMemcpyAsync(v.bbox, h_bbox, 24, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return e;
  if (v.nt > 0) hipLaunchKernelGGL(k_icp_bbox, dim3(qtr_div_up(v.nt, 256)), dim3(256), 0, st, v);
  return hipGetLastError();
}

// the cell grid of the view (it carries its grid now: icp_grid_of) and the initial state
static hipError_t icp_grid_enqueue(const IcpView& v, const QtrIcpState& init, hipStream_t st, bool voxels = false) {
  hipError_t e = hipMemsetAsync(v.cell_cnt, 0, (size_t)(v.ncell + 1) * 4, st);
  if (e != hipSuccess) return e;
  if (v.nt > 0) {
    hipLaunchKernelGGL(k_icp_count, dim3(qtr_div_up(v.nt, 256)), dim3(256), 0, st, v);
    if ((e = exclusive_scan_i32(v.cell_cnt, v.cell_start, v.ncell, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_icp_place, dim3(qtr_div_up(v.nt, 256)), dim3(256), 0, st, v);
    if (voxels) {  // (method 3: the cells' records)
      hipLaunchKernelGGL(k_icp_voxel_order, dim3(qtr_div_up(v.nt, 256)), dim3(256), 0, st, v);
      hipLaunchKernelGGL(k_icp_voxel_stats, dim3(qtr_div_up(v.nt, 256)), dim3(256), 0, st, v);
    }
  }
  hipLaunchKernelGGL(k_icp_init, dim3(1), dim3(64), 0, st, v, init);
  return hipGetLastError();
}

// ---- grouped launches (the lane's refine phase, capi.hip) ---------------------------------------------------------------
// dv: the group's views in device memory (the lane's ViewStage); dseqs: one mailbox sequence number per pair.
static hipError_t icp_box_enqueue_group(const IcpView* dv, int G, int max_nt, const int* dseqs, hipStream_t st) {
  const ViewExt<IcpView> x{dv, {0, 0, 0}};
  hipLaunchKernelGGL(k_icp_box_init_group, dim3(1, G), dim3(64), 0, st, x);
  hipLaunchKernelGGL(k_icp_bbox_group, dim3(qtr_div_up(max_nt, 256), G), dim3(256), 0, st, x, dseqs);
  return hipGetLastError();
}

// the cell grids of the group (views carry their grids now) and the initial states
static hipError_t icp_grid_enqueue_group(const IcpView* dv, const QtrIcpState* dinit, int G, int max_nt, int max_ncell,
                                         hipStream_t st, bool voxels = false) {
  const ViewExt<IcpView> x{dv, {0, 0, 0}};
  hipLaunchKernelGGL(k_icp_prep_group, dim3(std::min(qtr_div_up((long long)max_ncell + 1, 256), 1024), G), dim3(256), 0, st,
                     x, dinit);
  hipLaunchKernelGGL(k_icp_count_group, dim3(qtr_div_up(max_nt, 256), G), dim3(256), 0, st, x);
  hipLaunchKernelGGL(k_icp_scan_group, dim3(1, G), dim3(1024), 0, st, x);
  hipLaunchKernelGGL(k_icp_place_group, dim3(qtr_div_up(max_nt, 256), G), dim3(256), 0, st, x);
  if (voxels) {
    hipLaunchKernelGGL(k_icp_voxel_order_group, dim3(qtr_div_up(max_nt, 256), G), dim3(256), 0, st, x);
    hipLaunchKernelGGL(k_icp_voxel_stats_group, dim3(qtr_div_up(max_nt, 256), G), dim3(256), 0, st, x);
  }
  return hipGetLastError();
}

// `launches` iterations of the group (method: which instantiation), then every pair's state into its mailbox
static hipError_t icp_iter_enqueue_group(const IcpView* dv, int G, int max_nchunk, int launches, const int* dseqs,
                                         hipStream_t st, int method) {
  const ViewExt<IcpView> x{dv, {0, 0, 0}};
  for (int k = 0; k < launches; ++k) icp_iter_launch(method, dim3(max_nchunk, G), st, x);
  hipLaunchKernelGGL(k_icp_publish_group, dim3(G), dim3(64), 0, st, x, dseqs);
  return hipGetLastError();
}
