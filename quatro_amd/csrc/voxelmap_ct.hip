// voxelmap_ct.hip — the continuous-time registration of a RAW sweep against the voxel map (qtr_voxel_map_register_ct /
// qtr_voxel_map_ct_pose_at, include/quatro_voxelmap_ct.h).  The contract is include/qtr_vmap_ct_math.h: the unknown is the
// sensor's pose E at the sweep's end, its pose B at the beginning is fixed, and every point is carried by the pose interpolated
// at its own time inside every iteration.  With every time at t_end the call IS qtr_voxel_map_register, bit for bit.
//
// The two entry points are exports of the extension library, libquatro_ext.so (voxelmap.hip says how it is built);
// libquatro_hip.so carries this code and exports none of it.
//
//   k_vmap_ct_census   one launch before the loop: the skipped and the extrapolated points, which depend on the points, their
//                      normals and their times alone and not on the iterate; one ballot per wave, at most two integer atomics
//                      per wave.
//   k_vmap_iter_ct     d_vmap_iter's frame (voxelmap.hip) around the continuous-time terms: icp_iter_begin, the interval of the
//                      current E — the same for every thread: thread 0 builds it in LDS, one barrier —, one point per thread
//                      of chunk blockIdx.x, the hash lookup, qtr_vmap_ct_terms, corr = 0 / -1, icp_iter_finish.  A refused
//                      interval leaves every term zero, so the step stops with QTR_ICP_STOP_TOO_FEW.
// The host side is vmap_register_loop (voxelmap.hip: icp_loop on the slot's ICP arena with the empty grid) with k_vmap_iter_ct as
// its launch, so QTR_DBG_ICP_TRACE, _TIMES and _CORR serve the call like any map registration.  Points and normals are staged
// as vmap_stage stages them; host-resident times go into a buffer of the slot's own, grown to a call's need.
// The map is only read.  No kernel waits for another workgroup, none is launched cooperatively, all stores are plain vector
// stores; the only atomics beyond the iteration's ticket are the census's.
#include "../../include/quatro_voxelmap_ct.h"
#include "../../include/qtr_vmap_ct_math.h"

struct VmapCt {
  const float* times;  // [ns] the time of every source point
  double B[12];        // rows 0 - 2 of the fixed begin pose
  double t_begin, t_end;  // (the interval's divisor is qtr_deskew_interval's: t_begin - t_end)
};

enum { VC_CTR_SKIPPED = 0, VC_CTR_EXTRA, VC_CTR_INTS = 4 };

__global__ __launch_bounds__(256) void k_vmap_ct_census(const float4* __restrict__ src, const float4* __restrict__ nrm,
                                                        const float* __restrict__ times, int n, double tau, double div, int* ctr) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  int flags = 0;
  if (i < n) {
    const float4 p = src[i];
    const float4 a = nrm[i];
    flags = qtr_vmap_ct_flags(tau, div, p.x, p.y, p.z, a.x, a.y, a.z, times[i]);
  }
  // (every lane of every wave is here: no early return above)
  const u64 b_skip = __ballot(flags == QTR_VMAP_CT_SKIPPED), b_extra = __ballot(flags == QTR_VMAP_CT_EXTRAPOLATED);
  if (qk_lane() == 0) {
    if (b_skip) atomicAdd(ctr + VC_CTR_SKIPPED, __popcll(b_skip));
    if (b_extra) atomicAdd(ctr + VC_CTR_EXTRA, __popcll(b_extra));
  }
}

__global__ __launch_bounds__(256) void k_vmap_iter_ct(IcpView v, VmapView m, VmapCt c) {
  __shared__ QtrDeskewInterval s_iv;
  __shared__ int s_ok;
  double E[16], o[QTR_ICP_NT];
  if (!icp_iter_begin(v, E, o)) return;  // (uniform: every thread of the workgroup reaches the barrier or none does)
  if (threadIdx.x == 0) {
    double B[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) B[k] = c.B[k];
    QtrDeskewInterval iv;
    s_ok = qtr_vmap_ct_interval(c.t_begin, c.t_end, B, E, &iv) ? 1 : 0;
    s_iv = iv;
  }
  __syncthreads();
  const int blk = (int)blockIdx.x, nblk = (int)gridDim.x;
  const int i = blk * QTR_ICP_CHUNK + threadIdx.x;
  if (i < v.ns) {
    int best = -1;
    if (s_ok) {
      const float4 p = v.src[i];
      const float4 a = v.src_nrm[i];
      double T[12], q[3], r[3], s = 0.0;
      u64 key = 0;
      if (qtr_vmap_ct_query(&s_iv, p.x, p.y, p.z, a.x, a.y, a.z, c.times[i], m.side, T, q, r, &s, &key)) {
        const long long at = d_vmap_find(m, key);
        if (at >= 0) {
          const QtrIcpVoxel vx = m.rec[at];
          if (m.cnt[at] > 0 && vx.n > 0) {
            best = 0;
            qtr_vmap_ct_terms(T, q, r, s, a.x, a.y, a.z, &vx, o);
          }
        }
      }
    }
    v.corr[i] = best;
  }
  icp_iter_finish<QTR_ICP_T_W + 1>(v, o, blk, nblk);
}

// ---- host side ----------------------------------------------------------------------------------------------------
// the slot's own: host-resident times staged on the device (grown to a call's need), the census counters and their read-back
struct VmapCtBufs {
  float* times = nullptr;
  size_t cap = 0;      // floats
  int* ctr = nullptr;  // device, VC_CTR_INTS
  int* pin = nullptr;  // pinned, VC_CTR_INTS
};

static void vmap_ct_free(Slot& s) {
  if (!s.vct) return;
  if (s.vct->times) (void)hipFree(s.vct->times);
  if (s.vct->ctr) (void)hipFree(s.vct->ctr);
  if (s.vct->pin) (void)hipHostFree(s.vct->pin);
  delete s.vct;
  s.vct = nullptr;
}

// the buffers of a call that stages n_times floats (0: its times are device-resident)
static int vmap_ct_bufs(qtr_handle* h, Slot& s, size_t n_times) {
  if (!s.vct) {
    s.vct = new (std::nothrow) VmapCtBufs();
    if (!s.vct) return QTR_ERR_CAPACITY;
  }
  VmapCtBufs& b = *s.vct;
  if (!b.ctr) QTR_HIP_TRY(h, hipMalloc((void**)&b.ctr, VC_CTR_INTS * sizeof(int)));
  if (!b.pin) QTR_HIP_TRY(h, hipHostMalloc((void**)&b.pin, VC_CTR_INTS * sizeof(int)));
  if (n_times > b.cap) {  // (the slot's last call had completed when it returned: nothing reads the old buffer)
    if (b.times) (void)hipFree(b.times);
    b.times = nullptr;
    b.cap = 0;
    const size_t cap = (n_times + 4095) & ~(size_t)4095;
    QTR_HIP_TRY(h, hipMalloc((void**)&b.times, cap * sizeof(float)));
    b.cap = cap;
  }
  return QTR_OK;
}

// everything qtr_voxel_map_register_ct refuses, before anything is enqueued; guess: the caller's, or the begin pose
static int vmap_ct_check(qtr_handle* h, const qtr_voxel_map* m, const float* src4, int n, const float* nrm4, const float* times,
                         double t_begin, double t_end, const double* begin_pose, const double* guess, const qtr_icp_params* prm,
                         int mem) {
  QTR_TRY(vmap_check(h, m));
  QTR_TRY(check_icp_params(h, prm));
  if (prm->method != QTR_ICP_VOXEL_PLANE_TO_PLANE) {
    snprintf(h->err, sizeof(h->err), "voxel map register: method must be QTR_ICP_VOXEL_PLANE_TO_PLANE");
    return QTR_ERR_BAD_ARG;
  }
  QTR_TRY(vmap_check_cloud(h, "register", "src_normals4", nullptr, mem, n, src4, nrm4));
  if (n > 0 && !times) {
    snprintf(h->err, sizeof(h->err), "voxel map register: times is NULL");
    return QTR_ERR_BAD_ARG;
  }
  if (!begin_pose) {
    snprintf(h->err, sizeof(h->err), "voxel map register: begin_pose is NULL");
    return QTR_ERR_BAD_ARG;
  }
  QTR_TRY(vmap_check_pose(h, "register", "begin pose", begin_pose));
  QTR_TRY(vmap_check_pose(h, "register", "guess", guess));
  if (!icp_finite(t_begin) || !icp_finite(t_end) || !(t_begin < t_end) || !icp_finite(t_begin - t_end)) {
    snprintf(h->err, sizeof(h->err), "voxel map register: t_begin=%g, t_end=%g must be finite with t_begin < t_end", t_begin, t_end);
    return QTR_ERR_BAD_ARG;
  }
  QtrDeskewInterval iv;
  if (!qtr_vmap_ct_interval(t_begin, t_end, begin_pose, guess, &iv)) {
    snprintf(h->err, sizeof(h->err),
             "voxel map register: the guess differs from the begin pose by a rotation above pi / 2 (or a pose is no rotation)");
    return QTR_ERR_BAD_ARG;
  }
  return QTR_OK;
}

int qtr_voxel_map_register_ct(qtr_handle* h, int slot, const qtr_voxel_map* m, const float* src4, int n, const float* src_normals4,
                              const float* times, double t_begin, double t_end, const double begin_pose[16],
                              const double guess_end[16], const qtr_icp_params* prm, qtr_icp_result* res, int mem,
                              qtr_vmap_ct_info* info) {
  if (info) memset(info, 0, sizeof(*info));
  Slot* sp = get_slot(h, slot);
  if (!sp || !res) return QTR_ERR_BAD_ARG;
  memset(res, 0, sizeof(*res));
  Slot& s = *sp;
  const double* guess = guess_end ? guess_end : begin_pose;
  int rc = vmap_ct_check(h, m, src4, n, src_normals4, times, t_begin, t_end, begin_pose, guess, prm, mem);
  if (rc != QTR_OK) return res->status = rc;
  rc = [&]() -> int {
    const float4 *d_src = (const float4*)src4, *d_nrm = (const float4*)src_normals4;
    QTR_TRY(vmap_stage(h, s, "register", "src_normals4", nullptr, mem, n, &d_src, &d_nrm));
    double g[16];
    vmap_guess(guess, g);
    VmapCt c{};
    c.times = times;
    for (int k = 0; k < 12; ++k) c.B[k] = begin_pose[k];
    c.t_begin = t_begin;
    c.t_end = t_end;
    qtr_vmap_ct_info ci = {n, 0, 0};
    if (n > 0) {
      const hipStream_t st = s.stream;
      QTR_TRY(vmap_ct_bufs(h, s, mem == QTR_MEM_HOST ? (size_t)n : 0));
      VmapCtBufs& b = *s.vct;
      if (mem == QTR_MEM_HOST) {
        QTR_HIP_TRY(h, hipMemcpyAsync(b.times, times, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
        c.times = b.times;
      }
      QTR_HIP_TRY(h, hipMemsetAsync(b.ctr, 0, VC_CTR_INTS * sizeof(int), st));
      hipLaunchKernelGGL(k_vmap_ct_census, dim3(qtr_div_up(n, 256)), dim3(256), 0, st, d_src, d_nrm, c.times, n, t_end,
                         t_begin - t_end, b.ctr);
      QTR_HIP_TRY(h, hipGetLastError());
      QTR_HIP_TRY(h, hipMemcpyAsync(b.pin, b.ctr, VC_CTR_INTS * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    QTR_TRY(vmap_register_loop(h, s, m, d_src, n, d_nrm, g, prm, res, [&](hipStream_t st, dim3 chunks, const IcpView& w) {
      hipLaunchKernelGGL(k_vmap_iter_ct, chunks, dim3(256), 0, st, w, m->v, c);
    }));
    if (n > 0) {  // (the loop's last wait covers the counters' copy)
      ci.n_skipped = s.vct->pin[VC_CTR_SKIPPED];
      ci.n_extrapolated = s.vct->pin[VC_CTR_EXTRA];
    }
    if (info) *info = ci;
    return QTR_OK;
  }();
  return res->status = rc;
}

int qtr_voxel_map_ct_pose_at(double t_begin, double t_end, const double begin_pose[16], const double end_pose[16], double t,
                             double* T16) {
  if (!begin_pose || !end_pose || !T16) return QTR_ERR_BAD_ARG;
  if (!icp_finite(t_begin) || !icp_finite(t_end) || !(t_begin < t_end) || !icp_finite(t_begin - t_end)) return QTR_ERR_BAD_ARG;
  for (int k = 0; k < 12; ++k)
    if (!icp_finite(begin_pose[k]) || !icp_finite(end_pose[k])) return QTR_ERR_BAD_ARG;
  if (!qtr_vmap_ct_pose_at(t_begin, t_end, begin_pose, end_pose, t, T16)) return QTR_ERR_BAD_ARG;
  T16[12] = T16[13] = T16[14] = 0.0;
  T16[15] = 1.0;
  return QTR_OK;
}
