// deskew.hip — motion compensation of a raw sweep on the device (qtr_deskew / qtr_keyframe_create_deskewed /
// qtr_deskew_pose_at, include/quatro_deskew.h).  The contract is include/qtr_deskew_math.h.
//
// The three entry points are exports of the extension library, libquatro_ext.so (voxelmap.hip says how it is built);
// libquatro_hip.so carries this code hidden and exports none of it.
//
// The knot table — per interval tau_j, the divisor tau_{j+1} - tau_j, R_j, c_j, c_{j+1} - c_j and w_j = Log(R_j^T R_{j+1}),
// in front of it the reference pose — is computed by the HOST with qtr_deskew_table, the header's own function, into the
// slot's pinned buffer: the logs need K - 1 dependent chains of a few hundred binary64 operations, which is nothing for
// the host and would be a launch of one workgroup on the device, and judging the knots there would put a read-back in front
// of the refusals.  Both sides compile the header with -ffp-contract=off, so the device would compute the same bits.
//   k_deskew   one thread per point.  The workgroup copies the table (96 + 160 (K - 1) bytes, at most 40 896) from HBM
//              into dynamic LDS, every thread reads its point and its time, finds its interval by binary search in LDS,
//              evaluates qtr_deskew_point and writes its four floats with one 16-byte store: each thread reads its point
//              before it writes it, so out == in is allowed.  The three counts (points, skipped, extrapolated) are summed
//              per wave by ballot, per workgroup in LDS, and leave it as at most three atomics.
// qtr_keyframe_create_deskewed writes into the slot's raw-cloud buffer and goes on as qtr_keyframe_create on a cloud that is
// already staged (front_one_chain), as qtr_keyframe_merge does; the counts travel to pinned memory on the same stream and
// are read after the waits that chain has anyway.
// No kernel waits for another workgroup, none is launched cooperatively, all stores are plain vector stores.
#include "../../include/quatro_deskew.h"
#include "../../include/qtr_deskew_math.h"

static_assert(QTR_DESKEW_KNOTS_MAX == QTR_DESKEW_MAX_KNOTS, "the ABI's and the contract's knot limit");
static_assert(sizeof(QtrDeskewInterval) == 8 * QTR_DESKEW_IV_DOUBLES && sizeof(QtrDeskewPose) == 8 * QTR_DESKEW_POSE_DOUBLES,
              "the knot table is plain doubles");

enum { DK_CTR_POINTS = 0, DK_CTR_SKIPPED, DK_CTR_EXTRA, DK_CTR_INTS = 4 };

// doubles of the table of K knots: the reference pose, then K - 1 intervals
static inline int deskew_table_doubles(int K) { return QTR_DESKEW_POSE_DOUBLES + (K - 1) * QTR_DESKEW_IV_DOUBLES; }
static const size_t kDeskewTableBytes = 8 * (size_t)(QTR_DESKEW_POSE_DOUBLES + (QTR_DESKEW_MAX_KNOTS - 1) * QTR_DESKEW_IV_DOUBLES);
// the slot's device buffer: the counters (16 bytes), then the table.  The pinned one: 16 bytes of zeros, the table, and behind
// it the counters' read-back - so ONE copy up carries the table and clears the counters.
static const size_t kDeskewCtrBytes = DK_CTR_INTS * sizeof(int);
static const size_t kDeskewDevBytes = kDeskewCtrBytes + kDeskewTableBytes;
static const size_t kDeskewPinBytes = kDeskewDevBytes + kDeskewCtrBytes;

// dynamic LDS: n_tab doubles of table, then DK_CTR_INTS ints
__global__ __launch_bounds__(256) void k_deskew(const float4* in, const float* __restrict__ times, float4* out, int P, int K,
                                                const double* __restrict__ table, int n_tab, int* ctr) {
  extern __shared__ double s_tab[];
  int* s_cnt = (int*)(s_tab + n_tab);
  for (int i = threadIdx.x; i < n_tab; i += 256) s_tab[i] = table[i];
  if (threadIdx.x < DK_CTR_INTS) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const QtrDeskewPose* ref = (const QtrDeskewPose*)s_tab;
  const QtrDeskewInterval* tab = (const QtrDeskewInterval*)(s_tab + QTR_DESKEW_POSE_DOUBLES);
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  int flags = 0;
  const bool live = i < (long long)P;
  if (live) {
    const float4 p = in[i];
    const float pin[4] = {p.x, p.y, p.z, p.w};
    float q[4];
    flags = qtr_deskew_point(tab, K, ref, pin, times[i], q);
    out[i] = make_float4(q[0], q[1], q[2], q[3]);
  }
  // (every lane of every wave is here: no early return above)
  const u64 b_live = __ballot(live), b_skip = __ballot(flags == QTR_DESKEW_SKIPPED), b_extra = __ballot(flags == QTR_DESKEW_EXTRAPOLATED);
  if (qk_lane() == 0) {
    if (b_live) atomicAdd(s_cnt + DK_CTR_POINTS, __popcll(b_live));
    if (b_skip) atomicAdd(s_cnt + DK_CTR_SKIPPED, __popcll(b_skip));
    if (b_extra) atomicAdd(s_cnt + DK_CTR_EXTRA, __popcll(b_extra));
  }
  __syncthreads();
  if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(ctr + threadIdx.x, s_cnt[threadIdx.x]);
}

// ---- host side ----------------------------------------------------------------------------------------------------
static const char* deskew_refusal(int why) {
  switch (why) {
    case QTR_DESKEW_BAD_K: return "the number of knots must lie in 2 .. 256";
    case QTR_DESKEW_BAD_TIME: return "the knot times must be finite and strictly increasing";
    case QTR_DESKEW_BAD_POSE: return "a knot pose has a non-finite entry in rows 0 - 2";
    case QTR_DESKEW_BAD_ROTATION: return "two consecutive knots differ by a rotation above pi / 2 (or a knot pose is no rotation)";
    case QTR_DESKEW_BAD_TREF: return "t_ref is not finite";
  }
  return "refused";
}

// The argument checks of both entries and the knot table in the slot's pinned buffer.  Nothing is enqueued here.
static int deskew_prepare(qtr_handle* h, Slot& s, const char* who, bool have_arrays, int P, const double* knot_times,
                          const double* knot_poses, int K, double t_ref, int mem) {
  if (P < 0 || (P > 0 && !have_arrays) || (mem != QTR_MEM_HOST && mem != QTR_MEM_DEVICE)) {
    snprintf(h->err, sizeof(h->err), "%s: bad arguments (P=%d, NULL arrays with P > 0, or mem=%d)", who, P, mem);
    return QTR_ERR_BAD_ARG;
  }
  if (K < 2 || K > QTR_DESKEW_MAX_KNOTS || !knot_times || !knot_poses) {
    snprintf(h->err, sizeof(h->err), "%s: K=%d knots (2 .. %d, with their times and poses)", who, K, QTR_DESKEW_MAX_KNOTS);
    return QTR_ERR_BAD_ARG;
  }
  if (P > h->lim.max_points) {
    snprintf(h->err, sizeof(h->err), "%s: P=%d exceeds max_points=%d", who, P, h->lim.max_points);
    return QTR_ERR_CAPACITY;
  }
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  if (!s.deskew_pin) {
    QTR_HIP_TRY(h, hipHostMalloc(&s.deskew_pin, kDeskewPinBytes));
    memset(s.deskew_pin, 0, kDeskewPinBytes);
  }
  if (!s.deskew_dev) QTR_HIP_TRY(h, hipMalloc(&s.deskew_dev, kDeskewDevBytes));
  // (the slot's last deskew had completed when it returned: nothing reads the pinned table any more)
  double* pin = (double*)((char*)s.deskew_pin + kDeskewCtrBytes);
  const int why = qtr_deskew_table(knot_times, knot_poses, K, t_ref, (QtrDeskewInterval*)(pin + QTR_DESKEW_POSE_DOUBLES),
                                   (QtrDeskewPose*)pin);
  if (why != QTR_DESKEW_OK) {
    snprintf(h->err, sizeof(h->err), "%s: %s", who, deskew_refusal(why));
    return QTR_ERR_BAD_ARG;
  }
  return QTR_OK;
}

static int* deskew_pin_counters(Slot& s) { return (int*)((char*)s.deskew_pin + kDeskewDevBytes); }

// zeroed counters and the table up (one copy), the kernel, counters down: all on the slot's stream, no wait
static int deskew_enqueue(qtr_handle* h, Slot& s, const float4* d_in, const float* d_times, float4* d_out, int P, int K) {
  const int n_tab = deskew_table_doubles(K);
  int* d_ctr = (int*)s.deskew_dev;
  const double* d_tab = (const double*)((char*)s.deskew_dev + kDeskewCtrBytes);
  QTR_HIP_TRY(h, hipMemcpyAsync(s.deskew_dev, s.deskew_pin, kDeskewCtrBytes + (size_t)n_tab * 8, hipMemcpyHostToDevice, s.stream));
  hipLaunchKernelGGL(k_deskew, dim3(qtr_div_up(P, 256)), dim3(256), (size_t)n_tab * 8 + kDeskewCtrBytes, s.stream, d_in, d_times,
                     d_out, P, K, d_tab, n_tab, d_ctr);
  QTR_HIP_TRY(h, hipGetLastError());
  QTR_HIP_TRY(h, hipMemcpyAsync(deskew_pin_counters(s), d_ctr, kDeskewCtrBytes, hipMemcpyDeviceToHost, s.stream));
  return QTR_OK;
}

static void deskew_read_info(Slot& s, qtr_deskew_info* info) {
  if (!info) return;
  const int* c = deskew_pin_counters(s);
  info->n_points = c[DK_CTR_POINTS];
  info->n_skipped = c[DK_CTR_SKIPPED];
  info->n_extrapolated = c[DK_CTR_EXTRA];
}

int qtr_deskew(qtr_handle* h, int slot, const float* xyz4, const float* times, int P, const double* knot_times,
               const double* knot_poses, int K, double t_ref, float* out_xyz4, int mem, qtr_deskew_info* info) {
  if (info) memset(info, 0, sizeof(*info));
  Slot* sp = get_slot(h, slot);
  if (!sp) return QTR_ERR_BAD_ARG;
  Slot& s = *sp;
  QTR_TRY(deskew_prepare(h, s, "deskew", xyz4 && times && out_xyz4, P, knot_times, knot_poses, K, t_ref, mem));
  if (P == 0) return QTR_OK;
  s.times_pending = TIMES_NONE;
  const float4* d_in = (const float4*)xyz4;
  const float* d_times = times;
  float4* d_out = (float4*)out_xyz4;
  if (mem == QTR_MEM_HOST) {  // the cloud into the slot's raw-cloud buffer, deskewed in place there; the times beside it
    QTR_HIP_TRY(h, hipMemcpyAsync(s.in_src, xyz4, (size_t)P * 16, hipMemcpyHostToDevice, s.stream));
    QTR_HIP_TRY(h, hipMemcpyAsync(s.in_tgt, times, (size_t)P * 4, hipMemcpyHostToDevice, s.stream));
    d_in = d_out = s.in_src;
    d_times = (const float*)s.in_tgt;
  }
  QTR_TRY(deskew_enqueue(h, s, d_in, d_times, d_out, P, K));
  if (mem == QTR_MEM_HOST)
    QTR_HIP_TRY(h, hipMemcpyAsync(out_xyz4, s.in_src, (size_t)P * 16, hipMemcpyDeviceToHost, s.stream));
  QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
  deskew_read_info(s, info);
  return QTR_OK;
}

int qtr_keyframe_create_deskewed(qtr_handle* h, int slot, const float* raw4, const float* times, int P,
                                 const double* knot_times, const double* knot_poses, int K, double t_ref,
                                 const qtr_frontend_params* fp, int mem, qtr_keyframe** out, qtr_deskew_info* info) {
  if (out) *out = nullptr;
  if (info) memset(info, 0, sizeof(*info));
  Slot* sp = get_slot(h, slot);
  if (!sp || !fp || !out) return QTR_ERR_BAD_ARG;
  Slot& s = *sp;
  s.times_pending = TIMES_NONE;
  QTR_TRY(deskew_prepare(h, s, "keyframe of a deskewed sweep", raw4 && times, P, knot_times, knot_poses, K, t_ref, mem));
  QTR_TRY(front_one_check(h, raw4 != nullptr, P, fp));
  const float4* d_in = (const float4*)raw4;
  const float* d_times = times;
  if (mem == QTR_MEM_HOST) {
    QTR_HIP_TRY(h, hipMemcpyAsync(s.in_src, raw4, (size_t)P * 16, hipMemcpyHostToDevice, s.stream));
    QTR_HIP_TRY(h, hipMemcpyAsync(s.in_tgt, times, (size_t)P * 4, hipMemcpyHostToDevice, s.stream));
    d_in = s.in_src;
    d_times = (const float*)s.in_tgt;
  }
  QTR_TRY(deskew_enqueue(h, s, d_in, d_times, s.in_src, P, K));
  int n = 0, passed = 0;
  QTR_TRY(front_one_chain(h, s, s.in_src, P, fp, &n, &passed));  // (its waits cover the counters' copy)
  deskew_read_info(s, info);
  return keyframe_pack(h, s, fp, P, n, passed, out);
}

int qtr_deskew_pose_at(const double* knot_times, const double* knot_poses, int K, double t, double* T16) {
  if (!knot_times || !knot_poses || !T16 || K < 2 || K > QTR_DESKEW_MAX_KNOTS) return QTR_ERR_BAD_ARG;
  std::vector<QtrDeskewInterval> tab((size_t)K - 1);
  QtrDeskewPose ref;
  if (qtr_deskew_table(knot_times, knot_poses, K, t, tab.data(), &ref) != QTR_DESKEW_OK) return QTR_ERR_BAD_ARG;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T16[4 * r + c] = ref.R[3 * r + c];
    T16[4 * r + 3] = ref.c[r];
  }
  T16[12] = T16[13] = T16[14] = 0.0;
  T16[15] = 1.0;
  return QTR_OK;
}
