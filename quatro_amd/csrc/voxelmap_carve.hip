// voxelmap_carve.hip — visibility carving of the persistent voxel map (voxelmap.hip): a voxel leaves the map when enough
// scans, taken from known poses, measured returns clearly behind it (qtr_voxel_map_carve / qtr_voxel_map_carve_keyframes,
// include/quatro_voxelmap_carve.h).  The contract is include/qtr_vmap_carve_math.h.
//
// The three entry points are exports of the extension library, libquatro_ext.so (voxelmap.hip says how it is built);
// libquatro_hip.so carries this code hidden and exports none of it.
//
// A call with B scans (one cloud, or 1 .. 64 keyframes read in place):
//   (memset)        the B images to QTR_CARVE_EMPTY, one hipMemsetAsync
//   k_carve_image   one thread per point of each scan (blockIdx.y is the scan): range and pixel by qtr_carve_pixel, the
//                   minimum of the float's bit pattern into the scan's image with atomicMin — order-independent, so the
//                   images are the same bits in every run
//   k_carve_mark    a pass over the table's S slots that only reads the table, shaped like k_vmap_keep_mark.  The B poses
//                   (12 doubles each) sit in dynamic LDS.  A live voxel's mean is taken through every scan
//                   (qtr_carve_verdict: the window test against images that stay in L2, 256 KiB each at the defaults), the
//                   verdict goes to one byte per slot (0 no voxel, 1 kept, 2 carved), and the counts (kept, carved, tested,
//                   carved members as 64-bit) are summed per workgroup in LDS and leave it as at most four atomics
//   (host)          nothing carved: return, the table was only read.
//   (rebuild)       vmap_keep_rebuild (voxelmap_keep.hip), the end qtr_voxel_map_evict has too, with k_carve_stage as its
//                   staging kernel: d_vmap_stage_kept with the byte as the verdict, every survivor's key, count, acc and
//                   record into the eviction's staging; then k_vmap_clear and k_vmap_keep_put.  The table is rebuilt, never
//                   punched (voxelmap_keep.hip says why).
// The mark pass visits every slot and not a compacted list of the live ones: with capacity-sized tables most lanes see an
// empty key and leave at once, and a compaction would be a pass over the same S keys.  The two were not measured against
// each other.
// Memory: 64 poses (6 KiB) and B x rows x cols x 4 bytes of images in one allocation, one byte per table slot in
// another; both made on the first call that needs them, grown only, freed with the map.
// No kernel waits for another workgroup, none is launched cooperatively, all stores are plain vector stores.
#include "../../include/quatro_voxelmap_carve.h"
#include "../../include/qtr_vmap_carve_math.h"

static_assert(QTR_CARVE_MAX_KEYFRAMES == QTR_CARVE_MAX_SCANS, "the ABI's and the contract's scan limit");

// the scans of one call, inside the kernel arguments (64 pointers and 64 counts: 768 bytes)
struct CarveScans {
  const float4* pts[QTR_CARVE_MAX_SCANS];
  int n[QTR_CARVE_MAX_SCANS];
};

enum { CV_CTR_TESTED = 7 };  // beside voxelmap_keep.hip's VK_CTR_*: KEPT, EVICTED (the carved), MEMBERS64, STAGED, DUP
enum { CV_NONE = 0, CV_KEPT = 1, CV_CARVED = 2 };
static const size_t kCarvePoseBytes = (size_t)QTR_CARVE_MAX_SCANS * 12 * sizeof(double);
static const size_t kCarveHeadBytes = kCarvePoseBytes;  // the poses lie in front of the images (6144 bytes: a multiple of 256)

__global__ __launch_bounds__(256) void k_carve_image(CarveScans sc, QtrCarveCfg c, unsigned* img) {
  const int b = (int)blockIdx.y;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)sc.n[b]) return;
  const float4 p = sc.pts[b][i];
  double r = 0.0;
  int row = 0, col = 0;
  if (!qtr_carve_pixel(&c, (double)p.x, (double)p.y, (double)p.z, &r, &row, &col)) return;
  // (row in [0, rows) and col in [0, cols): qtr_carve_pixel returns nothing else)
  atomicMin(img + ((size_t)b * c.rows + row) * c.cols + col, qtr_carve_bits(r));
}

// dynamic LDS: 12 B doubles of poses
__global__ __launch_bounds__(256) void k_carve_mark(VmapView m, QtrCarveCfg c, const double* __restrict__ poses, int B,
                                                    const unsigned* __restrict__ img, unsigned char* mark, int* ctr) {
  extern __shared__ double s_pose[];
  __shared__ int s_kept, s_gone, s_tested;
  __shared__ u64 s_members;
  for (int i = threadIdx.x; i < 12 * B; i += 256) s_pose[i] = poses[i];
  if (threadIdx.x == 0) {
    s_kept = 0;
    s_gone = 0;
    s_tested = 0;
    s_members = 0;
  }
  __syncthreads();
  const size_t pixels = (size_t)c.rows * c.cols;
  int kept = 0, gone = 0, tested = 0;
  long long members = 0;
  for (u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x; e <= m.mask; e += (u64)gridDim.x * blockDim.x) {
    unsigned char v = CV_NONE;
    const int n = m.keys[e] == QTR_VMAP_EMPTY ? 0 : m.cnt[e];
    if (n > 0) {
      const double mu[3] = {m.rec[e].mu[0], m.rec[e].mu[1], m.rec[e].mu[2]};
      int votes = 0, any = 0;
      for (int b = 0; b < B; ++b) {
        const int vote = qtr_carve_verdict(&c, s_pose + 12 * b, mu, img + (size_t)b * pixels);
        any |= vote != QTR_CARVE_NO_VOTE;
        votes += vote == QTR_CARVE_SEEN_THROUGH ? 1 : 0;
      }
      const bool carve = votes >= c.min_votes;
      v = carve ? CV_CARVED : CV_KEPT;
      tested += any;
      kept += carve ? 0 : 1;
      gone += carve ? 1 : 0;
      members += carve ? n : 0;
    }
    mark[e] = v;
  }
  if (kept) atomicAdd(&s_kept, kept);
  if (tested) atomicAdd(&s_tested, tested);
  if (gone) {
    atomicAdd(&s_gone, gone);
    atomicAdd(&s_members, (u64)members);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_kept) atomicAdd(ctr + VK_CTR_KEPT, s_kept);
    if (s_tested) atomicAdd(ctr + CV_CTR_TESTED, s_tested);
    if (s_gone) {
      atomicAdd(ctr + VK_CTR_EVICTED, s_gone);
      atomicAdd((u64*)(ctr + VK_CTR_MEMBERS64), s_members);
    }
  }
}

// the rebuild's staging pass (d_vmap_stage_kept, voxelmap_keep.hip) with the mark byte as the verdict
__global__ __launch_bounds__(256) void k_carve_stage(VmapView m, const unsigned char* __restrict__ mark, VmapStage st, int n_kept) {
  d_vmap_stage_kept(m, st, n_kept, blockIdx.x * (u64)blockDim.x + threadIdx.x, (u64)gridDim.x * blockDim.x,
                    [&](u64 e) { return mark[e] == CV_KEPT; });
}

// ---- host side ----------------------------------------------------------------------------------------------------
void qtr_default_carve_params(qtr_carve_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->rows = 64;
  p->cols = 1024;
  p->window = 2;
  p->min_votes = 1;
  p->fov_up_deg = 2.5;
  p->fov_down_deg = -25.5;
  p->margin_abs = 0.0;
  p->margin_rel = 0.0;
  p->min_range = 1.0;
  p->max_range = 80.0;
}

static const char* carve_refusal(int why) {
  switch (why) {
    case QTR_CARVE_BAD_ROWS: return "rows must lie in 1 .. 256";
    case QTR_CARVE_BAD_COLS: return "cols must lie in 8 .. 4096";
    case QTR_CARVE_BAD_FOV: return "fov_up_deg and fov_down_deg must be finite, fov_up_deg above fov_down_deg";
    case QTR_CARVE_BAD_WINDOW: return "window must lie in 0 .. 3";
    case QTR_CARVE_BAD_VOTES: return "min_votes must lie in 1 .. the number of scans of the call";
    case QTR_CARVE_BAD_MARGIN: return "margin_abs and margin_rel must be finite and >= 0";
    case QTR_CARVE_BAD_RANGE: return "min_range and max_range must be finite, min_range below max_range";
  }
  return "refused";
}

// the checked parameters of a call with n_scans scans; nothing is enqueued here
static int carve_cfg(qtr_handle* h, const qtr_voxel_map* m, const qtr_carve_params* prm, int n_scans, QtrCarveCfg* c) {
  qtr_carve_params p;
  qtr_default_carve_params(&p);
  if (prm) p = *prm;
  const int why = qtr_carve_cfg_make(p.rows, p.cols, p.fov_up_deg, p.fov_down_deg, p.window, p.min_votes, p.margin_abs,
                                     p.margin_rel, p.min_range, p.max_range, n_scans, m->v.side, c);
  if (why != QTR_CARVE_OK) {
    snprintf(h->err, sizeof(h->err), "voxel map carve: %s (rows=%d cols=%d fov=[%g, %g] window=%d min_votes=%d of %d scans "
             "margins=%g, %g range=[%g, %g])", carve_refusal(why), p.rows, p.cols, p.fov_down_deg, p.fov_up_deg, p.window,
             p.min_votes, n_scans, p.margin_abs, p.margin_rel, p.min_range, p.max_range);
    return QTR_ERR_BAD_ARG;
  }
  return QTR_OK;
}

static int carve_check_pose(qtr_handle* h, const double* P, int k) {
  for (int j = 0; P && j < 12; ++j)
    if (!icp_finite(P[j])) {
      snprintf(h->err, sizeof(h->err), "voxel map carve: pose %d has a non-finite entry in rows 0 - 2", k);
      return QTR_ERR_BAD_ARG;
    }
  return QTR_OK;
}

// Everything a call with B scans allocates: the rebuild's staging for the map's voxels, the images and the byte array, on
// first need and grown only.  The entries call it before they enqueue anything, so a failed allocation leaves nothing in
// flight.
static int carve_reserve(qtr_handle* h, qtr_voxel_map* m, const QtrCarveCfg& c, int B, VmapStage* st) {
  QTR_TRY(vmap_keep_reserve(h, m, (size_t)m->info.n_voxels, st));
  const size_t need = kCarveHeadBytes + (size_t)B * c.rows * c.cols * 4;
  if (need > m->carve_img_bytes || !m->carve_img) {
    void* p = nullptr;
    QTR_HIP_TRY(h, hipMalloc(&p, need));
    if (m->carve_img) (void)hipFree(m->carve_img);
    m->carve_img = p;
    m->carve_img_bytes = need;
  }
  if (!m->carve_mark) QTR_HIP_TRY(h, hipMalloc((void**)&m->carve_mark, (size_t)m->v.mask + 1));
  return QTR_OK;
}

// The call on B device-resident scans whose arguments have all been checked and whose memory carve_reserve has made (st);
// poses12: B x 12 doubles (rows 0 - 2).
static int carve_device(qtr_handle* h, Slot& s, qtr_voxel_map* m, const CarveScans& sc, const double* poses12, int B,
                        const QtrCarveCfg& c, const VmapStage& st, qtr_voxel_map_carve_info* out) {
  qtr_voxel_map_carve_info info = {};
  const hipStream_t q = s.stream;
  double* d_poses = (double*)m->carve_img;
  unsigned* d_img = (unsigned*)((char*)m->carve_img + kCarveHeadBytes);
  const size_t img_bytes = (size_t)B * c.rows * c.cols * 4;
  int n_max = 0;
  for (int b = 0; b < B; ++b) n_max = std::max(n_max, sc.n[b]);
  const dim3 tgrid = vmap_keep_table_grid(m), blk(256);
  QTR_HIP_TRY(h, hipMemsetAsync(st.ctr, 0, VM_CTR_INTS * sizeof(int), q));
  QTR_HIP_TRY(h, hipMemsetAsync(d_img, 0xff, img_bytes, q));
  QTR_HIP_TRY(h, hipMemcpyAsync(d_poses, poses12, (size_t)B * 12 * sizeof(double), hipMemcpyHostToDevice, q));
  if (n_max > 0) hipLaunchKernelGGL(k_carve_image, dim3(qtr_div_up(n_max, 256), B), blk, 0, q, sc, c, d_img);
  hipLaunchKernelGGL(k_carve_mark, tgrid, blk, (size_t)B * 12 * sizeof(double), q, m->v, c, d_poses, B, d_img, m->carve_mark,
                     st.ctr);
  QTR_TRY(vmap_keep_read(h, m, st, q));  // (the wait: poses12 is the caller's until here)
  info.n_kept = m->pin[VK_CTR_KEPT];
  info.n_carved = m->pin[VK_CTR_EVICTED];
  info.n_tested = m->pin[CV_CTR_TESTED];
  memcpy(&info.n_members_carved, m->pin + VK_CTR_MEMBERS64, 8);
  QTR_TRY(vmap_keep_rebuild(h, m, st, q, "carve", info.n_kept, info.n_carved, info.n_members_carved, [&](dim3 grid, dim3 blk) {
    hipLaunchKernelGGL(k_carve_stage, grid, blk, 0, q, m->v, m->carve_mark, st, info.n_kept);
  }));
  if (out) *out = info;
  return QTR_OK;
}

int qtr_voxel_map_carve(qtr_handle* h, int slot, qtr_voxel_map* m, const float* xyz4, int n, const double pose[16],
                        const qtr_carve_params* prm, int mem, qtr_voxel_map_carve_info* out) {
  if (out) memset(out, 0, sizeof(*out));
  Slot* sp = get_slot(h, slot);
  if (!sp) return QTR_ERR_BAD_ARG;
  Slot& s = *sp;
  QTR_TRY(vmap_check(h, m));
  if (n < 0 || (n > 0 && !xyz4) || (mem != QTR_MEM_HOST && mem != QTR_MEM_DEVICE)) {
    snprintf(h->err, sizeof(h->err), "bad voxel map carve arguments (n=%d, a NULL cloud with n > 0, or mem=%d)", n, mem);
    return QTR_ERR_BAD_ARG;
  }
  QTR_TRY(carve_check_pose(h, pose, 0));
  QtrCarveCfg c;
  QTR_TRY(carve_cfg(h, m, prm, 1, &c));
  if (n > h->lim.max_points) {
    snprintf(h->err, sizeof(h->err), "voxel map carve: n=%d exceeds max_points=%d", n, h->lim.max_points);
    return QTR_ERR_CAPACITY;
  }
  if (m->info.n_voxels == 0) return QTR_OK;
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  VmapStage st;
  QTR_TRY(carve_reserve(h, m, c, 1, &st));
  CarveScans sc = {};
  sc.pts[0] = (const float4*)xyz4;
  sc.n[0] = n;
  if (mem == QTR_MEM_HOST && n > 0) {
    QTR_HIP_TRY(h, hipMemcpyAsync(s.in_src, xyz4, (size_t)n * 16, hipMemcpyHostToDevice, s.stream));
    sc.pts[0] = s.in_src;
  }
  double P[12];
  for (int k = 0; k < 12; ++k) P[k] = pose ? pose[k] : kIcpIdentity[k];
  return carve_device(h, s, m, sc, P, 1, c, st, out);
}

int qtr_voxel_map_carve_keyframes(qtr_handle* h, int slot, qtr_voxel_map* m, const qtr_keyframe* const* kfs, const double* poses,
                                  int n_kf, const qtr_carve_params* prm, qtr_voxel_map_carve_info* out) {
  if (out) memset(out, 0, sizeof(*out));
  Slot* sp = peek_slot(h, slot);
  if (!sp) return QTR_ERR_BAD_ARG;
  QTR_TRY(vmap_check(h, m));
  if (n_kf < 0 || n_kf > QTR_CARVE_MAX_KEYFRAMES || (n_kf > 0 && (!kfs || !poses))) {
    snprintf(h->err, sizeof(h->err), "voxel map carve: n_kf=%d keyframes (0 .. %d, with their poses)", n_kf, QTR_CARVE_MAX_KEYFRAMES);
    return QTR_ERR_BAD_ARG;
  }
  for (int k = 0; k < n_kf; ++k) {
    QTR_TRY(vmap_check_kf(h, kfs[k]));
    QTR_TRY(carve_check_pose(h, poses + 16 * (size_t)k, k));
  }
  QtrCarveCfg c;
  QTR_TRY(carve_cfg(h, m, prm, n_kf == 0 ? QTR_CARVE_MAX_KEYFRAMES : n_kf, &c));  // (no scan: only the fixed limits are judged)
  if (n_kf == 0 || m->info.n_voxels == 0) return QTR_OK;
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  VmapStage st;
  QTR_TRY(carve_reserve(h, m, c, n_kf, &st));
  CarveScans sc = {};
  std::vector<double> P((size_t)n_kf * 12);
  for (int k = 0; k < n_kf; ++k) {
    const VmapKfCloud kc = vmap_kf_cloud(kfs[k]);
    sc.pts[k] = kc.pts;
    sc.n[k] = kc.n;
    for (int j = 0; j < 12; ++j) P[(size_t)k * 12 + j] = poses[16 * (size_t)k + j];
  }
  return carve_device(h, *sp, m, sc, P.data(), n_kf, c, st, out);
}
