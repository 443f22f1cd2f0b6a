// voxelmap.hip — the persistent Gaussian voxel map (qtr_voxel_map_*, include/quatro_voxelmap.h): one record per voxel of a world-anchored grid, kept in
// HBM between calls.  Clouds and keyframes are inserted under poses, scans are registered against it with the VGICP
// iteration of icp.hip, and the voxel means come back as the map cloud.  The arithmetic is include/qtr_vmap_math.h.
//
// The entry points are exports of the extension library, libquatro_ext.so: the object of unity.hip that libquatro_hip.so is
// linked from, linked once more with exports_ext.map, so that it shares every structure of the handle with libquatro_hip.so,
// whose own symbol table (exports.map) stays the C ABI of include/quatro_hip.h.  A handle made by the product library is
// used by the extension library: both run the same code on the same HIP runtime, and no extension entry point touches a file-scope variable of capi.hip or solver.hip (each
// library has its own copy of g_handle_uid and t_hca_share; only the product library's are ever used).
//
// Table: open addressing with linear probing over S slots (a power of two >= 2 x capacity), 64-bit keys, QTR_VMAP_EMPTY for
// a free slot.  Everything a voxel owns lives at its slot: member count, the raw sums acc[9] and the FINISHED record
// (qtr_icp_voxel_finish, stored beside acc: a lookup is then one record load, as in method 3, instead of nine loads, six
// divisions and the finish per source point and iteration; the bits are the same either way).  Which slot a key lands in
// differs from run to run; nothing that leaves this file depends on it (fetches are in ascending key order).
//
// Insert of n points (the chain of method 3's build with a dense id per TOUCHED voxel in place of the cell number):
//   k_vmap_claim   member test, key, find-or-claim the slot with the returning 64-bit atomicCAS (agent scope: a probe sees
//                  other CUs' claims), rank among the call's members of that slot (atomic, order free)
//   k_vmap_assign  the rank-0 member of every touched slot takes a dense id d, notes the slot and its member count, and
//                  zeroes the slot's rank counter again
//   (host)         reads four counters back; more voxels than capacity: k_vmap_rollback frees the slots this call claimed
//                  (they still have n = 0, and with linear probing a key claimed by this call is never on the probe path of
//                  an older key) and the call returns QTR_ERR_CAPACITY with the map as it was
//   scan           exclusive_scan_i32 over the <= n dense ids
//   k_vmap_place   member i -> list[start[d] + rank]
//   k_vmap_order   its rank by ascending point index among the members of d (a count over the voxel's list)
//   k_vmap_fold    one thread per touched voxel: continues the stored acc over its members in ascending index, stores acc,
//                  the count and the finished record
// No kernel waits for another workgroup, none is launched cooperatively, all stores are plain vector stores.
//
// Registration: k_vmap_iter states only where its terms come from, the hash lookup in place of method 3's dense cell table,
// between the iteration frame of icp.hip (icp_iter_begin / icp_iter_finish: the stop flag's early return, T, the reduction
// tail, the step, the trace row, the ticket); the host side is capi.hip's icp_loop on the slot's IcpBufs with the empty grid
// and this kernel as its launch.  Lookups are plain loads: the table was written by earlier launches.
#include "../../include/quatro_voxelmap.h"
#include "../../include/qtr_vmap_math.h"

struct VmapView {
  u64* keys;          // [S]
  int* cnt;           // [S] members (0 with a key: claimed by an insert that has not folded yet)
  double* acc;        // [S][9]
  QtrIcpVoxel* rec;   // [S]
  u64 mask;           // S - 1
  double side;
};

enum { VM_CTR_MEMBERS = 0, VM_CTR_NEW, VM_CTR_TOUCHED, VM_CTR_OVERFLOW, VM_CTR_INTS = 16 };

struct VmapIns {
  const float4* pts;
  const float4* nrm;
  int n;
  double P[12];
  int* slot_of;   // [n] slot of member i (-1: not a member)
  int* rank;      // [n] atomic rank among the call's members of that slot
  int* tcnt;      // [S] the rank counters (zero between calls)
  int* did;       // [S] dense id of a touched slot (valid for the slots this call touched)
  int* dcnt;      // [n + 1] members per dense id
  int* dstart;    // [n + 1] its exclusive scan
  int* dslot;     // [n] slot of a dense id
  int* list;      // [n] members by dense id, atomic-rank order
  int* ord;       // [n] ... in ascending point index
  int* ctr;       // [VM_CTR_INTS]
};

__device__ __forceinline__ bool d_vmap_member(const VmapView& m, const VmapIns& a, int i, double* X, double* w, u64* key) {
  const float4 p = a.pts[i];
  const float4 b = a.nrm[i];
  double P[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) P[k] = a.P[k];
  return qtr_vmap_member(P, p.x, p.y, p.z, b.x, b.y, b.z, m.side, X, w, key);
}

__global__ __launch_bounds__(256) void k_vmap_claim(VmapView m, VmapIns a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  double X[3], w[3];
  u64 key = 0;
  if (!d_vmap_member(m, a, i, X, w, &key)) {
    a.slot_of[i] = -1;
    return;
  }
  u64 s = qtr_vmap_hash(key, m.mask);
  bool found = false;
  for (u64 probe = 0; probe <= m.mask; ++probe) {
    const u64 old = atomicCAS(m.keys + s, (u64)QTR_VMAP_EMPTY, key);  // (the returning CAS is the probe)
    if (old == QTR_VMAP_EMPTY) {
      atomicAdd(a.ctr + VM_CTR_NEW, 1);
      found = true;
      break;
    }
    if (old == key) {
      found = true;
      break;
    }
    s = (s + 1) & m.mask;
  }
  if (!found) {  // every slot holds another key: more voxels than slots, the call is refused
    atomicOr(a.ctr + VM_CTR_OVERFLOW, 1);
    a.slot_of[i] = -1;
    return;
  }
  a.slot_of[i] = (int)s;
  a.rank[i] = atomicAdd(a.tcnt + s, 1);
  atomicAdd(a.ctr + VM_CTR_MEMBERS, 1);
}

__global__ __launch_bounds__(256) void k_vmap_assign(VmapView m, VmapIns a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const int s = a.slot_of[i];
  if (s < 0 || a.rank[i] != 0) return;
  const int d = atomicAdd(a.ctr + VM_CTR_TOUCHED, 1);
  a.did[s] = d;
  a.dcnt[d] = a.tcnt[s];
  a.dslot[d] = s;
  a.tcnt[s] = 0;
}

// a refused insert: the slots it claimed (a key and still no member) are free again
__global__ __launch_bounds__(256) void k_vmap_rollback(VmapView m, VmapIns a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const int s = a.slot_of[i];
  if (s < 0 || a.rank[i] != 0) return;
  if (m.cnt[s] == 0) m.keys[s] = QTR_VMAP_EMPTY;
}

__global__ __launch_bounds__(256) void k_vmap_place(VmapIns a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const int s = a.slot_of[i];
  if (s < 0) return;
  a.list[a.dstart[a.did[s]] + a.rank[i]] = i;
}

__global__ __launch_bounds__(256) void k_vmap_order(VmapIns a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const int s = a.slot_of[i];
  if (s < 0) return;
  const int d = a.did[s];
  const int b = a.dstart[d], e = a.dstart[d + 1];
  int r = 0;
  for (int j = b; j < e; ++j) r += a.list[j] < i ? 1 : 0;
  a.ord[b + r] = i;
}

__global__ __launch_bounds__(256) void k_vmap_fold(VmapView m, VmapIns a, int n_touched) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= n_touched) return;
  const int s = a.dslot[d];
  const int b = a.dstart[d], e = a.dstart[d + 1];
  int n = m.cnt[s];
  double acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = n > 0 ? m.acc[(size_t)s * 9 + k] : 0.0;
  for (int r = b; r < e; ++r) {
    double X[3], w[3];
    u64 key;
    if (!d_vmap_member(m, a, a.ord[r], X, w, &key)) continue;  // (never: the list holds members)
    qtr_vmap_add(acc, X, w);
    ++n;
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) m.acc[(size_t)s * 9 + k] = acc[k];
  m.cnt[s] = n;
  QtrIcpVoxel vx;
  qtr_icp_voxel_finish(acc, n, 0, &vx);
  m.rec[s] = vx;
}

// the slot of a key written by an earlier launch (-1: no such voxel)
__device__ __forceinline__ long long d_vmap_find(const VmapView& m, u64 key) {
  u64 s = qtr_vmap_hash(key, m.mask);
  for (u64 probe = 0; probe <= m.mask; ++probe) {
    const u64 k = m.keys[s];
    if (k == key) return (long long)s;
    if (k == QTR_VMAP_EMPTY) return -1;
    s = (s + 1) & m.mask;
  }
  return -1;
}

// One workgroup (chunk `blk` of `nblk`) of one iteration of a registration against the map: d_icp_iter<3>'s frame around the
// hash lookup.  Shared by k_vmap_iter and the grouped k_vmap_iter_group (voxelmap_batch.hip).
__device__ __forceinline__ void d_vmap_iter(const IcpView& v, const VmapView& m, int blk, int nblk) {
  double T[16], o[QTR_ICP_NT];
  if (!icp_iter_begin(v, T, o)) return;
  const int i = blk * QTR_ICP_CHUNK + threadIdx.x;
  if (i < v.ns) {
    const float4 p = v.src[i];
    const float4 a = v.src_nrm[i];
    double q[3];
    u64 key = 0;
    int best = -1;
    if (qtr_vmap_query(T, p.x, p.y, p.z, a.x, a.y, a.z, m.side, q, &key)) {
      const long long s = d_vmap_find(m, key);
      if (s >= 0) {
        const QtrIcpVoxel vx = m.rec[s];
        if (m.cnt[s] > 0 && vx.n > 0) {
          best = 0;
          qtr_icp_vgicp_terms(T, q, a.x, a.y, a.z, &vx, o);
        }
      }
    }
    v.corr[i] = best;
  }
  icp_iter_finish<QTR_ICP_T_W + 1>(v, o, blk, nblk);
}

__global__ __launch_bounds__(256) void k_vmap_iter(IcpView v, VmapView m) { d_vmap_iter(v, m, (int)blockIdx.x, (int)gridDim.x); }

// a fetch section of the voxels at slots[0 .. n), in that order
__global__ __launch_bounds__(256) void k_vmap_gather(VmapView m, const int* __restrict__ slots, int n, int what, void* out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int s = slots[j];
  if (what == QTR_VMAP_SUMS) {
    for (int k = 0; k < 9; ++k) ((double*)out)[(size_t)j * 9 + k] = m.acc[(size_t)s * 9 + k];
  } else if (what == QTR_VMAP_RECORDS) {
    const QtrIcpVoxel vx = m.rec[s];
    for (int k = 0; k < 3; ++k) ((double*)out)[(size_t)j * 9 + k] = vx.mu[k];
    for (int k = 0; k < 6; ++k) ((double*)out)[(size_t)j * 9 + 3 + k] = vx.C[k];
  } else {  // QTR_VMAP_CLOUD
    const QtrIcpVoxel vx = m.rec[s];
    ((float4*)out)[j] = make_float4((float)vx.mu[0], (float)vx.mu[1], (float)vx.mu[2], (float)vx.n);
  }
}

__global__ __launch_bounds__(256) void k_vmap_clear(VmapView m, int* tcnt) {
  for (u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x; e <= m.mask; e += (u64)gridDim.x * blockDim.x) {
    m.keys[e] = QTR_VMAP_EMPTY;
    m.cnt[e] = 0;
    tcnt[e] = 0;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------
struct qtr_voxel_map {
  qtr_handle* owner = nullptr;
  void* table = nullptr;    // keys, cnt, acc, rec, tcnt, did
  void* scratch = nullptr;  // the insert's per-point arrays (max_points points), allocated on the first insert
  int* pin = nullptr;       // pinned: the counters' read-back
  void* stage = nullptr;    // evict / restore staging for stage_cap voxels (voxelmap_keep.hip), allocated on first need
  size_t stage_cap = 0;
  void* carve_img = nullptr;  // visibility carving (voxelmap_carve.hip): the call's poses and range images, allocated on first need
  size_t carve_img_bytes = 0;
  unsigned char* carve_mark = nullptr;  // ... and its verdict, one byte per table slot
  VmapView v{};
  VmapIns ins{};
  hipStream_t stream = nullptr;  // clear and fetch, which take no slot
  qtr_voxel_map_info info = {};
};

// rows 0 - 2 of an entry's (verb: "insert" / "register") pose or guess (noun); null: the identity
static int vmap_check_pose(qtr_handle* h, const char* verb, const char* noun, const double* P) {
  for (int k = 0; P && k < 12; ++k)
    if (!icp_finite(P[k])) {
      snprintf(h->err, sizeof(h->err), "voxel map %s: the %s has a non-finite entry in rows 0 - 2", verb, noun);
      return QTR_ERR_BAD_ARG;
    }
  return QTR_OK;
}

static int vmap_check(qtr_handle* h, const qtr_voxel_map* m) {
  if (!m) {
    snprintf(h->err, sizeof(h->err), "voxel map is NULL");
    return QTR_ERR_BAD_ARG;
  }
  if (m->owner != h) {
    snprintf(h->err, sizeof(h->err), "voxel map belongs to another handle");
    return QTR_ERR_BAD_ARG;
  }
  return QTR_OK;
}

static int vmap_check_kf(qtr_handle* h, const qtr_keyframe* kf) {
  if (!kf) {
    snprintf(h->err, sizeof(h->err), "keyframe is NULL");
    return QTR_ERR_BAD_ARG;
  }
  if (kf->owner != h) {
    snprintf(h->err, sizeof(h->err), "keyframe belongs to another handle");
    return QTR_ERR_BAD_ARG;
  }
  return QTR_OK;
}

// a keyframe as the map's entries read it, in place: its voxel centroids, their normals, their number
struct VmapKfCloud {
  const float4 *pts, *nrm;
  int n;
};
static VmapKfCloud vmap_kf_cloud(const qtr_keyframe* kf) {
  const KfLayout lay = kf_layout(kf->info.n_voxels);
  return {(const float4*)((const char*)kf->dev + lay.vox), (const float4*)((const char*)kf->dev + lay.normals), kf->info.n_voxels};
}

static void vmap_release(qtr_voxel_map* m) {
  if (m->stream) {
    (void)hipStreamSynchronize(m->stream);
    (void)hipStreamDestroy(m->stream);
  }
  if (m->table) (void)hipFree(m->table);
  if (m->scratch) (void)hipFree(m->scratch);
  if (m->stage) (void)hipFree(m->stage);
  if (m->carve_img) (void)hipFree(m->carve_img);
  if (m->carve_mark) (void)hipFree(m->carve_mark);
  if (m->pin) (void)hipHostFree(m->pin);
  delete m;
}

// the maps the caller did not destroy (qtr_destroy)
static void vmap_free_all(qtr_handle* h) {
  for (qtr_voxel_map* m : h->voxel_maps) vmap_release(m);
  h->voxel_maps.clear();
}

void qtr_default_voxel_map_params(qtr_voxel_map_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->voxel_size = 1.0;
  p->capacity = 1 << 20;
}

int qtr_voxel_map_create(qtr_handle* h, const qtr_voxel_map_params* params, qtr_voxel_map** out) {
  if (out) *out = nullptr;
  if (!h || !out) return QTR_ERR_BAD_ARG;
  qtr_voxel_map_params prm;
  qtr_default_voxel_map_params(&prm);
  if (params) prm = *params;
  if (!icp_finite(prm.voxel_size) || !(prm.voxel_size > 0)) {
    snprintf(h->err, sizeof(h->err), "voxel map: voxel_size %g must be finite and positive", prm.voxel_size);
    return QTR_ERR_BAD_ARG;
  }
  if (prm.capacity < 1 || prm.capacity > QTR_VMAP_MAX_CAPACITY) {
    snprintf(h->err, sizeof(h->err), "voxel map: capacity %d (1 .. %d)", prm.capacity, QTR_VMAP_MAX_CAPACITY);
    return QTR_ERR_BAD_ARG;
  }
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  size_t S = 64;
  while (S < (size_t)2 * (size_t)prm.capacity) S <<= 1;
  qtr_voxel_map* m = new (std::nothrow) qtr_voxel_map();
  if (!m) return QTR_ERR_CAPACITY;
  const size_t rec_bytes = qtr_up256(S * sizeof(QtrIcpVoxel));
  const size_t bytes = S * 8 + S * 72 + rec_bytes + 3 * S * 4 + 1024;
  hipError_t e = hipMalloc(&m->table, bytes);
  if (e == hipSuccess) e = hipHostMalloc((void**)&m->pin, VM_CTR_INTS * sizeof(int));
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
  if (e == hipSuccess) {
    char* p = (char*)m->table;
    m->v.keys = (u64*)p;
    p += S * 8;
    m->v.acc = (double*)p;
    p += S * 72;
    m->v.rec = (QtrIcpVoxel*)p;
    p += rec_bytes;
    m->v.cnt = (int*)p;
    p += S * 4;
    m->ins.tcnt = (int*)p;
    p += S * 4;
    m->ins.did = (int*)p;
    m->v.mask = (u64)S - 1;
    m->v.side = prm.voxel_size;
    hipLaunchKernelGGL(k_vmap_clear, dim3(std::min(qtr_div_up((long long)S, 256), 2048)), dim3(256), 0, m->stream, m->v, m->ins.tcnt);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    snprintf(h->err, sizeof(h->err), "voxel map: %zu bytes for %d voxels: %s", bytes, prm.capacity, hipGetErrorString(e));
    vmap_release(m);
    return QTR_ERR_HIP;
  }
  m->owner = h;
  m->info.voxel_size = prm.voxel_size;
  m->info.capacity = prm.capacity;
  {
    std::lock_guard<std::mutex> lk(h->kf_mu);
    h->voxel_maps.push_back(m);
  }
  *out = m;
  return QTR_OK;
}

void qtr_voxel_map_destroy(qtr_handle* h, qtr_voxel_map* m) {
  if (!h || !m || m->owner != h) return;
  {
    std::lock_guard<std::mutex> lk(h->kf_mu);
    auto it = std::find(h->voxel_maps.begin(), h->voxel_maps.end(), m);
    if (it == h->voxel_maps.end()) return;
    h->voxel_maps.erase(it);
  }
  (void)hipSetDevice(h->device);
  vmap_release(m);
}

int qtr_voxel_map_clear(qtr_handle* h, int slot, qtr_voxel_map* m) {
  Slot* sp = peek_slot(h, slot);
  if (!sp) return QTR_ERR_BAD_ARG;
  QTR_TRY(vmap_check(h, m));
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  const size_t S = (size_t)m->v.mask + 1;
  hipLaunchKernelGGL(k_vmap_clear, dim3(std::min(qtr_div_up((long long)S, 256), 2048)), dim3(256), 0, sp->stream, m->v, m->ins.tcnt);
  QTR_HIP_TRY(h, hipGetLastError());
  QTR_HIP_TRY(h, hipStreamSynchronize(sp->stream));
  m->info.n_voxels = 0;
  m->info.n_inserts = 0;
  m->info.n_members = 0;
  return QTR_OK;
}

int qtr_voxel_map_get_info(const qtr_voxel_map* m, qtr_voxel_map_info* info) {
  if (!m || !info) return QTR_ERR_BAD_ARG;
  *info = m->info;
  return QTR_OK;
}

static int vmap_scratch(qtr_handle* h, qtr_voxel_map* m) {
  if (m->scratch) return QTR_OK;
  const size_t np = ((size_t)h->lim.max_points + 64 + 63) & ~(size_t)63;
  QTR_HIP_TRY(h, hipMalloc(&m->scratch, 7 * np * 4 + VM_CTR_INTS * 4));
  int* p = (int*)m->scratch;
  m->ins.slot_of = p;
  m->ins.rank = p + np;
  m->ins.dcnt = p + 2 * np;
  m->ins.dstart = p + 3 * np;
  m->ins.dslot = p + 4 * np;
  m->ins.list = p + 5 * np;
  m->ins.ord = p + 6 * np;
  m->ins.ctr = p + 7 * np;
  return QTR_OK;
}

// the insert of n device-resident points with their normals
static int vmap_insert_device(qtr_handle* h, Slot& s, qtr_voxel_map* m, const float4* d_pts, const float4* d_nrm, int n,
                              const double* pose, qtr_voxel_map_insert_info* out) {
  qtr_voxel_map_insert_info info = {};
  info.n_points = n;
  if (n > 0) {
    QTR_TRY(vmap_scratch(h, m));
    VmapIns& a = m->ins;
    a.pts = d_pts;
    a.nrm = d_nrm;
    a.n = n;
    for (int k = 0; k < 12; ++k) a.P[k] = pose ? pose[k] : kIcpIdentity[k];
    const hipStream_t st = s.stream;
    const dim3 grid(qtr_div_up(n, 256)), blk(256);
    QTR_HIP_TRY(h, hipMemsetAsync(a.ctr, 0, VM_CTR_INTS * sizeof(int), st));
    hipLaunchKernelGGL(k_vmap_claim, grid, blk, 0, st, m->v, a);
    hipLaunchKernelGGL(k_vmap_assign, grid, blk, 0, st, m->v, a);
    QTR_HIP_TRY(h, hipGetLastError());
    QTR_HIP_TRY(h, hipMemcpyAsync(m->pin, a.ctr, VM_CTR_INTS * sizeof(int), hipMemcpyDeviceToHost, st));
    QTR_HIP_TRY(h, hipStreamSynchronize(st));
    const int n_new = m->pin[VM_CTR_NEW], n_touched = m->pin[VM_CTR_TOUCHED];
    if (m->pin[VM_CTR_OVERFLOW] || (long long)m->info.n_voxels + n_new > (long long)m->info.capacity) {
      hipLaunchKernelGGL(k_vmap_rollback, grid, blk, 0, st, m->v, a);
      QTR_HIP_TRY(h, hipGetLastError());
      QTR_HIP_TRY(h, hipStreamSynchronize(st));
      if (m->pin[VM_CTR_OVERFLOW])
        snprintf(h->err, sizeof(h->err), "voxel map: the insert needs more than %d new voxels on top of %d, which exceeds capacity=%d",
                 n_new, m->info.n_voxels, m->info.capacity);
      else
        snprintf(h->err, sizeof(h->err), "voxel map: the insert needs %d new voxels on top of %d, which exceeds capacity=%d", n_new,
                 m->info.n_voxels, m->info.capacity);
      return QTR_ERR_CAPACITY;
    }
    if (n_touched > 0) {
      QTR_HIP_TRY(h, exclusive_scan_i32(a.dcnt, a.dstart, n_touched, st));
      hipLaunchKernelGGL(k_vmap_place, grid, blk, 0, st, a);
      hipLaunchKernelGGL(k_vmap_order, grid, blk, 0, st, a);
      hipLaunchKernelGGL(k_vmap_fold, dim3(qtr_div_up(n_touched, 256)), blk, 0, st, m->v, a, n_touched);
      QTR_HIP_TRY(h, hipGetLastError());
      QTR_HIP_TRY(h, hipStreamSynchronize(st));
    }
    info.n_members = m->pin[VM_CTR_MEMBERS];
    info.n_new_voxels = n_new;
    info.n_touched_voxels = n_touched;
    m->info.n_voxels += n_new;
    m->info.n_members += info.n_members;
  }
  m->info.n_inserts += 1;
  if (out) *out = info;
  return QTR_OK;
}

// The check of a cloud given by pointers, for every entry that takes one, in the entry's own words (verb: "insert" /
// "register" / "evaluate"; nrm_name: its normals' argument; pose: the insert's, null where a guess or pose is checked apart).
static int vmap_check_cloud(qtr_handle* h, const char* verb, const char* nrm_name, const double* pose, int mem, int n,
                            const void* pts, const void* nrm) {
  if (n < 0 || (n > 0 && !pts) || (mem != QTR_MEM_HOST && mem != QTR_MEM_DEVICE)) {
    snprintf(h->err, sizeof(h->err), "bad voxel map %s arguments", verb);
    return QTR_ERR_BAD_ARG;
  }
  if (!nrm) {
    snprintf(h->err, sizeof(h->err), "voxel map %s: %s is NULL (the cloud entries do not compute normals)", verb, nrm_name);
    return QTR_ERR_BAD_ARG;
  }
  QTR_TRY(vmap_check_pose(h, verb, "pose", pose));
  if (n > h->lim.max_points) {
    snprintf(h->err, sizeof(h->err), "voxel map %s: n=%d exceeds max_points=%d", verb, n, h->lim.max_points);
    return QTR_ERR_CAPACITY;
  }
  return QTR_OK;
}

// What the two cloud entries do with their cloud before anything runs: vmap_check_cloud, then a host cloud and its normals
// into in_src / in_tgt.  pts / nrm come back as device pointers.
static int vmap_stage(qtr_handle* h, Slot& s, const char* verb, const char* nrm_name, const double* pose, int mem, int n,
                      const float4** pts, const float4** nrm) {
  QTR_TRY(vmap_check_cloud(h, verb, nrm_name, pose, mem, n, *pts, *nrm));
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  if (mem == QTR_MEM_HOST && n > 0) {
    QTR_HIP_TRY(h, hipMemcpyAsync(s.in_src, *pts, (size_t)n * 16, hipMemcpyHostToDevice, s.stream));
    QTR_HIP_TRY(h, hipMemcpyAsync(s.in_tgt, *nrm, (size_t)n * 16, hipMemcpyHostToDevice, s.stream));
    *pts = s.in_src;
    *nrm = s.in_tgt;
  }
  return QTR_OK;
}

int qtr_voxel_map_insert(qtr_handle* h, int slot, qtr_voxel_map* m, const float* xyz4, const float* normals4, int n,
                         const double pose[16], int mem, qtr_voxel_map_insert_info* out) {
  if (out) memset(out, 0, sizeof(*out));
  Slot* sp = get_slot(h, slot);
  if (!sp) return QTR_ERR_BAD_ARG;
  Slot& s = *sp;
  QTR_TRY(vmap_check(h, m));
  const float4 *d_pts = (const float4*)xyz4, *d_nrm = (const float4*)normals4;
  QTR_TRY(vmap_stage(h, s, "insert", "normals4", pose, mem, n, &d_pts, &d_nrm));
  return vmap_insert_device(h, s, m, d_pts, d_nrm, n, pose, out);
}

int qtr_voxel_map_insert_keyframe(qtr_handle* h, int slot, qtr_voxel_map* m, const qtr_keyframe* kf, const double pose[16],
                                  qtr_voxel_map_insert_info* out) {
  if (out) memset(out, 0, sizeof(*out));
  Slot* sp = get_slot(h, slot);
  if (!sp) return QTR_ERR_BAD_ARG;
  QTR_TRY(vmap_check(h, m));
  QTR_TRY(vmap_check_kf(h, kf));
  QTR_TRY(vmap_check_pose(h, "insert", "pose", pose));
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  const VmapKfCloud c = vmap_kf_cloud(kf);
  return vmap_insert_device(h, *sp, m, c.pts, c.nrm, c.n, pose, out);
}

// the registration of ns device-resident points with their normals: icp_loop (capi.hip) with the empty grid, only the
// state's initialisation before the loop, and `launch` (st, chunks, view) as its launch: k_vmap_iter, or the continuous-time
// iteration of voxelmap_ct.hip
template <class Launch>
static int vmap_register_loop(qtr_handle* h, Slot& s, const qtr_voxel_map* m, const float4* d_src, int ns, const float4* d_nrm,
                              const double* guess, const qtr_icp_params* prm, qtr_icp_result* res, Launch launch) {
  const hipStream_t st = s.stream;
  IcpView& v = s.icp.v;
  const auto bind = [&]() -> int {
    QTR_HIP_TRY(h, icp_reserve(s.icp, std::max(h->lim.max_voxels, h->lim.max_points), QTR_ICP_MAX_ITERATIONS));
    icp_view_bind(v, prm, d_src, ns, d_nrm, nullptr, 0, nullptr);
    v.ncell = v.dims[0] = v.dims[1] = v.dims[2] = 0;
    v.cfg.max_d2 = m->v.side * m->v.side;  // (not read: the side is the map's)
    return QTR_OK;
  };
  const auto before = [&](bool*) -> int {
    QtrIcpState st0;
    qtr_icp_init(&st0, guess);
    hipLaunchKernelGGL(k_icp_init, dim3(1), dim3(64), 0, st, v, st0);
    QTR_HIP_TRY(h, hipGetLastError());
    return QTR_OK;
  };
  const dim3 chunks(qtr_div_up(ns, QTR_ICP_CHUNK));
  return icp_loop(h, s, ns, ns == 0, guess, prm, res, bind, before, [&](const IcpView& w) { launch(st, chunks, w); });
}

static int vmap_register_device(qtr_handle* h, Slot& s, const qtr_voxel_map* m, const float4* d_src, int ns,
                                const float4* d_nrm, const double* guess, const qtr_icp_params* prm, qtr_icp_result* res) {
  return vmap_register_loop(h, s, m, d_src, ns, d_nrm, guess, prm, res, [&](hipStream_t st, dim3 chunks, const IcpView& w) {
    hipLaunchKernelGGL(k_vmap_iter, chunks, dim3(256), 0, st, w, m->v);
  });
}

static int vmap_check_register(qtr_handle* h, const qtr_voxel_map* m, const double* guess, const qtr_icp_params* prm) {
  QTR_TRY(vmap_check(h, m));
  QTR_TRY(check_icp_params(h, prm));
  if (prm->method != QTR_ICP_VOXEL_PLANE_TO_PLANE) {
    snprintf(h->err, sizeof(h->err), "voxel map register: method must be QTR_ICP_VOXEL_PLANE_TO_PLANE");
    return QTR_ERR_BAD_ARG;
  }
  return vmap_check_pose(h, "register", "guess", guess);
}

// the guess as the state takes it: rows 0 - 2 the caller's, row 3 (0 0 0 1)
static void vmap_guess(const double* guess, double* g) {
  for (int k = 0; k < 16; ++k) g[k] = kIcpIdentity[k];
  if (guess)
    for (int k = 0; k < 12; ++k) g[k] = guess[k];
}

int qtr_voxel_map_register(qtr_handle* h, int slot, const qtr_voxel_map* m, const float* src4, int n, const float* src_normals4,
                           const double guess[16], const qtr_icp_params* prm, qtr_icp_result* res, int mem) {
  Slot* sp = get_slot(h, slot);
  if (!sp || !res) return QTR_ERR_BAD_ARG;
  memset(res, 0, sizeof(*res));
  Slot& s = *sp;
  int rc = vmap_check_register(h, m, guess, prm);
  if (rc != QTR_OK) return res->status = rc;
  const float4 *d_src = (const float4*)src4, *d_nrm = (const float4*)src_normals4;
  rc = vmap_stage(h, s, "register", "src_normals4", nullptr, mem, n, &d_src, &d_nrm);
  if (rc != QTR_OK) return res->status = rc;
  double g[16];
  vmap_guess(guess, g);
  return res->status = vmap_register_device(h, s, m, d_src, n, d_nrm, g, prm, res);
}

int qtr_voxel_map_register_keyframe(qtr_handle* h, int slot, const qtr_voxel_map* m, const qtr_keyframe* kf,
                                    const double guess[16], const qtr_icp_params* prm, qtr_icp_result* res) {
  Slot* sp = get_slot(h, slot);
  if (!sp || !res) return QTR_ERR_BAD_ARG;
  memset(res, 0, sizeof(*res));
  int rc = vmap_check_register(h, m, guess, prm);
  if (rc == QTR_OK) rc = vmap_check_kf(h, kf);
  if (rc != QTR_OK) return res->status = rc;
  rc = [&]() -> int {
    QTR_HIP_TRY(h, hipSetDevice(h->device));
    const VmapKfCloud c = vmap_kf_cloud(kf);
    double g[16];
    vmap_guess(guess, g);
    return vmap_register_device(h, *sp, m, c.pts, c.n, c.nrm, g, prm, res);
  }();
  return res->status = rc;
}

long long qtr_voxel_map_fetch(qtr_handle* h, const qtr_voxel_map* m, int what, void* dst, size_t bytes) {
  if (!h || !m || m->owner != h) return -1;
  size_t per = 0;
  switch (what) {
    case QTR_VMAP_COORDS: per = 12; break;
    case QTR_VMAP_COUNT: per = 4; break;
    case QTR_VMAP_SUMS:
    case QTR_VMAP_RECORDS: per = 72; break;
    case QTR_VMAP_CLOUD: per = 16; break;
    default: return -1;
  }
  const size_t nv = (size_t)m->info.n_voxels, have = nv * per;
  const size_t want = have < bytes ? have : bytes;
  if (!dst || want == 0) return (long long)have;
  if (hipSetDevice(h->device) != hipSuccess) return -1;
  // the occupied slots in ascending key order (sorted on the host: not a hot path)
  const size_t S = (size_t)m->v.mask + 1;
  std::vector<u64> keys(S);
  std::vector<int> cnt(S);
  if (hipMemcpy(keys.data(), m->v.keys, S * 8, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (hipMemcpy(cnt.data(), m->v.cnt, S * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  std::vector<int> slots;
  slots.reserve(nv);
  for (size_t s = 0; s < S; ++s)
    if (keys[s] != QTR_VMAP_EMPTY && cnt[s] > 0) slots.push_back((int)s);
  std::sort(slots.begin(), slots.end(), [&](int a, int b) { return keys[a] < keys[b]; });
  if (slots.size() != nv) return -1;
  std::vector<char> out(have);
  if (what == QTR_VMAP_COORDS) {
    for (size_t j = 0; j < nv; ++j) qtr_vmap_key_coords(keys[slots[j]], (int*)out.data() + 3 * j);
  } else if (what == QTR_VMAP_COUNT) {
    for (size_t j = 0; j < nv; ++j) ((int*)out.data())[j] = cnt[slots[j]];
  } else {
    void* d = nullptr;
    if (hipMalloc(&d, have + nv * 4) != hipSuccess) return -1;
    int* d_slots = (int*)((char*)d + have);
    bool ok = hipMemcpy(d_slots, slots.data(), nv * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
      hipLaunchKernelGGL(k_vmap_gather, dim3(qtr_div_up((long long)nv, 256)), dim3(256), 0, m->stream, m->v, d_slots, (int)nv,
                         what, d);
      ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(m->stream) == hipSuccess &&
           hipMemcpy(out.data(), d, have, hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(d);
    if (!ok) return -1;
  }
  memcpy(dst, out.data(), want);
  return (long long)have;
}
