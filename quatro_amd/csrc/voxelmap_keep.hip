// voxelmap_keep.hip — upkeep of the persistent voxel map (voxelmap.hip): sliding-window eviction and restore from fetched
// sections (qtr_voxel_map_evict / qtr_voxel_map_restore, include/quatro_voxelmap_keep.h).  The contract is
// include/qtr_vmap_keep_math.h.
//
// The two entry points are exports of the extension library, libquatro_ext.so (voxelmap.hip says how it is built);
// libquatro_hip.so carries this code hidden and exports none of it.
//
// The table is open addressing with linear probing and d_vmap_find stops at the first empty slot, so a voxel is never
// deleted in place: a hole would cut every probe chain that runs through it.  Both entries end in the same device path
// instead, "put a list of finished voxels into a clean table":
//   k_vmap_keep_put    one thread per staged voxel (key, count, acc[9], and for evict the stored record) claims its slot
//                      with the returning 64-bit atomicCAS at agent scope — k_vmap_claim's probe — and writes count, acc
//                      and the record with plain stores; a null record list means qtr_icp_voxel_finish here (restore).
//                      old == key on the claim is the duplicate flag.  An empty key in the list is skipped.
// The table it leaves was built by claims alone: no tombstones, tcnt all zero (k_vmap_clear), and k_vmap_rollback's
// argument holds for the next insert as it does in a map that only ever grew.  d_vmap_find and k_vmap_iter are untouched.
//
// Evict (two phases around one host read-back, as insert reads its counters):
//   k_vmap_keep_mark   a pass over the S keys that only reads: the rule, counts of kept and evicted voxels and of evicted
//                      members (64-bit), summed per workgroup
//   (host)             nothing evicted: return, the table was only read.
//   (rebuild)          vmap_keep_rebuild, the end evict shares with carve (voxelmap_carve.hip): k_vmap_keep_stage — every
//                      survivor takes a staging index (a workgroup reserves its survivors' range with one atomic; the order
//                      is free) and its key, count, acc and record go to staging —, k_vmap_clear, k_vmap_keep_put.  The
//                      staging pass is d_vmap_stage_kept under the caller's verdict: the window here, carve's mark byte there.
// The staging index is given in phase two and not in phase one: the pass that usually ends the call then writes nothing
// and takes no atomic per voxel.
// Restore: the caller's arrays go to the staging buffer as they are (coords into the record area, which a restore does
// not use), k_vmap_keep_keys validates range and count and forms the keys (an empty key for a refused voxel), then
// k_vmap_keep_put with the finish in it; one read-back; any flag -> k_vmap_clear and the refusal.
//
// Staging: 164 bytes per voxel (key 8, acc 72, record 80, count 4) + 64 bytes of counters, allocated on first need for the
// map's n_voxels (evict) or n (restore), never for the table, and grown only.
// No kernel waits for another workgroup, none is launched cooperatively, all stores are plain vector stores.
#include "../../include/quatro_voxelmap_keep.h"
#include "../../include/qtr_vmap_keep_math.h"

struct VmapStage {
  u64* keys;         // [cap]
  double* acc;       // [cap][9]
  QtrIcpVoxel* rec;  // [cap] (evict); restore keeps its int coords[n][3] here and passes null to the put
  int* cnt;          // [cap]
  int* ctr;          // [VM_CTR_INTS]
};

// ctr: ints 0 - 3, one 64-bit count at ints 4 - 5, then the staging cursor
enum { VK_CTR_KEPT = 0, VK_CTR_EVICTED, VK_CTR_DUP, VK_CTR_BAD, VK_CTR_MEMBERS64 = 4, VK_CTR_STAGED = 6 };

// the member count of slot e if it holds a voxel the window keeps (*keep) or rejects, 0 for a slot without a voxel
__device__ __forceinline__ int d_vmap_keep_verdict(const VmapView& m, const QtrVmapWindow& w, u64 e, u64* key, bool* keep) {
  *keep = false;
  *key = m.keys[e];
  if (*key == QTR_VMAP_EMPTY) return 0;
  const int n = m.cnt[e];
  if (n <= 0) return 0;
  *keep = qtr_vmap_kept_key(&w, *key);
  return n;
}

// Phase one only reads the table.  The counts are summed per workgroup in LDS and leave it as three atomics: one atomic
// per survivor on one address took 0.27 ms of a 0.32 ms pass at 50 k voxels in 2^21 slots.
__global__ __launch_bounds__(256) void k_vmap_keep_mark(VmapView m, QtrVmapWindow w, int* ctr) {
  __shared__ int s_kept, s_gone;
  __shared__ u64 s_members;
  if (threadIdx.x == 0) {
    s_kept = 0;
    s_gone = 0;
    s_members = 0;
  }
  __syncthreads();
  int kept = 0, gone = 0;
  long long members = 0;
  for (u64 e = blockIdx.x * (u64)blockDim.x + threadIdx.x; e <= m.mask; e += (u64)gridDim.x * blockDim.x) {
    u64 key;
    bool keep;
    const int n = d_vmap_keep_verdict(m, w, e, &key, &keep);
    kept += (n > 0 && keep) ? 1 : 0;
    gone += (n > 0 && !keep) ? 1 : 0;
    members += keep ? 0 : n;
  }
  if (kept) atomicAdd(&s_kept, kept);
  if (gone) {
    atomicAdd(&s_gone, gone);
    atomicAdd(&s_members, (u64)members);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_kept) atomicAdd(ctr + VK_CTR_KEPT, s_kept);
    if (s_gone) {
      atomicAdd(ctr + VK_CTR_EVICTED, s_gone);
      atomicAdd((u64*)(ctr + VK_CTR_MEMBERS64), s_members);
    }
  }
}

// The staging pass of a rebuild: the survivors' key, count, acc and record into staging.  keep(e) is the verdict on slot e:
// the window here, the mark byte in voxelmap_carve.hip.  A workgroup counts the survivors among its slots, reserves that
// many staging indices with one atomic, and hands them out in a second pass over the same slots (a wave's ballot and a
// cursor in LDS: the order is free).  A thread walks the slots first, first + stride, ... (the kernel states its grid, as
// d_vmap_iter's callers do); S and the stride are multiples of the wave, so a wave is in the loop with all its lanes or with
// none.
template <class Keep>
__device__ __forceinline__ void d_vmap_stage_kept(const VmapView& m, const VmapStage& st, int n_kept, u64 first, u64 stride,
                                                  const Keep& keep) {
  __shared__ int s_n, s_base, s_cursor;
  if (threadIdx.x == 0) {
    s_n = 0;
    s_cursor = 0;
  }
  __syncthreads();
  int mine = 0;
  for (u64 e = first; e <= m.mask; e += stride) mine += keep(e) ? 1 : 0;
  if (mine) atomicAdd(&s_n, mine);
  __syncthreads();
  if (threadIdx.x == 0) s_base = s_n ? atomicAdd(st.ctr + VK_CTR_STAGED, s_n) : 0;
  __syncthreads();
  if (s_n == 0) return;
  const int base = s_base;
  for (u64 e = first; e <= m.mask; e += stride) {
    const bool kept = keep(e);
    const u64 bal = __ballot(kept);
    if (!bal) continue;  // (the whole wave)
    int at = 0;
    if (qk_lane() == 0) at = atomicAdd(&s_cursor, __popcll(bal));
    at = __shfl(at, 0, 64);
    const int j = base + at + __popcll(bal & lanemask_lt());
    if (kept && j >= 0 && j < n_kept) {  // (the bounds: never outside, the mark pass counted exactly these slots)
      st.keys[j] = m.keys[e];
      st.cnt[j] = m.cnt[e];
#pragma unroll
      for (int k = 0; k < 9; ++k) st.acc[(size_t)j * 9 + k] = m.acc[(size_t)e * 9 + k];
      st.rec[j] = m.rec[e];
    }
  }
}

// phase two of evict, first kernel: the window is the verdict, as in phase one
__global__ __launch_bounds__(256) void k_vmap_keep_stage(VmapView m, QtrVmapWindow w, VmapStage st, int n_kept) {
  d_vmap_stage_kept(m, st, n_kept, blockIdx.x * (u64)blockDim.x + threadIdx.x, (u64)gridDim.x * blockDim.x, [&](u64 e) {
    u64 key;
    bool keep;
    d_vmap_keep_verdict(m, w, e, &key, &keep);
    return keep;
  });
}

// restore: range and count of every voxel, its key (the empty key for a refused one), the sum of the counts
__global__ __launch_bounds__(256) void k_vmap_keep_keys(const int* __restrict__ coords, VmapStage st, int n) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  long long members = 0;
  if (j < n) {
    const int c[3] = {coords[3 * (size_t)j], coords[3 * (size_t)j + 1], coords[3 * (size_t)j + 2]};
    const int cnt = st.cnt[j];
    u64 key = QTR_VMAP_EMPTY;
    const int why = qtr_vmap_restore_key(c, cnt, &key);
    if (why != QTR_VMAP_RESTORE_OK) {
      atomicOr(st.ctr + VK_CTR_BAD, why);
      key = QTR_VMAP_EMPTY;
    } else {
      members = cnt;
    }
    st.keys[j] = key;
  }
  for (int o = 32; o > 0; o >>= 1) members += __shfl_down(members, o, 64);  // (the whole wave is here: no early return)
  if ((threadIdx.x & 63) == 0 && members) atomicAdd((u64*)(st.ctr + VK_CTR_MEMBERS64), (u64)members);
}

// the put path of both entries: n staged voxels into a table that holds none of them
__global__ __launch_bounds__(256) void k_vmap_keep_put(VmapView m, VmapStage st, int n) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const u64 key = st.keys[j];
  if (key == QTR_VMAP_EMPTY) return;
  u64 s = qtr_vmap_hash(key, m.mask);
  bool mine = false;
  for (u64 probe = 0; probe <= m.mask; ++probe) {
    const u64 old = atomicCAS(m.keys + s, (u64)QTR_VMAP_EMPTY, key);  // (the returning CAS is the probe)
    if (old == QTR_VMAP_EMPTY) {
      mine = true;
      break;
    }
    if (old == key) break;
    s = (s + 1) & m.mask;
  }
  if (!mine) {  // the key twice in the list (or, never with n <= capacity, no free slot)
    atomicOr(st.ctr + VK_CTR_DUP, 1);
    return;
  }
  const int cnt = st.cnt[j];
  double acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = st.acc[(size_t)j * 9 + k];
#pragma unroll
  for (int k = 0; k < 9; ++k) m.acc[(size_t)s * 9 + k] = acc[k];
  m.cnt[s] = cnt;
  QtrIcpVoxel vx;
  if (st.rec)
    vx = st.rec[j];
  else
    qtr_icp_voxel_finish(acc, cnt, 0, &vx);
  m.rec[s] = vx;
}

// ---- host side ----------------------------------------------------------------------------------------------------
static const size_t kVmapStageBytes = 8 + 72 + sizeof(QtrIcpVoxel) + 4;  // per staged voxel

// staging for n voxels: allocated on first need, grown only
static int vmap_keep_reserve(qtr_handle* h, qtr_voxel_map* m, size_t n, VmapStage* st) {
  if (n > m->stage_cap || !m->stage) {
    const size_t cap = (std::max(n, (size_t)1) + 1023) & ~(size_t)1023;
    void* p = nullptr;
    QTR_HIP_TRY(h, hipMalloc(&p, cap * kVmapStageBytes + VM_CTR_INTS * sizeof(int)));
    if (m->stage) (void)hipFree(m->stage);
    m->stage = p;
    m->stage_cap = cap;
  }
  const size_t cap = m->stage_cap;
  char* p = (char*)m->stage;
  st->keys = (u64*)p;
  p += cap * 8;
  st->acc = (double*)p;
  p += cap * 72;
  st->rec = (QtrIcpVoxel*)p;
  p += cap * sizeof(QtrIcpVoxel);
  st->cnt = (int*)p;
  p += cap * 4;
  st->ctr = (int*)p;
  return QTR_OK;
}

static dim3 vmap_keep_table_grid(const qtr_voxel_map* m) {
  return dim3(std::min(qtr_div_up((long long)m->v.mask + 1, 256), 2048));
}

// the counters back on the host (m->pin), after everything enqueued so far
static int vmap_keep_read(qtr_handle* h, qtr_voxel_map* m, const VmapStage& st, hipStream_t s) {
  QTR_HIP_TRY(h, hipGetLastError());
  QTR_HIP_TRY(h, hipMemcpyAsync(m->pin, st.ctr, VM_CTR_INTS * sizeof(int), hipMemcpyDeviceToHost, s));
  QTR_HIP_TRY(h, hipStreamSynchronize(s));
  return QTR_OK;
}

// How evict and carve (verb) end, with the mark pass's counters on the host: n_kept survivors, n_gone voxels that leave
// with members_gone members.  Nothing leaves: the table was only read.  Otherwise the table is rebuilt: stage(grid, block)
// launches the caller's staging kernel for the n_kept survivors, then k_vmap_clear, k_vmap_keep_put and one read-back.
template <class Stage>
static int vmap_keep_rebuild(qtr_handle* h, qtr_voxel_map* m, const VmapStage& st, hipStream_t s, const char* verb, int n_kept,
                             int n_gone, long long members_gone, const Stage& stage) {
  if (n_kept + n_gone != m->info.n_voxels) {
    snprintf(h->err, sizeof(h->err), "voxel map %s: the table holds %d voxels, the map says %d", verb, n_kept + n_gone,
             m->info.n_voxels);
    return QTR_ERR_HIP;
  }
  if (n_gone == 0) return QTR_OK;
  const dim3 tgrid = vmap_keep_table_grid(m), blk(256);
  if (n_kept > 0) stage(tgrid, blk);
  hipLaunchKernelGGL(k_vmap_clear, tgrid, blk, 0, s, m->v, m->ins.tcnt);
  if (n_kept > 0) hipLaunchKernelGGL(k_vmap_keep_put, dim3(qtr_div_up(n_kept, 256)), blk, 0, s, m->v, st, n_kept);
  QTR_TRY(vmap_keep_read(h, m, st, s));
  m->info.n_voxels = n_kept;
  m->info.n_members -= members_gone;
  if (m->pin[VK_CTR_DUP]) {  // (never: the survivors' keys are distinct and fewer than the slots)
    snprintf(h->err, sizeof(h->err), "voxel map %s: the rebuild met a key twice", verb);
    return QTR_ERR_HIP;
  }
  return QTR_OK;
}

int qtr_voxel_map_evict(qtr_handle* h, int slot, qtr_voxel_map* m, const double centre[3], double radius,
                        qtr_voxel_map_evict_info* out) {
  if (out) memset(out, 0, sizeof(*out));
  Slot* sp = peek_slot(h, slot);
  if (!sp) return QTR_ERR_BAD_ARG;
  QTR_TRY(vmap_check(h, m));
  if (!centre) {
    snprintf(h->err, sizeof(h->err), "voxel map evict: centre is NULL");
    return QTR_ERR_BAD_ARG;
  }
  QtrVmapWindow w;
  if (!qtr_vmap_window(centre, radius, m->v.side, &w)) {
    snprintf(h->err, sizeof(h->err),
             "voxel map evict: centre (%g, %g, %g) must be finite and inside the grid, radius %g finite, >= 0 and below 2^22 "
             "voxels of %g",
             centre[0], centre[1], centre[2], radius, m->v.side);
    return QTR_ERR_BAD_ARG;
  }
  qtr_voxel_map_evict_info info = {};
  if (m->info.n_voxels > 0) {
    QTR_HIP_TRY(h, hipSetDevice(h->device));
    VmapStage st;
    QTR_TRY(vmap_keep_reserve(h, m, (size_t)m->info.n_voxels, &st));
    const hipStream_t s = sp->stream;
    QTR_HIP_TRY(h, hipMemsetAsync(st.ctr, 0, VM_CTR_INTS * sizeof(int), s));
    hipLaunchKernelGGL(k_vmap_keep_mark, vmap_keep_table_grid(m), dim3(256), 0, s, m->v, w, st.ctr);
    QTR_TRY(vmap_keep_read(h, m, st, s));
    info.n_kept = m->pin[VK_CTR_KEPT];
    info.n_evicted = m->pin[VK_CTR_EVICTED];
    memcpy(&info.n_members_evicted, m->pin + VK_CTR_MEMBERS64, 8);
    QTR_TRY(vmap_keep_rebuild(h, m, st, s, "evict", info.n_kept, info.n_evicted, info.n_members_evicted, [&](dim3 grid, dim3 blk) {
      hipLaunchKernelGGL(k_vmap_keep_stage, grid, blk, 0, s, m->v, w, st, info.n_kept);
    }));
  }
  if (out) *out = info;
  return QTR_OK;
}

int qtr_voxel_map_restore(qtr_handle* h, int slot, qtr_voxel_map* m, const int* coords, const int* count, const double* sums,
                          int n, int mem) {
  Slot* sp = peek_slot(h, slot);
  if (!sp) return QTR_ERR_BAD_ARG;
  QTR_TRY(vmap_check(h, m));
  if (n < 0 || (n > 0 && (!coords || !count || !sums)) || (mem != QTR_MEM_HOST && mem != QTR_MEM_DEVICE)) {
    snprintf(h->err, sizeof(h->err), "bad voxel map restore arguments");
    return QTR_ERR_BAD_ARG;
  }
  if (m->info.n_voxels != 0) {
    snprintf(h->err, sizeof(h->err), "voxel map restore: the map holds %d voxels (restore takes a map that holds none)",
             m->info.n_voxels);
    return QTR_ERR_BAD_ARG;
  }
  if (n > m->info.capacity) {
    snprintf(h->err, sizeof(h->err), "voxel map restore: n=%d exceeds capacity=%d", n, m->info.capacity);
    return QTR_ERR_CAPACITY;
  }
  long long members = 0;
  if (n > 0) {
    QTR_HIP_TRY(h, hipSetDevice(h->device));
    VmapStage st;
    QTR_TRY(vmap_keep_reserve(h, m, (size_t)n, &st));
    const hipStream_t s = sp->stream;
    const hipMemcpyKind kind = mem == QTR_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    int* d_coords = (int*)st.rec;  // (12 of the record area's 80 bytes per voxel)
    QTR_HIP_TRY(h, hipMemsetAsync(st.ctr, 0, VM_CTR_INTS * sizeof(int), s));
    QTR_HIP_TRY(h, hipMemcpyAsync(d_coords, coords, (size_t)n * 12, kind, s));
    QTR_HIP_TRY(h, hipMemcpyAsync(st.cnt, count, (size_t)n * 4, kind, s));
    QTR_HIP_TRY(h, hipMemcpyAsync(st.acc, sums, (size_t)n * 72, kind, s));
    const dim3 grid(qtr_div_up(n, 256)), blk(256);
    hipLaunchKernelGGL(k_vmap_keep_keys, grid, blk, 0, s, d_coords, st, n);
    VmapStage fin = st;
    fin.rec = nullptr;
    hipLaunchKernelGGL(k_vmap_keep_put, grid, blk, 0, s, m->v, fin, n);
    QTR_TRY(vmap_keep_read(h, m, st, s));
    const int bad = m->pin[VK_CTR_BAD], dup = m->pin[VK_CTR_DUP];
    if (bad || dup) {
      hipLaunchKernelGGL(k_vmap_clear, vmap_keep_table_grid(m), blk, 0, s, m->v, m->ins.tcnt);
      QTR_HIP_TRY(h, hipGetLastError());
      QTR_HIP_TRY(h, hipStreamSynchronize(s));
      if (bad & QTR_VMAP_RESTORE_BAD_COORD)
        snprintf(h->err, sizeof(h->err), "voxel map restore: a coordinate lies outside [-2^20, 2^20)");
      else if (bad & QTR_VMAP_RESTORE_BAD_COUNT)
        snprintf(h->err, sizeof(h->err), "voxel map restore: a count is <= 0");
      else
        snprintf(h->err, sizeof(h->err), "voxel map restore: a coordinate triple occurs twice");
      return QTR_ERR_BAD_ARG;
    }
    memcpy(&members, m->pin + VK_CTR_MEMBERS64, 8);
  }
  m->info.n_voxels = n;
  m->info.n_members = members;
  m->info.n_inserts = 0;
  return QTR_OK;
}
