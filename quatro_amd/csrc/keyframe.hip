// keyframe.hip — device-resident keyframes: the products of ONE scan's front end kept in an allocation sized to the scan,
// and the two copy kernels between such an allocation and a slot's cloud arenas.
//   pack  (qtr_keyframe_create)       slot cloud 0 -> keyframe, after the one-cloud voxel grid + FPFH chain + mean
//   load  (qtr_register_keyframes,    two keyframes -> a slot's cloud[0] / cloud[1]: voxels, normals, descriptors, mean,
//          qtr_submit_batch_keyframes) counters, and the matcher's per-descriptor preparation that k2_fpfh does on the
//                                     whole path (|d|^2, hash, entry in the duplicate table), so that the matcher starts at
//                                     its operand tables with prep_done = true
//   merge (qtr_keyframe_merge)        K keyframes' voxels -> a slot's raw-cloud buffer, each member under its pose
//                                     (k_kf_gather, include/qtr_submap_math.h); the one-cloud front end and the pack follow
// Stored per voxel: 16 (point) + 16 (normal, curvature) + 132 (descriptor) + 4 (|d|^2) + 8 (descriptor hash) = 176 bytes.
// Not stored: neighbour lists, SPFH, sort buffers, the cell table, the duplicate table (its size follows the handle's
// max_voxels, not the scan: the load rebuilds it from the stored hashes) and the matcher's per-pair tables.
#include "common.h"
#include "frontend.h"
#include "../../include/qtr_submap_math.h"

#define KF_HDR_BYTES 256  // 16 counters (CNT_*), then the 4 floats of the sequential mean
#define KF_ALIGN 256

// byte offsets of the sections of a keyframe of n voxels
struct KfLayout {
  size_t vox, normals, fpfh, norms, hash, total;
};
static inline KfLayout kf_layout(int n) {
  auto up = [](size_t b) { return (b + KF_ALIGN - 1) & ~(size_t)(KF_ALIGN - 1); };
  KfLayout L;
  L.vox = KF_HDR_BYTES;
  L.normals = L.vox + up((size_t)n * 16);
  L.fpfh = L.normals + up((size_t)n * 16);
  L.norms = L.fpfh + up((size_t)n * 132);
  L.hash = L.norms + up((size_t)n * 4);
  L.total = L.hash + up((size_t)n * 8);
  return L;
}

// One cloud of a pack / load launch: the keyframe's allocation and the slot arenas on the other side.
struct KfView {
  char* kf;
  int n;
  int dd_mask;      // load: slots of the duplicate table - 1
  int* counts;
  float* mean;
  float4* vox;
  float4* normals;
  float* fpfh;
  float* norms;
  u64* dd_hash;
  u64* dd_table;    // load only (cleared before the launch: k_match_init / k_kf_clear)
  size_t o_normals, o_fpfh, o_norms, o_hash;  // kf_layout (the point section starts at KF_HDR_BYTES)
};
struct KfViews2 {
  KfView c[2];
};

// `bytes` (a multiple of 4) between two 16-byte aligned sections: 128-bit loads and stores, grid-stride; the last words alone
template <bool LOAD>
__device__ __forceinline__ void kf_copy_section(char* kf_sec, void* slot_sec, size_t bytes, int gid, int gsz) {
  const uint4* __restrict__ s = (const uint4*)(LOAD ? (const void*)kf_sec : (const void*)slot_sec);
  uint4* __restrict__ d = (uint4*)(LOAD ? slot_sec : (void*)kf_sec);
  const size_t n16 = bytes >> 4;
  for (size_t i = (size_t)gid; i < n16; i += (size_t)gsz) d[i] = s[i];
  const int tail = (int)((bytes & 15) >> 2);
  if (gid < tail) ((u32*)d)[n16 * 4 + gid] = ((const u32*)s)[n16 * 4 + gid];
}

// grid (g, clouds, pairs): blockIdx.y = cloud of the pair, blockIdx.z = pair (EXT: the views live in device memory)
template <bool EXT, bool LOAD>
__global__ __launch_bounds__(256) void k_kf_copy(ViewExt<KfView> x, KfViews2 two) {
  const KfView& V = EXT ? x.ext[blockIdx.z * 2 + blockIdx.y] : two.c[blockIdx.y];  // (inline on purpose: see ViewExt)
  const int gid = blockIdx.x * blockDim.x + threadIdx.x, gsz = gridDim.x * blockDim.x;
  const size_t n = (size_t)V.n;
  if (gid < 16) {
    int* hdr = (int*)V.kf;
    if (LOAD) {
      // the words a whole-path call checks after its matcher were checked when the keyframe was made: the slot gets them clean
      const int w = hdr[gid];
      V.counts[gid] = (gid == CNT_VOX_TAILERR || gid == CNT_NBR_CAPACITY || gid == CNT_NBR_OVERFLOW) ? 0 : w;
    } else {
      hdr[gid] = V.counts[gid];
    }
  } else if (gid < 20) {
    float* hm = (float*)(V.kf + 64);
    if (LOAD) V.mean[gid - 16] = hm[gid - 16];
    else hm[gid - 16] = V.mean[gid - 16];
  }
  kf_copy_section<LOAD>(V.kf + KF_HDR_BYTES, V.vox, n * 16, gid, gsz);
  kf_copy_section<LOAD>(V.kf + V.o_normals, V.normals, n * 16, gid, gsz);
  kf_copy_section<LOAD>(V.kf + V.o_fpfh, V.fpfh, n * 132, gid, gsz);
  kf_copy_section<LOAD>(V.kf + V.o_norms, V.norms, n * 4, gid, gsz);
  kf_copy_section<LOAD>(V.kf + V.o_hash, V.dd_hash, n * 8, gid, gsz);
  if (LOAD) {
    // the duplicate table, as d_desc_prep / the end of k2_fpfh fill it: slot sequence from the low hash bits, tag = high 32
    // bits, value = lowest row with that tag (which slot a tag lands in depends on arrival order; what a probe finds does not)
    const u64* __restrict__ hashes = (const u64*)(V.kf + V.o_hash);
    u64* table = V.dd_table;
    const u32 mask = (u32)V.dd_mask;
    for (int i = gid; i < V.n; i += gsz) {
      const u64 h = hashes[i];
      const u64 tag = h & 0xffffffff00000000ULL;
      u32 slot = (u32)h & mask;
      for (u32 probe = 0; probe <= mask; ++probe) {
        u64 cur = table[slot];
        if (cur == ~0ULL) {
          const u64 old = atomicCAS(&table[slot], ~0ULL, tag | (u32)i);
          if (old == ~0ULL) break;
          cur = old;
        }
        if ((cur & 0xffffffff00000000ULL) == tag) {
          if ((u32)cur > (u32)i) atomicMin(&table[slot], tag | (u32)i);
          break;
        }
        slot = (slot + 1) & mask;
      }
    }
  }
}

// the duplicate tables of the clouds of a grouped load (a single pair's are cleared by its k_match_init)
__global__ __launch_bounds__(256) void k_kf_clear(ViewExt<KfView> x) {
  const KfView& V = x.ext[blockIdx.z * 2 + blockIdx.y];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i <= V.dd_mask; i += gridDim.x * blockDim.x) V.dd_table[i] = ~0ULL;
}

static KfView kf_view(void* kf, int n, CloudBufs& C, int dd_slots) {
  const KfLayout L = kf_layout(n);
  KfView v;
  memset(&v, 0, sizeof(v));
  v.kf = (char*)kf;
  v.n = n;
  v.dd_mask = dd_slots - 1;
  v.counts = C.counts;
  v.mean = C.mean;
  v.vox = C.vox;
  v.normals = C.normals;
  v.fpfh = C.fpfh;
  v.norms = C.norms;
  v.dd_hash = C.dd_hash;
  v.dd_table = C.dd_table;
  v.o_normals = L.normals;
  v.o_fpfh = L.fpfh;
  v.o_norms = L.norms;
  v.o_hash = L.hash;
  return v;
}
static inline int kf_grid(int n) {  // one 16-byte unit of the widest section (descriptors) per thread, grid-stride beyond
  const long long units = ((long long)n * 132 + 15) / 16;
  const long long g = (units + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

// slot cloud 0 -> keyframe
hipError_t kf_pack_enqueue(FrontBufs& F, void* kf, int n, hipStream_t st) {
  KfViews2 two;
  two.c[0] = kf_view(kf, n, F.cloud[0], F.dd_slots);
  two.c[1] = two.c[0];
  hipLaunchKernelGGL((k_kf_copy<false, false>), dim3(kf_grid(n), 1, 1), dim3(256), 0, st, (ViewExt<KfView>{nullptr, {0, 0, 0}}), two);
  return hipGetLastError();
}
// two keyframes -> the slot's cloud[0] (source) / cloud[1] (target); the duplicate tables must have been cleared on `st`
hipError_t kf_load_enqueue(FrontBufs& F, void* kf_s, int ns, void* kf_t, int nt, hipStream_t st) {
  KfViews2 two;
  two.c[0] = kf_view(kf_s, ns, F.cloud[0], F.dd_slots);
  two.c[1] = kf_view(kf_t, nt, F.cloud[1], F.dd_slots);
  hipLaunchKernelGGL((k_kf_copy<false, true>), dim3(kf_grid(max(ns, nt)), 2, 1), dim3(256), 0, st,
                     (ViewExt<KfView>{nullptr, {0, 0, 0}}), two);
  return hipGetLastError();
}
// the same for G pairs (kf / n: two entries per pair), clearing the duplicate tables first
hipError_t kf_load_enqueue_group(FrontBufs* const* F, int G, void* const* kf, const int* n, ViewStage* stage, hipStream_t st) {
  std::vector<KfView> v((size_t)2 * G);
  int maxn = 1, max_slots = 1;
  for (int g = 0; g < G; ++g)
    for (int c = 0; c < 2; ++c) {
      v[2 * g + c] = kf_view(kf[2 * g + c], n[2 * g + c], F[g]->cloud[c], F[g]->dd_slots);
      maxn = max(maxn, n[2 * g + c]);
      max_slots = max(max_slots, F[g]->dd_slots);
    }
  const KfView* dv = (const KfView*)stage_push(stage, v.data(), sizeof(KfView) * v.size(), st);
  if (!dv) return hipErrorOutOfMemory;
  KfViews2 two;
  two.c[0] = two.c[1] = v[0];
  hipLaunchKernelGGL(k_kf_clear, dim3(min(1024, (max_slots + 1023) / 1024), 2, G), dim3(256), 0, st, (ViewExt<KfView>{dv, {0, 0, 0}}));
  hipLaunchKernelGGL((k_kf_copy<true, true>), dim3(kf_grid(maxn), 2, G), dim3(256), 0, st, (ViewExt<KfView>{dv, {0, 0, 0}}), two);
  return hipGetLastError();
}

// ---- merge: the voxels of K keyframes, each under its pose, concatenated in member order -----------------------------------
// One member of a merge.  The table of a whole merge (up to QTR_SUBMAP_MAX_KEYFRAMES records of 112 bytes: 7 kB) does not fit
// the 4 kB of kernel arguments: it travels through pinned host memory into the slot's merge scratch (capi.hip).
struct KfGatherMember {
  const float4* vox;  // the member's stored voxels (its allocation + KF_HDR_BYTES)
  int n;              // ... how many
  int prefix;         // records of the members before it
  double T[12];       // rows 0 - 2 of the member's pose
};

// grid (g, K): blockIdx.y = member, grid-stride in x over its voxels.  One 128-bit load, qtr_submap_point, one 128-bit store
// per record; out holds prefix[K - 1] + n[K - 1] records (the host checked the sum against the buffer's size).
__global__ __launch_bounds__(256) void k_kf_gather(ViewExt<KfGatherMember> x, float4* __restrict__ out) {
  const KfGatherMember& M = x.ext[blockIdx.y];
  const float4* __restrict__ in = M.vox;
  const int n = M.n;
  float4* __restrict__ dst = out + M.prefix;
  double T[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) T[k] = M.T[k];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float4 p = in[i];
    float4 q;
    qtr_submap_point(T, p.x, p.y, p.z, &q.x, &q.y, &q.z);
    q.w = p.w;
    dst[i] = q;
  }
}

// members: the table in DEVICE memory (K records); max_n: the largest member
hipError_t kf_gather_enqueue(const KfGatherMember* members, int K, int max_n, float4* out, hipStream_t st) {
  const int g = min(256, max(1, (max_n + 255) / 256));
  hipLaunchKernelGGL(k_kf_gather, dim3(g, K, 1), dim3(256), 0, st, (ViewExt<KfGatherMember>{members, {0, 0, 0}}), out);
  return hipGetLastError();
}
