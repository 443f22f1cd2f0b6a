// voxelmap_group.hip — the host frame of a call that takes a group of clouds or keyframes under poses against one voxel map
// (voxelmap_batch.hip, voxelmap_eval.hip): the slot's arena, the item check, the staging of the host clouds and the fetch
// tail.  Where the sections lie is vmap_group_plan.h (no HIP, tested on the CPU); this file holds what needs the runtime.
//
// The arena is the slot's own, one per user (Slot::vbatch, Slot::veval).  Keyframes and device-resident clouds are read in
// place, so items that name the same keyframe or the same device pointers share their source arrays; host items with the
// same pointers share one staged copy.  Allocated on the slot's first call, grown to a call's need, freed with the handle.
#include "../../include/quatro_voxelmap_batch.h"  // qtr_vmap_reg_item: the item of both users

enum { VG_EV_MAX = 3 };

// what a user's arena struct starts with (VmapBatch, VmapEval derive from it and add what they keep for their fetch)
struct VmapArena {
  void* dev = nullptr;  // the arena
  size_t dev_bytes = 0;
  char* pin = nullptr;  // pinned, a fixed size per user: the views and what travels with them, then the read-back
  hipEvent_t ev[VG_EV_MAX] = {};
  int B = -1;  // the items of the slot's last call, whose sections the fetch serves (-1: none)
};

template <class A>
static void vmap_arena_free(A*& a) {
  if (!a) return;
  if (a->dev) (void)hipFree(a->dev);
  if (a->pin) (void)hipHostFree(a->pin);
  for (hipEvent_t e : a->ev)
    if (e) (void)hipEventDestroy(e);
  delete a;
  a = nullptr;
}

// the slot's arena struct, its pinned block and its first n_ev events, each made when it is missing
template <class A>
static int vmap_arena_open(qtr_handle* h, A*& a, size_t pin_bytes, int n_ev) {
  if (!a && !(a = new (std::nothrow) A())) return QTR_ERR_CAPACITY;  // (from here on the handle frees whatever of it exists)
  if (!a->pin) QTR_HIP_TRY(h, hipHostMalloc((void**)&a->pin, pin_bytes));
  for (int k = 0; k < n_ev; ++k)
    if (!a->ev[k]) QTR_HIP_TRY(h, hipEventCreate(&a->ev[k]));
  return QTR_OK;
}

// `need` bytes for a call that is about to write the arena; the last call's sections are gone from here on
static int vmap_arena_grow(qtr_handle* h, VmapArena& a, size_t need, hipStream_t st) {
  a.B = -1;
  if (need > a.dev_bytes) {
    QTR_HIP_TRY(h, hipStreamSynchronize(st));
    if (a.dev) (void)hipFree(a.dev);
    a.dev = nullptr;
    a.dev_bytes = 0;
    QTR_HIP_TRY(h, hipMalloc(&a.dev, need));
    a.dev_bytes = need;
  }
  return QTR_OK;
}

// The B items of a call in the caller's words (verb "register" / "evaluate", noun "guess" / "pose", prefix "batch item" /
// "evaluate item"): a keyframe of this handle or vmap_check_cloud, then the guess; it[i] is the cloud as given.
template <class Item>
static int vmap_group_check(qtr_handle* h, const char* verb, const char* noun, const char* prefix, const qtr_vmap_reg_item* items,
                            int B, Item* it) {
  for (int i = 0; i < B; ++i) {
    const qtr_vmap_reg_item& a = items[i];
    int rc = a.kf ? vmap_check_kf(h, a.kf) : vmap_check_cloud(h, verb, "src_normals4", nullptr, a.mem, a.n, a.src4, a.src_normals4);
    if (rc == QTR_OK) rc = vmap_check_pose(h, verb, noun, a.guess);
    if (rc != QTR_OK) {
      char msg[sizeof(h->err)];
      snprintf(msg, sizeof(msg), "%s", h->err);
      snprintf(h->err, sizeof(h->err), "%s %d: %.480s", prefix, i, msg);
      return rc;
    }
    if (a.kf) {
      const VmapKfCloud c = vmap_kf_cloud(a.kf);
      it[i].src = c.pts;
      it[i].nrm = c.nrm;
      it[i].n = c.n;
      it[i].host = false;
    } else {
      it[i].src = a.src4;
      it[i].nrm = a.src_normals4;
      it[i].n = a.n;
      it[i].host = a.mem == QTR_MEM_HOST;
    }
  }
  return QTR_OK;
}

// the distinct host clouds of a planned group into the arena `dev`; every item's src / nrm are device pointers afterwards
template <class Item>
static int vmap_group_upload(qtr_handle* h, char* dev, Item* it, int B, hipStream_t st) {
  for (int i = 0; i < B; ++i) {
    if (!it[i].host || it[i].n <= 0) continue;
    if (it[i].same_as < 0) {
      QTR_HIP_TRY(h, hipMemcpyAsync(dev + it[i].o_src, it[i].src, (size_t)it[i].n * 16, hipMemcpyHostToDevice, st));
      QTR_HIP_TRY(h, hipMemcpyAsync(dev + it[i].o_nrm, it[i].nrm, (size_t)it[i].n * 16, hipMemcpyHostToDevice, st));
    }
    it[i].src = dev + it[i].o_src;
    it[i].nrm = dev + it[i].o_nrm;
  }
  return QTR_OK;
}

// the tail of a fetch of a device section of the slot's last call: min(have, bytes) bytes of it into dst, `have` returned
static long long vmap_group_fetch(qtr_handle* h, Slot& s, const void* src, size_t have, void* dst, size_t bytes) {
  const size_t n = have < bytes ? have : bytes;
  if (dst && n > 0) {
    if (hipSetDevice(h->device) != hipSuccess) return -1;
    if (hipStreamSynchronize(s.stream) != hipSuccess) return -1;
    if (hipMemcpy(dst, src, n, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  }
  return (long long)have;
}
