// vmap_keep_ref.cpp — host restatement of the voxel map's upkeep (quatro_amd/csrc/voxelmap_keep.hip) for the tests, on top of
// vmap_ref.cpp, which it includes as it stands (so a map made by either library's vmap_ref_new is the same structure): erase
// from the std::map by include/qtr_vmap_keep_math.h's rule, and restore from the three sections.  Nothing of the device's
// staging, clearing or re-hashing is restated: the std::map has no probe chains to protect.
// Built by the tests with g++ -O2 -ffp-contract=off -shared -fPIC.
#include "vmap_ref.cpp"

#include "qtr_vmap_keep_math.h"

extern "C" {

// 1, the centre's voxel C3[3] and R^2: the window; 0: refused
int vmap_keep_window(const double* centre, double radius, double side, int* C3, long long* R2) {
  QtrVmapWindow w;
  if (!qtr_vmap_window(centre, radius, side, &w)) return 0;
  for (int a = 0; a < 3; ++a) C3[a] = w.C[a];
  *R2 = w.R2;
  return 1;
}

// the verdict of the window (centre, radius) on the voxel i[3]: 1 kept, 0 evicted, -1 the window is refused
int vmap_keep_verdict(const double* centre, double radius, double side, const int* i) {
  QtrVmapWindow w;
  if (!qtr_vmap_window(centre, radius, side, &w)) return -1;
  return qtr_vmap_kept(&w, i) ? 1 : 0;
}

// info: n_kept, n_evicted; members: the evicted voxels' members.  Returns 0, or 2 (QTR_ERR_BAD_ARG) with the map untouched.
int vmap_keep_evict(void* p, const double* centre, double radius, int* info, long long* members) {
  RefMap* m = (RefMap*)p;
  QtrVmapWindow w;
  info[0] = info[1] = 0;
  *members = 0;
  if (!qtr_vmap_window(centre, radius, m->side, &w)) return 2;
  for (auto it = m->vox.begin(); it != m->vox.end();) {
    if (qtr_vmap_kept_key(&w, it->first)) {
      ++info[0];
      ++it;
    } else {
      ++info[1];
      *members += it->second.n;
      it = m->vox.erase(it);
    }
  }
  return 0;
}

// Returns 0 and the sum of the counts, 2 (QTR_ERR_BAD_ARG) or 3 (QTR_ERR_CAPACITY); after a refusal the map is empty (a map
// that held voxels keeps them: that refusal comes first).
int vmap_keep_restore(void* p, const int* coords, const int* count, const double* sums, int n, long long* members) {
  RefMap* m = (RefMap*)p;
  *members = 0;
  if (n < 0 || !m->vox.empty()) return 2;
  if (n > m->capacity) return 3;
  for (int j = 0; j < n; ++j) {
    unsigned long long key = 0;
    if (qtr_vmap_restore_key(coords + 3 * j, count[j], &key) != QTR_VMAP_RESTORE_OK || m->vox.count(key)) {
      m->vox.clear();
      *members = 0;
      return 2;
    }
    Rec r;
    r.n = count[j];
    memcpy(r.acc, sums + 9 * j, 72);
    m->vox[key] = r;
    *members += count[j];
  }
  return 0;
}

}  // extern "C"
