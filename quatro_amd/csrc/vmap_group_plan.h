// vmap_group_plan.h — where a group of clouds goes in a slot's arena (voxelmap_group.hip and its two users, the grouped
// registration and evaluation against the voxel map): the 256-byte line, the arena's cursor, and which host clouds are
// staged once.  Plain functions of pointers and sizes, no HIP (tests/test_vmap_group_plan_cpu.py compiles them into a CPU
// program).
#pragma once
#include <stddef.h>

// every arena section starts on a 256-byte line
static constexpr size_t qtr_up256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// the cursor over an arena's sections for one call; a zero-byte section still takes one line, so no two share an address
struct VmapCursor {
  size_t need = 0;  // the end of the last section: what the call needs
  size_t take(size_t bytes) {
    const size_t at = need;
    need += qtr_up256(bytes ? bytes : 1);
    return at;
  }
};

// one item as a run sees it: device-resident, or host-resident and to be staged
struct VmapGroupItem {
  const void *src = nullptr, *nrm = nullptr;  // n points and their normals, 16 bytes each (host or device)
  int n = 0;
  bool host = false;
  int same_as = -1;  // host item: the first earlier host item with the same pointers and size, whose staged copy it reads
  size_t o_src = 0, o_nrm = 0;  // host item with n > 0: its staged copy's offsets into the arena
};

// The staged copies of B items (Item: VmapGroupItem or a struct derived from it).  Device items and empty items are never
// staged; a host item shares the copy of the first earlier host item with equal src, nrm and n, and takes two sections
// otherwise.
template <class Item>
static inline void vmap_group_plan(Item* it, int B, VmapCursor& cur) {
  for (int i = 0; i < B; ++i) {
    it[i].same_as = -1;
    if (!it[i].host || it[i].n <= 0) continue;
    for (int j = 0; j < i && it[i].same_as < 0; ++j)
      if (it[j].host && it[j].n == it[i].n && it[j].src == it[i].src && it[j].nrm == it[i].nrm) it[i].same_as = j;
    if (it[i].same_as < 0) {
      it[i].o_src = cur.take((size_t)it[i].n * 16);
      it[i].o_nrm = cur.take((size_t)it[i].n * 16);
    } else {
      it[i].o_src = it[it[i].same_as].o_src;
      it[i].o_nrm = it[it[i].same_as].o_nrm;
    }
  }
}
