// front_verdict.h — what the front-end drivers of capi.hip decide from a cloud's device counters: plain functions of
// integers, no HIP (tests/test_front_verdict_cpu.py compiles them into a CPU program).
#pragma once

// per-cloud device counters (CloudBufs::counts, 16 ints)
enum { CNT_NVOX = 0, CNT_VOX_OVERFLOW = 1, CNT_NBR_TOTAL = 2, CNT_NBR_OVERFLOW = 3, CNT_GRID_OVERFLOW = 4, CNT_KMAX = 5,
       CNT_SORT_BITS = 6 /* significant bits of the voxel sort's keys */,
       CNT_NBR_ARENA = 7 /* entries of the long-list arena handed out */, CNT_NBR_CAPACITY = 8 /* ... it was too small */,
       CNT_VOX_TAILERR = 9 /* sticky: SOME tile of k2_vox_centroids (or of k2_cell_scan) gave up its look-back */,
       CNT_NCELL = 10 /* cells of the neighbour-search grid over this cloud's bounding box (voxel stage, for the cell side
                         the caller named): up to QTR_CELL_CAP the FPFH chain places the points by a dense cell table */ };
// CNT_NBR_OVERFLOW: some point of the cloud has more than QTR_KMAX neighbours (k2_neighbors_big has work to do);
// CNT_KMAX: the longest such list

// The voxel stage's verdict on one cloud of P points.  The reasons in the order they are looked at:
//   VOX_TIMEOUT         CNT_NVOX < 0: a tile of k2_vox_centroids never published its count (bounded look-back), nothing
//                       usable was written
//   VOX_PASS_TOO_LARGE  the grid would overflow int32 and the cloud passes through as it is — pcl::VoxelGrid::applyFilter,
//                       "Leaf size is too small for the input dataset. Integer indices would overflow": output = input,
//                       and so does the reference's `voxelize` (include/quatro.hpp:49-68) — but its P points exceed max_voxels
//   VOX_TOO_MANY        more voxels than max_voxels
//   VOX_EMPTY           no voxel at all
// n is the cloud's size after the stage (P when it passed through) whatever the reason, except after a time-out (0).
// The callers map a reason to their own status code and message, and they differ: qtr_voxelize hands a passed-through or
// an empty cloud out as it is (its bound is the caller's capacity); an empty result is QTR_ERR_BAD_ARG for a keyframe,
// QTR_ERR_CAPACITY for a pair of a batch, and the pair path (front_device) does not look at it.
enum VoxReason { VOX_OK = 0, VOX_TIMEOUT, VOX_PASS_TOO_LARGE, VOX_TOO_MANY, VOX_EMPTY };
struct VoxVerdict {
  int n;
  bool passed;  // the cloud passed through (CNT_VOX_OVERFLOW)
  VoxReason reason;
};
static inline VoxVerdict vox_verdict(const int* counters, int P, int max_voxels) {
  VoxVerdict v = {0, false, VOX_TIMEOUT};
  if (counters[CNT_NVOX] < 0) return v;
  v.passed = counters[CNT_VOX_OVERFLOW] != 0;
  v.n = v.passed ? P : counters[CNT_NVOX];
  v.reason = v.n > max_voxels ? (v.passed ? VOX_PASS_TOO_LARGE : VOX_TOO_MANY) : v.n <= 0 ? VOX_EMPTY : VOX_OK;
  return v;
}

// The voxel sort needs ceil(bits / 8) radix passes, bits = significant bits of the grid's cell index (CNT_SORT_BITS) — known
// on the device only.  A launch that returns at once still costs ~5 us on the chain, so a driver launches what the previous
// call on its slot needed (vox_passes: 3 for a lidar scan at 0.3 m; 4, which always suffices, on a slot's first call) and
// asks here afterwards: true = under-launched on the first attempt, the centroids are garbage and the stage runs again,
// with 4.  Fewer passes are launched only after four calls in a row that would have done with fewer (vox_fewer counts
// them: alternating scenes would thrash).
static inline bool vox_passes_next(int& vox_passes, int& vox_fewer, int sort_bits, int launched, int attempt) {
  int needed = (sort_bits + 7) / 8;
  needed = needed < 1 ? 1 : needed > 4 ? 4 : needed;
  if (needed > launched && attempt == 0) {
    vox_passes = 4;
    vox_fewer = 0;
    return true;
  }
  if (needed < launched) {
    if (++vox_fewer >= 4) {
      vox_passes = needed;
      vox_fewer = 0;
    }
  } else {
    vox_fewer = 0;
  }
  return false;
}

// The neighbour lists' verdict after an FPFH chain, from the counter line(s) of its cloud(s) (cnt1: the second cloud's, or
// null), in this order:
//   LISTS_TILE_ERROR  CNT_VOX_TAILERR: a MIDDLE tile of k2_vox_centroids gave up its look-back (its centroids were never
//                     written) although the last tile's came out whole and mailed a valid count
//   LISTS_CAPACITY    CNT_NBR_CAPACITY: the long-list arena (qtr_limits.max_long_neighbors) was too small
//   LISTS_NEED_LONG   CNT_NBR_OVERFLOW and a chain that ran without k2_neighbors_big (long_lists false): a point has more than
//                     QTR_KMAX neighbours — voxel-grid centroids at the demo's leaf never have, so the launch is left out until
//                     a cloud needs it — and the descriptors of this call are not usable: the caller turns the handle's
//                     long_lists on and goes round again
// (qtr_fpfh always runs with long lists and has only ever read CNT_NBR_CAPACITY: it keeps its own one-word test.)
enum ListsVerdict { LISTS_OK = 0, LISTS_TILE_ERROR, LISTS_CAPACITY, LISTS_NEED_LONG };
static inline ListsVerdict lists_verdict(const int* cnt0, const int* cnt1, bool long_lists) {
  auto any = [&](int w) { return cnt0[w] != 0 || (cnt1 && cnt1[w] != 0); };
  if (any(CNT_VOX_TAILERR)) return LISTS_TILE_ERROR;
  if (any(CNT_NBR_CAPACITY)) return LISTS_CAPACITY;
  if (!long_lists && any(CNT_NBR_OVERFLOW)) return LISTS_NEED_LONG;
  return LISTS_OK;
}
