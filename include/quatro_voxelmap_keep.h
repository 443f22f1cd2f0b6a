/* quatro_voxelmap_keep.h - C ABI of the voxel map's upkeep, exported by quatro_amd/libquatro_ext.so.
 *
 * The two entry points below work on the handles of libquatro_hip.so (include/quatro_hip.h) and the maps of
 * include/quatro_voxelmap.h, which says what the extension library is.  Both libraries must come from the same build.
 * The contract, exact in integers, is include/qtr_vmap_keep_math.h.
 *   evict    sliding-window eviction: with C = floor(centre / voxel_size) per axis and R = floor(radius / voxel_size), a
 *            voxel with coordinates i stays iff |i - C|^2 <= R^2 (int64).  The map afterwards is the map before without the
 *            other voxels: every fetch section is, bit for bit, the rows of the section before that pass; n_voxels and
 *            n_members drop by what left, n_inserts is unchanged.  A kept voxel's sums go on under later inserts as if
 *            nothing had happened; an evicted voxel that is touched again starts anew.  A window that rejects nothing
 *            leaves the table untouched.  Refused with QTR_ERR_BAD_ARG before anything is enqueued: a non-finite centre, a
 *            centre whose voxel lies outside [-2^20, 2^20), a negative or non-finite radius, R >= 2^22.
 *   restore  puts n voxels given as the fetch sections QTR_VMAP_COORDS (int32[n][3]), QTR_VMAP_COUNT (int32[n]) and
 *            QTR_VMAP_SUMS (double[n][9]), in host or device memory (`mem` as in qtr_voxel_map_insert), into a map that
 *            holds no voxel.  Afterwards all five fetch sections equal those of the map the arrays were fetched from,
 *            n_members = sum of count and n_inserts = 0; the target's capacity (and table size) may differ from the
 *            source's.  n is bounded by the map's capacity, not by max_points.  Refusals: a map that holds voxels
 *            (QTR_ERR_BAD_ARG), n > capacity (QTR_ERR_CAPACITY), and - found on the device, QTR_ERR_BAD_ARG - a coordinate
 *            outside [-2^20, 2^20), a count <= 0, the same coordinate triple twice.  After every refusal the map is empty
 *            and usable.
 * Device memory: 164 bytes of staging per voxel (evict: the map's n_voxels at the call; restore: n), allocated on the first
 * call that needs it and grown only, freed with the map.
 * Both calls are host-synchronous and WRITE the map: the caller serialises them against inserts, clear, each other and
 * registrations on that map.  Messages go through qtr_last_error. */
#ifndef QUATRO_VOXELMAP_KEEP_C_H
#define QUATRO_VOXELMAP_KEEP_C_H

#include "quatro_voxelmap.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef QTR_EXT_API /* (libquatro_ext.so's exports: csrc/exports_ext.map lists them, csrc/exports.map does not) */
#define QTR_EXT_API QTR_API
#endif

typedef struct qtr_voxel_map_evict_info {
  int n_kept, n_evicted;       /* voxels */
  long long n_members_evicted; /* their members */
} qtr_voxel_map_evict_info;

QTR_EXT_API int qtr_voxel_map_evict(qtr_handle* h, int slot, qtr_voxel_map* map, const double centre[3], double radius,
                                    qtr_voxel_map_evict_info* info /* may be NULL */);
QTR_EXT_API int qtr_voxel_map_restore(qtr_handle* h, int slot, qtr_voxel_map* map, const int* coords, const int* count,
                                      const double* sums, int n, int mem);

#ifdef __cplusplus
}
#endif
#endif /* QUATRO_VOXELMAP_KEEP_C_H */
