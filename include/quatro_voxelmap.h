/* quatro_voxelmap.h - C ABI of the persistent Gaussian voxel map, exported by quatro_amd/libquatro_ext.so.
 *
 * libquatro_ext.so is the extension library beside libquatro_hip.so (include/quatro_hip.h, whose entry points stay exactly
 * what they were): it is linked from the same object, shares the handle, the slots, the keyframes and the slot's ICP state
 * with it, and exports the entry points of this header and of the other extension headers (quatro_voxelmap_keep.h,
 * quatro_voxelmap_carve.h, quatro_voxelmap_batch.h, quatro_voxelmap_eval.h, quatro_deskew.h, quatro_place_batch.h,
 * quatro_voxelmap_ct.h) and nothing else.  A program creates its handle with qtr_create, links both libraries
 * (-lquatro_hip -lquatro_ext) and passes the handle to the calls here; qtr_last_error returns their messages and
 * qtr_debug_fetch their traces like any other call's.  Both libraries must come from the same build. */
#ifndef QUATRO_VOXELMAP_C_H
#define QUATRO_VOXELMAP_C_H

#include "quatro_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef QTR_EXT_API /* (libquatro_ext.so's exports: csrc/exports_ext.map lists them, csrc/exports.map does not) */
#define QTR_EXT_API QTR_API
#endif

/* Persistent Gaussian voxel map: the world-frame map the optimised poses are for, and a refinement target that spans any
 * number of sweeps (fast_gicp's GaussianVoxelMap / small_gicp's IncrementalVoxelMap).  One Gaussian per voxel of a grid that
 * is anchored at the world origin (voxel coordinate floor(X / voxel_size), valid in [-2^20, 2^20) per axis) and depends on
 * nothing that was inserted.  The arithmetic and every order of summation are include/qtr_vmap_math.h.
 *   insert    the cloud's points under `pose` (row-major 4x4, cloud frame -> world, rows 0 - 2 read; NULL = identity).  A
 *             member is a finite point with a usable normal whose world position is finite and inside the grid; everything
 *             else is silently skipped.  A voxel's record is the running fold over everything inserted so far, in call
 *             order and inside a call in ascending point index: the map after inserts A then B is the map of their
 *             concatenation.  Any number of inserts, no member limit.
 *   register  the voxelised plane-to-plane iteration (method 3) against the map: q = T p is matched to the voxel it falls
 *             into, no distance test.  prm->method must be QTR_ICP_VOXEL_PLANE_TO_PLANE (anything else: QTR_ERR_BAD_ARG);
 *             prm->max_correspondence_distance is IGNORED — the voxel side is the map's; prm->normal_radius is not used
 *             (the cloud entries take the normals from the caller, the keyframe entries read QTR_KF_NORMALS in place).
 *             With a target whose minimum is exactly (0, 0, 0), inserted under the identity, the result is qtr_gicp's
 *             method 3 at max_correspondence_distance = voxel_size bit for bit.  Row 3 of `guess` is taken as (0 0 0 1).
 *             QTR_DBG_ICP_TRACE / _TIMES serve the slot's last map registration like any refinement; QTR_DBG_ICP_CORR holds
 *             0 for a matched source point and -1 for one without a voxel.
 *   fetch     sections in ascending key order (key = ((kz 2^21) + ky) 2^21 + kx, k = coordinate + 2^20); return value as
 *             qtr_keyframe_fetch: the bytes the section holds, up to `bytes` of them copied, < 0 on error.
 *   capacity  an insert that would bring the number of voxels above `capacity` returns QTR_ERR_CAPACITY and leaves the
 *             map exactly as it was.  Device memory: 172 bytes per table slot, 2 x capacity slots rounded up to a power of
 *             two (the default capacity takes 344 MiB), plus 28 bytes x max_points of insert scratch from the first insert.
 * Every argument is checked before anything is enqueued: pointers, the map's and the keyframe's owner, 0 <= n <= max_points
 * (above: QTR_ERR_CAPACITY), finite rows 0 - 2 of pose / guess, non-NULL normals in the cloud entries.
 * All calls are host-synchronous.  Registration only READS the map: any number of slots and threads may register against
 * one map at once.  Inserts and clear on one map are the caller's to serialise, against each other and against
 * registrations.  A map that was not destroyed dies with its handle. */
typedef struct qtr_voxel_map qtr_voxel_map; /* opaque, owned by the handle that made it */
#define QTR_VMAP_MAX_CAPACITY (1 << 24)
typedef struct qtr_voxel_map_params {
  double voxel_size; /* 1.0 */
  int capacity;      /* voxels, 1 << 20 */
  int reserved[5];
} qtr_voxel_map_params;
typedef struct qtr_voxel_map_info {
  double voxel_size;
  int capacity, n_voxels, n_inserts;
  long long n_members;
} qtr_voxel_map_info;
typedef struct qtr_voxel_map_insert_info {
  int n_points, n_members, n_new_voxels, n_touched_voxels;
} qtr_voxel_map_insert_info;
#define QTR_VMAP_COORDS 1  /* int32[n][3] voxel coordinates */
#define QTR_VMAP_COUNT 2   /* int32[n] member counts */
#define QTR_VMAP_SUMS 3    /* double[n][9] the raw sums: X (3), m m^T (00 01 02 11 12 22) */
#define QTR_VMAP_RECORDS 4 /* double[n][9] mu (3) and C_b (6) of the finished record */
#define QTR_VMAP_CLOUD 5   /* float4[n] mu rounded once to float, w = (float)members: the map as a point cloud */
QTR_EXT_API void qtr_default_voxel_map_params(qtr_voxel_map_params* p);
QTR_EXT_API int qtr_voxel_map_create(qtr_handle* h, const qtr_voxel_map_params* params /* NULL = defaults */, qtr_voxel_map** out);
QTR_EXT_API void qtr_voxel_map_destroy(qtr_handle* h, qtr_voxel_map* map);
QTR_EXT_API int qtr_voxel_map_clear(qtr_handle* h, int slot, qtr_voxel_map* map);
QTR_EXT_API int qtr_voxel_map_get_info(const qtr_voxel_map* map, qtr_voxel_map_info* info);
QTR_EXT_API int qtr_voxel_map_insert(qtr_handle* h, int slot, qtr_voxel_map* map, const float* xyz4, const float* normals4, int n,
                                const double pose[16] /* NULL = identity */, int mem,
                                qtr_voxel_map_insert_info* info /* may be NULL */);
QTR_EXT_API int qtr_voxel_map_insert_keyframe(qtr_handle* h, int slot, qtr_voxel_map* map, const qtr_keyframe* kf,
                                         const double pose[16], qtr_voxel_map_insert_info* info);
QTR_EXT_API int qtr_voxel_map_register(qtr_handle* h, int slot, const qtr_voxel_map* map, const float* src4, int n,
                                  const float* src_normals4, const double guess[16], const qtr_icp_params* prm,
                                  qtr_icp_result* res, int mem);
QTR_EXT_API int qtr_voxel_map_register_keyframe(qtr_handle* h, int slot, const qtr_voxel_map* map, const qtr_keyframe* kf,
                                           const double guess[16], const qtr_icp_params* prm, qtr_icp_result* res);
QTR_EXT_API long long qtr_voxel_map_fetch(qtr_handle* h, const qtr_voxel_map* map, int what, void* dst, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* QUATRO_VOXELMAP_C_H */
