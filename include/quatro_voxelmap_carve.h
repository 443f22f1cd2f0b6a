/* quatro_voxelmap_carve.h - C ABI of visibility carving of the voxel map, exported by quatro_amd/libquatro_ext.so.
 *
 * The three entry points below work on the handles and keyframes of libquatro_hip.so (include/quatro_hip.h) and the maps of
 * include/quatro_voxelmap.h, which says what the extension library is.  Both libraries must come from the same build.
 * The contract, exact in binary64, is include/qtr_vmap_carve_math.h.
 *
 * The map forgets by EVIDENCE: a voxel leaves when enough scans, taken from known poses, measured returns clearly behind it
 * along the line of sight to it.  Each scan becomes a range image in its own frame (rows x cols pixels, the nearest return
 * per pixel).  A voxel's mean, as QTR_VMAP_RECORDS reports it, is brought into the scan's frame by the scan's pose and
 * projected to a pixel.  The scan has no vote when the pixel lies outside the image, the voxel's range lies outside
 * [min_range, max_range], or the centre pixel is empty: a beam that came back with nothing says nothing.  Otherwise it votes
 * "seen through" iff no filled pixel of the (2 window + 1)^2 neighbourhood holds a range <= r_v + margin_abs +
 * margin_rel r_v (columns wrap, rows outside the image and empty pixels are neutral, equality keeps the voxel).  A voxel is
 * carved iff its votes over the call's scans reach min_votes.
 *
 * The result has the contract of an eviction: the map afterwards is the map before without the carved voxels; every fetch
 * section is, bit for bit, the kept rows of the section before; n_voxels and n_members drop by what left, n_inserts is
 * unchanged; a kept voxel's sums go on under later inserts as if nothing had happened, a carved voxel that is touched again
 * starts anew.  A call that carves nothing leaves the table untouched.
 *
 * What to carve with.
 *   - The RAW sweep, or a keyframe made of it.  A ground-removed cloud carves almost nothing above the road: the beams that
 *     would prove that space free were removed with the ground.
 *   - Never a merged (submap) keyframe: it has no single viewpoint, and its range image means nothing.
 *   - An image no finer than the sensor: the rule needs the centre pixel filled.
 *
 * Every argument is checked before anything is enqueued: pointers, the map's and the keyframes' owner, 0 <= n <= max_points
 * (above: QTR_ERR_CAPACITY), 1 <= n_kf <= 64 (0 returns at once), finite rows 0 - 2 of every pose, and every limit of the
 * parameters below, min_votes <= the number of scans of the call among them (the cloud entry has one scan).  After a
 * refusal (QTR_ERR_BAD_ARG unless said otherwise) the map is exactly as it was.  n_kf = 0 or a map without voxels returns
 * at once with zero counts.
 * Device memory: n_scans x rows x cols x 4 bytes of images (256 KiB each at the defaults) and one byte per table slot,
 * allocated on the first call that needs them and grown only, plus the 164 bytes of staging per voxel an eviction takes;
 * all freed with the map.
 * The calls are host-synchronous and WRITE the map: the caller serialises them against inserts, clear, evict, restore, each
 * other and registrations on that map.  Messages go through qtr_last_error. */
#ifndef QUATRO_VOXELMAP_CARVE_C_H
#define QUATRO_VOXELMAP_CARVE_C_H

#include "quatro_voxelmap.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef QTR_EXT_API /* (libquatro_ext.so's exports: csrc/exports_ext.map lists them, csrc/exports.map does not) */
#define QTR_EXT_API QTR_API
#endif

#define QTR_CARVE_MAX_KEYFRAMES 64

typedef struct qtr_carve_params {
  int rows;            /* 64      1 .. 256 */
  int cols;            /* 1024    8 .. 4096 */
  int window;          /* 2       0 .. 3: the neighbourhood is (2 window + 1)^2 pixels */
  int min_votes;       /* 1       1 .. the number of scans of the call */
  double fov_up_deg;   /* 2.5     the top of the image, above fov_down_deg */
  double fov_down_deg; /* -25.5   its bottom */
  double margin_abs;   /* 0       metres, finite and >= 0; 0 means the map's voxel_size */
  double margin_rel;   /* 0       per metre of range, finite and >= 0 */
  double min_range;    /* 1       metres, below max_range */
  double max_range;    /* 80 */
  int reserved[8];
} qtr_carve_params;

typedef struct qtr_voxel_map_carve_info {
  int n_kept, n_carved;        /* voxels */
  int n_tested;                /* voxels at least one scan could vote on */
  int reserved;
  long long n_members_carved;  /* the carved voxels' members */
} qtr_voxel_map_carve_info;

QTR_EXT_API void qtr_default_carve_params(qtr_carve_params* p);
/* one cloud (n records of 16 bytes, x y z and a fourth float that is not read) in host or device memory (`mem` as in
 * qtr_voxel_map_insert), taken at `pose` (row-major 4x4, scan frame -> map frame, rows 0 - 2 read; NULL = identity) */
QTR_EXT_API int qtr_voxel_map_carve(qtr_handle* h, int slot, qtr_voxel_map* map, const float* xyz4, int n,
                                    const double pose[16], const qtr_carve_params* prm /* NULL = defaults */, int mem,
                                    qtr_voxel_map_carve_info* info /* may be NULL */);
/* n_kf keyframes of this handle, their stored voxels read in place, each under its pose (poses: n_kf x 16 doubles) */
QTR_EXT_API int qtr_voxel_map_carve_keyframes(qtr_handle* h, int slot, qtr_voxel_map* map, const qtr_keyframe* const* kfs,
                                              const double* poses, int n_kf, const qtr_carve_params* prm,
                                              qtr_voxel_map_carve_info* info);

#ifdef __cplusplus
}
#endif
#endif /* QUATRO_VOXELMAP_CARVE_C_H */
