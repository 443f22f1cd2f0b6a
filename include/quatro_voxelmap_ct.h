/* quatro_voxelmap_ct.h - C ABI of the continuous-time registration of a RAW sweep against a voxel map, exported by
 * quatro_amd/libquatro_ext.so.
 *
 * The two entry points below work on the handles of libquatro_hip.so (include/quatro_hip.h) and the maps of
 * include/quatro_voxelmap.h, which says what the extension library is.  Both libraries must come from the same build.  The
 * arithmetic is include/qtr_vmap_ct_math.h.
 *
 * qtr_voxel_map_register takes a cloud that somebody deskewed under a guess of the sensor's motion and fits ONE rigid pose to
 * it.  qtr_voxel_map_register_ct takes the sweep as the sensor recorded it, with the time of every point, and fits the
 * sensor's pose at the END of the sweep, t_end, while its pose at the beginning, begin_pose at t_begin, is held fixed (the
 * previous sweep's end).  Inside every iteration each point is carried by the pose interpolated at its own time (rotation
 * along the geodesic, translation linearly: the rule of include/qtr_deskew_math.h), so the deskew is the registration's
 * result.  res->T is that end pose; the sweep is then deskewed under the two knots (t_begin, begin_pose), (t_end, res->T)
 * with qtr_deskew / qtr_keyframe_create_deskewed.  If every time equals t_end the call IS qtr_voxel_map_register under the
 * same guess, bit for bit.
 *
 * src4 / src_normals4: n records of 16 bytes (x, y, z, *), times: n floats, all in `mem`.  A point with a non-finite
 * coordinate or time or an unusable normal takes no part (info->n_skipped); a time outside [t_begin, t_end] extrapolates,
 * the point still takes part (info->n_extrapolated, counted among the points that are not skipped).
 *
 * Every argument is checked before anything is enqueued, in qtr_voxel_map_register's manner and with its codes: a map of
 * another handle, a method other than QTR_ICP_VOXEL_PLANE_TO_PLANE, n < 0, a NULL array with n > 0, a NULL begin_pose, a
 * non-finite entry in rows 0 - 2 of either pose, t_begin or t_end not finite, t_begin >= t_end, a difference that overflows,
 * and a guess that differs from begin_pose by a rotation above pi / 2 are QTR_ERR_BAD_ARG; n above max_points is
 * QTR_ERR_CAPACITY.  The map is only read: any number of slots may register against one map at once.  QTR_DBG_ICP_TRACE,
 * QTR_DBG_ICP_TIMES and QTR_DBG_ICP_CORR (qtr_debug_fetch) serve the call like any map registration. */
#ifndef QUATRO_VOXELMAP_CT_C_H
#define QUATRO_VOXELMAP_CT_C_H

#include "quatro_voxelmap.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef QTR_EXT_API /* (libquatro_ext.so's exports: csrc/exports_ext.map lists them, csrc/exports.map does not) */
#define QTR_EXT_API QTR_API
#endif

typedef struct qtr_vmap_ct_info {
  int n_points, n_skipped, n_extrapolated;
} qtr_vmap_ct_info;

QTR_EXT_API int qtr_voxel_map_register_ct(qtr_handle* h, int slot, const qtr_voxel_map* map, const float* src4, int n,
                                          const float* src_normals4, const float* times, double t_begin, double t_end,
                                          const double begin_pose[16], const double guess_end[16] /* NULL = begin_pose */,
                                          const qtr_icp_params* prm, qtr_icp_result* res, int mem,
                                          qtr_vmap_ct_info* info /* may be NULL */);
/* host only: the pose at time t between (t_begin, begin_pose) and (t_end, end_pose) by the registration's rule, row 3 =
 * (0 0 0 1).  QTR_ERR_BAD_ARG: a NULL pointer, times that are not finite with t_begin < t_end, or a refused interval */
QTR_EXT_API int qtr_voxel_map_ct_pose_at(double t_begin, double t_end, const double begin_pose[16], const double end_pose[16],
                                         double t, double* T16);

#ifdef __cplusplus
}
#endif
#endif /* QUATRO_VOXELMAP_CT_C_H */
