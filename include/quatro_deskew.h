/* quatro_deskew.h - C ABI of motion compensation ("deskew") of a raw LiDAR sweep, exported by quatro_amd/libquatro_ext.so.
 *
 * libquatro_ext.so is the extension library beside libquatro_hip.so (include/quatro_hip.h, whose entry points stay exactly
 * what they were): it is built from the same sources and works on the handles libquatro_hip.so made; the three entry
 * points below are among its exports.  Both libraries must come from the same build.
 * The contract, bit-exact in binary64, is include/qtr_deskew_math.h.
 *
 * A spinning LiDAR takes the points of one sweep at different times while the sensor moves.  Given the time of every point
 * and K timed poses of the sensor ("knots": IMU or odometry samples, or the two ends of a constant-velocity guess), every
 * point is carried into the sensor frame at one reference time:
 *     q_i = T(t_ref)^-1 T(t_i) p_i,    T(t) = [ R_j Exp(s Log(R_j^T R_j+1)) | c_j + s (c_j+1 - c_j) ]
 * with j the knot interval of t and s the fraction inside it (rotation along the geodesic, translation linearly).  Times
 * before the first or after the last knot extrapolate the first or last interval and are counted.
 *   knot_times   K doubles, finite and strictly increasing, 2 <= K <= QTR_DESKEW_KNOTS_MAX; host memory, always
 *   knot_poses   K x 16 doubles, row-major 4x4 each, rows 0 - 2 read: sensor frame at knot_times[k] -> any fixed frame;
 *                consecutive knots may differ by a rotation of at most pi / 2; host memory, always
 *   times        P floats, the time of every point on the knots' time axis (`mem` says where xyz4, times and out live)
 *   t_ref        the time whose sensor frame the output is expressed in (the sweep's start for "poses at sweep start")
 * A point with a non-finite x, y, z or time is copied unchanged and counted as skipped; the fourth float of every record
 * is copied bit for bit.
 *   qtr_deskew                     xyz4 -> out_xyz4 (P records of 4 floats; out_xyz4 == xyz4 is allowed).  QTR_MEM_HOST: the
 *                                  buffers are staged and the call is complete on return; QTR_MEM_DEVICE: device pointers,
 *                                  used on the slot's stream, complete on return as well (the counts are read back).
 *   qtr_keyframe_create_deskewed   the sweep is deskewed into the slot's raw-cloud buffer and the call goes on as
 *                                  qtr_keyframe_create on that cloud, without a host wait in between and without the
 *                                  sweep returning to the host: the keyframe is, in every fetchable item, the one
 *                                  qtr_keyframe_create makes of qtr_deskew's output.
 *   qtr_deskew_pose_at             host only: T16 = T(t), row-major 4x4, by the same arithmetic.
 * Refused before anything is enqueued, with QTR_ERR_BAD_ARG: K < 2, K > 256, a non-finite or non-increasing knot time, a
 * non-finite entry in rows 0 - 2 of a knot pose, an interval rotation above the limit, a non-finite t_ref, NULL arrays
 * with P > 0, P < 0;  with QTR_ERR_CAPACITY: P > max_points.  P == 0: qtr_deskew returns QTR_OK with nothing done (the
 * knots are still judged); qtr_keyframe_create_deskewed refuses it as qtr_keyframe_create does.  Messages go through
 * qtr_last_error.  Device memory: 41 kB per slot, allocated on the slot's first call. */
#ifndef QUATRO_DESKEW_C_H
#define QUATRO_DESKEW_C_H

#include "quatro_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef QTR_EXT_API /* (libquatro_ext.so's exports: csrc/exports_ext.map lists them, csrc/exports.map does not) */
#define QTR_EXT_API QTR_API
#endif

#define QTR_DESKEW_KNOTS_MAX 256

typedef struct qtr_deskew_info {
  int n_points, n_skipped, n_extrapolated;
} qtr_deskew_info;

QTR_EXT_API int qtr_deskew(qtr_handle* h, int slot, const float* xyz4, const float* times, int P,
                           const double* knot_times, const double* knot_poses /* K x 16 */, int K, double t_ref,
                           float* out_xyz4, int mem, qtr_deskew_info* info /* may be NULL */);

QTR_EXT_API int qtr_keyframe_create_deskewed(qtr_handle* h, int slot, const float* raw4, const float* times, int P,
                                             const double* knot_times, const double* knot_poses, int K, double t_ref,
                                             const qtr_frontend_params* fp, int mem, qtr_keyframe** out,
                                             qtr_deskew_info* info /* may be NULL */);

QTR_EXT_API int qtr_deskew_pose_at(const double* knot_times, const double* knot_poses, int K, double t, double* T16);

#ifdef __cplusplus
}
#endif
#endif /* QUATRO_DESKEW_C_H */
