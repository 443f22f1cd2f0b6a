/* quatro_hip.h — C ABI of libquatro_hip.so, the MI355X (gfx950) back end behind the Quatro API.
 *
 * Plain C types only (no STL / Eigen / PCL / torch), never throws across the boundary: every call
 * returns an int status and the handle keeps a human-readable message (qtr_last_error).
 *
 * Each entry point replaces one call site of the reference (url-kaist/Quatro, cited as file:line):
 *   qtr_voxelize       <- voxelize<T>()                    include/quatro.hpp:49-68 (pcl::VoxelGrid)
 *   qtr_fpfh           <- teaser::FPFHEstimation::computeFPFHFeatures (4-arg)
 *                                                          src/teaser_utils/fpfh.cc:44-75
 *   qtr_match          <- teaser::Matcher::calculateCorrespondences
 *                                                          include/teaser_utils/feature_matcher.h:42-74,
 *                                                          src/teaser_utils/feature_matcher.cc:18-265
 *   qtr_solve          <- Quatro::computeTransformation(Eigen::Matrix4d&)
 *                                                          include/quatro.hpp:769-936
 *                         (computeTIMs :307, solveForScale :355, teaser::Graph + MaxCliqueSolver
 *                          include/teaser/graph.h:29-274 + src/graph.cc:12-104, solveForRotation2D :430,
 *                          solveForTranslation/estimate :585-747)
 *   qtr_max_clique     <- teaser::MaxCliqueSolver::findMaxClique(teaser::Graph)
 *                                                          include/teaser/graph.h:219-274, src/graph.cc:12-104
 *   qtr_compute_tims / qtr_scale_mask / qtr_gnc_rotation2d / qtr_cote_estimate
 *                      <- the public stage methods computeTIMs :307-344, solveForScale :355-386,
 *                         solveForRotation2D :430-572, estimate :618-747 of include/quatro.hpp
 *   qtr_patchwork      <- PatchWork::estimate_ground    include/patchwork.hpp:329-476
 *   qtr_segment_cloud  <- ImageProjection::segmentCloud ("Patchwork" mode) + getValidSegments / getOutliers
 *                                                          include/imageProjection.hpp:244-258,273-581
 *   qtr_submit_batch / qtr_wait <- the demo's loop over scan pairs (one Quatro object, reset() between
 *                         registrations)                   examples/run_global_registration.cpp:97-108
 *   qtr_icp / qtr_refine_pair <- pcl::IterativeClosestPoint(WithNormals)::align after the registration (the
 *                         reference class derives from pcl::Registration, include/quatro.hpp:131,151)
 *   qtr_gicp          <- pcl::GeneralizedIterativeClosestPoint::align, the plane-to-plane refinement usually paired
 *                         with Quatro (same pcl::Registration surface; covariances from the normals of both clouds)
 *   qtr_register_pair  <- the demo's whole path        examples/run_global_registration.cpp:206-246
 *                         (voxelize x2, FPFHManager::setFeaturePair include/fpfh_manager.hpp:98-153,
 *                          setInputSource/setInputTarget/computeTransformation)
 *
 * Point layout everywhere: float32 x,y,z,pad — 16 bytes per point, i.e. pcl::PointXYZ and the KITTI
 * .bin record (x,y,z,intensity; reference examples/run_global_registration.cpp:377-402) can be passed
 * without repacking.  The 4th float is ignored on input and written as 0 on output.
 *
 * Memory: `mem` selects where caller buffers live — QTR_MEM_HOST (pageable/pinned host memory; the
 * library stages through its own device arenas) or QTR_MEM_DEVICE (HBM pointers valid on the handle's
 * device; nothing is staged, results are written to the device buffers and the small qtr_result
 * record to host).  The caller owns all buffers; the library owns only its arenas inside the handle.
 *
 * Threading: one handle = one device + n_slots independent stream slots.  Calls on different slots
 * may be issued from different host threads; calls on the same slot must be externally serialised.
 */
#ifndef QUATRO_HIP_H
#define QUATRO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the entry points below are its whole dynamic symbol table. */
#if defined(__GNUC__)
#define QTR_API __attribute__((visibility("default")))
#else
#define QTR_API
#endif

#define QTR_OK 0
#define QTR_ERR_BAD_ARG 1          /* std::invalid_argument in the reference */
#define QTR_ERR_CLIQUE_TOO_SMALL 2 /* reference: solution_.valid = false, output untouched (quatro.hpp:809-813) */
#define QTR_ERR_CAPACITY 3         /* a qtr_limits bound or a caller buffer capacity was exceeded */
#define QTR_ERR_HIP 4              /* HIP runtime error (message in qtr_last_error) */
#define QTR_ERR_UNSUPPORTED 5      /* mode accepted by the reference's API but not built here */
#define QTR_ERR_IO 6               /* file missing / unreadable / malformed (qtr_read_*, qtr_write_*) */
#define QTR_ERR_NOT_RUN 7          /* batched pair whose record was never produced: the job failed before it was started
                                      (qtr_submit_batch fills every record with this until the pair's result is final) */

#define QTR_MEM_HOST 0
#define QTR_MEM_DEVICE 1

/* INLIER_SELECTION_MODE, reference include/quatro.hpp:184-189 */
#define QTR_INLIER_PMC_EXACT 0
#define QTR_INLIER_PMC_HEU 1
#define QTR_INLIER_KCORE_HEU 2
#define QTR_INLIER_NONE 3

typedef struct qtr_handle qtr_handle;

typedef struct qtr_limits {
  int max_points; /* raw points per cloud            (default 262144; reference loader caps at 250000) */
  int max_voxels; /* down-sampled points per cloud   (default 65536; at most 2^20 - 32: qtr_create refuses more) */
  int max_corr;   /* correspondences into the solver (default 24576) */
  int n_slots;    /* independent stream slots        (default 1) */
  int max_long_neighbors; /* per cloud: total entries of the radius-neighbour lists that are LONGER than 256 entries
                             (dense / un-voxelised clouds; a list of up to 256 entries costs nothing here).
                             0 = default = 128 * max_voxels.  pcl's radius search has no cap
                             (reference src/teaser_utils/fpfh.cc:58-72): exceeding this returns QTR_ERR_CAPACITY */
} qtr_limits;

/* The fields of Quatro::Params that the path consumes (reference include/quatro.hpp:202-268), plus the
 * public member noise_bound_ (:269, used by COTE :600-601) and estimated_RyRx_ (:159). */
#define QTR_REG_QUATRO 0
#define QTR_REG_TEASER 1
typedef struct qtr_params {
  double noise_bound;               /* 0.3 */
  double cbar2;                     /* 1.0 */
  double rotation_gnc_factor;       /* 1.4 */
  double rotation_cost_threshold;   /* 1e-6 (Params default); demo yaml 1.1e-4 */
  double kcore_heuristic_threshold; /* 0.5 */
  double cote_noise_bound;          /* Quatro::noise_bound_ = 0.3 */
  double ryrx[9];                   /* row-major estimated_RyRx_, identity */
  int rotation_max_iterations;      /* 100 (Params default); demo yaml 50 */
  int inlier_selection_mode;        /* QTR_INLIER_PMC_HEU */
  int cote_median;                  /* 1 = cote_mode "median", 0 = "weighted_mean" */
  int using_rot_inliers_when_estimating_cote; /* 0 */
  int using_pre_estimated_ryrx;     /* 0 */
  int reg_mode;                     /* QTR_REG_QUATRO (Params::reg_name "Quatro", yaw) or QTR_REG_TEASER (3-DoF, row (f)4) */
  double max_clique_time_limit;     /* 3600 s (include/quatro.hpp:267,800).  PMC_EXACT only; <= 0 = none.  When the limit
                                       is hit the heuristic's clique is returned (the reference returns PMC's best so far)
                                       and qtr_exact_stats reports it.  Per call: two threads with different limits on
                                       different slots do not see each other's */
} qtr_params;

/* Front-end knobs of the demo (reference examples/run_global_registration.cpp:37-55, config/params.yaml:22-25)
 * and of FPFHManager::setFeaturePair's matcher call (include/fpfh_manager.hpp:126-127). */
typedef struct qtr_frontend_params {
  float voxel_size;      /* 0.3 */
  float normal_radius;   /* 0.5 */
  float fpfh_radius;     /* 0.75 */
  float tuple_scale;     /* 0.95 */
  int use_crosscheck;    /* 1 */
  int use_tuple_test;    /* 1 */
  unsigned long long seed; /* tuple-test RNG seed (the reference seeds with time(NULL)) */
} qtr_frontend_params;

typedef struct qtr_result {
  int status;        /* same value the call returned */
  int valid;         /* solution_.valid */
  double T[16];      /* row-major 4x4 [R t; 0 1] */
  double cost;       /* Quatro::cost_ */
  int gnc_iters;
  int n_clique;      /* getNumMaxCliqueInliers() */
  int n_rot_inliers; /* getNumRotaionInliers() */
  int n_final;       /* getFinalInliersIndices().size() */
  int max_core;
  int n_edges;       /* undirected edges of the consistency graph */
  int n_card[3];     /* COTE consensus-set cardinality per axis */
  int n_src, n_tgt;  /* voxelised cloud sizes (qtr_register_pair) */
  int n_corr;        /* correspondences handed to the solver */
} qtr_result;

/* Per-stage GPU time of the last call on a slot, milliseconds (hipEvent based).  qtr_register_pair_corr runs its back end
 * BESIDE its front end (on a stream of its own): there graph is measured from the back end's start on that stream, clique
 * and solve on that stream, total from the call's first event to the point where the two streams have joined — so the
 * stage times of that entry point add up to MORE than total (under QTR_CORR_OVERLAP=0 graph starts at the matcher's end
 * and they add up to it, as elsewhere). */
typedef struct qtr_stage_times {
  float voxelize, fpfh, match, graph, clique, solve, total;
  float nn_kernel;  /* sum of the nearest-neighbour kernel launches of the last match (events on the launch stream) */
  int nn_launches;
  float graph_kernel; /* k_graph_build alone */
} qtr_stage_times;

QTR_API int qtr_create(int device, const qtr_limits* limits /* NULL = defaults */, qtr_handle** out);
QTR_API void qtr_destroy(qtr_handle* h);
QTR_API const char* qtr_last_error(const qtr_handle* h);
QTR_API void qtr_default_limits(qtr_limits* l);
QTR_API void qtr_default_params(qtr_params* p);                   /* Quatro::Params defaults */
QTR_API void qtr_demo_params(qtr_params* p);                      /* config/params.yaml values */
QTR_API void qtr_default_frontend_params(qtr_frontend_params* p);
QTR_API int qtr_num_slots(const qtr_handle* h);
QTR_API void* qtr_slot_stream(qtr_handle* h, int slot); /* hipStream_t of a slot */

/* K1.  out_xyz4 capacity `cap` points; *n_out receives the voxel count (output order = ascending
 * linear voxel index, as PCL).  If the grid would overflow int32 PCL passes the input through; so
 * does this call (then *n_out == P). */
QTR_API int qtr_voxelize(qtr_handle* h, int slot, const float* xyz4, int P, float leaf, float* out_xyz4, int cap, int* n_out,
                 int mem);

/* K2-K4.  normals4 (nx,ny,nz,curvature; may be NULL) and desc33 (n x 33 floats) */
QTR_API int qtr_fpfh(qtr_handle* h, int slot, const float* xyz4, int n, float r_normal, float r_fpfh, float* normals4,
             float* desc33, int mem);

/* K5-K8.  corr2 = L x (src index, tgt index), sorted lexicographically, capacity `cap` pairs. */
QTR_API int qtr_match(qtr_handle* h, int slot, const float* xyz4_s, int n_s, const float* desc33_s, const float* xyz4_t,
              int n_t, const float* desc33_t, const qtr_frontend_params* fp, int* corr2, int cap, int* L_out, int mem);

/* K9-K16.  src4/tgt4: the two equal-length matched keypoint clouds (setInputSource / setInputTarget).
 * clique / rot_inliers / final_inliers: optional int buffers of capacity `cap` (counts in *res). */
QTR_API int qtr_solve(qtr_handle* h, int slot, const float* src4, const float* tgt4, int L, const qtr_params* prm,
              qtr_result* res, int* clique, int* rot_inliers, int* final_inliers, int cap, int mem);

/* K10-K12 alone: the clique search on a caller-supplied graph.  adj = symmetric bit matrix, L rows of
 * ceil(L/64) uint64 words (bit j of row i set <=> edge i-j; the diagonal and bits >= L are ignored).
 * mode: QTR_INLIER_PMC_EXACT, QTR_INLIER_PMC_HEU or QTR_INLIER_KCORE_HEU (teaser CLIQUE_SOLVER_MODE 0 / 1 / 2).
 * PMC_EXACT ("next" row (f)4, src/graph.cc:106-127): the heuristic's clique when it is maximum, otherwise the first
 * maximum clique in the canonical depth-first order; at most 32768 vertices.  clique receives
 * the member ids in ascending order (capacity cap); *n_out their count; *max_core_out (may be NULL) the
 * largest core number. */
QTR_API int qtr_max_clique(qtr_handle* h, int slot, const unsigned long long* adj, int L, int mode, double kcore_thr,
                   double time_limit /* PMC_EXACT: MaxCliqueSolver::Params::time_limit, seconds; <= 0 = none */,
                   int* clique, int cap, int* n_out, int* max_core_out, int mem);

/* The reference class keeps its stages individually callable (computeTIMs :307, solveForScale :355,
 * solveForRotation2D :430, estimate :618); these entry points serve them from the same device code the fused
 * path uses.  Host buffers only; matrices are ROW-major (3 x N means three rows of N doubles).
 * Capacity: every call stages through the slot's solver arena — K (TIM columns) and M / N are limited to what
 * max_corr provides (3 K doubles <= 36 * max_corr doubles per operand); QTR_ERR_CAPACITY otherwise. */
QTR_API int qtr_compute_tims(qtr_handle* h, int slot, const double* v3n, int N, double* tims3k /* 3 x N(N-1)/2 */,
                     int* map2k /* 2 x N(N-1)/2: (i, j) of every column */);
QTR_API int qtr_scale_mask(qtr_handle* h, int slot, const double* tims_src3k, const double* tims_dst3k, long long K,
                   double noise_bound, double cbar2, unsigned char* mask /* K */);
QTR_API int qtr_gnc_rotation2d(qtr_handle* h, int slot, const double* src2m, const double* dst2m, int M, double noise_bound,
                       double gnc_factor, int max_iterations, double cost_threshold, double* R4 /* row-major 2x2 */,
                       double* cost, int* iterations, unsigned char* inliers /* M, weight >= 0.4 */);
/* "Next" row (f)4, second half: the 3-DoF rotation of reg_name "TEASER" (solveForRotation throws for it in the
 * reference, include/quatro.hpp:409-411; teaser::utils::svdRot, include/teaser/utils.h:123-149, is what it would
 * call): TEASER++'s GNC-TLS loop over 3-D TIMs.  Also reachable through qtr_solve with reg_mode = QTR_REG_TEASER. */
QTR_API int qtr_gnc_rotation3d(qtr_handle* h, int slot, const double* src3m, const double* dst3m, int M, double noise_bound,
                       double gnc_factor, int max_iterations, double cost_threshold, double* R9 /* row-major 3x3 */,
                       double* cost, int* iterations, unsigned char* inliers /* M, weight >= 0.4 */);
QTR_API int qtr_cote_estimate(qtr_handle* h, int slot, const double* X, int N, double range /* uniform */, int median_selection,
                      double* estimate, unsigned char* inliers /* N */, int* n_card);
/* the same with one range per element (estimate() takes a RowVectorXd of ranges, include/quatro.hpp:618-630) */
QTR_API int qtr_cote_estimate_ranges(qtr_handle* h, int slot, const double* X, const double* ranges, int N, int median_selection,
                             double* estimate, unsigned char* inliers /* N */, int* n_card);

/* PMC_EXACT only: search-tree nodes of the slot's last exact search and whether its time limit
 * (qtr_params.max_clique_time_limit / qtr_max_clique's time_limit) was hit. */
QTR_API int qtr_exact_stats(qtr_handle* h, int slot, unsigned long long* nodes, int* aborted);

/* "Next" row (f)3: on-disk formats either side of the path (host code, no GPU work, no handle).
 *   qtr_read_kitti_bin <- getCloud, examples/run_global_registration.cpp:377-402: float32 x,y,z,intensity records,
 *                         at most max_points of them (the demo reads 1 000 000 floats = 250 000 points).
 *   qtr_write_pcd_xyz / qtr_read_pcd_xyz <- the matched-pair cache of FPFHManager::saveFeaturePair / loadFeaturePair
 *                         (include/fpfh_manager.hpp:179-232): PCD v0.7, fields x y z.  binary = 0 writes what
 *                         pcl::io::savePCDFile writes by default (DATA ascii, 8 significant digits); the reader takes
 *                         ascii, binary and binary_compressed files and picks x, y, z by field name.
 * Points are 16-byte x,y,z,w records like everywhere else in this ABI (w: intensity for .bin, 0 for PCD).
 * qtr_read_pcd_xyz always reports the file's point count; QTR_ERR_CAPACITY when cap is smaller. */
QTR_API int qtr_read_kitti_bin(const char* path, float* xyzi, int max_points, int* n_points);
QTR_API int qtr_write_pcd_xyz(const char* path, const float* xyz4, int n, int binary);
QTR_API int qtr_read_pcd_xyz(const char* path, float* xyz4, int cap, int* n_points);

/* "Next" row (f)2: Patchwork ground segmentation, the first stage of the reference demo on raw scans
 * (PatchWork::estimate_ground, include/patchwork.hpp:329-476; parameters config/patchwork_params.yaml).
 * ground_xyzw / nonground_xyzw: the input records (16 bytes each, 4th float preserved) in the reference's output
 * order (zone, ring, sector; ascending height inside a patch); capacities in points (P always suffices). */
typedef struct qtr_pw_params {
  double sensor_height;                     /* 1.723 */
  int num_iter, num_lpr, num_min_pts;       /* 3, 20, 80 */
  double th_seeds, th_dist, max_range, min_range, uprightness_thr, adaptive_seed_selection_margin;
  int using_global_thr;
  double global_elevation_thr;
  int num_zones;                            /* <= 4 */
  int num_sectors_each_zone[4], num_rings_each_zone[4];
  double min_ranges[4];
  int num_thr;                              /* size of the two threshold vectors (<= 8) */
  double elevation_thr[8], flatness_thr[8];
} qtr_pw_params;
QTR_API void qtr_pw_default_params(qtr_pw_params* p); /* config/patchwork_params.yaml */
QTR_API int qtr_patchwork(qtr_handle* h, int slot, const float* xyz4, int P, const qtr_pw_params* pw, float* ground_xyzw,
                  int cap_ground, int* n_ground, float* nonground_xyzw, int cap_nonground, int* n_nonground, int mem);

/* "Next" row (f)1: range-image projection + sub-cluster rejection, the stage before voxelisation in the reference
 * demo (ImageProjection::segmentCloud in "Patchwork" mode + getValidSegments / getOutliers,
 * include/imageProjection.hpp:244-258,273-294).  Input: the non-ground points of one scan in sensor order.
 * valid_xyzl: x,y,z,label of every pixel of a valid segment, row-major over the range image; outl_xyzi: the
 * rejected sub-clusters (x, y, z, row + col/10000 as in the reference :345).  Capacities in points
 * (n_scan * horizon_scan always suffices).  labelmat (optional, host only): n_scan x horizon_scan int32,
 * -1 no return / 999999 rejected / label >= 1. */
typedef struct qtr_ip_params {
  int n_scan, horizon_scan;            /* 64, 1800 for "Velodyne-64-HDE" */
  float ang_res_x, ang_res_y, ang_bottom;
  int neighbor_mode;                   /* 0 "4Neighbor", 1 "8Neighbor", 2 "4CrossNeighbor" */
  int num_min_pts;                     /* numMinPtsForSubclustering, 30 */
  float segment_theta;                 /* 60 deg in rad */
  int valid_point_num, valid_line_num; /* 5, 3 */
} qtr_ip_params;
/* lidar_type: "Velodyne-64-HDE", "VLP-16", "HDL-32E", "Ouster-OS1-16", "Ouster-OS1-64"; neighbor_mode: as above.
 * Returns QTR_ERR_BAD_ARG for names the reference's constructor rejects (:131, :140). */
QTR_API int qtr_ip_default_params(const char* lidar_type, const char* neighbor_mode, qtr_ip_params* p);
QTR_API int qtr_segment_cloud(qtr_handle* h, int slot, const float* xyz4, int P, const qtr_ip_params* ip, float* valid_xyzl,
                      int cap_valid, int* n_valid, float* outl_xyzi, int cap_outl, int* n_outl, int* n_segments,
                      int* labelmat, int mem);

/* Whole path on one slot: raw scans -> transform. */
QTR_API int qtr_register_pair(qtr_handle* h, int slot, const float* src_raw4, int Ps, const float* tgt_raw4, int Pt,
                      const qtr_frontend_params* fp, const qtr_params* prm, qtr_result* res, int* clique,
                      int* final_inliers, int cap, int mem);

/* The whole path of one pair whose back end runs on correspondences the CALLER brings (a cache of matched keypoints:
 * FPFHManager::loadFeaturePair, include/fpfh_manager.hpp:211-232; another matcher) while the scans still go through the
 * front end — the single-pair form of a qtr_pair_desc with both scans and src_corr4 / tgt_corr4 set (see
 * qtr_submit_batch), and the unit of work BASELINE's metric is quoted on: a KITTI-64 pair's voxel grid + FPFH + matching
 * AND a ~5 k-correspondence computeTransformation, as ONE call.  The back end reads the caller's correspondences alone,
 * so it is enqueued on a stream of its own as soon as the voxel grid is on its way and runs BESIDE the front end; the
 * call returns when both are done (a front end that fails returns its status and counts, after the back end has let go
 * of the correspondences).  The back end is still ordered behind whatever the slot's stream (qtr_slot_stream) held when
 * the call was made: device correspondences written there — the device outputs of an earlier call, a caller's own
 * matcher — need not be complete, only enqueued.  QTR_CORR_OVERLAP=0 in the environment at qtr_create keeps the serial order — the back end
 * enqueued when the matcher's counters arrive, behind the front end as in qtr_register_pair; results are the same bit for
 * bit.  res->n_src / n_tgt report the voxel counts, res->n_corr = n_corr; n_matched (optional) receives the
 * matcher's own correspondence count.  corr_*4: n_corr 16-byte records each, same `mem` as the scans. */
QTR_API int qtr_register_pair_corr(qtr_handle* h, int slot, const float* src_raw4, int Ps, const float* tgt_raw4, int Pt,
                                   const qtr_frontend_params* fp, const float* corr_src4, const float* corr_tgt4, int n_corr,
                                   const qtr_params* prm, qtr_result* res, int* n_matched, int* clique, int* final_inliers,
                                   int cap, int mem);

/* Front end of one pair on one slot: raw scans -> matched keypoint clouds.  What the reference's caller does between
 * loading two scans and handing the keypoints to Quatro (examples/run_global_registration.cpp:206-221): `voxelize` x2
 * (include/quatro.hpp:49-68), FPFHManager::setFeaturePair (include/fpfh_manager.hpp:98-153: FPFH x2 + reciprocal
 * matching with cross check and tuple test), getSrcKps / getTgtKps / getCorrespondences (:172-177,234).  The same
 * launch chain as qtr_register_pair up to the solver.  n_src / n_tgt (optional) receive the voxelised cloud sizes, *L
 * the number of correspondences; src_kps4 / tgt_kps4 (optional, capacity `cap` 16-byte records) the matched keypoints in
 * correspondence order, corr2 (optional, cap x 2 ints) the (source, target) voxel indices.  mem = QTR_MEM_HOST: outputs
 * complete on return; QTR_MEM_DEVICE: outputs are written on the slot's stream (qtr_slot_stream).  The matched clouds
 * also stay in the slot, where a following qtr_solve on device pointers can be issued without a copy. */
QTR_API int qtr_feature_pair(qtr_handle* h, int slot, const float* src_raw4, int Ps, const float* tgt_raw4, int Pt,
                     const qtr_frontend_params* fp, int* n_src, int* n_tgt, int* L, float* src_kps4, float* tgt_kps4,
                     int* corr2, int cap, int mem);

/* Batched registration (BASELINE configs[2] / [3]; the reference's usage is one Quatro object reused over many pairs,
 * examples/run_global_registration.cpp:97-108).  B independent pairs go through the SAME kernels as qtr_register_pair,
 * a group of pairs per launch (blockIdx.z = pair): the handle's stream slots are split into two lanes of
 * n_slots / 2 pairs each, a lane runs voxelise -> FPFH + matching -> solver as three launch chains with ONE host
 * read-back of the device-side sizes per chain and group (not per pair), and the two lanes alternate so that one's
 * kernels cover the other's read-back.  Results are bit-identical to B sequential qtr_register_pair calls.
 *   qtr_submit_batch  validates, records the job and enqueues the first chains; returns without waiting.
 *   qtr_wait          drives the job to completion (call it from the same thread).  results[i] receives pair i's
 *                     record (its own status: QTR_OK, QTR_ERR_CLIQUE_TOO_SMALL, QTR_ERR_CAPACITY ...); the return
 *                     value is QTR_OK unless the job itself failed (HIP error, bad argument) — then every pair that
 *                     had finished keeps its record, pairs that were in flight read QTR_ERR_HIP, pairs never started
 *                     QTR_ERR_NOT_RUN, and the handle is drained and usable.  A job of qtr_submit_batch_refine
 *                     (below) also fills refined[i]; on a job failure a pair's refined record reads the same status
 *                     as its result, or QTR_ERR_HIP when its registration finished and its refinement did not.
 * pairs / results must stay valid until qtr_wait returns; one job at a time per handle; every slot of the handle is
 * used (do not run slot calls concurrently).  mem as elsewhere (raw scans and the optional index lists). */
typedef struct qtr_pair_desc {
  const float* src_raw4; /* raw source scan, 16-byte x,y,z,* records (NULL together with tgt_raw4: no front end, see below) */
  int n_src;
  const float* tgt_raw4;
  int n_tgt;
  unsigned long long seed; /* tuple-test RNG seed of this pair (qtr_frontend_params.seed is ignored) */
  int* clique;             /* optional: getMaxCliques indices, capacity `cap` ints (NULL: not wanted) */
  int* final_inliers;      /* optional: getFinalInliersIndices */
  int cap;
  /* Pre-matched correspondences (optional; all three zero: the matcher's own output feeds the back end).  The
   * reference's loop hands Quatro whatever matched keypoint clouds its caller has — setInputSource / setInputTarget /
   * computeTransformation, examples/run_global_registration.cpp:243-246, include/quatro.hpp:769 — so a pair may bring
   * them along: src_corr4[i] <-> tgt_corr4[i], n_corr 16-byte records each, same `mem` as the scans.
   *   scans NULL, correspondences given : the back end alone (qtr_solve's work, batched); n_src / n_tgt ignored
   *   scans AND correspondences given   : the front end runs on the scans (result.n_src / n_tgt report its voxel
   *                                       counts) and the back end runs on the GIVEN correspondences instead of the
   *                                       matcher's — the unit of work BASELINE's metric is quoted on (a KITTI-64
   *                                       pair's front end + a ~5 k-correspondence back end) for callers whose
   *                                       correspondences come from elsewhere (a cache: FPFHManager::loadFeaturePair,
   *                                       include/fpfh_manager.hpp:211-232)
   * result.n_corr reports the correspondences the back end ran on.  n_corr = 0 with both pointers set is the
   * reference's "clique too small" outcome; n_corr > max_corr is QTR_ERR_CAPACITY in the pair's record. */
  const float* src_corr4;
  const float* tgt_corr4;
  int n_corr;
} qtr_pair_desc;
QTR_API int qtr_submit_batch(qtr_handle* h, const qtr_pair_desc* pairs, int B, const qtr_frontend_params* fp,
                     const qtr_params* prm, qtr_result* results, int mem);
QTR_API int qtr_wait(qtr_handle* h);
/* Raw sweeps through the batched entry: with parameters set here qtr_submit_batch runs the demo's STEP 2 and 3 in front of
 * the voxel grid on every scan it is given (reference examples/run_global_registration.cpp:136-160:
 * PatchWork::estimate_ground -> non-ground points -> ImageProjection::segmentCloud -> getValidSegments), i.e. the pair
 * descriptors then carry raw scans WITH their ground returns and a batch reproduces the demo's whole sequence per pair.
 * pw = ip = NULL switches it off again (the default).  A scan that is all ground gets QTR_ERR_BAD_ARG in its own record. */
QTR_API int qtr_set_batch_preprocess(qtr_handle* h, const qtr_pw_params* pw, const qtr_ip_params* ip);

/* Multi-GPU (BASELINE configs[3]): pairs are independent, so every process / device registers its own block of pair
 * ids and the ONLY exchange is the final gather of the fixed-size result records — RCCL over xGMI (one ncclAllGather of
 * n_local * sizeof(qtr_result) bytes per rank; latency-bound, far from link bandwidth).  One handle = one rank.
 *   qtr_comm_unique_id   rank 0 creates the 128-byte rendezvous id; the host application hands it to the other ranks
 *                        (MPI, a file, torch.distributed.broadcast ...)
 *   qtr_comm_init        joins the communicator on the handle's device (collective: every rank calls it)
 *   qtr_gather_results   all-gather: `all` receives world * n_local records in rank order on EVERY rank; n_local must
 *                        be the same on all ranks (QTR_ERR_BAD_ARG on every rank otherwise — nothing is overrun)
 *   qtr_gather_results_v the same for blocks of DIFFERENT lengths (a block partition of B pairs over `world` ranks
 *                        differs by one record between ranks; BASELINE configs[3]: 4096 pairs over any world size):
 *                        the counts are exchanged first, the blocks padded to the longest for the fixed-size
 *                        collective and trimmed on the way out.  `all` (capacity cap_all records) receives the
 *                        sum(counts) records in rank order, counts[world] (optional) every rank's count, *n_all
 *                        (optional) the total.  Collective: every rank calls it, also with n_local = 0.  When the
 *                        records do not fit SOME rank's cap_all, EVERY rank returns QTR_ERR_CAPACITY (the capacities
 *                        travel with the counts, so no rank is left waiting in the second collective).
 * librccl is opened at run time (dlopen), so single-GPU users do not need it.  QTR_ERR_HIP with the RCCL message in
 * qtr_last_error on failure. */
#define QTR_COMM_ID_BYTES 128
QTR_API int qtr_comm_unique_id(char id[QTR_COMM_ID_BYTES]);
QTR_API int qtr_comm_init(qtr_handle* h, const char id[QTR_COMM_ID_BYTES], int rank, int world);
QTR_API int qtr_gather_results(qtr_handle* h, const qtr_result* local, int n_local, qtr_result* all);
QTR_API int qtr_gather_results_v(qtr_handle* h, const qtr_result* local, int n_local, qtr_result* all, int cap_all, int* counts,
                         int* n_all);
QTR_API void qtr_comm_destroy(qtr_handle* h);

QTR_API int qtr_get_stage_times(qtr_handle* h, int slot, qtr_stage_times* out);
/* Instrumentation (no reference counterpart; the demo times its stages with std::chrono around the calls,
 * examples/run_global_registration.cpp:206-246).  qtr_set_stage_events(0) stops recording events altogether (every
 * stage field of qtr_stage_times and its total then read 0: an event record is a marker the queue retires before the
 * next launch starts, and a call recorded three to six of them); the two nearest-neighbour launches keep their event pairs, whose
 * elapsed times accumulate per slot: qtr_get_nn_totals returns (and optionally resets) the sum and the launch count
 * without a per-call query.  An event pair attached to a launch costs ~5 us of queue time on either side of it (four
 * such gaps per registration): qtr_set_nn_event_stride(h, n) attaches the pairs to every n-th match of a slot only
 * (default 1: every match; 0: never) — the totals then cover the launches that were timed. */
QTR_API int qtr_set_stage_events(qtr_handle* h, int on);
QTR_API int qtr_set_nn_event_stride(qtr_handle* h, int every);
QTR_API int qtr_get_nn_totals(qtr_handle* h, int slot, double* total_ms, long long* launches, int reset);
/* The two launches behind qtr_stage_times.nn_kernel apart, milliseconds (0 when the last match carried no events): every
 * row of the smaller cloud against the larger one, and the rows of the larger cloud that were chosen against the smaller
 * one — the two FLANN searches of teaser::Matcher::advancedMatching (src/teaser_utils/feature_matcher.cc:100-122).  A
 * call of its own rather than two more fields: qtr_stage_times keeps its size for callers built against earlier headers. */
QTR_API int qtr_get_nn_dir_times(qtr_handle* h, int slot, float* dir1_ms, float* dir2_ms);

/* 6-DoF ICP refinement of a registration (the step after a global registration: Quatro recovers yaw and translation only,
 * roll / pitch come from the caller's estimated_RyRx_).  pcl::IterativeClosestPoint's knobs (pcl::Registration /
 * DefaultConvergenceCriteria); the whole loop runs on the device, one launch per iteration and no host read-back inside it.
 *   correspondence: the NEAREST target point within max_correspondence_distance of R p + t (binary64 distances, ties
 *                   to the lowest target index); non-finite points of either cloud are ignored; point-to-plane also drops
 *                   a correspondence whose target normal is not finite
 *   point-to-plane: one Gauss-Newton step of sum ((q - t) . n)^2 per iteration (6x6 LDL^T; rotation increment from the
 *                   normalised quaternion (1, w/2)); point-to-point: the closed-form rotation of the cross-covariance
 *   plane-to-plane: Generalized ICP (pcl::GeneralizedIterativeClosestPoint / fast_gicp) with the plane-regularised
 *                   covariances C = I - (1 - eps) n n^T of BOTH clouds' normals, eps = QTR_ICP_GICP_EPSILON = 1e-3
 *                   (include/qtr_icp_math.h; a constant, because this struct may not grow): one Gauss-Newton step of
 *                   sum d^T (C_b + R C_a R^T)^-1 d per iteration, d = q - t, the same 6x6 solve and increment.  A source
 *                   point whose normal is not finite or has zero length is skipped; a correspondence whose target normal
 *                   is not finite or has zero length is dropped.  rmse = sqrt(mean d^T M d), fitness = mean d^2
 *   voxelised plane-to-plane: VGICP (Koide et al., ICRA 2021; fast_gicp's FastVGICP) — the search is replaced by a lookup.
 *                   The target is summarised once per call as one Gaussian per voxel of side max_correspondence_distance
 *                   (grid origin: the minimum of the finite target points; never coarsened: a grid of more than 2^22 cells
 *                   is QTR_ERR_CAPACITY): member count N, mean mu of the members, C_b = I - (1 - eps) mean(n n^T); members
 *                   are the finite target points with a usable normal, summed in ascending index.  A transformed source
 *                   point is matched to the voxel it falls into (none outside the grid or in a voxel without members; no
 *                   distance test): d = q - mu, weight N, one Gauss-Newton step of sum N d^T (C_b + R C_a R^T)^-1 d.
 *                   Unlike the three search methods the result depends on the grid, hence on the distance as voxel side.
 *                   fitness = mean d^2, rmse = sqrt(sum N d^T M d / sum N); QTR_DBG_ICP_CORR reports a voxel as the
 *                   lowest target index among its members.  The contract is include/qtr_icp_math.h's
 *   stopping:       max_iterations updates; max |dT - I| <= transformation_epsilon; |mse - mse_prev| <=
 *                   euclidean_fitness_epsilon * mse_prev; fewer than min_correspondences correspondences (valid = 0, T the
 *                   last good transform); a rank-deficient system, e.g. a single plane (valid = 0, T the last good one)
 * Sizes above qtr_limits.max_voxels per cloud: QTR_ERR_CAPACITY.  Empty clouds: QTR_OK with valid = 0 and T = guess.
 * The arena is allocated on a slot's first ICP call. */
#define QTR_ICP_POINT_TO_PLANE 0
#define QTR_ICP_POINT_TO_POINT 1
#define QTR_ICP_PLANE_TO_PLANE 2
#define QTR_ICP_VOXEL_PLANE_TO_PLANE 3
#define QTR_ICP_MAX_ITERATIONS 1000 /* largest max_iterations accepted */
/* qtr_icp_result.stop_reason */
#define QTR_ICP_STOP_NONE 0
#define QTR_ICP_STOP_MAX_ITERATIONS 1
#define QTR_ICP_STOP_TRANSFORMATION 2
#define QTR_ICP_STOP_FITNESS 3
#define QTR_ICP_STOP_TOO_FEW 4
#define QTR_ICP_STOP_DEGENERATE 5
typedef struct qtr_icp_params {
  double max_correspondence_distance; /* 1.0 m (setMaxCorrespondenceDistance) */
  double transformation_epsilon;      /* 1e-7: max |dT - I| of an update (setTransformationEpsilon) */
  double euclidean_fitness_epsilon;   /* 1e-6: relative change of the correspondences' MSE (setEuclideanFitnessEpsilon) */
  int max_iterations;                 /* 30 (setMaximumIterations), 1 .. QTR_ICP_MAX_ITERATIONS */
  int method;                         /* QTR_ICP_POINT_TO_PLANE (default), _POINT_TO_POINT, _PLANE_TO_PLANE,
                                         _VOXEL_PLANE_TO_PLANE */
  int min_correspondences;            /* 0 = the method's minimum: 6 point-to-plane, 3 point-to-point,
                                         4 plane-to-plane (voxelised or not) */
  float normal_radius;                /* 0.5 m: normals of qtr_icp / qtr_gicp that the caller does not pass (the FPFH
                                         stage's normal estimation); qtr_refine_pair uses the registration's normals */
} qtr_icp_params;
typedef struct qtr_icp_result {
  int status, valid, converged, stop_reason, iterations, n_corr;
  double T[16];   /* row-major, maps source into target */
  double fitness; /* mean squared distance of the last evaluated correspondences (pcl getFitnessScore) */
  double rmse;    /* sqrt of the mean squared residual the method minimises (point-to-plane distance / point distance) */
} qtr_icp_result;
QTR_API void qtr_default_icp_params(qtr_icp_params* p);
/* src4 (n_s) / tgt4 (n_t): 16-byte records; tgt_normals4: n_t records nx,ny,nz,* (point-to-plane and plane-to-plane; NULL:
 * computed at normal_radius).  guess: row-major 4x4 (NULL = identity).  mem: where the clouds live.  Plane-to-plane
 * computes the source normals at normal_radius: qtr_icp(method 2 or 3) is qtr_gicp with src_normals4 = NULL. */
QTR_API int qtr_icp(qtr_handle* h, int slot, const float* src4, int n_s, const float* tgt4, int n_t, const float* tgt_normals4,
                    const double guess[16], const qtr_icp_params* prm, qtr_icp_result* res, int mem);
/* Plane-to-plane for callers who bring both normal sets: src_normals4 (n_s records, source frame) / tgt_normals4 (n_t
 * records); either may be NULL (computed at normal_radius).  prm->method must be QTR_ICP_PLANE_TO_PLANE or
 * QTR_ICP_VOXEL_PLANE_TO_PLANE (QTR_ERR_BAD_ARG otherwise).  Validation, capacity, empty clouds, mem and the QTR_DBG_ICP_* items as qtr_icp. */
QTR_API int qtr_gicp(qtr_handle* h, int slot, const float* src4, int n_s, const float* src_normals4, const float* tgt4, int n_t,
                     const float* tgt_normals4, const double guess[16], const qtr_icp_params* prm, qtr_icp_result* res, int mem);
/* Refines the slot's last qtr_register_pair / qtr_register_pair_corr on its voxelised clouds (the CALLER's source and
 * target) and the normals its FPFH stage left in the slot (the target's; plane-to-plane: the source's too): no copy, no
 * recomputation.  guess NULL = that call's T.
 * QTR_ERR_BAD_ARG when the slot's last call was not a registration.  Leaves the registration's state untouched (it may be
 * refined again, with other parameters). */
QTR_API int qtr_refine_pair(qtr_handle* h, int slot, const double guess[16], const qtr_icp_params* prm, qtr_icp_result* res);
/* Batched registration AND refinement: qtr_submit_batch's contract (validation, one job per handle, qtr_wait drives it),
 * and refined[i] receives pair i's ICP refinement with `icp`.  results[i] are bit-identical to qtr_submit_batch's;
 * refined[i] is bit-identical (T, iterations, stop_reason, n_corr, fitness, rmse, valid, converged) to what
 * qtr_refine_pair(h, slot, NULL, icp, ...) returns right after a qtr_register_pair of that pair: ICP on the pair's voxelised
 * clouds (the pre-processed sweeps' with qtr_set_batch_preprocess on) and the target normals of its FPFH stage, from the
 * registration's T.  A pair with scans AND correspondences is refined on the scans' clouds from the T of the given
 * correspondences.  Refined: pairs that ran the front end and whose result status is QTR_OK or QTR_ERR_CLIQUE_TOO_SMALL
 * (refined[i].status = QTR_OK).  Every other pair — correspondences only, or a failed registration — gets
 * refined[i].status = QTR_ERR_NOT_RUN, valid = 0 and T = results[i].T.  A NULL or invalid icp, or refined = NULL with
 * B > 0: QTR_ERR_BAD_ARG with nothing enqueued.  pairs / results / refined must stay valid until qtr_wait returns; the
 * records are host structs whatever `mem` says.  Each slot's ICP arena is allocated on the first refining batch.  After
 * the job, qtr_refine_pair on any slot returns QTR_ERR_BAD_ARG, as after qtr_submit_batch. */
QTR_API int qtr_submit_batch_refine(qtr_handle* h, const qtr_pair_desc* pairs, int B, const qtr_frontend_params* fp,
                                    const qtr_params* prm, const qtr_icp_params* icp, qtr_result* results,
                                    qtr_icp_result* refined, int mem);

/* Keyframes: the products of ONE scan's front end (voxel grid, normals, FPFH, the matcher's sequential mean and its
 * per-descriptor preparation) kept on the device, in an allocation sized to the scan, so that a scan that is registered
 * more than once pays for its front end once.  Loop closing registers one query against K candidates with K + 1 front
 * ends instead of 2 K; odometry reuses scan k's keyframe as the source of pair (k, k + 1), the reference's
 * FPFHManager::is_odometry_test_ / swapTgt2Src (include/fpfh_manager.hpp:111-118) without the trip through host vectors.
 * Results are bit-identical to the raw-scan entries (qtr_register_pair, qtr_submit_batch, qtr_submit_batch_refine).
 *   qtr_keyframe_create     runs the one-cloud front end on `slot` — with qtr_register_pair's rules: the pcl::VoxelGrid
 *                           pass-through, the capacity errors and their messages — and packs what a registration needs
 *                           into one device allocation: 176 bytes per voxel plus alignment, device_bytes <=
 *                           256 * n_voxels + 4096 (about 3 MB for a 16 k-voxel KITTI scan).  A set-up call: it returns
 *                           after the pack has completed, whatever `mem` says; the caller's scan is free on return and
 *                           nothing of the keyframe aliases slot memory.  The keyframe belongs to the handle;
 *                           qtr_destroy frees the keyframes the caller did not destroy.
 *   qtr_keyframe_fetch      copies a stored item to host memory, like qtr_debug_fetch: up to `bytes` bytes to `dst`, returns
 *                           the bytes the item holds or < 0
 *   qtr_keyframe_destroy    frees it.  Destroying a keyframe that a pending batch names is the caller's error, as is using
 *                           one afterwards.
 *   qtr_register_keyframes  the whole path of qtr_register_pair with the two front ends replaced by ONE copy launch that
 *                           loads both keyframes into the slot's cloud arenas; the matcher, the solver and everything that
 *                           reads the slot afterwards (qtr_refine_pair with every method, QTR_DBG_VOX_SRC / _TGT, QTR_DBG_CORR)
 *                           work as after qtr_register_pair.  fp->voxel_size, normal_radius and fpfh_radius must equal BOTH
 *                           keyframes' (compared as float bits; QTR_ERR_BAD_ARG otherwise); tuple_scale, use_crosscheck,
 *                           use_tuple_test and seed are free per call.  A keyframe of another handle: QTR_ERR_BAD_ARG.
 *                           kf_src == kf_tgt is legal.  res->n_src / n_tgt are the keyframes' voxel counts;
 *                           qtr_stage_times.voxelize and .fpfh read 0 (.match covers the load and the matcher).  clique /
 *                           final_inliers are host buffers.  Keyframes are immutable: any number of slots, from different
 *                           host threads, may register against the same keyframe at once. */
typedef struct qtr_keyframe qtr_keyframe; /* opaque, owned by the handle that made it */
typedef struct qtr_keyframe_info {
  int n_points, n_voxels;                       /* raw points in, down-sampled points kept */
  float voxel_size, normal_radius, fpfh_radius; /* the front-end knobs baked into it */
  int passed_through;                           /* 1: pcl::VoxelGrid's int32-overflow pass-through happened */
  unsigned long long device_bytes;              /* HBM this keyframe holds */
} qtr_keyframe_info;
#define QTR_KF_VOX 1     /* float4[n_voxels] */
#define QTR_KF_NORMALS 2 /* float4[n_voxels] nx,ny,nz,curvature */
#define QTR_KF_FPFH 3    /* float[n_voxels][33] */
#define QTR_KF_MEAN 4    /* float[4] sequential float mean of the voxels (Matcher::normalizePoints) */
QTR_API int qtr_keyframe_create(qtr_handle* h, int slot, const float* raw4, int P, const qtr_frontend_params* fp, int mem,
                                qtr_keyframe** out);
QTR_API int qtr_keyframe_get_info(const qtr_keyframe* kf, qtr_keyframe_info* info);
QTR_API long long qtr_keyframe_fetch(qtr_handle* h, const qtr_keyframe* kf, int what, void* dst, size_t bytes);
QTR_API void qtr_keyframe_destroy(qtr_handle* h, qtr_keyframe* kf);
QTR_API int qtr_register_keyframes(qtr_handle* h, int slot, const qtr_keyframe* kf_src, const qtr_keyframe* kf_tgt,
                                   const qtr_frontend_params* fp, const qtr_params* prm, qtr_result* res, int* clique,
                                   int* final_inliers, int cap);
/* Batched registration of keyframe pairs: qtr_submit_batch's lanes with the voxel chain gone and the FPFH chain replaced
 * by one grouped load; the solver chain and, with icp != NULL, the refinement phases of qtr_submit_batch_refine are the
 * same.  results[i] / refined[i] are bit-identical to what those entries produce for the raw scans of the keyframes.
 * One query against K candidates is K descriptors with the same src.  icp = NULL: no refinement, and refined must be NULL
 * too; icp != NULL: refined is required.  Contract as qtr_submit_batch: one job per handle, driven by qtr_wait, every
 * record pre-filled with QTR_ERR_NOT_RUN, per-pair statuses, qtr_refine_pair refused afterwards.  All arguments are
 * validated before anything is enqueued — a NULL or foreign keyframe, or one whose radii differ from fp's, in ANY pair:
 * QTR_ERR_BAD_ARG and no job.  pairs, results, refined AND every keyframe named must stay valid until qtr_wait returns;
 * clique / final_inliers are host buffers. */
typedef struct qtr_kf_pair_desc {
  const qtr_keyframe* src;
  const qtr_keyframe* tgt;
  unsigned long long seed; /* tuple-test RNG seed of this pair (qtr_frontend_params.seed is ignored) */
  int* clique;             /* optional, capacity `cap` ints */
  int* final_inliers;      /* optional */
  int cap;
} qtr_kf_pair_desc;
QTR_API int qtr_submit_batch_keyframes(qtr_handle* h, const qtr_kf_pair_desc* pairs, int B, const qtr_frontend_params* fp,
                                       const qtr_params* prm, const qtr_icp_params* icp, qtr_result* results,
                                       qtr_icp_result* refined);

/* Submap keyframes: K keyframes fused under K poses into ONE keyframe, on the device.  Loop closing in LiDAR SLAM registers a
 * query against the 2n + 1 keyframes around a candidate, moved into one frame by their odometry poses (the reference's
 * historyKeyframeSearchNum, include/utility.h:127-131), not against one sweep.  The members' stored voxels (QTR_KF_VOX)
 * are read where they are, each record moved by its member's pose with the arithmetic of include/qtr_submap_math.h
 * (binary64 products and sums in a fixed association, one rounding to binary32, w copied) and written in member order —
 * stored voxel order within a member — into the slot's raw-cloud buffer; the one-cloud front end and the pack of
 * qtr_keyframe_create follow.  *out is the keyframe qtr_keyframe_create(h, slot, cat, N, fp, QTR_MEM_HOST, ..) returns for
 * that concatenation `cat` of N = sum of the members' n_voxels records: every fetchable item bit-identical, every info
 * field equal (n_points = N).  It is an ordinary keyframe: registration, the place index, fetch and destroy take it.
 *   poses   K x 16 doubles, row-major 4 x 4 per member, rows 0 - 2 used; NULL: identities.
 *   fp      the SUBMAP's knobs; the members' own leaf and radii play no part (only their voxels are read).
 * QTR_ERR_BAD_ARG: K < 1, K > QTR_SUBMAP_MAX_KEYFRAMES, a NULL member or one of another handle, NULL fp or out, a non-finite
 * entry in rows 0 - 2 of a pose.  QTR_ERR_CAPACITY: N (summed in 64 bits) exceeds qtr_limits.max_points.  Both are found
 * before anything is enqueued; *out = NULL on every failure.  The front end's own errors and messages are
 * qtr_keyframe_create's (max_voxels, the long-list arena, the pass-through).  A member may appear more than once.  A set-up
 * call like qtr_keyframe_create: it returns after the pack has completed.  Members are only read: several slots, from
 * different host threads, may merge from the same members at once. */
#define QTR_SUBMAP_MAX_KEYFRAMES 64
QTR_API int qtr_keyframe_merge(qtr_handle* h, int slot, const qtr_keyframe* const* kfs,
                               const double* poses /* K x 16, NULL = identities */, int K,
                               const qtr_frontend_params* fp, qtr_keyframe** out);

/* Place index: WHICH keyframes are worth registering against.  One Scan Context descriptor (Kim & Kim, IROS 2018) per added
 * keyframe — a num_rings x num_sectors polar image of the maximum height, row-major float32, plus the squared norm of
 * every column — kept in device memory, and an exhaustive search: every entry of an id range is compared with the query
 * under all num_sectors column shifts, the k most similar come back with their shift.  The shift is a yaw estimate, and
 * Quatro is a yaw + translation solver: the two agree on what a revisit looks like (roll / pitch small).  The arithmetic,
 * to the bit, is include/qtr_place_math.h's (host and device compile the same functions):
 *   descriptor   per finite point: zh = z + height_offset (skipped unless > 0), r = sqrt(x^2 + y^2) (skipped unless
 *                < max_range), ring = floor(r * num_rings / max_range), sector from atan2(y, x) + pi in num_sectors equal
 *                bins; cell = max zh, 0 when empty.  A function of the point SET, not of its order.
 *   distance     d(s) = mean over the columns j where both the query's column j and the entry's column (j + s) mod S are
 *                non-zero of 1 - cosine; no such column: 1.  distance = min_s d(s), ties to the lowest s = shift;
 *                yaw = shift * 2 pi / S wrapped to (-pi, pi]: the yaw of the transform that maps the QUERY into the
 *                entry's frame, comparable with the yaw of qtr_register_keyframes(query, entry)'s T.
 *   qtr_place_index_create   capacity entries of device memory (about 5 kB each at 20 x 60), owned by the handle;
 *                            params NULL = the defaults.  qtr_destroy frees the indexes the caller did not destroy.
 *   qtr_place_describe       the descriptor of n points (16-byte records, host or device per `mem`; n = 0: all zero) to
 *                            `desc` (num_rings * num_sectors floats, in the same memory space).  Complete on return.
 *   qtr_place_index_add      the descriptor of a keyframe's stored voxels (QTR_KF_VOX) becomes the next entry; ids are
 *                            0, 1, 2, ... in order of addition.  A full index: QTR_ERR_CAPACITY, index unchanged.  A
 *                            keyframe or an index of another handle: QTR_ERR_BAD_ARG.  Complete on return.
 *   qtr_place_index_add_desc the same for a descriptor the caller made earlier (qtr_place_describe, or fetched from an
 *                            index of a previous session: an index is saved with qtr_place_index_fetch and reloaded with
 *                            this call).  Cells must be finite and >= 0 (not checked).
 *   qtr_place_index_fetch    copies a stored item of entry `id` to host memory, like qtr_keyframe_fetch.
 *   qtr_place_query          scores the entries id_lo <= id < id_hi (clamped to [0, size]; excluding the most recent
 *                            keyframes is a smaller id_hi) against the keyframe's descriptor and writes the
 *                            min(k, candidates) best to `out` (host) in ascending (distance, id) order, *n_out their
 *                            number.  k: 1 .. 64.  An empty range: QTR_OK, *n_out = 0.  Complete on return, after ONE host
 *                            wait.  The query's descriptor must have the index's shape: a keyframe always has.
 *   qtr_place_query_desc     the same for a descriptor in host or device memory.
 * Threading: a query only reads the index — any number of slots, from different host threads, may query one index at
 * once.  An add writes it: add and query (and two adds) on the same index must be serialised by the caller. */
typedef struct qtr_place_params {
  int num_rings;       /* 20  (4 .. 32) */
  int num_sectors;     /* 60  (8 .. 64: one wavefront lane per shift) */
  float max_range;     /* 80.0 m, > 0 */
  float height_offset; /* 2.0 m added to z (the sensor's height), so that heights are positive */
} qtr_place_params;
typedef struct qtr_place_match {
  int id;         /* entry */
  int shift;      /* column shift of the minimum */
  float distance; /* 0 (the same place) .. 1 */
  float yaw;      /* shift * 2 pi / num_sectors in (-pi, pi]: query -> entry */
} qtr_place_match;
typedef struct qtr_place_index qtr_place_index; /* opaque, owned by the handle that made it */
typedef struct qtr_place_index_info {
  qtr_place_params params;
  int size, capacity;              /* entries held, entries it can hold */
  unsigned long long device_bytes; /* HBM this index holds */
} qtr_place_index_info;
#define QTR_PLACE_DESC 1     /* float[num_rings][num_sectors] */
#define QTR_PLACE_COLNORM2 2 /* float[num_sectors] squared column norms */
QTR_API void qtr_default_place_params(qtr_place_params* p);
QTR_API int qtr_place_index_create(qtr_handle* h, const qtr_place_params* params, int capacity, qtr_place_index** out);
QTR_API void qtr_place_index_destroy(qtr_handle* h, qtr_place_index* index);
QTR_API int qtr_place_index_get_info(const qtr_place_index* index, qtr_place_index_info* info);
QTR_API int qtr_place_describe(qtr_handle* h, int slot, const qtr_place_params* params, const float* xyz4, int n, float* desc,
                               int mem);
QTR_API int qtr_place_index_add(qtr_handle* h, int slot, qtr_place_index* index, const qtr_keyframe* kf, int* id_out);
QTR_API int qtr_place_index_add_desc(qtr_handle* h, int slot, qtr_place_index* index, const float* desc, int mem, int* id_out);
QTR_API long long qtr_place_index_fetch(qtr_handle* h, const qtr_place_index* index, int id, int what, void* dst, size_t bytes);
QTR_API int qtr_place_query(qtr_handle* h, int slot, const qtr_place_index* index, const qtr_keyframe* query, int id_lo,
                            int id_hi, int k, qtr_place_match* out, int* n_out);
QTR_API int qtr_place_query_desc(qtr_handle* h, int slot, const qtr_place_index* index, const float* desc, int mem, int id_lo,
                                 int id_hi, int k, qtr_place_match* out, int* n_out);

/* Evaluation of a registration: what a caller settles before (T) becomes an edge (T, Omega) of a pose graph — Open3D's
 * evaluate_registration and get_information_matrix_from_point_clouds, plus the Hessian of the point-to-plane cost at T
 * (the point-to-point information matrix has full rank for any three non-collinear points: it cannot show a corridor or a
 * single plane; the point-to-plane Hessian can).  The arithmetic is include/qtr_eval_math.h; one kernel launch per call.
 *   considered:     the finite source points (n_source of them)
 *   correspondence: the ICP's — the NEAREST finite target point within max_correspondence_distance of R p + t (binary64
 *                   distances, ties to the lowest target index).  A non-finite target normal does not drop it: it only
 *                   keeps it out of the plane sums (n_plane, plane_rmse, hessian_plane)
 *   overlap         n_corr / n_source (Open3D's fitness); inlier_rmse = sqrt(sum_d2 / n_corr); sum_d2 and n_corr are the
 *                   numbers one point-to-point ICP iteration from T forms
 *   information     row-major 6x6, rotation first: sum G^T G, G = [ -[t]x | I ] on the target point of every correspondence
 *   hessian_plane   row-major 6x6: sum J^T J, J = [ q x n | n ]; all zero with n_plane = 0 without target normals
 * Both matrices are exactly symmetric.  valid = n_corr > 0.  The evaluation has an arena of its own per slot (allocated on
 * the first call, grown on demand): the ICP arena, its QTR_DBG_ICP_* items and a registration's state are left alone.
 * QTR_ERR_BAD_ARG, before anything is enqueued: a NULL keyframe or one of another handle, B outside 1 .. QTR_EVAL_MAX_PAIRS,
 * a NULL T or one with a non-finite entry in rows 0 - 2, a distance that is not finite and positive.  Sizes above
 * qtr_limits.max_voxels per cloud: QTR_ERR_CAPACITY.  Empty clouds or no finite target point: QTR_OK, valid = 0. */
#define QTR_EVAL_MAX_PAIRS 64
typedef struct qtr_eval_params {
  double max_correspondence_distance; /* 1.0 m, like the ICP's */
  int reserved[2];
} qtr_eval_params;
typedef struct qtr_eval_result {
  int status, valid, n_source, n_corr, n_plane, reserved;
  double T[16]; /* the transform evaluated */
  double overlap, sum_d2, inlier_rmse, plane_rmse, information[36], hessian_plane[36];
} qtr_eval_result;
typedef struct qtr_eval_kf_pair {
  const qtr_keyframe* source;
  const qtr_keyframe* target;
  double T[16];
} qtr_eval_kf_pair;
QTR_API void qtr_default_eval_params(qtr_eval_params* p);
/* src4 (n_s) / tgt4 (n_t): 16-byte records; tgt_normals4: n_t records nx,ny,nz,* or NULL (no plane sums).  T: row-major
 * 4x4, maps source into target.  mem: where the clouds live. */
QTR_API int qtr_evaluate(qtr_handle* h, int slot, const float* src4, int n_s, const float* tgt4, int n_t,
                         const float* tgt_normals4, const double T[16], const qtr_eval_params* prm, qtr_eval_result* res, int mem);
/* The slot's last registration, on its voxelised clouds and the target's normals where they lie (qtr_refine_pair's rules:
 * QTR_ERR_BAD_ARG when the slot's last call was not a registration, and after a batch job).  T NULL = that call's T.  Leaves
 * the registration's state untouched: a qtr_refine_pair may follow it, and it may follow a qtr_refine_pair. */
QTR_API int qtr_evaluate_pair(qtr_handle* h, int slot, const double T[16], const qtr_eval_params* prm, qtr_eval_result* res);
/* Two keyframes, read where they lie (the voxels of both, the normals of the target); no registration needs to precede it
 * and the slot's clouds are not written. */
QTR_API int qtr_evaluate_keyframes(qtr_handle* h, int slot, const qtr_keyframe* source, const qtr_keyframe* target,
                                   const double T[16], const qtr_eval_params* prm, qtr_eval_result* res);
/* B pairs (1 .. QTR_EVAL_MAX_PAIRS) in one grouped launch chain on `slot`, two host waits in all; results[b] is
 * bit-identical to qtr_evaluate_keyframes on pair b.  A keyframe may appear in any number of pairs.  An argument error
 * refuses the whole batch. */
QTR_API int qtr_evaluate_keyframes_batch(qtr_handle* h, int slot, const qtr_eval_kf_pair* pairs, int B,
                                         const qtr_eval_params* prm, qtr_eval_result* results);

/* Robust pose-graph optimisation: from the edges (T, Omega) that qtr_evaluate* emits to corrected keyframe poses — Open3D's
 * GlobalOptimizationLevenbergMarquardt with the line process of Choi et al. 2015 over the uncertain edges, on the device,
 * bit-reproducible.  The arithmetic and every order of summation are include/qtr_pgo_math.h.
 *   poses      n_nodes row-major 4x4, keyframe i's frame -> map frame (what qtr_keyframe_merge takes as poses[i])
 *   fixed      one byte per node, non-zero = held; NULL = node 0 alone is held
 *   edge e     Z[e] maps keyframe src[e]'s frame into keyframe dst[e]'s frame (a registration's T with src = the source /
 *              query, dst = the target / candidate); info[e] is the evaluation's `information` (row-major 6x6, [omega | v],
 *              upper triangle read); uncertain[e] non-zero = under the line process (NULL: none)
 *   residual   vee(X_dst^-1 X_src Z^-1): Z^-1 on the RIGHT, the perturbation the information matrix was formed under
 *              (Open3D puts it on the left)
 *   weights    w = 1 for a certain edge, (mu / (mu + chi2))^2 for an uncertain one, mu = line_process_weight (<= 0: off);
 *              weight_out[e] is the final one, n_pruned counts the uncertain edges below edge_prune_threshold
 * The linear system of every step is solved by block-Jacobi preconditioned conjugate gradients inside ONE workgroup.
 * Synchronous and stateless; an arena of its own per slot (allocated on first use, grown on demand); one host wait per LM
 * iteration.  Registration, ICP and evaluation state of the slot are left alone.  A connected component without a fixed node
 * is not an error (the damping keeps the system definite; the component keeps its gauge).  No edge, or no free node: QTR_OK,
 * stop_reason QTR_PGO_STOP_NOTHING, poses_out = poses, weights 1, objectives 0.
 * QTR_ERR_BAD_ARG, before anything is enqueued: a NULL array, n_nodes < 1, n_edges < 0, an edge index out of range or
 * src = dst, a non-finite entry in rows 0 - 2 of a pose or a Z or in the upper triangle of an info, no fixed node, a
 * tolerance (rel_tol, step_tol, tau, pcg_tol) that is not finite and positive, an iteration count out of range, a weight or
 * threshold that is not finite.  n_nodes > QTR_PGO_MAX_NODES or n_edges > QTR_PGO_MAX_EDGES: QTR_ERR_CAPACITY. */
#define QTR_PGO_MAX_NODES 65536
#define QTR_PGO_MAX_EDGES (1 << 20)
#define QTR_PGO_MAX_ITERATIONS 65536
#define QTR_PGO_STOP_MAX_ITERATIONS 1 /* trial steps evaluated */
#define QTR_PGO_STOP_RELATIVE 2       /* an accepted step lowered the objective by no more than rel_tol of it */
#define QTR_PGO_STOP_STEP 3           /* max |delta| < step_tol */
#define QTR_PGO_STOP_LAMBDA 4         /* the damping passed its ceiling (1e32) */
#define QTR_PGO_STOP_NOTHING 5        /* no edge or no free node */
typedef struct qtr_pgo_params {
  int max_iterations;          /* 100 LM trial steps */
  int pcg_max_iterations;      /* 500 per step */
  double rel_tol;              /* 1e-6 */
  double step_tol;             /* 1e-9 */
  double tau;                  /* 1e-5: lambda_0 = tau max diag(H) */
  double pcg_tol;              /* 1e-8: |res|^2 <= pcg_tol^2 |g|^2 */
  double line_process_weight;  /* 0: off */
  double edge_prune_threshold; /* 0.25 */
  int reserved[8];
} qtr_pgo_params;
typedef struct qtr_pgo_result {
  int status, valid, iterations, accepted, pcg_iterations_total, stop_reason, n_pruned, reserved;
  double objective_initial, objective_final, lambda_final;
} qtr_pgo_result;
QTR_API void qtr_default_pgo_params(qtr_pgo_params* p);
/* poses / poses_out: 16 n_nodes doubles; Z: 16 n_edges; info: 36 n_edges; weight_out: n_edges doubles or NULL.  All in host
 * memory.  poses_out may be poses. */
QTR_API int qtr_pgo_optimize(qtr_handle* h, int slot, int n_nodes, const double* poses, const unsigned char* fixed, int n_edges,
                             const int* src, const int* dst, const double* Z, const double* info,
                             const unsigned char* uncertain, const qtr_pgo_params* prm, double* poses_out, double* weight_out,
                             qtr_pgo_result* res);

/* Inspection of intermediates of the LAST call on a slot (tests / parity debugging).  Copies up to
 * `bytes` bytes to host memory `dst`; returns the number of bytes the item holds, or <0 on error. */
#define QTR_DBG_GRAPH_BITMAP 1   /* uint64[L][ceil(L/64)] adjacency, original labels */
#define QTR_DBG_CORE 2           /* int32[L] core numbers: exact at or above QTR_DBG_SOLVER_STATE[29] (the floor of the last
                                    solve, 0 = all exact; always 0 in the k-core heuristic mode), below it an upper bound
                                    that is itself below the floor */
#define QTR_DBG_PERM 3           /* int32[L] vertex id at each rank of the (core,id) order */
#define QTR_DBG_NBR_OFFSETS 4    /* int32[n+1] CSR offsets of the sorted radius-neighbour lists (last qtr_fpfh) */
#define QTR_DBG_NBR_INDEX 5      /* int32[...] neighbour indices */
#define QTR_DBG_NBR_DIST2 6      /* float[...] squared distances */
#define QTR_DBG_SPFH 7           /* float[n][33] */
#define QTR_DBG_NN_LARGE_OF_SMALL 8 /* int32[n_small] */
#define QTR_DBG_NN_SMALL_OF_LARGE 9 /* int32[n_large] (-1 where not queried) */
#define QTR_DBG_VOX_SRC 10       /* float4[n_src] voxelised source of the last qtr_register_pair */
#define QTR_DBG_VOX_TGT 11
#define QTR_DBG_CORR 12          /* int32[L][2] */
#define QTR_DBG_MATCH_STATS 13   /* int32[16]: [0] L, [3] cross-checked pairs, [4] tuple-test survivors, [5] swapped,
                                    [8],[9] rows sent to the exact NN re-check (dir 0/1), [10],[11] rows settled by the
                                    two-candidate exact compare */
#define QTR_DBG_SOLVER_STATE 14  /* int32[32]: mc, best_r, pos, done, t0, ub, batch, max_core, n_edges2, clique rounds,
                                    [10] k-core peeling rounds / iterations, [22] 1: the clique stage ran twice (second
                                    time with exact core numbers), [29] floor of the core numbers (0: all exact) */
#define QTR_DBG_ICP_CORR 15      /* int32[n_s] target index of every source point in the last ICP iteration (-1: none) */
#define QTR_DBG_ICP_TRACE 16     /* double[iterations][18] per update of the last ICP call: T after it (16), MSE, count */
#define QTR_DBG_ICP_TIMES 17     /* float[2] last ICP call: grid build, iterations (device milliseconds) */
#define QTR_DBG_EVAL_CORR 18     /* int32[n_s] target index of every source point of the last evaluation (a batch: its
                                    first pair); -1: none */
#define QTR_DBG_PGO_TRACE 19     /* double[1 + iterations][8] of the last optimisation; row 0 the start, row k trial step k:
                                    F at the trial poses, lambda after the decision, rho, accepted, PCG iterations of the
                                    step, F kept, the gain's denominator, max |delta| */
QTR_API long long qtr_debug_fetch(qtr_handle* h, int slot, int what, void* dst, size_t bytes);

/* Evaluates the shared deterministic math (include/qtr_math.h) ON THE DEVICE, for the test that pins
 * host/device bit-equality: fn 0 atan2f(a,b), 1 acosf(a), 2 sinf(a) (theta in [0,1.2]), 3 cosf(a) — and the SPFH
 * kernel's decisions, as floats: fn 4 the bin 0 .. 10 of the first block that k2_spfh stores for the arc tangent's arguments
 * (y, x) = (a, b), floor(11 (atan2f(a,b) + pi) / 2 pi): the shortcut below, then the arc tangent where it is not sure;
 * fn 5 the role swap acosf(|a|) > acosf(|b|) as 1 / 0; fn 6 the bin shortcut alone (five cross products, no arc tangent):
 * the bin, or -1 where it is not sure (y = +-0, a non-finite argument, |a| + |b| outside (1e-30, 1e30), a direction
 * within 1e-6 of a bin boundary). */
QTR_API int qtr_debug_math(qtr_handle* h, int fn, const float* a, const float* b, float* out, int n);

#ifdef __cplusplus
}
#endif
#endif /* QUATRO_HIP_H */
