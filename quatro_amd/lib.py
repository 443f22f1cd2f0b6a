"""ctypes binding of libquatro_hip.so (the C ABI in include/quatro_hip.h).

The product path has NO CPU fallback: if the HIP library is missing this module raises, loudly.
Build it with ``python -m quatro_amd.build`` (hipcc cross-compiles for gfx950 without a GPU).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# QTR_LIB: another build of the same library (the diagnostic / candidate builds of tests/probe); it has to exist like the default
LIB_PATH = os.environ.get("QTR_LIB") or os.path.join(_HERE, "libquatro_hip.so")

QTR_OK, QTR_ERR_BAD_ARG, QTR_ERR_CLIQUE_TOO_SMALL, QTR_ERR_CAPACITY, QTR_ERR_HIP, QTR_ERR_UNSUPPORTED = range(6)
MEM_HOST, MEM_DEVICE = 0, 1
INLIER_PMC_EXACT, INLIER_PMC_HEU, INLIER_KCORE_HEU, INLIER_NONE = range(4)
REG_QUATRO, REG_TEASER = 0, 1

DBG_GRAPH_BITMAP, DBG_CORE, DBG_PERM, DBG_NBR_OFFSETS, DBG_NBR_INDEX, DBG_NBR_DIST2, DBG_SPFH = 1, 2, 3, 4, 5, 6, 7
DBG_NN_LARGE_OF_SMALL, DBG_NN_SMALL_OF_LARGE, DBG_VOX_SRC, DBG_VOX_TGT, DBG_CORR, DBG_MATCH_STATS = 8, 9, 10, 11, 12, 13
DBG_SOLVER_STATE = 14
DBG_ICP_CORR, DBG_ICP_TRACE, DBG_ICP_TIMES = 15, 16, 17
ICP_POINT_TO_PLANE, ICP_POINT_TO_POINT, ICP_PLANE_TO_PLANE, ICP_VOXEL_PLANE_TO_PLANE = 0, 1, 2, 3
ICP_STOP_NONE, ICP_STOP_MAX_ITERATIONS, ICP_STOP_TRANSFORMATION, ICP_STOP_FITNESS, ICP_STOP_TOO_FEW, ICP_STOP_DEGENERATE = range(6)


class Limits(C.Structure):
    _fields_ = [("max_points", C.c_int), ("max_voxels", C.c_int), ("max_corr", C.c_int), ("n_slots", C.c_int),
                ("max_long_neighbors", C.c_int)]


class Params(C.Structure):
    _fields_ = [
        ("noise_bound", C.c_double), ("cbar2", C.c_double), ("rotation_gnc_factor", C.c_double),
        ("rotation_cost_threshold", C.c_double), ("kcore_heuristic_threshold", C.c_double),
        ("cote_noise_bound", C.c_double), ("ryrx", C.c_double * 9),
        ("rotation_max_iterations", C.c_int), ("inlier_selection_mode", C.c_int), ("cote_median", C.c_int),
        ("using_rot_inliers_when_estimating_cote", C.c_int), ("using_pre_estimated_ryrx", C.c_int),
        ("reg_mode", C.c_int), ("max_clique_time_limit", C.c_double),
    ]


class FrontendParams(C.Structure):
    _fields_ = [("voxel_size", C.c_float), ("normal_radius", C.c_float), ("fpfh_radius", C.c_float),
                ("tuple_scale", C.c_float), ("use_crosscheck", C.c_int), ("use_tuple_test", C.c_int),
                ("seed", C.c_ulonglong)]


class Result(C.Structure):
    _fields_ = [
        ("status", C.c_int), ("valid", C.c_int), ("T", C.c_double * 16), ("cost", C.c_double),
        ("gnc_iters", C.c_int), ("n_clique", C.c_int), ("n_rot_inliers", C.c_int), ("n_final", C.c_int),
        ("max_core", C.c_int), ("n_edges", C.c_int), ("n_card", C.c_int * 3),
        ("n_src", C.c_int), ("n_tgt", C.c_int), ("n_corr", C.c_int),
    ]


class PairDesc(C.Structure):
    _fields_ = [("src_raw4", C.c_void_p), ("n_src", C.c_int), ("tgt_raw4", C.c_void_p), ("n_tgt", C.c_int),
                ("seed", C.c_ulonglong), ("clique", C.c_void_p), ("final_inliers", C.c_void_p), ("cap", C.c_int),
                ("src_corr4", C.c_void_p), ("tgt_corr4", C.c_void_p), ("n_corr", C.c_int)]


class StageTimes(C.Structure):
    _fields_ = ([(n, C.c_float) for n in ("voxelize", "fpfh", "match", "graph", "clique", "solve", "total",
                                          "nn_kernel")] + [("nn_launches", C.c_int), ("graph_kernel", C.c_float)])


class PwParams(C.Structure):
    _fields_ = [("sensor_height", C.c_double), ("num_iter", C.c_int), ("num_lpr", C.c_int), ("num_min_pts", C.c_int),
                ("th_seeds", C.c_double), ("th_dist", C.c_double), ("max_range", C.c_double), ("min_range", C.c_double),
                ("uprightness_thr", C.c_double), ("adaptive_seed_selection_margin", C.c_double),
                ("using_global_thr", C.c_int), ("global_elevation_thr", C.c_double), ("num_zones", C.c_int),
                ("num_sectors_each_zone", C.c_int * 4), ("num_rings_each_zone", C.c_int * 4),
                ("min_ranges", C.c_double * 4), ("num_thr", C.c_int), ("elevation_thr", C.c_double * 8),
                ("flatness_thr", C.c_double * 8)]


class IpParams(C.Structure):
    _fields_ = [("n_scan", C.c_int), ("horizon_scan", C.c_int), ("ang_res_x", C.c_float), ("ang_res_y", C.c_float),
                ("ang_bottom", C.c_float), ("neighbor_mode", C.c_int), ("num_min_pts", C.c_int),
                ("segment_theta", C.c_float), ("valid_point_num", C.c_int), ("valid_line_num", C.c_int)]


class IcpParams(C.Structure):
    _fields_ = [("max_correspondence_distance", C.c_double), ("transformation_epsilon", C.c_double),
                ("euclidean_fitness_epsilon", C.c_double), ("max_iterations", C.c_int), ("method", C.c_int),
                ("min_correspondences", C.c_int), ("normal_radius", C.c_float)]


class IcpResult(C.Structure):
    _fields_ = [("status", C.c_int), ("valid", C.c_int), ("converged", C.c_int), ("stop_reason", C.c_int),
                ("iterations", C.c_int), ("n_corr", C.c_int), ("T", C.c_double * 16), ("fitness", C.c_double),
                ("rmse", C.c_double)]


class EvalParams(C.Structure):
    _fields_ = [("max_correspondence_distance", C.c_double), ("reserved", C.c_int * 2)]


class EvalResult(C.Structure):
    _fields_ = [("status", C.c_int), ("valid", C.c_int), ("n_source", C.c_int), ("n_corr", C.c_int), ("n_plane", C.c_int),
                ("reserved", C.c_int), ("T", C.c_double * 16), ("overlap", C.c_double), ("sum_d2", C.c_double),
                ("inlier_rmse", C.c_double), ("plane_rmse", C.c_double), ("information", C.c_double * 36),
                ("hessian_plane", C.c_double * 36)]


class EvalKfPair(C.Structure):
    _fields_ = [("source", C.c_void_p), ("target", C.c_void_p), ("T", C.c_double * 16)]


class PgoParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int), ("pcg_max_iterations", C.c_int), ("rel_tol", C.c_double),
                ("step_tol", C.c_double), ("tau", C.c_double), ("pcg_tol", C.c_double),
                ("line_process_weight", C.c_double), ("edge_prune_threshold", C.c_double), ("reserved", C.c_int * 8)]


class PgoResult(C.Structure):
    _fields_ = [("status", C.c_int), ("valid", C.c_int), ("iterations", C.c_int), ("accepted", C.c_int),
                ("pcg_iterations_total", C.c_int), ("stop_reason", C.c_int), ("n_pruned", C.c_int), ("reserved", C.c_int),
                ("objective_initial", C.c_double), ("objective_final", C.c_double), ("lambda_final", C.c_double)]


class KeyframeInfo(C.Structure):
    _fields_ = [("n_points", C.c_int), ("n_voxels", C.c_int), ("voxel_size", C.c_float), ("normal_radius", C.c_float),
                ("fpfh_radius", C.c_float), ("passed_through", C.c_int), ("device_bytes", C.c_ulonglong)]


class KfPairDesc(C.Structure):
    _fields_ = [("src", C.c_void_p), ("tgt", C.c_void_p), ("seed", C.c_ulonglong), ("clique", C.c_void_p),
                ("final_inliers", C.c_void_p), ("cap", C.c_int)]


class PlaceParams(C.Structure):
    _fields_ = [("num_rings", C.c_int), ("num_sectors", C.c_int), ("max_range", C.c_float), ("height_offset", C.c_float)]


class PlaceMatch(C.Structure):
    _fields_ = [("id", C.c_int), ("shift", C.c_int), ("distance", C.c_float), ("yaw", C.c_float)]


class PlaceIndexInfo(C.Structure):
    _fields_ = [("params", PlaceParams), ("size", C.c_int), ("capacity", C.c_int), ("device_bytes", C.c_ulonglong)]


class PlaceQueryItem(C.Structure):  # qtr_place_query_item (include/quatro_place_batch.h)
    _fields_ = [("kf", C.c_void_p), ("desc", C.c_void_p), ("from_", C.c_void_p), ("entry", C.c_int), ("mem", C.c_int),
                ("id_lo", C.c_int), ("id_hi", C.c_int)]


class VoxelMapParams(C.Structure):
    _fields_ = [("voxel_size", C.c_double), ("capacity", C.c_int), ("reserved", C.c_int * 5)]


class VoxelMapInfo(C.Structure):
    _fields_ = [("voxel_size", C.c_double), ("capacity", C.c_int), ("n_voxels", C.c_int), ("n_inserts", C.c_int),
                ("n_members", C.c_longlong)]


class VoxelMapInsertInfo(C.Structure):
    _fields_ = [("n_points", C.c_int), ("n_members", C.c_int), ("n_new_voxels", C.c_int), ("n_touched_voxels", C.c_int)]


class VoxelMapEvictInfo(C.Structure):
    _fields_ = [("n_kept", C.c_int), ("n_evicted", C.c_int), ("n_members_evicted", C.c_longlong)]


class DeskewInfo(C.Structure):
    _fields_ = [("n_points", C.c_int), ("n_skipped", C.c_int), ("n_extrapolated", C.c_int)]


class CarveParams(C.Structure):
    _fields_ = [("rows", C.c_int), ("cols", C.c_int), ("window", C.c_int), ("min_votes", C.c_int),
                ("fov_up_deg", C.c_double), ("fov_down_deg", C.c_double), ("margin_abs", C.c_double),
                ("margin_rel", C.c_double), ("min_range", C.c_double), ("max_range", C.c_double), ("reserved", C.c_int * 8)]


class VoxelMapCarveInfo(C.Structure):
    _fields_ = [("n_kept", C.c_int), ("n_carved", C.c_int), ("n_tested", C.c_int), ("reserved", C.c_int),
                ("n_members_carved", C.c_longlong)]


class VmapRegItem(C.Structure):
    _fields_ = [("kf", C.c_void_p), ("src4", C.c_void_p), ("src_normals4", C.c_void_p), ("n", C.c_int), ("mem", C.c_int),
                ("guess", C.c_double * 16)]


class VmapEvalParams(C.Structure):
    _fields_ = [("per_point", C.c_int), ("reserved", C.c_int * 3)]


class VmapEvalResult(C.Structure):
    _fields_ = [("status", C.c_int), ("valid", C.c_int), ("n_source", C.c_int), ("n_corr", C.c_int),
                ("overlap", C.c_double), ("sum_d2", C.c_double), ("inlier_rmse", C.c_double), ("sum_w", C.c_double),
                ("chi2", C.c_double), ("rmse", C.c_double), ("information", C.c_double * 36), ("hessian", C.c_double * 36),
                ("gradient", C.c_double * 6)]


class VmapCtInfo(C.Structure):
    _fields_ = [("n_points", C.c_int), ("n_skipped", C.c_int), ("n_extrapolated", C.c_int)]


VMAP_BATCH_MAX = 64
VMAP_EVAL_MAX = 1024
VMAP_EVAL_CORR, VMAP_EVAL_POINT, VMAP_EVAL_TIMES = 1, 2, 3
VMAP_BATCH_TRACE, VMAP_BATCH_CORR, VMAP_BATCH_TIMES = 1, 2, 3
KF_VOX, KF_NORMALS, KF_FPFH, KF_MEAN = 1, 2, 3, 4
DESKEW_MAX_KNOTS = 256
CARVE_MAX_KEYFRAMES = 64
VMAP_COORDS, VMAP_COUNT, VMAP_SUMS, VMAP_RECORDS, VMAP_CLOUD = 1, 2, 3, 4, 5
VMAP_MAX_CAPACITY = 1 << 24
PLACE_DESC, PLACE_COLNORM2 = 1, 2
PLACE_MAX_K = 64
PLACE_BATCH_MAX, PLACE_BATCH_MAX_PAIRS = 1024, 1 << 26
PLACE_BATCH_DIST, PLACE_BATCH_SHIFT = 1, 2
PLACE_MATCH_DTYPE = np.dtype([("id", "<i4"), ("shift", "<i4"), ("distance", "<f4"), ("yaw", "<f4")])  # qtr_place_match
SUBMAP_MAX_KEYFRAMES = 64
EVAL_MAX_PAIRS = 64
DBG_EVAL_CORR = 18
DBG_PGO_TRACE = 19
PGO_MAX_NODES, PGO_MAX_EDGES, PGO_MAX_ITERATIONS, PGO_TRACE = 65536, 1 << 20, 65536, 8
PGO_STOP_MAX_ITERATIONS, PGO_STOP_RELATIVE, PGO_STOP_STEP, PGO_STOP_LAMBDA, PGO_STOP_NOTHING = 1, 2, 3, 4, 5

EXPORTS = [
    "qtr_create", "qtr_destroy", "qtr_last_error", "qtr_default_limits", "qtr_default_params", "qtr_demo_params",
    "qtr_default_frontend_params", "qtr_num_slots", "qtr_slot_stream", "qtr_voxelize", "qtr_fpfh", "qtr_match",
    "qtr_solve", "qtr_max_clique", "qtr_compute_tims", "qtr_scale_mask", "qtr_gnc_rotation2d",
    "qtr_cote_estimate", "qtr_cote_estimate_ranges", "qtr_ip_default_params", "qtr_segment_cloud", "qtr_pw_default_params", "qtr_patchwork", "qtr_gnc_rotation3d", "qtr_exact_stats", "qtr_read_kitti_bin", "qtr_write_pcd_xyz", "qtr_read_pcd_xyz", "qtr_register_pair", "qtr_register_pair_corr", "qtr_feature_pair", "qtr_get_stage_times", "qtr_get_nn_dir_times", "qtr_set_stage_events", "qtr_set_nn_event_stride", "qtr_get_nn_totals", "qtr_debug_fetch", "qtr_debug_math", "qtr_submit_batch", "qtr_wait", "qtr_set_batch_preprocess", "qtr_comm_unique_id", "qtr_comm_init", "qtr_gather_results", "qtr_gather_results_v", "qtr_comm_destroy",
    "qtr_default_icp_params", "qtr_icp", "qtr_refine_pair", "qtr_submit_batch_refine", "qtr_gicp",
    "qtr_keyframe_create", "qtr_keyframe_get_info", "qtr_keyframe_fetch", "qtr_keyframe_destroy", "qtr_register_keyframes",
    "qtr_submit_batch_keyframes", "qtr_keyframe_merge",
    "qtr_default_place_params", "qtr_place_index_create", "qtr_place_index_destroy", "qtr_place_index_get_info",
    "qtr_place_describe", "qtr_place_index_add", "qtr_place_index_add_desc", "qtr_place_index_fetch", "qtr_place_query",
    "qtr_place_query_desc",
    "qtr_default_eval_params", "qtr_evaluate", "qtr_evaluate_pair", "qtr_evaluate_keyframes",
    "qtr_evaluate_keyframes_batch",
    "qtr_default_pgo_params", "qtr_pgo_optimize",
]
# the C ABI of the extension headers, per header; libquatro_ext.so exports their concatenation over the same handle.  A new
# header include/quatro_<name>.h brings its list <NAME>_EXPORTS and joins EXT_EXPORTS (tests/ext_abi.py holds it to that)
VOXELMAP_EXPORTS = [  # include/quatro_voxelmap.h
    "qtr_default_voxel_map_params", "qtr_voxel_map_create", "qtr_voxel_map_destroy", "qtr_voxel_map_clear",
    "qtr_voxel_map_get_info", "qtr_voxel_map_insert", "qtr_voxel_map_insert_keyframe", "qtr_voxel_map_register",
    "qtr_voxel_map_register_keyframe", "qtr_voxel_map_fetch",
]
VOXELMAP_KEEP_EXPORTS = ["qtr_voxel_map_evict", "qtr_voxel_map_restore"]  # include/quatro_voxelmap_keep.h
DESKEW_EXPORTS = ["qtr_deskew", "qtr_keyframe_create_deskewed", "qtr_deskew_pose_at"]  # include/quatro_deskew.h
VOXELMAP_CARVE_EXPORTS = ["qtr_default_carve_params", "qtr_voxel_map_carve", "qtr_voxel_map_carve_keyframes"]  # ..._carve.h
VOXELMAP_BATCH_EXPORTS = ["qtr_voxel_map_register_batch", "qtr_voxel_map_batch_fetch"]  # include/quatro_voxelmap_batch.h
VOXELMAP_EVAL_EXPORTS = ["qtr_default_vmap_eval_params", "qtr_voxel_map_evaluate", "qtr_voxel_map_evaluate_keyframe",
                         "qtr_voxel_map_evaluate_batch", "qtr_voxel_map_eval_fetch"]  # include/quatro_voxelmap_eval.h
PLACE_BATCH_EXPORTS = ["qtr_place_query_batch", "qtr_place_batch_fetch"]  # include/quatro_place_batch.h
VMAP_CT_EXPORTS = ["qtr_voxel_map_register_ct", "qtr_voxel_map_ct_pose_at"]  # include/quatro_voxelmap_ct.h
EXT_EXPORTS = (VOXELMAP_EXPORTS + VOXELMAP_KEEP_EXPORTS + DESKEW_EXPORTS + VOXELMAP_CARVE_EXPORTS + VOXELMAP_BATCH_EXPORTS
               + VOXELMAP_EVAL_EXPORTS + PLACE_BATCH_EXPORTS + VMAP_CT_EXPORTS)

_lib = None


QTR_ERR_IO = 6
QTR_ERR_NOT_RUN = 7


def read_kitti_bin(path: str, max_points: int = 250000) -> np.ndarray:
    """getCloud of the demo (examples/run_global_registration.cpp:377-402): (n, 4) float32 x, y, z, intensity."""
    out = np.zeros((max(max_points, 1), 4), dtype=np.float32)
    n = C.c_int()
    rc = load().qtr_read_kitti_bin(os.fsencode(path), out.ctypes.data, max_points, C.byref(n))
    if rc != QTR_OK:
        raise OSError(f"error: failed to load {path}")
    return out[:n.value].copy()


def write_pcd_xyz(path: str, xyz, binary: bool = False) -> None:
    a = np.asarray(xyz, dtype=np.float32).reshape(-1, np.asarray(xyz).shape[-1] if np.asarray(xyz).ndim == 2 else 3)
    if a.shape[1] == 3:
        a = np.concatenate([a, np.zeros((a.shape[0], 1), dtype=np.float32)], axis=1)
    a = _f4(a[:, :4])
    rc = load().qtr_write_pcd_xyz(os.fsencode(path), a.ctypes.data, a.shape[0], 1 if binary else 0)
    if rc != QTR_OK:
        raise OSError(f"failed to write {path}")


def read_pcd_xyz(path: str) -> np.ndarray:
    """(n, 4) float32 x, y, z, 0 from an ascii / binary / binary_compressed PCD holding fields x y z."""
    n = C.c_int()
    rc = load().qtr_read_pcd_xyz(os.fsencode(path), None, 0, C.byref(n))
    if rc not in (QTR_OK, QTR_ERR_CAPACITY):
        raise OSError(f"failed to read {path}")
    out = np.zeros((max(n.value, 1), 4), dtype=np.float32)
    rc = load().qtr_read_pcd_xyz(os.fsencode(path), out.ctypes.data, n.value, C.byref(n))
    if rc != QTR_OK:
        raise OSError(f"failed to read {path}")
    return out[:n.value].copy()


def pw_params() -> PwParams:
    p = PwParams()
    load().qtr_pw_default_params(C.byref(p))
    return p


def ip_params(lidar: str = "Velodyne-64-HDE", neighbor_mode: str = "4CrossNeighbor", num_min_pts: int = 30) -> IpParams:
    p = IpParams()
    rc = load().qtr_ip_default_params(lidar.encode(), neighbor_mode.encode(), C.byref(p))
    if rc != QTR_OK:
        raise ValueError("[ImageProjection]:Check your paramter. Lidar Type / neighbor selection mode is wrong!")
    p.num_min_pts = num_min_pts
    return p


class QuatroHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libquatro_hip status {code}: {msg}")
        self.code = code


_libs = {}
TEST_ENGINES_LIB_PATH = os.path.join(_HERE, "libquatro_hip_testengines.so")  # the -DQTR_TEST_ENGINES build (tests only)


def _open(path: str, signatures, product_first: bool = False):
    """What load() and load_ext() share: the library at `path`, opened once with its ctypes signatures set.  Raises if it
    has not been built — there is no software fallback."""
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: the HIP extension has not been built. Run `python -m quatro_amd.build` "
            "(or __graft_entry__.build()). quatro_amd has no CPU fallback.")
    # torch ships its own libamdhip64.so.7; importing it first makes both share ONE HIP runtime.
    import torch  # noqa: F401
    if product_first:
        load()
    lib = C.CDLL(path)
    signatures(lib)
    _libs[path] = lib
    return lib


def load(path: str | None = None):
    """Loads libquatro_hip.so (or another build of it: the tests' comparison-engine build, a probe's candidate)."""
    global _lib
    lib = _open(path or LIB_PATH, _signatures)
    if path is None:
        _lib = lib
    return lib


def _signatures(lib):
    lib.qtr_last_error.restype = C.c_char_p
    lib.qtr_slot_stream.restype = C.c_void_p
    lib.qtr_debug_fetch.restype = C.c_longlong
    lib.qtr_debug_fetch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    lib.qtr_create.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.qtr_destroy.argtypes = [C.c_void_p]
    lib.qtr_last_error.argtypes = [C.c_void_p]
    lib.qtr_slot_stream.argtypes = [C.c_void_p, C.c_int]
    lib.qtr_num_slots.argtypes = [C.c_void_p]
    lib.qtr_voxelize.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_int,
                                 C.POINTER(C.c_int), C.c_int]
    lib.qtr_fpfh.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                             C.c_int]
    lib.qtr_match.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                              C.POINTER(FrontendParams), C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int]
    lib.qtr_solve.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(Params),
                              C.POINTER(Result), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.qtr_register_pair.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                      C.POINTER(FrontendParams), C.POINTER(Params), C.POINTER(Result), C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_int]
    lib.qtr_register_pair_corr.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                           C.POINTER(FrontendParams), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(Params),
                                           C.POINTER(Result), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.qtr_feature_pair.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                     C.POINTER(FrontendParams), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                     C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.qtr_set_batch_preprocess.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.qtr_get_stage_times.argtypes = [C.c_void_p, C.c_int, C.POINTER(StageTimes)]
    if hasattr(lib, "qtr_get_nn_dir_times"):
        lib.qtr_get_nn_dir_times.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.qtr_set_stage_events.argtypes = [C.c_void_p, C.c_int]
    lib.qtr_set_nn_event_stride.argtypes = [C.c_void_p, C.c_int]
    lib.qtr_get_nn_totals.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.c_int]
    lib.qtr_max_clique.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_int,
                                   C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    lib.qtr_compute_tims.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.qtr_scale_mask.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_double, C.c_double,
                                   C.c_void_p]
    lib.qtr_gnc_rotation2d.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double,
                                       C.c_int, C.c_double, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int),
                                       C.c_void_p]
    lib.qtr_gnc_rotation3d.argtypes = lib.qtr_gnc_rotation2d.argtypes
    lib.qtr_cote_estimate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_int,
                                      C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_int)]
    lib.qtr_cote_estimate_ranges.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                             C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_int)]
    lib.qtr_exact_stats.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_int)]
    lib.qtr_read_kitti_bin.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.qtr_write_pcd_xyz.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int]
    lib.qtr_read_pcd_xyz.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.qtr_pw_default_params.argtypes = [C.POINTER(PwParams)]
    lib.qtr_pw_default_params.restype = None
    lib.qtr_patchwork.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(PwParams), C.c_void_p, C.c_int,
                                  C.POINTER(C.c_int), C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int]
    lib.qtr_ip_default_params.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(IpParams)]
    lib.qtr_segment_cloud.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(IpParams), C.c_void_p, C.c_int,
                                      C.POINTER(C.c_int), C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                      C.c_void_p, C.c_int]
    lib.qtr_debug_math.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.qtr_submit_batch.argtypes = [C.c_void_p, C.POINTER(PairDesc), C.c_int, C.POINTER(FrontendParams),
                                     C.POINTER(Params), C.POINTER(Result), C.c_int]
    lib.qtr_wait.argtypes = [C.c_void_p]
    lib.qtr_comm_unique_id.argtypes = [C.c_char_p]
    lib.qtr_comm_init.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
    lib.qtr_gather_results.argtypes = [C.c_void_p, C.POINTER(Result), C.c_int, C.POINTER(Result)]
    lib.qtr_gather_results_v.argtypes = [C.c_void_p, C.POINTER(Result), C.c_int, C.POINTER(Result), C.c_int,
                                         C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.qtr_comm_destroy.argtypes = [C.c_void_p]
    lib.qtr_default_icp_params.argtypes = [C.POINTER(IcpParams)]
    lib.qtr_icp.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                            C.POINTER(IcpParams), C.POINTER(IcpResult), C.c_int]
    lib.qtr_gicp.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                             C.POINTER(IcpParams), C.POINTER(IcpResult), C.c_int]
    lib.qtr_refine_pair.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(IcpParams), C.POINTER(IcpResult)]
    lib.qtr_submit_batch_refine.argtypes = [C.c_void_p, C.POINTER(PairDesc), C.c_int, C.POINTER(FrontendParams),
                                            C.POINTER(Params), C.POINTER(IcpParams), C.POINTER(Result),
                                            C.POINTER(IcpResult), C.c_int]
    lib.qtr_comm_destroy.restype = None
    lib.qtr_keyframe_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(FrontendParams), C.c_int,
                                        C.POINTER(C.c_void_p)]
    lib.qtr_keyframe_get_info.argtypes = [C.c_void_p, C.POINTER(KeyframeInfo)]
    lib.qtr_keyframe_fetch.restype = C.c_longlong
    lib.qtr_keyframe_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    lib.qtr_keyframe_destroy.restype = None
    lib.qtr_keyframe_destroy.argtypes = [C.c_void_p, C.c_void_p]
    lib.qtr_register_keyframes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(FrontendParams),
                                           C.POINTER(Params), C.POINTER(Result), C.c_void_p, C.c_void_p, C.c_int]
    lib.qtr_submit_batch_keyframes.argtypes = [C.c_void_p, C.POINTER(KfPairDesc), C.c_int, C.POINTER(FrontendParams),
                                               C.POINTER(Params), C.POINTER(IcpParams), C.POINTER(Result),
                                               C.POINTER(IcpResult)]
    lib.qtr_keyframe_merge.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.c_int,
                                       C.POINTER(FrontendParams), C.POINTER(C.c_void_p)]
    lib.qtr_default_place_params.restype = None
    lib.qtr_default_eval_params.argtypes = [C.POINTER(EvalParams)]
    lib.qtr_default_eval_params.restype = None
    lib.qtr_evaluate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                 C.POINTER(EvalParams), C.POINTER(EvalResult), C.c_int]
    lib.qtr_evaluate_pair.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(EvalParams), C.POINTER(EvalResult)]
    lib.qtr_evaluate_keyframes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EvalParams),
                                           C.POINTER(EvalResult)]
    lib.qtr_evaluate_keyframes_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(EvalKfPair), C.c_int, C.POINTER(EvalParams),
                                                 C.POINTER(EvalResult)]
    lib.qtr_default_pgo_params.argtypes = [C.POINTER(PgoParams)]
    lib.qtr_default_pgo_params.restype = None
    lib.qtr_pgo_optimize.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PgoParams), C.c_void_p, C.c_void_p,
                                     C.POINTER(PgoResult)]
    lib.qtr_default_place_params.argtypes = [C.POINTER(PlaceParams)]
    lib.qtr_place_index_create.argtypes = [C.c_void_p, C.POINTER(PlaceParams), C.c_int, C.POINTER(C.c_void_p)]
    lib.qtr_place_index_destroy.restype = None
    lib.qtr_place_index_destroy.argtypes = [C.c_void_p, C.c_void_p]
    lib.qtr_place_index_get_info.argtypes = [C.c_void_p, C.POINTER(PlaceIndexInfo)]
    lib.qtr_place_describe.argtypes = [C.c_void_p, C.c_int, C.POINTER(PlaceParams), C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.qtr_place_index_add.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    lib.qtr_place_index_add_desc.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.qtr_place_index_fetch.restype = C.c_longlong
    lib.qtr_place_index_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    lib.qtr_place_query.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                    C.POINTER(PlaceMatch), C.POINTER(C.c_int)]
    lib.qtr_place_query_desc.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.POINTER(PlaceMatch), C.POINTER(C.c_int)]


# QTR_EXT_LIB: the extension library that belongs to QTR_LIB's build
EXT_LIB_PATH = os.environ.get("QTR_EXT_LIB") or os.path.join(_HERE, "libquatro_ext.so")


def load_ext():
    """libquatro_ext.so: the entry points of the extension headers (EXT_EXPORTS).  They take the handles, keyframes, indexes
    and maps of load()'s library, which is loaded first; both are linked from one object (quatro_amd.build.build)."""
    return _open(EXT_LIB_PATH, _ext_signatures, product_first=True)


def _ext_signatures(lib):
    lib.qtr_default_voxel_map_params.argtypes = [C.POINTER(VoxelMapParams)]
    lib.qtr_default_voxel_map_params.restype = None
    lib.qtr_voxel_map_create.argtypes = [C.c_void_p, C.POINTER(VoxelMapParams), C.POINTER(C.c_void_p)]
    lib.qtr_voxel_map_destroy.restype = None
    lib.qtr_voxel_map_destroy.argtypes = [C.c_void_p, C.c_void_p]
    lib.qtr_voxel_map_clear.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.qtr_voxel_map_get_info.argtypes = [C.c_void_p, C.POINTER(VoxelMapInfo)]
    lib.qtr_voxel_map_insert.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                         C.POINTER(VoxelMapInsertInfo)]
    lib.qtr_voxel_map_insert_keyframe.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.POINTER(VoxelMapInsertInfo)]
    lib.qtr_voxel_map_register.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                           C.POINTER(IcpParams), C.POINTER(IcpResult), C.c_int]
    lib.qtr_voxel_map_register_keyframe.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.POINTER(IcpParams), C.POINTER(IcpResult)]
    lib.qtr_voxel_map_fetch.restype = C.c_longlong
    lib.qtr_voxel_map_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    lib.qtr_voxel_map_evict.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_double * 3), C.c_double,
                                        C.POINTER(VoxelMapEvictInfo)]
    lib.qtr_voxel_map_restore.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.qtr_deskew.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                               C.c_double, C.c_void_p, C.c_int, C.POINTER(DeskewInfo)]
    lib.qtr_keyframe_create_deskewed.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_int, C.c_double, C.POINTER(FrontendParams), C.c_int,
                                                 C.POINTER(C.c_void_p), C.POINTER(DeskewInfo)]
    lib.qtr_deskew_pose_at.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p]
    lib.qtr_default_carve_params.argtypes = [C.POINTER(CarveParams)]
    lib.qtr_default_carve_params.restype = None
    lib.qtr_voxel_map_carve.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                        C.POINTER(CarveParams), C.c_int, C.POINTER(VoxelMapCarveInfo)]
    lib.qtr_voxel_map_carve_keyframes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_int,
                                                  C.POINTER(CarveParams), C.POINTER(VoxelMapCarveInfo)]
    lib.qtr_voxel_map_register_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(VmapRegItem), C.c_int,
                                                 C.POINTER(IcpParams), C.POINTER(IcpResult)]
    lib.qtr_voxel_map_batch_fetch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    lib.qtr_voxel_map_batch_fetch.restype = C.c_longlong
    lib.qtr_default_vmap_eval_params.argtypes = [C.POINTER(VmapEvalParams)]
    lib.qtr_default_vmap_eval_params.restype = None
    lib.qtr_voxel_map_evaluate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                           C.c_void_p, C.POINTER(VmapEvalParams), C.POINTER(VmapEvalResult)]
    lib.qtr_voxel_map_evaluate_keyframe.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.POINTER(VmapEvalParams), C.POINTER(VmapEvalResult)]
    lib.qtr_voxel_map_evaluate_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(VmapRegItem), C.c_int,
                                                 C.POINTER(VmapEvalParams), C.POINTER(VmapEvalResult)]
    lib.qtr_voxel_map_eval_fetch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    lib.qtr_voxel_map_eval_fetch.restype = C.c_longlong
    lib.qtr_place_query_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(PlaceQueryItem), C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p]
    lib.qtr_place_batch_fetch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    lib.qtr_place_batch_fetch.restype = C.c_longlong
    lib.qtr_voxel_map_register_ct.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.POINTER(IcpParams),
                                              C.POINTER(IcpResult), C.c_int, C.POINTER(VmapCtInfo)]
    lib.qtr_voxel_map_ct_pose_at.argtypes = [C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]


def ct_pose_at(t_begin: float, t_end: float, begin_pose, end_pose, t: float) -> np.ndarray:
    """qtr_voxel_map_ct_pose_at: the 4 x 4 pose at time t between (t_begin, begin_pose) and (t_end, end_pose) by the rule of
    VoxelMap.register_ct (host only).  ValueError where the two poses differ by a rotation above pi / 2 or the times are
    not finite with t_begin < t_end."""
    B, E, T = _guess16(begin_pose), _guess16(end_pose), np.zeros(16, dtype=np.float64)
    rc = load_ext().qtr_voxel_map_ct_pose_at(float(t_begin), float(t_end), B.ctypes.data, E.ctypes.data, float(t), T.ctypes.data)
    if rc != QTR_OK:
        raise ValueError("ct_pose_at: refused (times not finite with t_begin < t_end, a non-finite pose, or a rotation above pi / 2)")
    return T.reshape(4, 4)


def default_vmap_eval_params(per_point: bool = False) -> VmapEvalParams:
    p = VmapEvalParams()
    load_ext().qtr_default_vmap_eval_params(C.byref(p))
    p.per_point = 1 if per_point else 0
    return p


def _vmap_eval_dict(res: VmapEvalResult) -> dict:
    return {"status": res.status, "valid": bool(res.valid), "n_source": res.n_source, "n_corr": res.n_corr,
            "overlap": res.overlap, "sum_d2": res.sum_d2, "inlier_rmse": res.inlier_rmse, "sum_w": res.sum_w,
            "chi2": res.chi2, "rmse": res.rmse, "information": np.array(res.information[:]).reshape(6, 6),
            "hessian": np.array(res.hessian[:]).reshape(6, 6), "gradient": np.array(res.gradient[:])}


def default_carve_params(**kw) -> CarveParams:
    """qtr_default_carve_params (64 x 1024 pixels over [-25.5, 2.5] degrees, window 2, min_votes 1, margin_abs 0 = the map's
    voxel_size, ranges 1 .. 80 m), with the given fields replaced."""
    p = CarveParams()
    load_ext().qtr_default_carve_params(C.byref(p))
    for k, v in kw.items():
        if k not in dict(CarveParams._fields_) or k == "reserved":
            raise TypeError(f"default_carve_params: no parameter {k!r}")
        setattr(p, k, v)
    return p


def _knots(knot_times, knot_poses):
    """(times [K] float64, poses [K, 16] float64), contiguous host arrays."""
    kt = np.ascontiguousarray(np.asarray(knot_times, dtype=np.float64).reshape(-1))
    kp = np.ascontiguousarray(np.asarray(knot_poses, dtype=np.float64).reshape(-1, 16))
    if kt.shape[0] != kp.shape[0]:
        raise ValueError(f"{kt.shape[0]} knot times, {kp.shape[0]} knot poses")
    return kt, kp


def deskew_pose_at(knot_times, knot_poses, t: float) -> np.ndarray:
    """qtr_deskew_pose_at (host only): the 4 x 4 pose the knots give at time t by the deskew's rule — rotation along the
    geodesic of the knot interval, translation linearly, the first / last interval extrapolated outside the knots."""
    kt, kp = _knots(knot_times, knot_poses)
    T = np.zeros(16, dtype=np.float64)
    rc = load_ext().qtr_deskew_pose_at(kt.ctypes.data, kp.ctypes.data, int(kt.shape[0]), float(t), T.ctypes.data)
    if rc != QTR_OK:
        raise QuatroHipError(rc, "qtr_deskew_pose_at: the knots are refused (2 .. 256 of them, finite and strictly increasing "
                                 "times, finite poses, at most pi / 2 of rotation between two)")
    return T.reshape(4, 4)


def comm_unique_id() -> bytes:
    """The rendezvous id rank 0 creates for qtr_comm_init (128 bytes)."""
    buf = C.create_string_buffer(128)
    if load().qtr_comm_unique_id(buf) != QTR_OK:
        raise RuntimeError("qtr_comm_unique_id failed (librccl not available?)")
    return buf.raw


def default_params() -> Params:
    p = Params()
    load().qtr_default_params(C.byref(p))
    return p


def demo_params(**kw) -> Params:
    """config/params.yaml values (what the reference demo actually runs)."""
    p = Params()
    load().qtr_demo_params(C.byref(p))
    for k, v in kw.items():
        if k == "ryrx":
            for i, x in enumerate(np.asarray(v, dtype=np.float64).reshape(-1)):
                p.ryrx[i] = float(x)
        else:
            setattr(p, k, v)
    return p


def default_frontend_params(**kw) -> FrontendParams:
    p = FrontendParams()
    load().qtr_default_frontend_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_icp_params(**kw) -> IcpParams:
    """pcl::IterativeClosestPoint-style knobs (qtr_default_icp_params), fields overridden by keyword."""
    p = IcpParams()
    load().qtr_default_icp_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_eval_params(**kw) -> EvalParams:
    """The evaluation's knob (qtr_default_eval_params: 1.0 m, like the ICP's), overridden by keyword."""
    p = EvalParams()
    load().qtr_default_eval_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_pgo_params(**kw) -> PgoParams:
    """The pose-graph optimisation's knobs (qtr_default_pgo_params), overridden by keyword."""
    p = PgoParams()
    load().qtr_default_pgo_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def pgo_arrays(poses, edges, fixed=None):
    """The arrays qtr_pgo_optimize takes, from poses (N x 4 x 4) and edges: (s, t, Z 4x4, information 6x6, uncertain)
    tuples.  Returns (poses [N, 16], fixed uint8 [N] or None, src, dst int32 [E], Z [E, 16], info [E, 36], uncertain uint8)."""
    X = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 16))
    E = len(edges)
    src = np.ascontiguousarray([e[0] for e in edges], dtype=np.int32).reshape(E)
    dst = np.ascontiguousarray([e[1] for e in edges], dtype=np.int32).reshape(E)
    Z = np.ascontiguousarray(np.asarray([np.asarray(e[2], dtype=np.float64).reshape(16) for e in edges],
                                        dtype=np.float64).reshape(E, 16))
    info = np.ascontiguousarray(np.asarray([np.asarray(e[3], dtype=np.float64).reshape(36) for e in edges],
                                           dtype=np.float64).reshape(E, 36))
    unc = np.ascontiguousarray([1 if e[4] else 0 for e in edges], dtype=np.uint8).reshape(E)
    fx = None if fixed is None else np.ascontiguousarray(np.asarray(fixed).astype(bool).astype(np.uint8).reshape(-1))
    return X, fx, src, dst, Z, info, unc


def _pgo_dict(res: PgoResult) -> dict:
    return {"status": res.status, "valid": bool(res.valid), "iterations": res.iterations, "accepted": res.accepted,
            "pcg_iterations_total": res.pcg_iterations_total, "stop_reason": res.stop_reason, "n_pruned": res.n_pruned,
            "objective_initial": res.objective_initial, "objective_final": res.objective_final,
            "lambda_final": res.lambda_final}


def _eval_dict(res: EvalResult) -> dict:
    return {"status": res.status, "valid": bool(res.valid), "n_source": res.n_source, "n_corr": res.n_corr,
            "n_plane": res.n_plane, "T": np.array(res.T[:]).reshape(4, 4), "overlap": res.overlap, "sum_d2": res.sum_d2,
            "inlier_rmse": res.inlier_rmse, "plane_rmse": res.plane_rmse,
            "information": np.array(res.information[:]).reshape(6, 6),
            "hessian_plane": np.array(res.hessian_plane[:]).reshape(6, 6)}


def default_place_params(**kw) -> PlaceParams:
    """Scan Context's usual shape (qtr_default_place_params: 20 rings x 60 sectors, 80 m, +2 m), fields overridden by keyword."""
    p = PlaceParams()
    load().qtr_default_place_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _guess16(guess):
    if guess is None:
        return None
    g = np.ascontiguousarray(np.asarray(guess, dtype=np.float64).reshape(16))
    return g


def _icp_dict(res: IcpResult) -> dict:
    return {"status": res.status, "valid": bool(res.valid), "converged": bool(res.converged),
            "stop_reason": res.stop_reason, "iterations": res.iterations, "n_corr": res.n_corr,
            "T": np.array(res.T[:]).reshape(4, 4), "fitness": res.fitness, "rmse": res.rmse}


def _ptr(a):
    """numpy array -> (host pointer, MEM_HOST); torch CUDA tensor -> (device pointer, MEM_DEVICE)."""
    if a is None:
        return None, None
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return a.ctypes.data, MEM_HOST
    # torch tensor
    assert a.is_contiguous()
    return a.data_ptr(), (MEM_DEVICE if a.is_cuda else MEM_HOST)


def _f4(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    assert a.ndim == 2 and a.shape[1] == 4, "points must be [N,4] float32 (x,y,z,pad)"
    return a


class Keyframe:
    """One scan's front end kept on the device (qtr_keyframe): made by Handle.keyframe, read-only, freed by close() / the
    context manager — or by the handle's close() at the latest (it is then dead: do not use it afterwards)."""

    deskew = None  # n_points, n_skipped, n_extrapolated of the deskew, for a keyframe made of a raw sweep with its times

    def __init__(self, handle: "Handle", ptr: int):
        self._handle, self._kf = handle, C.c_void_p(ptr)
        info = KeyframeInfo()
        handle._check(handle._lib.qtr_keyframe_get_info(self._kf, C.byref(info)))
        self.info = {n: getattr(info, n) for n, _ in KeyframeInfo._fields_}

    def fetch(self, what: int = KF_VOX) -> np.ndarray:
        """KF_VOX / KF_NORMALS -> [n, 4], KF_FPFH -> [n, 33], KF_MEAN -> [4] float32, copied to the host."""
        h = self._handle
        nbytes = h._lib.qtr_keyframe_fetch(h._h, self._kf, what, None, 0)
        if nbytes < 0:
            raise QuatroHipError(-1, "qtr_keyframe_fetch failed")
        out = np.zeros(nbytes // 4, dtype=np.float32)
        if nbytes and h._lib.qtr_keyframe_fetch(h._h, self._kf, what, out.ctypes.data, nbytes) < 0:
            raise QuatroHipError(-1, "qtr_keyframe_fetch failed")
        return out.reshape(-1, 33) if what == KF_FPFH else out if what == KF_MEAN else out.reshape(-1, 4)

    def close(self):
        if self._kf and getattr(self._handle, "_h", None):
            self._handle._lib.qtr_keyframe_destroy(self._handle._h, self._kf)
        self._kf = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class VoxelMap:
    """A persistent Gaussian voxel map on the device (qtr_voxel_map): made by Handle.voxel_map, freed by destroy() / the
    context manager — or by the handle's close() at the latest.  Registrations only read it (any number of slots at once);
    insert / insert_keyframe / clear are the caller's to serialise."""

    def __init__(self, handle: "Handle", ptr: int):
        self._handle, self._m, self._vlib = handle, C.c_void_p(ptr), load_ext()

    def info(self) -> dict:
        info = VoxelMapInfo()
        self._handle._check(self._vlib.qtr_voxel_map_get_info(self._m, C.byref(info)))
        return {n: getattr(info, n) for n, _ in VoxelMapInfo._fields_}

    def __len__(self) -> int:
        return self.info()["n_voxels"]

    @staticmethod
    def _cloud(xyz4, normals4):
        """(points pointer, normals pointer, n, mem) of numpy arrays (host) or torch tensors (all on the device)."""
        if isinstance(xyz4, np.ndarray) or not hasattr(xyz4, "data_ptr"):
            xyz4 = _f4(xyz4)
            normals4 = None if normals4 is None else _f4(normals4)
            assert normals4 is None or normals4.shape == xyz4.shape
            return xyz4, normals4, xyz4.ctypes.data, None if normals4 is None else normals4.ctypes.data, MEM_HOST
        (pp, m1), (pn, m2) = _ptr(xyz4), _ptr(normals4)
        assert m1 == MEM_DEVICE and m2 in (None, MEM_DEVICE), "torch tensors must all be on the device"
        assert xyz4.shape[-1] == 4 and (normals4 is None or normals4.shape == xyz4.shape)
        return xyz4, normals4, pp, pn, MEM_DEVICE

    @staticmethod
    def _ins_dict(info: VoxelMapInsertInfo) -> dict:
        return {n: getattr(info, n) for n, _ in VoxelMapInsertInfo._fields_}

    def insert(self, xyz4, normals4, pose=None, slot: int = 0) -> dict:
        """Folds the cloud's points under pose (4 x 4, cloud frame -> world; None = identity) into the map
        (qtr_voxel_map_insert); returns n_points, n_members, n_new_voxels, n_touched_voxels."""
        h = self._handle
        keep_p, keep_n, pp, pn, mem = self._cloud(xyz4, normals4)
        g, info = _guess16(pose), VoxelMapInsertInfo()
        h._check(self._vlib.qtr_voxel_map_insert(h._h, slot, self._m, pp, pn, int(keep_p.shape[0]),
                                             None if g is None else g.ctypes.data, mem, C.byref(info)))
        return self._ins_dict(info)

    def insert_keyframe(self, kf: Keyframe, pose=None, slot: int = 0) -> dict:
        """insert of the keyframe's stored voxels and normals, read in place (qtr_voxel_map_insert_keyframe)."""
        h = self._handle
        g, info = _guess16(pose), VoxelMapInsertInfo()
        h._check(self._vlib.qtr_voxel_map_insert_keyframe(h._h, slot, self._m, kf._kf, None if g is None else g.ctypes.data,
                                                      C.byref(info)))
        return self._ins_dict(info)

    def register(self, src4, src_normals4, guess=None, params: IcpParams | None = None, slot: int = 0) -> dict:
        """Voxelised plane-to-plane refinement of the scan against the map (qtr_voxel_map_register); params None = the
        defaults with method = ICP_VOXEL_PLANE_TO_PLANE.  max_correspondence_distance is ignored: the side is the map's."""
        h = self._handle
        prm = params or default_icp_params(method=ICP_VOXEL_PLANE_TO_PLANE)
        keep_p, keep_n, pp, pn, mem = self._cloud(src4, src_normals4)
        g, res = _guess16(guess), IcpResult()
        rc = self._vlib.qtr_voxel_map_register(h._h, slot, self._m, pp, int(keep_p.shape[0]), pn,
                                           None if g is None else g.ctypes.data, C.byref(prm), C.byref(res), mem)
        h._check(rc)
        return _icp_dict(res)

    def register_keyframe(self, kf: Keyframe, guess=None, params: IcpParams | None = None, slot: int = 0) -> dict:
        """register of the keyframe's stored voxels and normals, read in place (qtr_voxel_map_register_keyframe)."""
        h = self._handle
        prm = params or default_icp_params(method=ICP_VOXEL_PLANE_TO_PLANE)
        g, res = _guess16(guess), IcpResult()
        rc = self._vlib.qtr_voxel_map_register_keyframe(h._h, slot, self._m, kf._kf, None if g is None else g.ctypes.data,
                                                    C.byref(prm), C.byref(res))
        h._check(rc)
        return _icp_dict(res)

    def register_ct(self, cloud, normals, times, t_begin: float, t_end: float, begin_pose, guess_end=None,
                    icp: IcpParams | None = None, slot: int = 0) -> dict:
        """Continuous-time registration of a RAW sweep against the map (qtr_voxel_map_register_ct): `times` [n] float32 holds
        the time of every point, begin_pose (4 x 4, sensor at t_begin -> world) is held fixed and the sensor's pose at t_end
        is fitted from guess_end (None: begin_pose), every point carried by the pose interpolated at its own time.  Returns
        register's dict — T is the END pose — plus "info": n_points, n_skipped (a non-finite coordinate or time, an unusable
        normal), n_extrapolated (times outside [t_begin, t_end]; they still take part).  cloud, normals and times are numpy
        arrays, or torch tensors that all live on the device."""
        h = self._handle
        prm = icp or default_icp_params(method=ICP_VOXEL_PLANE_TO_PLANE)
        keep_p, keep_n, pp, pn, mem = self._cloud(cloud, normals)
        if isinstance(times, np.ndarray) or not hasattr(times, "data_ptr"):
            times = np.ascontiguousarray(times, dtype=np.float32).reshape(-1)
        else:
            import torch
            assert times.dtype == torch.float32
        pt, mt = _ptr(times)
        n = int(keep_p.shape[0])
        if mt != mem:
            raise ValueError("cloud, normals and times must all be host arrays or all be device tensors")
        if int(times.shape[0]) != n or len(times.shape) != 1:
            raise ValueError(f"{n} points, times of shape {tuple(times.shape)}")
        B, g, res, info = _guess16(begin_pose), _guess16(guess_end), IcpResult(), VmapCtInfo()
        rc = load_ext().qtr_voxel_map_register_ct(h._h, slot, self._m, pp, n, pn, pt, float(t_begin), float(t_end),
                                                   None if B is None else B.ctypes.data, None if g is None else g.ctypes.data,
                                                   C.byref(prm), C.byref(res), mem, C.byref(info))
        h._check(rc)
        out = _icp_dict(res)
        out["info"] = {k: getattr(info, k) for k, _ in VmapCtInfo._fields_}
        return out

    def _batch_items(self, items):
        """The C items of [(Keyframe, guess) | (xyz4, normals4, guess)] and the arrays that must outlive the call."""
        arr, keep = (VmapRegItem * max(len(items), 1))(), []
        for a, item in zip(arr, items):
            if len(item) == 2:
                a.kf, guess = item[0]._kf.value, item[1]
            else:
                keep_p, keep_n, pp, pn, mem = self._cloud(item[0], item[1])
                keep += [keep_p, keep_n]
                a.kf, a.src4, a.src_normals4, a.n, a.mem, guess = None, pp, pn, int(keep_p.shape[0]), mem, item[2]
            g = np.eye(4).reshape(16) if guess is None else _guess16(guess)
            a.guess[:] = [float(v) for v in g]
        return arr, keep

    def register_batch_raw(self, items, params: IcpParams | None = None, slot: int = 0):
        """qtr_voxel_map_register_batch on at most VMAP_BATCH_MAX items as it stands: (return code, the IcpResult array)."""
        h, blib = self._handle, load_ext()
        prm = params or default_icp_params(method=ICP_VOXEL_PLANE_TO_PLANE)
        items = list(items)
        arr, keep = self._batch_items(items)
        res = (IcpResult * max(len(items), 1))()
        rc = blib.qtr_voxel_map_register_batch(h._h, slot, self._m, arr, len(items), C.byref(prm), res)
        del keep
        return rc, res

    def register_batch(self, items, params: IcpParams | None = None, slot: int = 0) -> list:
        """A batch of registrations against the map in one chain of launches (qtr_voxel_map_register_batch).  items: a list of
        (Keyframe, guess) or (xyz4, normals4, guess), the clouds numpy arrays (host) or contiguous torch device tensors,
        guess 4 x 4 (None = identity).  Returns one ICP dict per item, each what register / register_keyframe returns for
        that item alone, bit for bit.  More than VMAP_BATCH_MAX items run in chunks of VMAP_BATCH_MAX in list order (then
        batch_fetch serves the last chunk).  params None = the defaults with method = ICP_VOXEL_PLANE_TO_PLANE."""
        items, out = list(items), []
        for a in range(0, len(items), VMAP_BATCH_MAX):
            chunk = items[a:a + VMAP_BATCH_MAX]
            rc, res = self.register_batch_raw(chunk, params, slot)
            self._handle._check(rc)
            out += [_icp_dict(res[i]) for i in range(len(chunk))]
        return out

    def batch_fetch(self, item: int, what: int = VMAP_BATCH_TRACE, slot: int = 0) -> np.ndarray:
        """Of item `item` of the slot's last batch (qtr_voxel_map_batch_fetch): VMAP_BATCH_TRACE -> float64 [iterations, 18],
        VMAP_BATCH_CORR -> int32 [n] (0 matched, -1 none, at the last evaluation), VMAP_BATCH_TIMES -> float32 [2] (device ms
        before the loop and of the loop; the whole batch's)."""
        h, blib = self._handle, load_ext()
        dtype, cols = {VMAP_BATCH_TRACE: (np.float64, 18), VMAP_BATCH_CORR: (np.int32, 0), VMAP_BATCH_TIMES: (np.float32, 0)}[what]
        nbytes = blib.qtr_voxel_map_batch_fetch(h._h, slot, item, what, None, 0)
        if nbytes < 0:
            raise QuatroHipError(-1, "qtr_voxel_map_batch_fetch failed")
        out = np.zeros(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        if nbytes and blib.qtr_voxel_map_batch_fetch(h._h, slot, item, what, out.ctypes.data, nbytes) < 0:
            raise QuatroHipError(-1, "qtr_voxel_map_batch_fetch failed")
        return out.reshape(-1, cols) if cols else out

    def evaluate(self, xyz4, normals4, T, per_point: bool = False, slot: int = 0) -> dict:
        """The scan evaluated against the map under the pose T (4 x 4, scan frame -> map frame), without stepping it
        (qtr_voxel_map_evaluate): valid, n_source, n_corr, overlap, sum_d2, inlier_rmse (distance to the voxel means), sum_w,
        chi2, rmse (the registration's at T), information (6 x 6, Open3D's form, rotation first, on the voxel means), hessian
        (the registration's normal matrix at T) and gradient.  per_point keeps the labels eval_fetch serves."""
        h, elib = self._handle, load_ext()
        keep_p, keep_n, pp, pn, mem = self._cloud(xyz4, normals4)
        g, prm, res = _guess16(T), default_vmap_eval_params(per_point), VmapEvalResult()
        rc = elib.qtr_voxel_map_evaluate(h._h, slot, self._m, pp, pn, int(keep_p.shape[0]), mem,
                                         None if g is None else g.ctypes.data, C.byref(prm), C.byref(res))
        h._check(rc)
        return _vmap_eval_dict(res)

    def evaluate_keyframe(self, kf: Keyframe, T, per_point: bool = False, slot: int = 0) -> dict:
        """evaluate of the keyframe's stored voxels and normals, read in place (qtr_voxel_map_evaluate_keyframe)."""
        h, elib = self._handle, load_ext()
        g, prm, res = _guess16(T), default_vmap_eval_params(per_point), VmapEvalResult()
        rc = elib.qtr_voxel_map_evaluate_keyframe(h._h, slot, self._m, kf._kf, None if g is None else g.ctypes.data,
                                                  C.byref(prm), C.byref(res))
        h._check(rc)
        return _vmap_eval_dict(res)

    def evaluate_batch_raw(self, items, per_point: bool = False, slot: int = 0):
        """qtr_voxel_map_evaluate_batch on the items as they stand: (return code, the VmapEvalResult array)."""
        h, elib = self._handle, load_ext()
        items = list(items)
        arr, keep = self._batch_items(items)
        prm, res = default_vmap_eval_params(per_point), (VmapEvalResult * max(len(items), 1))()
        rc = elib.qtr_voxel_map_evaluate_batch(h._h, slot, self._m, arr, len(items), C.byref(prm), res)
        del keep
        return rc, res

    def evaluate_batch(self, items, per_point: bool = False, slot: int = 0) -> list:
        """A batch of evaluations in one launch (qtr_voxel_map_evaluate_batch).  items: register_batch's forms, (Keyframe, T)
        or (xyz4, normals4, T).  Returns one evaluation dict per item, each what evaluate / evaluate_keyframe returns for
        that item alone, bit for bit.  More than the limit (VMAP_EVAL_MAX, with per_point VMAP_BATCH_MAX) run in chunks in
        list order (then eval_fetch serves the last chunk)."""
        items, out = list(items), []
        lim = VMAP_BATCH_MAX if per_point else VMAP_EVAL_MAX
        for a in range(0, len(items), lim):
            chunk = items[a:a + lim]
            rc, res = self.evaluate_batch_raw(chunk, per_point, slot)
            self._handle._check(rc)
            out += [_vmap_eval_dict(res[i]) for i in range(len(chunk))]
        return out

    def eval_fetch(self, item: int, what: int = VMAP_EVAL_CORR, slot: int = 0) -> np.ndarray:
        """Of item `item` of the slot's last evaluation (qtr_voxel_map_eval_fetch): VMAP_EVAL_CORR -> int32 [n] (0 matched, -1
        none), VMAP_EVAL_POINT -> float64 [n, 2] ((w d^T M d, w) of a matched point, (0, 0) otherwise; both only after a
        per_point call), VMAP_EVAL_TIMES -> float32 [1] (device ms of the upload and the launch)."""
        h, elib = self._handle, load_ext()
        dtype, cols = {VMAP_EVAL_CORR: (np.int32, 0), VMAP_EVAL_POINT: (np.float64, 2), VMAP_EVAL_TIMES: (np.float32, 0)}[what]
        nbytes = elib.qtr_voxel_map_eval_fetch(h._h, slot, item, what, None, 0)
        if nbytes < 0:
            raise QuatroHipError(-1, "qtr_voxel_map_eval_fetch failed")
        out = np.zeros(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        if nbytes and elib.qtr_voxel_map_eval_fetch(h._h, slot, item, what, out.ctypes.data, nbytes) < 0:
            raise QuatroHipError(-1, "qtr_voxel_map_eval_fetch failed")
        return out.reshape(-1, cols) if cols else out

    def fetch(self, what: int = VMAP_CLOUD) -> np.ndarray:
        """In ascending key order: VMAP_COORDS -> int32 [n, 3], VMAP_COUNT -> int32 [n], VMAP_SUMS / VMAP_RECORDS ->
        float64 [n, 9], VMAP_CLOUD -> float32 [n, 4] (the means, w = members)."""
        h = self._handle
        dtype, cols = {VMAP_COORDS: (np.int32, 3), VMAP_COUNT: (np.int32, 0), VMAP_SUMS: (np.float64, 9),
                       VMAP_RECORDS: (np.float64, 9), VMAP_CLOUD: (np.float32, 4)}[what]
        nbytes = self._vlib.qtr_voxel_map_fetch(h._h, self._m, what, None, 0)
        if nbytes < 0:
            raise QuatroHipError(-1, "qtr_voxel_map_fetch failed")
        out = np.zeros(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        if nbytes and self._vlib.qtr_voxel_map_fetch(h._h, self._m, what, out.ctypes.data, nbytes) < 0:
            raise QuatroHipError(-1, "qtr_voxel_map_fetch failed")
        return out.reshape(-1, cols) if cols else out

    def clear(self, slot: int = 0) -> None:
        """Empties the map; its voxel size and capacity stay (qtr_voxel_map_clear)."""
        self._handle._check(self._vlib.qtr_voxel_map_clear(self._handle._h, slot, self._m))

    def evict(self, centre, radius: float, slot: int = 0) -> dict:
        """Sliding-window eviction (qtr_voxel_map_evict): with C = floor(centre / voxel_size) and R = floor(radius /
        voxel_size), the voxels with |coordinates - C|^2 > R^2 (in integers) leave the map; the others stay bit for bit.
        Returns n_kept, n_evicted, n_members_evicted."""
        h, klib = self._handle, load_ext()
        c = (C.c_double * 3)(*[float(x) for x in np.asarray(centre, dtype=np.float64).reshape(3)])
        info = VoxelMapEvictInfo()
        h._check(klib.qtr_voxel_map_evict(h._h, slot, self._m, C.byref(c), float(radius), C.byref(info)))
        return {n: getattr(info, n) for n, _ in VoxelMapEvictInfo._fields_}

    def carve(self, xyz4, pose=None, params: "CarveParams | None" = None, slot: int = 0) -> dict:
        """Visibility carving with one scan (qtr_voxel_map_carve): xyz4 [n, 4] float32 (numpy, or a contiguous torch device
        tensor) taken at pose (4 x 4, scan frame -> map frame; None = identity).  A voxel whose mean the scan saw through
        — the centre pixel of its range image is filled and no filled pixel of the window around it holds a range
        <= r_v + margin — leaves the map; the others stay bit for bit.  Carve with the raw sweep, not a ground-removed
        cloud.  Returns n_kept, n_carved, n_tested, n_members_carved."""
        h, clib = self._handle, load_ext()
        if isinstance(xyz4, np.ndarray) or not hasattr(xyz4, "data_ptr"):
            xyz4 = _f4(xyz4)
        else:
            assert xyz4.shape[-1] == 4
        pp, mem = _ptr(xyz4)
        g, info = _guess16(pose), VoxelMapCarveInfo()
        h._check(clib.qtr_voxel_map_carve(h._h, slot, self._m, pp, int(xyz4.shape[0]), None if g is None else g.ctypes.data,
                                          None if params is None else C.byref(params), mem, C.byref(info)))
        return self._carve_dict(info)

    def carve_keyframes(self, kfs, poses, params: "CarveParams | None" = None, slot: int = 0) -> dict:
        """Visibility carving with 0 .. 64 keyframes of this handle, each under its pose ([K, 4, 4]), their stored voxels read
        in place (qtr_voxel_map_carve_keyframes); a voxel leaves when at least params.min_votes of them saw through it.
        Not for merged (submap) keyframes: they have no single viewpoint."""
        h, clib = self._handle, load_ext()
        kfs = list(kfs)
        P = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 16))
        if P.shape[0] != len(kfs):
            raise ValueError(f"{len(kfs)} keyframes, {P.shape[0]} poses")
        arr = (C.c_void_p * max(len(kfs), 1))(*[k._kf.value for k in kfs])
        info = VoxelMapCarveInfo()
        h._check(clib.qtr_voxel_map_carve_keyframes(h._h, slot, self._m, arr, P.ctypes.data, len(kfs),
                                                    None if params is None else C.byref(params), C.byref(info)))
        return self._carve_dict(info)

    @staticmethod
    def _carve_dict(info: "VoxelMapCarveInfo") -> dict:
        return {n: getattr(info, n) for n in ("n_kept", "n_carved", "n_tested", "n_members_carved")}

    def restore(self, coords, count, sums, slot: int = 0) -> None:
        """Puts voxels given as the fetch sections VMAP_COORDS (int32 [n, 3]), VMAP_COUNT (int32 [n]) and VMAP_SUMS (float64
        [n, 9]) into this map, which must hold no voxel (qtr_voxel_map_restore): numpy arrays (host) or contiguous torch
        tensors, all three on the device."""
        h, klib = self._handle, load_ext()
        if isinstance(coords, np.ndarray) or not hasattr(coords, "data_ptr"):
            coords = np.ascontiguousarray(coords, dtype=np.int32).reshape(-1, 3)
            count = np.ascontiguousarray(count, dtype=np.int32).reshape(-1)
            sums = np.ascontiguousarray(sums, dtype=np.float64).reshape(-1, 9)
        else:
            import torch
            assert (coords.dtype, count.dtype, sums.dtype) == (torch.int32, torch.int32, torch.float64)
        n = int(coords.shape[0])
        assert tuple(coords.shape) == (n, 3) and tuple(count.shape) == (n,) and tuple(sums.shape) == (n, 9)
        (pc, m1), (pn, m2), (ps, m3) = _ptr(coords), _ptr(count), _ptr(sums)
        assert m1 == m2 == m3, "coords, count and sums must all be host arrays or all be device tensors"
        h._check(klib.qtr_voxel_map_restore(h._h, slot, self._m, pc, pn, ps, n, m1))

    def save(self, path) -> None:
        """The whole state of the map as one .npz file (np.savez, which appends ".npz" to a name without it): voxel_size,
        capacity and the sections coords, count and sums.  Handle.load_voxel_map reads it back."""
        info = self.info()
        np.savez(path, voxel_size=np.float64(info["voxel_size"]), capacity=np.int64(info["capacity"]),
                 coords=self.fetch(VMAP_COORDS), count=self.fetch(VMAP_COUNT), sums=self.fetch(VMAP_SUMS))

    def destroy(self):
        if self._m and getattr(self._handle, "_h", None):
            self._vlib.qtr_voxel_map_destroy(self._handle._h, self._m)
        self._m = C.c_void_p()

    close = destroy

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.destroy()


class PlaceIndex:
    """A Scan Context place index on the device (qtr_place_index): made by Handle.place_index, freed by close() / the context
    manager — or by the handle's close() at the latest.  Queries only read it (any number of slots at once); add / add_desc
    write it and must not overlap a query or each other."""

    def __init__(self, handle: "Handle", ptr: int):
        self._handle, self._ix = handle, C.c_void_p(ptr)
        self.params = PlaceParams()
        info = self.info()
        self.params = PlaceParams(*[getattr(info["params"], n) for n, _ in PlaceParams._fields_])
        self.shape = (self.params.num_rings, self.params.num_sectors)

    def info(self) -> dict:
        i = PlaceIndexInfo()
        self._handle._check(self._handle._lib.qtr_place_index_get_info(self._ix, C.byref(i)))
        return {"params": i.params, "size": i.size, "capacity": i.capacity, "device_bytes": i.device_bytes}

    def __len__(self) -> int:
        return self.info()["size"]

    def _desc(self, desc):
        if isinstance(desc, np.ndarray):
            desc = np.ascontiguousarray(desc, dtype=np.float32)
        assert tuple(desc.shape) == self.shape, f"descriptor must be {self.shape}"
        return desc

    def describe(self, xyz4, slot: int = 0) -> np.ndarray:
        """qtr_place_describe with this index's parameters: [num_rings, num_sectors] float32 (see Handle.place_describe)."""
        return self._handle.place_describe(xyz4, self.params, slot)

    def add(self, kf: Keyframe, slot: int = 0) -> int:
        """qtr_place_index_add: the keyframe's descriptor becomes the next entry; returns its id."""
        h, out = self._handle, C.c_int(-1)
        h._check(h._lib.qtr_place_index_add(h._h, slot, self._ix, kf._kf, C.byref(out)))
        return out.value

    def add_desc(self, desc, slot: int = 0) -> int:
        """qtr_place_index_add_desc: a descriptor made earlier (numpy, or a contiguous torch device tensor)."""
        h, out = self._handle, C.c_int(-1)
        ptr, mem = _ptr(self._desc(desc))
        h._check(h._lib.qtr_place_index_add_desc(h._h, slot, self._ix, ptr, mem, C.byref(out)))
        return out.value

    def fetch(self, id: int, what: int = PLACE_DESC) -> np.ndarray:
        """PLACE_DESC -> [num_rings, num_sectors], PLACE_COLNORM2 -> [num_sectors] float32 of entry `id`."""
        h = self._handle
        nbytes = h._lib.qtr_place_index_fetch(h._h, self._ix, int(id), what, None, 0)
        if nbytes < 0:
            raise QuatroHipError(-1, "qtr_place_index_fetch failed")
        out = np.zeros(nbytes // 4, dtype=np.float32)
        if h._lib.qtr_place_index_fetch(h._h, self._ix, int(id), what, out.ctypes.data, nbytes) < 0:
            raise QuatroHipError(-1, "qtr_place_index_fetch failed")
        return out.reshape(self.shape) if what == PLACE_DESC else out

    @staticmethod
    def _matches(out, n: int) -> list:
        return [{"id": out[i].id, "shift": out[i].shift, "distance": np.float32(out[i].distance), "yaw": float(out[i].yaw)}
                for i in range(n)]

    def query(self, kf: Keyframe, k: int = 10, id_lo: int = 0, id_hi: int | None = None, slot: int = 0) -> list:
        """qtr_place_query: the min(k, candidates) entries of [id_lo, id_hi) most similar to the keyframe, as dicts
        id / shift / distance / yaw in ascending (distance, id) order."""
        h, n = self._handle, C.c_int(0)
        out = (PlaceMatch * PLACE_MAX_K)()
        hi = 2 ** 31 - 1 if id_hi is None else int(id_hi)
        h._check(h._lib.qtr_place_query(h._h, slot, self._ix, kf._kf, int(id_lo), hi, int(k), out, C.byref(n)))
        return self._matches(out, n.value)

    def query_desc(self, desc, k: int = 10, id_lo: int = 0, id_hi: int | None = None, slot: int = 0) -> list:
        """qtr_place_query_desc: the same for a descriptor."""
        h, n = self._handle, C.c_int(0)
        out = (PlaceMatch * PLACE_MAX_K)()
        hi = 2 ** 31 - 1 if id_hi is None else int(id_hi)
        ptr, mem = _ptr(self._desc(desc))
        h._check(h._lib.qtr_place_query_desc(h._h, slot, self._ix, ptr, mem, int(id_lo), hi, int(k), out, C.byref(n)))
        return self._matches(out, n.value)

    def _batch_item(self, item, keep: list) -> PlaceQueryItem:
        """One item of query_batch: a Keyframe, a descriptor (numpy, or a contiguous torch device tensor), an entry id of this
        index or (PlaceIndex, id) — alone, or as (source, (id_lo, id_hi)).  `keep` holds what the pointers point into."""
        rng = None
        if (isinstance(item, tuple) and len(item) == 2 and not isinstance(item[0], PlaceIndex)
                and (item[1] is None or isinstance(item[1], (tuple, list)))):
            item, rng = item  # ((PlaceIndex, id), range) comes through here too: its first member is a tuple
        it = PlaceQueryItem()
        it.id_lo, it.id_hi = (0, 2 ** 31 - 1) if rng is None else (int(rng[0]), 2 ** 31 - 1 if rng[1] is None else int(rng[1]))
        it.entry = -1
        if isinstance(item, Keyframe):
            it.kf = item._kf
        elif isinstance(item, tuple) and len(item) == 2 and isinstance(item[0], PlaceIndex):
            it.from_, it.entry = item[0]._ix, int(item[1])
        elif isinstance(item, (int, np.integer)):
            it.entry = int(item)
        else:
            d = self._desc(item)
            keep.append(d)
            it.desc, it.mem = _ptr(d)
        return it

    def query_batch(self, items, k: int = 10, slot: int = 0, raw: bool = False):
        """qtr_place_query_batch: every item's query in one chain of launches and one host wait.  Returns one list of
        match dicts per item (what query / query_desc return for it); raw=True returns the records themselves, a
        [Q, k] array of PLACE_MATCH_DTYPE (rows filled up to n[q], the rest zero) and n, int32 [Q]."""
        h, keep = self._handle, []
        Q = len(items)
        arr = (PlaceQueryItem * max(Q, 1))(*[self._batch_item(x, keep) for x in items])
        out = np.zeros((Q, max(int(k), 0)), dtype=PLACE_MATCH_DTYPE)
        n = np.zeros(Q, dtype=np.int32)
        h._check(load_ext().qtr_place_query_batch(h._h, slot, self._ix, arr, Q, int(k), out.ctypes.data, n.ctypes.data))
        if raw:
            return out, n
        return [[{"id": int(r["id"]), "shift": int(r["shift"]), "distance": np.float32(r["distance"]), "yaw": float(r["yaw"])}
                 for r in out[q, :n[q]]] for q in range(Q)]

    def batch_fetch(self, query: int, what: int = PLACE_BATCH_DIST, slot: int = 0) -> np.ndarray:
        """qtr_place_batch_fetch: PLACE_BATCH_DIST -> float32, PLACE_BATCH_SHIFT -> int32, one value per entry of the
        clamped range of query `query` of the slot's last query_batch, in id order."""
        h, lib = self._handle, load_ext()
        nbytes = lib.qtr_place_batch_fetch(h._h, slot, int(query), what, None, 0)
        if nbytes < 0:
            raise QuatroHipError(-1, "qtr_place_batch_fetch failed")
        out = np.zeros(nbytes // 4, dtype=np.float32 if what == PLACE_BATCH_DIST else np.int32)
        if nbytes and lib.qtr_place_batch_fetch(h._h, slot, int(query), what, out.ctypes.data, nbytes) < 0:
            raise QuatroHipError(-1, "qtr_place_batch_fetch failed")
        return out

    def close(self):
        if self._ix and getattr(self._handle, "_h", None):
            self._handle._lib.qtr_place_index_destroy(self._handle._h, self._ix)
        self._ix = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Handle:
    """One device + n_slots stream slots (qtr_handle)."""

    def __init__(self, device: int = 0, max_points: int = 262144, max_voxels: int = 65536, max_corr: int = 24576,
                 n_slots: int = 1, max_long_neighbors: int = 0, lib_path: str | None = None):
        self._lib = load(lib_path)
        lim = Limits(max_points, max_voxels, max_corr, n_slots, max_long_neighbors)
        self._h = C.c_void_p()
        rc = self._lib.qtr_create(device, C.byref(lim), C.byref(self._h))
        if rc != QTR_OK:
            msg = self._lib.qtr_last_error(self._h).decode() if self._h else "qtr_create failed"
            if self._h:
                self._lib.qtr_destroy(self._h)
                self._h = C.c_void_p()
            raise QuatroHipError(rc, msg)
        self.limits = lim
        self._time_limit = 3600.0  # MaxCliqueSolver::Params::time_limit default (reference include/teaser/graph.h)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.qtr_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self) -> str:
        return self._lib.qtr_last_error(self._h).decode()

    def _check(self, rc: int, ok=(QTR_OK,)):
        if rc not in ok:
            raise QuatroHipError(rc, self.last_error())
        return rc

    def stream_ptr(self, slot: int = 0) -> int:
        return int(self._lib.qtr_slot_stream(self._h, slot) or 0)

    # ---- host-array convenience wrappers (numpy in / numpy out) ---------------------------------
    def voxelize(self, xyz4, leaf: float, slot: int = 0):
        xyz4 = _f4(xyz4)
        out = np.zeros_like(xyz4)
        n = C.c_int()
        self._check(self._lib.qtr_voxelize(self._h, slot, xyz4.ctypes.data, xyz4.shape[0], leaf, out.ctypes.data,
                                           out.shape[0], C.byref(n), MEM_HOST))
        return out[: n.value].copy()

    def fpfh(self, xyz4, r_normal: float, r_fpfh: float, slot: int = 0):
        xyz4 = _f4(xyz4)
        n = xyz4.shape[0]
        nrm = np.zeros((n, 4), dtype=np.float32)
        desc = np.zeros((n, 33), dtype=np.float32)
        self._check(self._lib.qtr_fpfh(self._h, slot, xyz4.ctypes.data, n, r_normal, r_fpfh, nrm.ctypes.data,
                                       desc.ctypes.data, MEM_HOST))
        return nrm, desc

    def match(self, xyz_s, desc_s, xyz_t, desc_t, fp: FrontendParams | None = None, slot: int = 0):
        xyz_s, xyz_t = _f4(xyz_s), _f4(xyz_t)
        desc_s = np.ascontiguousarray(desc_s, dtype=np.float32)
        desc_t = np.ascontiguousarray(desc_t, dtype=np.float32)
        fp = fp or default_frontend_params()
        # cross-checked lists hold at most min(n_s, n_t) pairs; without the cross-check up to n_s + n_t
        cap = max(min(xyz_s.shape[0], xyz_t.shape[0]) if fp.use_crosscheck else xyz_s.shape[0] + xyz_t.shape[0], 1)
        corr = np.zeros((cap, 2), dtype=np.int32)
        L = C.c_int()
        self._check(self._lib.qtr_match(self._h, slot, xyz_s.ctypes.data, xyz_s.shape[0], desc_s.ctypes.data,
                                        xyz_t.ctypes.data, xyz_t.shape[0], desc_t.ctypes.data, C.byref(fp),
                                        corr.ctypes.data, cap, C.byref(L), MEM_HOST))
        return corr[: L.value].copy()

    def solve(self, src4, tgt4, params: Params | None = None, slot: int = 0):
        src4, tgt4 = _f4(src4), _f4(tgt4)
        L = src4.shape[0]
        assert tgt4.shape[0] == L
        prm = params or demo_params()
        res = Result()
        cap = max(L, 1)
        cl = np.zeros(cap, dtype=np.int32)
        rot = np.zeros(cap, dtype=np.int32)
        fin = np.zeros(cap, dtype=np.int32)
        rc = self._lib.qtr_solve(self._h, slot, src4.ctypes.data, tgt4.ctypes.data, L, C.byref(prm), C.byref(res),
                                 cl.ctypes.data, rot.ctypes.data, fin.ctypes.data, cap, MEM_HOST)
        self._check(rc, ok=(QTR_OK, QTR_ERR_CLIQUE_TOO_SMALL))
        return _result_dict(res, cl, rot, fin)

    def max_clique(self, bitmap, mode: int = 1, kcore_thr: float = 0.5, slot: int = 0, time_limit=None):
        """teaser::MaxCliqueSolver::findMaxClique on a bit-matrix graph [L][ceil(L/64)] uint64 -> (ids, max_core)."""
        bitmap = np.ascontiguousarray(bitmap, dtype=np.uint64)
        L = bitmap.shape[0]
        assert bitmap.ndim == 2 and (L == 0 or bitmap.shape[1] == (L + 63) // 64)
        cl = np.zeros(max(L, 1), dtype=np.int32)
        n, mcore = C.c_int(), C.c_int()
        tl = self._time_limit if time_limit is None else float(time_limit)
        self._check(self._lib.qtr_max_clique(self._h, slot, bitmap.ctypes.data, L, mode, kcore_thr, tl, cl.ctypes.data,
                                             cl.size, C.byref(n), C.byref(mcore), MEM_HOST))
        return cl[: n.value].copy(), mcore.value

    def set_clique_time_limit(self, seconds: float):
        """default MaxCliqueSolver::Params::time_limit of this wrapper's max_clique() calls (the C ABI takes the limit per
        call: qtr_max_clique's time_limit, qtr_params.max_clique_time_limit)"""
        self._time_limit = float(seconds)

    def exact_stats(self, slot: int = 0):
        n, a = C.c_ulonglong(), C.c_int()
        self._check(self._lib.qtr_exact_stats(self._h, slot, C.byref(n), C.byref(a)))
        return dict(nodes=int(n.value), aborted=bool(a.value))

    # ---- Patchwork ground segmentation (PatchWork::estimate_ground)
    def patchwork(self, xyz4, pp: "PwParams | None" = None, slot: int = 0):
        xyz4 = _f4(xyz4)
        pp = pp or pw_params()
        P = xyz4.shape[0]
        g = np.zeros((max(P, 1), 4), dtype=np.float32)
        n = np.zeros((max(P, 1), 4), dtype=np.float32)
        ng, nn = C.c_int(), C.c_int()
        self._check(self._lib.qtr_patchwork(self._h, slot, xyz4.ctypes.data, P, C.byref(pp), g.ctypes.data, max(P, 1),
                                            C.byref(ng), n.ctypes.data, max(P, 1), C.byref(nn), MEM_HOST))
        return dict(ground=g[:ng.value].copy(), nonground=n[:nn.value].copy())

    # ---- range-image projection + sub-cluster rejection (ImageProjection::segmentCloud, "Patchwork" mode)
    def segment_cloud(self, xyz4, ipp: "IpParams | None" = None, slot: int = 0, want_labels: bool = True):
        xyz4 = _f4(xyz4)
        ipp = ipp or ip_params()
        NP = ipp.n_scan * ipp.horizon_scan
        out = np.zeros((NP, 4), dtype=np.float32)
        outl = np.zeros((NP, 4), dtype=np.float32)
        lab = np.zeros(NP, dtype=np.int32) if want_labels else None
        nv, no, nseg = C.c_int(), C.c_int(), C.c_int()
        self._check(self._lib.qtr_segment_cloud(self._h, slot, xyz4.ctypes.data, xyz4.shape[0], C.byref(ipp),
                                                out.ctypes.data, NP, C.byref(nv), outl.ctypes.data, NP, C.byref(no),
                                                C.byref(nseg), lab.ctypes.data if want_labels else None, MEM_HOST))
        return dict(valid=out[:nv.value].copy(), outliers=outl[:no.value].copy(), n_segments=nseg.value,
                    labels=lab.reshape(ipp.n_scan, ipp.horizon_scan) if want_labels else None)

    # ---- the reference class's individually callable stages (row-major matrices) -------------------
    def compute_tims(self, v3n, slot: int = 0):
        v = np.ascontiguousarray(v3n, dtype=np.float64)
        N = v.shape[1]
        K = N * (N - 1) // 2
        tims = np.zeros((3, K), dtype=np.float64)
        mp = np.zeros((2, K), dtype=np.int32)
        self._check(self._lib.qtr_compute_tims(self._h, slot, v.ctypes.data, N, tims.ctypes.data, mp.ctypes.data))
        return tims, mp

    def scale_mask(self, tims_src, tims_dst, noise_bound: float, cbar2: float = 1.0, slot: int = 0):
        a = np.ascontiguousarray(tims_src, dtype=np.float64)
        b = np.ascontiguousarray(tims_dst, dtype=np.float64)
        K = a.shape[1]
        mask = np.zeros(K, dtype=np.uint8)
        self._check(self._lib.qtr_scale_mask(self._h, slot, a.ctypes.data, b.ctypes.data, K, noise_bound, cbar2,
                                             mask.ctypes.data))
        return mask.astype(bool)

    def gnc_rotation2d(self, src2, dst2, noise_bound: float, gnc_factor: float = 1.4, max_iter: int = 50,
                       cost_thr: float = 1.1e-4, slot: int = 0):
        """src2/dst2: (M, 2) arrays as the oracle's gnc_rotation2d takes them."""
        s2 = np.ascontiguousarray(np.asarray(src2, dtype=np.float64).T)
        d2 = np.ascontiguousarray(np.asarray(dst2, dtype=np.float64).T)
        M = s2.shape[1]
        R = np.zeros(4)
        cost, iters = C.c_double(), C.c_int()
        inl = np.zeros(M, dtype=np.uint8)
        self._check(self._lib.qtr_gnc_rotation2d(self._h, slot, s2.ctypes.data, d2.ctypes.data, M, noise_bound,
                                                 gnc_factor, max_iter, cost_thr, R.ctypes.data, C.byref(cost),
                                                 C.byref(iters), inl.ctypes.data))
        return R.reshape(2, 2), cost.value, iters.value, inl.astype(bool)

    def gnc_rotation3d(self, src3, dst3, noise_bound: float, gnc_factor: float = 1.4, max_iter: int = 50,
                       cost_thr: float = 1.1e-4, slot: int = 0):
        """src3/dst3: (M, 3) TIMs -> (R 3x3, cost, iterations, inlier mask); reg_name "TEASER"."""
        s3 = np.ascontiguousarray(np.asarray(src3, dtype=np.float64).T)
        d3 = np.ascontiguousarray(np.asarray(dst3, dtype=np.float64).T)
        M = s3.shape[1]
        R = np.zeros(9)
        cost, iters = C.c_double(), C.c_int()
        inl = np.zeros(M, dtype=np.uint8)
        self._check(self._lib.qtr_gnc_rotation3d(self._h, slot, s3.ctypes.data, d3.ctypes.data, M, noise_bound,
                                                 gnc_factor, max_iter, cost_thr, R.ctypes.data, C.byref(cost),
                                                 C.byref(iters), inl.ctypes.data))
        return R.reshape(3, 3), cost.value, iters.value, inl.astype(bool)

    def cote_estimate(self, X, rng: float, median: bool = True, slot: int = 0):
        X = np.ascontiguousarray(X, dtype=np.float64)
        inl = np.zeros(X.shape[0], dtype=np.uint8)
        est, nc = C.c_double(), C.c_int()
        self._check(self._lib.qtr_cote_estimate(self._h, slot, X.ctypes.data, X.shape[0], rng, 1 if median else 0,
                                                C.byref(est), inl.ctypes.data, C.byref(nc)))
        return est.value, inl.astype(bool), nc.value

    def cote_estimate_ranges(self, X, ranges, median: bool = True, slot: int = 0):
        X = np.ascontiguousarray(X, dtype=np.float64)
        R = np.ascontiguousarray(ranges, dtype=np.float64)
        inl = np.zeros(X.shape[0], dtype=np.uint8)
        est, nc = C.c_double(), C.c_int()
        self._check(self._lib.qtr_cote_estimate_ranges(self._h, slot, X.ctypes.data, R.ctypes.data, X.shape[0],
                                                       1 if median else 0, C.byref(est), inl.ctypes.data, C.byref(nc)))
        return est.value, inl.astype(bool), nc.value

    def register_pair(self, src_raw4, tgt_raw4, fp: FrontendParams | None = None, params: Params | None = None,
                      slot: int = 0):
        src_raw4, tgt_raw4 = _f4(src_raw4), _f4(tgt_raw4)
        fp = fp or default_frontend_params()
        prm = params or demo_params()
        res = Result()
        cap = int(self.limits.max_corr)
        cl = np.zeros(cap, dtype=np.int32)
        fin = np.zeros(cap, dtype=np.int32)
        rc = self._lib.qtr_register_pair(self._h, slot, src_raw4.ctypes.data, src_raw4.shape[0], tgt_raw4.ctypes.data,
                                         tgt_raw4.shape[0], C.byref(fp), C.byref(prm), C.byref(res), cl.ctypes.data,
                                         fin.ctypes.data, cap, MEM_HOST)
        self._check(rc, ok=(QTR_OK, QTR_ERR_CLIQUE_TOO_SMALL))
        return _result_dict(res, cl, None, fin)

    def feature_pair(self, src_raw4, tgt_raw4, fp: FrontendParams | None = None, slot: int = 0):
        """voxelize x2 + FPFHManager::setFeaturePair (reference include/fpfh_manager.hpp:98-153) in one launch chain:
        raw scans -> {n_src, n_tgt, L, src_kps [L,4], tgt_kps [L,4], corr [L,2]}."""
        src_raw4, tgt_raw4 = _f4(src_raw4), _f4(tgt_raw4)
        fp = fp or default_frontend_params()
        cap = int(self.limits.max_corr)
        sk = np.zeros((cap, 4), dtype=np.float32)
        tk = np.zeros((cap, 4), dtype=np.float32)
        corr = np.zeros((cap, 2), dtype=np.int32)
        ns, nt, L = C.c_int(), C.c_int(), C.c_int()
        self._check(self._lib.qtr_feature_pair(self._h, slot, src_raw4.ctypes.data, src_raw4.shape[0],
                                               tgt_raw4.ctypes.data, tgt_raw4.shape[0], C.byref(fp), C.byref(ns),
                                               C.byref(nt), C.byref(L), sk.ctypes.data, tk.ctypes.data,
                                               corr.ctypes.data, cap, MEM_HOST))
        return {"n_src": ns.value, "n_tgt": nt.value, "L": L.value, "src_kps": sk[:L.value].copy(),
                "tgt_kps": tk[:L.value].copy(), "corr": corr[:L.value].copy()}

    # ---- device-resident entry points (torch CUDA tensors or raw pointers) -----------------------
    def feature_pair_dev(self, src_ptr: int, Ps: int, tgt_ptr: int, Pt: int, fp: FrontendParams, slot: int = 0):
        """front end on device-resident scans; the matched clouds stay in the slot.  Returns (rc, n_src, n_tgt, L)."""
        ns, nt, L = C.c_int(), C.c_int(), C.c_int()
        rc = self._lib.qtr_feature_pair(self._h, slot, src_ptr, Ps, tgt_ptr, Pt, C.byref(fp), C.byref(ns), C.byref(nt),
                                        C.byref(L), None, None, None, 0, MEM_DEVICE)
        return rc, ns.value, nt.value, L.value

    def register_pair_dev(self, src_ptr: int, Ps: int, tgt_ptr: int, Pt: int, fp: FrontendParams, prm: Params,
                          res: Result, slot: int = 0) -> int:
        return self._lib.qtr_register_pair(self._h, slot, src_ptr, Ps, tgt_ptr, Pt, C.byref(fp), C.byref(prm),
                                           C.byref(res), None, None, 0, MEM_DEVICE)

    def register_pair_corr_dev(self, src_ptr: int, Ps: int, tgt_ptr: int, Pt: int, fp: FrontendParams, cs_ptr: int,
                               ct_ptr: int, n_corr: int, prm: Params, res: Result, slot: int = 0) -> int:
        """qtr_register_pair_corr on device-resident scans and correspondences: front end of the scans, back end on the given
        correspondences, one call"""
        return self._lib.qtr_register_pair_corr(self._h, slot, src_ptr, Ps, tgt_ptr, Pt, C.byref(fp), cs_ptr, ct_ptr, n_corr,
                                                C.byref(prm), C.byref(res), None, None, None, 0, MEM_DEVICE)

    def register_pair_corr(self, src_raw4, tgt_raw4, corr_src4, corr_tgt4, fp: FrontendParams | None = None,
                           params: Params | None = None, slot: int = 0):
        src_raw4, tgt_raw4, corr_src4, corr_tgt4 = _f4(src_raw4), _f4(tgt_raw4), _f4(corr_src4), _f4(corr_tgt4)
        fp = fp or default_frontend_params()
        prm = params or demo_params()
        res = Result()
        L = corr_src4.shape[0]
        cap = max(L, 1)
        cl = np.zeros(cap, dtype=np.int32)
        fin = np.zeros(cap, dtype=np.int32)
        nm = C.c_int()
        rc = self._lib.qtr_register_pair_corr(self._h, slot, src_raw4.ctypes.data, src_raw4.shape[0], tgt_raw4.ctypes.data,
                                              tgt_raw4.shape[0], C.byref(fp), corr_src4.ctypes.data, corr_tgt4.ctypes.data, L,
                                              C.byref(prm), C.byref(res), C.addressof(nm), cl.ctypes.data, fin.ctypes.data, cap,
                                              MEM_HOST)
        self._check(rc, ok=(QTR_OK, QTR_ERR_CLIQUE_TOO_SMALL))
        out = _result_dict(res, cl, None, fin)
        out["n_matched"] = nm.value
        return out

    def solve_dev(self, src_ptr: int, tgt_ptr: int, L: int, prm: Params, res: Result, slot: int = 0) -> int:
        return self._lib.qtr_solve(self._h, slot, src_ptr, tgt_ptr, L, C.byref(prm), C.byref(res), None, None, None,
                                   0, MEM_DEVICE)

    # ---- batched registration (qtr_submit_batch / qtr_wait): every slot of the handle is used
    def register_batch(self, pairs, fp: FrontendParams | None = None, params: Params | None = None, want_lists=True):
        """pairs: sequence of (src [n,4] float32, tgt [m,4] float32, seed) — or (src, tgt, seed, corr_src [L,4], corr_tgt
        [L,4]) for a pair that brings pre-matched correspondences (qtr_pair_desc.src_corr4 / tgt_corr4): src = tgt = None
        runs the back end alone on them, scans AND correspondences run the scans' front end and the back end on the given
        correspondences.  Returns one result dict per pair, in order — the same dicts register_pair returns."""
        return self._batch_host(pairs, fp, params, None, want_lists)

    def register_batch_refine(self, pairs, fp: FrontendParams | None = None, params: Params | None = None,
                              icp: IcpParams | None = None, want_lists=True):
        """register_batch, and every registered pair refined by ICP on its voxelised clouds (qtr_submit_batch_refine).
        Returns (results, refined): register_batch's result dicts and one ICP dict per pair — refine_pair's dict; a pair
        that was not refined (no scans, failed registration) has status QTR_ERR_NOT_RUN and the registration's T."""
        return self._batch_host(pairs, fp, params, icp or default_icp_params(), want_lists)

    def _batch_host(self, pairs, fp, params, icp, want_lists):
        fp = fp or default_frontend_params()
        prm = params or demo_params()
        B = len(pairs)
        descs = (PairDesc * max(B, 1))()
        results = (Result * max(B, 1))()
        keep = []
        cap = int(self.limits.max_corr)
        for i, item in enumerate(pairs):
            s_, t_, seed = item[0], item[1], item[2]
            cs_, ct_ = (item[3], item[4]) if len(item) > 3 else (None, None)
            s_, t_ = (None if s_ is None else _f4(s_)), (None if t_ is None else _f4(t_))
            cs_, ct_ = (None if cs_ is None else _f4(cs_)), (None if ct_ is None else _f4(ct_))
            n_c = 0 if cs_ is None else cs_.shape[0]
            if cs_ is not None and n_c == 0:  # (an empty array may have no address: "zero correspondences" needs pointers)
                cs_, ct_ = np.zeros((1, 4), np.float32), np.zeros((1, 4), np.float32)
            cl = np.zeros(cap if want_lists else 1, dtype=np.int32)
            fin = np.zeros(cap if want_lists else 1, dtype=np.int32)
            keep.append((s_, t_, cl, fin, cs_, ct_))
            descs[i] = PairDesc(None if s_ is None else s_.ctypes.data, 0 if s_ is None else s_.shape[0],
                                None if t_ is None else t_.ctypes.data, 0 if t_ is None else t_.shape[0], int(seed),
                                cl.ctypes.data if want_lists else None, fin.ctypes.data if want_lists else None, cap,
                                None if cs_ is None else cs_.ctypes.data, None if ct_ is None else ct_.ctypes.data, n_c)
        if icp is None:
            self._check(self._lib.qtr_submit_batch(self._h, descs, B, C.byref(fp), C.byref(prm), results, MEM_HOST))
        else:
            refined = (IcpResult * max(B, 1))()
            self._check(self._lib.qtr_submit_batch_refine(self._h, descs, B, C.byref(fp), C.byref(prm), C.byref(icp),
                                                          results, refined, MEM_HOST))
        self._check(self._lib.qtr_wait(self._h))
        out = []
        for i in range(B):
            cl, fin = keep[i][2], keep[i][3]
            r = results[i]
            if want_lists and r.status in (QTR_OK, QTR_ERR_CLIQUE_TOO_SMALL):
                out.append(_result_dict(r, cl, None, fin))
            else:
                out.append({"status": r.status, "valid": bool(r.valid), "T": np.array(r.T[:]).reshape(4, 4),
                            "cost": r.cost, "n_src": r.n_src, "n_tgt": r.n_tgt, "L": r.n_corr,
                            "n_clique": r.n_clique, "n_final": r.n_final, "n_rot_inliers": r.n_rot_inliers})
        if icp is None:
            return out
        return out, [_icp_dict(refined[i]) for i in range(B)]

    # ---- keyframes: a scan's front end once, registrations against it many times
    def keyframe(self, raw4, fp: FrontendParams | None = None, slot: int = 0, times=None, knot_times=None, knot_poses=None,
                 t_ref: float = 0.0) -> Keyframe:
        """qtr_keyframe_create on a host scan ([P, 4] float32) or a contiguous torch device tensor.

        times, knot_times and knot_poses given (all three): the scan is a raw sweep that is deskewed on the device first
        (qtr_keyframe_create_deskewed: per-point times [P] float32 where the scan lives, knots as for Handle.deskew); the
        counts of that pass are left in the keyframe's `deskew` attribute."""
        fp = fp or default_frontend_params()
        if isinstance(raw4, np.ndarray):
            raw4 = _f4(raw4)
        ptr, mem = _ptr(raw4)
        kf = C.c_void_p()
        if times is not None or knot_times is not None or knot_poses is not None:
            if times is None or knot_times is None or knot_poses is None:
                raise ValueError("a deskewed keyframe needs times, knot_times and knot_poses")
            times, pt, kt, kp = self._deskew_args(raw4, times, mem, knot_times, knot_poses)
            info = DeskewInfo()
            self._check(load_ext().qtr_keyframe_create_deskewed(
                self._h, slot, ptr, pt, int(raw4.shape[0]), kt.ctypes.data, kp.ctypes.data, int(kt.shape[0]), float(t_ref),
                C.byref(fp), mem, C.byref(kf), C.byref(info)))
            out = Keyframe(self, kf.value)
            out.deskew = {n: getattr(info, n) for n, _ in DeskewInfo._fields_}
            return out
        self._check(self._lib.qtr_keyframe_create(self._h, slot, ptr, int(raw4.shape[0]), C.byref(fp), mem, C.byref(kf)))
        return Keyframe(self, kf.value)

    def _deskew_args(self, cloud, times, mem, knot_times, knot_poses):
        """(times, their pointer, knot times, knot poses) for a cloud that lives in `mem`: the caller holds the returned
        arrays while the pointers are in use."""
        if isinstance(times, np.ndarray) or not hasattr(times, "data_ptr"):
            times = np.ascontiguousarray(times, dtype=np.float32).reshape(-1)
        else:
            import torch
            assert times.dtype == torch.float32
        pt, mt = _ptr(times)
        if mt != mem:
            raise ValueError("cloud and times must both be host arrays or both be device tensors")
        if int(times.shape[0]) != int(cloud.shape[0]) or len(times.shape) != 1:
            raise ValueError(f"{int(cloud.shape[0])} points, times of shape {tuple(times.shape)}")
        kt, kp = _knots(knot_times, knot_poses)
        return times, pt, kt, kp

    def deskew(self, cloud, times, knot_times, knot_poses, t_ref: float = 0.0, slot: int = 0, out=None):
        """qtr_deskew: the sweep `cloud` ([P, 4] float32, host array or contiguous torch device tensor) with the time of
        every point (`times`, [P] float32, where the cloud lives) carried into the sensor frame at t_ref, given K knots:
        knot_times [K] (finite, strictly increasing) and knot_poses [K, 4, 4] (sensor frame at that time -> a fixed frame),
        host arrays.  Returns (deskewed cloud, info): a new numpy array for a host cloud; for a device tensor a new tensor,
        or `out` (which may be the cloud itself: in place).  info: n_points, n_skipped (points with a non-finite
        coordinate or time, copied unchanged), n_extrapolated (times outside the knots)."""
        if isinstance(cloud, np.ndarray) or not hasattr(cloud, "data_ptr"):
            cloud = _f4(cloud)
            assert out is None, "out= is for device tensors"
            out = np.empty_like(cloud)
        elif out is None:
            import torch
            out = torch.empty_like(cloud)
        (pc, mem), (po, mo) = _ptr(cloud), _ptr(out)
        assert mem == mo and tuple(out.shape) == tuple(cloud.shape)
        times, pt, kt, kp = self._deskew_args(cloud, times, mem, knot_times, knot_poses)
        info = DeskewInfo()
        self._check(load_ext().qtr_deskew(self._h, slot, pc, pt, int(cloud.shape[0]), kt.ctypes.data, kp.ctypes.data,
                                             int(kt.shape[0]), float(t_ref), po, mem, C.byref(info)))
        return out, {n: getattr(info, n) for n, _ in DeskewInfo._fields_}

    def merge_keyframes(self, kfs, poses=None, fp: FrontendParams | None = None, slot: int = 0) -> Keyframe:
        """qtr_keyframe_merge: the keyframes' stored voxels, member k moved by poses[k] ([K, 4, 4] float64; None: identities),
        concatenated on the device and run through the one-cloud front end with fp — the submap as an ordinary Keyframe."""
        fp = fp or default_frontend_params()
        K = len(kfs)
        members = (C.c_void_p * max(K, 1))(*[k._kf.value for k in kfs])
        p16 = None
        if poses is not None:
            p16 = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(K, 16))
        kf = C.c_void_p()
        self._check(self._lib.qtr_keyframe_merge(self._h, slot, members, None if p16 is None else p16.ctypes.data, K,
                                                 C.byref(fp), C.byref(kf)))
        return Keyframe(self, kf.value)

    def register_keyframes(self, kf_src: Keyframe, kf_tgt: Keyframe, fp: FrontendParams | None = None,
                           params: Params | None = None, slot: int = 0):
        """qtr_register_keyframes: register_pair's dict for two keyframes (fp's radii must be the keyframes')."""
        fp = fp or default_frontend_params()
        prm = params or demo_params()
        res = Result()
        cap = int(self.limits.max_corr)
        cl = np.zeros(cap, dtype=np.int32)
        fin = np.zeros(cap, dtype=np.int32)
        rc = self._lib.qtr_register_keyframes(self._h, slot, kf_src._kf, kf_tgt._kf, C.byref(fp), C.byref(prm),
                                              C.byref(res), cl.ctypes.data, fin.ctypes.data, cap)
        self._check(rc, ok=(QTR_OK, QTR_ERR_CLIQUE_TOO_SMALL))
        return _result_dict(res, cl, None, fin)

    def register_batch_keyframes(self, pairs, fp: FrontendParams | None = None, params: Params | None = None,
                                 icp: IcpParams | None = None, want_lists=True):
        """pairs: sequence of (Keyframe src, Keyframe tgt, seed) through qtr_submit_batch_keyframes / qtr_wait.  Returns what
        register_batch returns, or with icp what register_batch_refine returns: (results, refined)."""
        fp = fp or default_frontend_params()
        prm = params or demo_params()
        B = len(pairs)
        descs = (KfPairDesc * max(B, 1))()
        results = (Result * max(B, 1))()
        refined = None if icp is None else (IcpResult * max(B, 1))()
        cap = int(self.limits.max_corr)
        keep = []
        for i, (ks, kt, seed) in enumerate(pairs):
            cl = np.zeros(cap if want_lists else 1, dtype=np.int32)
            fin = np.zeros(cap if want_lists else 1, dtype=np.int32)
            keep.append((cl, fin))
            descs[i] = KfPairDesc(ks._kf, kt._kf, int(seed), cl.ctypes.data if want_lists else None,
                                  fin.ctypes.data if want_lists else None, cap)
        self._check(self._lib.qtr_submit_batch_keyframes(self._h, descs, B, C.byref(fp), C.byref(prm),
                                                         None if icp is None else C.byref(icp), results, refined))
        self._check(self._lib.qtr_wait(self._h))
        out = []
        for i in range(B):
            r = results[i]
            if want_lists and r.status in (QTR_OK, QTR_ERR_CLIQUE_TOO_SMALL):
                out.append(_result_dict(r, keep[i][0], None, keep[i][1]))
            else:
                out.append({"status": r.status, "valid": bool(r.valid), "T": np.array(r.T[:]).reshape(4, 4),
                            "cost": r.cost, "n_src": r.n_src, "n_tgt": r.n_tgt, "L": r.n_corr,
                            "n_clique": r.n_clique, "n_final": r.n_final, "n_rot_inliers": r.n_rot_inliers})
        if icp is None:
            return out
        return out, [_icp_dict(refined[i]) for i in range(B)]

    # ---- place index: which keyframes to register against
    def place_index(self, capacity: int, params: PlaceParams | None = None) -> PlaceIndex:
        """qtr_place_index_create: room for `capacity` Scan Context descriptors on the device."""
        ix = C.c_void_p()
        self._check(self._lib.qtr_place_index_create(self._h, None if params is None else C.byref(params), int(capacity),
                                                     C.byref(ix)))
        return PlaceIndex(self, ix.value)

    def voxel_map(self, voxel_size: float = 1.0, capacity: int = 1 << 20) -> VoxelMap:
        """A new, empty Gaussian voxel map of this handle (qtr_voxel_map_create): world-anchored voxels of side voxel_size,
        room for `capacity` of them."""
        if self._lib is not load():  # (another build of the library has other structures behind the handle)
            raise QuatroHipError(QTR_ERR_BAD_ARG, "voxel maps belong to handles of the product library libquatro_hip.so")
        vlib = load_ext()
        prm, out = VoxelMapParams(), C.c_void_p()
        vlib.qtr_default_voxel_map_params(C.byref(prm))
        prm.voxel_size, prm.capacity = float(voxel_size), int(capacity)
        self._check(vlib.qtr_voxel_map_create(self._h, C.byref(prm), C.byref(out)))
        return VoxelMap(self, out.value)

    def load_voxel_map(self, path, capacity: int | None = None) -> VoxelMap:
        """A new voxel map of this handle with the voxels of a file written by VoxelMap.save (qtr_voxel_map_restore);
        capacity None: the saved map's."""
        with np.load(path) as f:
            side, cap = float(f["voxel_size"]), int(f["capacity"])
            coords, count, sums = f["coords"], f["count"], f["sums"]
        vm = self.voxel_map(side, cap if capacity is None else int(capacity))
        try:
            vm.restore(coords, count, sums)
        except Exception:
            vm.destroy()
            raise
        return vm

    def place_describe(self, xyz4, params: PlaceParams | None = None, slot: int = 0):
        """qtr_place_describe: the [num_rings, num_sectors] descriptor of a host cloud ([n, 4] float32 -> numpy) or of a
        contiguous torch device tensor (-> a torch tensor on the same device)."""
        p = params or default_place_params()
        if isinstance(xyz4, np.ndarray):
            xyz4 = _f4(xyz4)
            out = np.zeros((p.num_rings, p.num_sectors), dtype=np.float32)
        else:
            import torch
            out = torch.zeros((p.num_rings, p.num_sectors), dtype=torch.float32, device=xyz4.device)
        ptr, mem = _ptr(xyz4)
        optr, _ = _ptr(out)
        self._check(self._lib.qtr_place_describe(self._h, slot, C.byref(p), ptr if xyz4.shape[0] else None, int(xyz4.shape[0]),
                                                 optr, mem))
        return out

    def set_batch_preprocess(self, pw: "PwParams | None" = None, ip: "IpParams | None" = None, on: bool = True):
        """Raw sweeps through register_batch: Patchwork ground removal + range-image segmentation in front of the voxel
        grid (qtr_set_batch_preprocess); on=False switches it off again."""
        if not on:
            self._check(self._lib.qtr_set_batch_preprocess(self._h, None, None))
            return
        self._pre = (pw or pw_params(), ip or ip_params())
        self._check(self._lib.qtr_set_batch_preprocess(self._h, C.byref(self._pre[0]), C.byref(self._pre[1])))

    def register_batch_dev(self, items, prm: Params, fp: FrontendParams | None = None, scans: bool = True,
                           corr: bool = False):
        """items: dicts with device tensors "src" / "tgt" and a FrontendParams "fp" (its seed is the pair's seed), and —
        with corr=True — the pre-matched correspondences "cs" / "ct" the back end runs on (scans=False: the back end
        alone).  Inputs stay in HBM; only the result records come back.  Returns a list of dicts (status, valid, T,
        sizes)."""
        return self._batch_dev(items, prm, fp, scans, corr, None)

    def register_batch_dev_refine(self, items, prm: Params, icp: IcpParams | None = None, fp: FrontendParams | None = None,
                                  scans: bool = True, corr: bool = False):
        """register_batch_dev with the refinement of qtr_submit_batch_refine: returns (results, refined), the result dicts
        of register_batch_dev and one ICP dict per pair (refine_pair's)."""
        return self._batch_dev(items, prm, fp, scans, corr, icp or default_icp_params())

    def _batch_dev(self, items, prm, fp, scans, corr, icp):
        fp = fp or default_frontend_params()
        B = len(items)
        descs = (PairDesc * max(B, 1))()
        results = (Result * max(B, 1))()
        for i, it in enumerate(items):
            descs[i] = PairDesc(it["src"].data_ptr() if scans else None, it["src"].shape[0] if scans else 0,
                                it["tgt"].data_ptr() if scans else None, it["tgt"].shape[0] if scans else 0,
                                int(it["fp"].seed), None, None, 0,
                                it["cs"].data_ptr() if corr else None, it["ct"].data_ptr() if corr else None,
                                it["cs"].shape[0] if corr else 0)
        if icp is None:
            self._check(self._lib.qtr_submit_batch(self._h, descs, B, C.byref(fp), C.byref(prm), results, MEM_DEVICE))
        else:
            refined = (IcpResult * max(B, 1))()
            self._check(self._lib.qtr_submit_batch_refine(self._h, descs, B, C.byref(fp), C.byref(prm), C.byref(icp),
                                                          results, refined, MEM_DEVICE))
        self._check(self._lib.qtr_wait(self._h))
        out = [{"status": r.status, "valid": bool(r.valid), "T": np.array(r.T[:]).reshape(4, 4), "cost": r.cost,
                "n_src": r.n_src, "n_tgt": r.n_tgt, "L": r.n_corr, "n_clique": r.n_clique, "n_final": r.n_final,
                "n_rot_inliers": r.n_rot_inliers, "gnc_iters": r.gnc_iters}
               for r in results[:B]]
        if icp is None:
            return out
        return out, [_icp_dict(refined[i]) for i in range(B)]

    # ---- multi-GPU: RCCL all-gather of the result records through the C ABI (one handle = one rank)
    def comm_init(self, unique_id: bytes, rank: int, world: int):
        self._check(self._lib.qtr_comm_init(self._h, unique_id, rank, world))

    def gather_results(self, results, world: int):
        """results: ctypes array (Result * n_local).  Returns a (Result * (world * n_local)) array, rank order."""
        n = len(results)
        out = (Result * max(world * n, 1))()
        self._check(self._lib.qtr_gather_results(self._h, results, n, out))
        return out

    def gather_results_v(self, results, n_local: int, world: int, cap_all: int):
        """Blocks of different lengths (qtr_gather_results_v).  results: ctypes array holding at least n_local records
        (None for n_local = 0).  Returns (array of the gathered records in rank order, per-rank counts)."""
        out = (Result * max(cap_all, 1))()
        counts = (C.c_int * max(world, 1))()
        n_all = C.c_int()
        self._check(self._lib.qtr_gather_results_v(self._h, results, n_local, out, cap_all, counts, C.byref(n_all)))
        return out, [int(c) for c in counts[:world]], n_all.value

    def set_stage_events(self, on: bool) -> None:
        self._lib.qtr_set_stage_events(self._h, 1 if on else 0)

    def set_nn_event_stride(self, every: int) -> None:
        """every n-th match of a slot carries the nearest-neighbour event pairs (1: all, 0: none)"""
        self._check(self._lib.qtr_set_nn_event_stride(self._h, int(every)))

    def nn_totals(self, slot: int = 0, reset: bool = False):
        """(summed milliseconds, launches) of the nearest-neighbour kernel since the last reset"""
        ms, n = C.c_double(0), C.c_longlong(0)
        self._check(self._lib.qtr_get_nn_totals(self._h, slot, C.byref(ms), C.byref(n), 1 if reset else 0))
        return ms.value, n.value

    def stage_times(self, slot: int = 0) -> dict:
        t = StageTimes()
        self._lib.qtr_get_stage_times(self._h, slot, C.byref(t))
        out = {n: getattr(t, n) for n, _ in StageTimes._fields_}
        d1, d2 = C.c_float(), C.c_float()
        if hasattr(self._lib, "qtr_get_nn_dir_times"):  # (QTR_LIB may name an older build of the library: A/B runs)
            self._lib.qtr_get_nn_dir_times(self._h, slot, C.byref(d1), C.byref(d2))
        out["nn_dir1"], out["nn_dir2"] = d1.value, d2.value  # the two nearest-neighbour launches behind nn_kernel apart
        return out

    def icp(self, src4, tgt4, tgt_normals4=None, guess=None, params: IcpParams | None = None, slot: int = 0) -> dict:
        """6-DoF ICP of src4 onto tgt4 (qtr_icp).  numpy arrays (host) or contiguous [N,4] float32 torch device tensors
        (all on the device: mem = QTR_MEM_DEVICE).  tgt_normals4 None: the target normals are computed at
        params.normal_radius (point-to-plane; plane-to-plane, voxelised or not, computes the source's as well: gicp with src_normals4 = None).
        Returns the result record as a dict (T row-major 4x4)."""
        prm = params or default_icp_params()
        if isinstance(src4, np.ndarray) or isinstance(tgt4, np.ndarray):
            src4, tgt4 = _f4(src4), _f4(tgt4)
            tgt_normals4 = None if tgt_normals4 is None else _f4(tgt_normals4)
            ps, pt, pn, mem = src4.ctypes.data, tgt4.ctypes.data, (None if tgt_normals4 is None else
                                                                   tgt_normals4.ctypes.data), MEM_HOST
        else:
            (ps, m1), (pt, m2) = _ptr(src4), _ptr(tgt4)
            pn, m3 = _ptr(tgt_normals4)
            assert m1 == m2 == MEM_DEVICE and m3 in (None, MEM_DEVICE), "torch tensors must all be on the device"
            assert src4.dtype == tgt4.dtype and src4.shape[-1] == 4 and tgt4.shape[-1] == 4
            mem = MEM_DEVICE
        g = _guess16(guess)
        res = IcpResult()
        rc = self._lib.qtr_icp(self._h, slot, ps, int(src4.shape[0]), pt, int(tgt4.shape[0]), pn,
                               None if g is None else g.ctypes.data, C.byref(prm), C.byref(res), mem)
        self._check(rc)
        return _icp_dict(res)

    def gicp(self, src4, tgt4, src_normals4=None, tgt_normals4=None, guess=None, params: IcpParams | None = None,
             slot: int = 0) -> dict:
        """Plane-to-plane (Generalized) ICP of src4 onto tgt4 with both normal sets (qtr_gicp); a normal set given as None
        is computed at params.normal_radius.  Arrays as for icp (numpy on the host, or torch tensors all on the device);
        params None = the defaults with method = ICP_PLANE_TO_PLANE; method = ICP_VOXEL_PLANE_TO_PLANE is its voxelised form
        (VGICP: one Gaussian per target voxel of side max_correspondence_distance, a lookup in place of the search)."""
        prm = params or default_icp_params(method=ICP_PLANE_TO_PLANE)
        if isinstance(src4, np.ndarray) or isinstance(tgt4, np.ndarray):
            src4, tgt4 = _f4(src4), _f4(tgt4)
            src_normals4 = None if src_normals4 is None else _f4(src_normals4)
            tgt_normals4 = None if tgt_normals4 is None else _f4(tgt_normals4)
            ps, pt, mem = src4.ctypes.data, tgt4.ctypes.data, MEM_HOST
            pa = None if src_normals4 is None else src_normals4.ctypes.data
            pn = None if tgt_normals4 is None else tgt_normals4.ctypes.data
        else:
            (ps, m1), (pt, m2) = _ptr(src4), _ptr(tgt4)
            (pa, m3), (pn, m4) = _ptr(src_normals4), _ptr(tgt_normals4)
            assert m1 == m2 == MEM_DEVICE and m3 in (None, MEM_DEVICE) and m4 in (None, MEM_DEVICE), \
                "torch tensors must all be on the device"
            assert src4.dtype == tgt4.dtype and src4.shape[-1] == 4 and tgt4.shape[-1] == 4
            mem = MEM_DEVICE
        g = _guess16(guess)
        res = IcpResult()
        rc = self._lib.qtr_gicp(self._h, slot, ps, int(src4.shape[0]), pa, pt, int(tgt4.shape[0]), pn,
                                None if g is None else g.ctypes.data, C.byref(prm), C.byref(res), mem)
        self._check(rc)
        return _icp_dict(res)

    def refine_pair(self, guess=None, params: IcpParams | None = None, slot: int = 0) -> dict:
        """Refines the slot's last register_pair / register_pair_corr on its voxelised clouds (qtr_refine_pair); guess
        None = that registration's T."""
        prm = params or default_icp_params()
        g = _guess16(guess)
        res = IcpResult()
        rc = self._lib.qtr_refine_pair(self._h, slot, None if g is None else g.ctypes.data, C.byref(prm), C.byref(res))
        self._check(rc)
        return _icp_dict(res)

    def evaluate(self, src4, tgt4, T, tgt_normals4=None, params: EvalParams | None = None, slot: int = 0) -> dict:
        """Evaluates T (maps src4 into tgt4) on two clouds (qtr_evaluate): overlap, inlier RMSE, the 6x6 information matrix
        and, with tgt_normals4, the point-to-plane Hessian.  Arrays as for icp (numpy on the host, or torch tensors all on
        the device).  Returns the record as a dict, the matrices as 6x6 float64."""
        prm = params or default_eval_params()
        if isinstance(src4, np.ndarray) or isinstance(tgt4, np.ndarray):
            src4, tgt4 = _f4(src4), _f4(tgt4)
            tgt_normals4 = None if tgt_normals4 is None else _f4(tgt_normals4)
            ps, pt, pn, mem = src4.ctypes.data, tgt4.ctypes.data, (None if tgt_normals4 is None else
                                                                   tgt_normals4.ctypes.data), MEM_HOST
        else:
            (ps, m1), (pt, m2) = _ptr(src4), _ptr(tgt4)
            pn, m3 = _ptr(tgt_normals4)
            assert m1 == m2 == MEM_DEVICE and m3 in (None, MEM_DEVICE), "torch tensors must all be on the device"
            assert src4.dtype == tgt4.dtype and src4.shape[-1] == 4 and tgt4.shape[-1] == 4
            mem = MEM_DEVICE
        g = _guess16(T)
        res = EvalResult()
        rc = self._lib.qtr_evaluate(self._h, slot, ps, int(src4.shape[0]), pt, int(tgt4.shape[0]), pn,
                                    None if g is None else g.ctypes.data, C.byref(prm), C.byref(res), mem)
        self._check(rc)
        return _eval_dict(res)

    def evaluate_pair(self, T=None, params: EvalParams | None = None, slot: int = 0) -> dict:
        """Evaluates the slot's last registration on its voxelised clouds (qtr_evaluate_pair); T None = its own T."""
        prm = params or default_eval_params()
        g = _guess16(T)
        res = EvalResult()
        rc = self._lib.qtr_evaluate_pair(self._h, slot, None if g is None else g.ctypes.data, C.byref(prm), C.byref(res))
        self._check(rc)
        return _eval_dict(res)

    def evaluate_keyframes(self, kf_src: Keyframe, kf_tgt: Keyframe, T, params: EvalParams | None = None,
                           slot: int = 0) -> dict:
        """Evaluates T between two keyframes, read where they lie (qtr_evaluate_keyframes)."""
        prm = params or default_eval_params()
        g = _guess16(T)
        res = EvalResult()
        rc = self._lib.qtr_evaluate_keyframes(self._h, slot, None if kf_src is None else kf_src._kf,
                                              None if kf_tgt is None else kf_tgt._kf,
                                              None if g is None else g.ctypes.data, C.byref(prm), C.byref(res))
        self._check(rc)
        return _eval_dict(res)

    def evaluate_keyframes_batch(self, pairs, params: EvalParams | None = None, slot: int = 0) -> list:
        """pairs: (source Keyframe, target Keyframe, T) triples, 1 .. EVAL_MAX_PAIRS of them, evaluated in one grouped
        launch chain (qtr_evaluate_keyframes_batch).  Returns one record dict per pair."""
        prm = params or default_eval_params()
        B = len(pairs)
        arr = (EvalKfPair * max(B, 1))()
        for i, (a, b, T) in enumerate(pairs[:len(arr)]):
            arr[i].source = None if a is None else a._kf.value
            arr[i].target = None if b is None else b._kf.value
            arr[i].T[:] = list(np.asarray(T, dtype=np.float64).reshape(16))
        res = (EvalResult * max(B, 1))()
        self._check(self._lib.qtr_evaluate_keyframes_batch(self._h, slot, arr, B, C.byref(prm), res))
        return [_eval_dict(res[i]) for i in range(B)]

    def optimize_pose_graph(self, poses, edges, fixed=None, params: PgoParams | None = None, slot: int = 0):
        """Robust pose-graph optimisation on the device (qtr_pgo_optimize).  poses: N x 4 x 4 (keyframe frame -> map frame);
        edges: (s, t, Z, information, uncertain) tuples, Z mapping keyframe s's frame into keyframe t's; fixed: N flags
        (None: node 0).  Returns (poses_out [N, 4, 4], weights [E], result dict)."""
        prm = params or default_pgo_params()
        X, fx, src, dst, Z, info, unc = pgo_arrays(poses, edges, fixed)
        if fx is not None and fx.shape[0] != X.shape[0]:
            raise ValueError("fixed must have one flag per node")
        out, w, res = np.zeros_like(X), np.zeros(len(edges)), PgoResult()
        rc = self._lib.qtr_pgo_optimize(self._h, slot, int(X.shape[0]), X.ctypes.data, None if fx is None else fx.ctypes.data,
                                        len(edges), src.ctypes.data, dst.ctypes.data, Z.ctypes.data, info.ctypes.data,
                                        unc.ctypes.data, C.byref(prm), out.ctypes.data, w.ctypes.data, C.byref(res))
        self._check(rc)
        return out.reshape(-1, 4, 4), w, _pgo_dict(res)

    def debug_fetch(self, what: int, dtype, slot: int = 0) -> np.ndarray:
        nbytes = self._lib.qtr_debug_fetch(self._h, slot, what, None, 0)
        if nbytes < 0:
            raise QuatroHipError(-1, "qtr_debug_fetch failed")
        out = np.zeros(max(nbytes // np.dtype(dtype).itemsize, 0), dtype=dtype)
        if nbytes:
            self._lib.qtr_debug_fetch(self._h, slot, what, out.ctypes.data, nbytes)
        return out

    def debug_math(self, fn: int, a, b=None) -> np.ndarray:
        a = np.ascontiguousarray(a, dtype=np.float32)
        b = np.ascontiguousarray(b if b is not None else a, dtype=np.float32)
        out = np.zeros_like(a)
        self._check(self._lib.qtr_debug_math(self._h, fn, a.ctypes.data, b.ctypes.data, out.ctypes.data, a.size))
        return out


def _result_dict(res: Result, cl, rot, fin) -> dict:
    return {
        "status": res.status, "valid": bool(res.valid), "T": np.array(res.T[:]).reshape(4, 4), "cost": res.cost,
        "gnc_iters": res.gnc_iters, "clique": cl[: res.n_clique].copy(),
        "rot_inliers": None if rot is None else rot[: res.n_rot_inliers].copy(),
        "final_inliers": fin[: res.n_final].copy(), "max_core": res.max_core, "n_edges": res.n_edges,
        "n_card": list(res.n_card), "n_src": res.n_src, "n_tgt": res.n_tgt, "L": res.n_corr,
        "n_rot_inliers": res.n_rot_inliers,
    }
