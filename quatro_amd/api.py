"""Host-side mirror of the reference's interface for this path, in Python, above the C ABI.

Same names, argument meaning and error behaviour as the reference so that tests read like the
reference's demo (examples/run_global_registration.cpp:103-108, 206-221, 243-246):

    quatro = Quatro(); quatro.reset(params)
    src_feat, tgt_feat = voxelize(src, 0.3), voxelize(tgt, 0.3)
    fm = FPFHManager(normal_radius, fpfh_radius); fm.flushAllFeatures(); fm.setFeaturePair(src_feat, tgt_feat)
    quatro.setInputSource(fm.getSrcKps()); quatro.setInputTarget(fm.getTgtKps())
    T = quatro.computeTransformation()

Clouds are numpy [N,4] float32 (x,y,z,pad) — the layout of pcl::PointXYZ.  Everything numerical happens
in libquatro_hip.so; this module holds state and argument checks only.
"""
from __future__ import annotations

import enum
import math
from dataclasses import dataclass, field

import numpy as np

from . import lib as _ql


class INLIER_SELECTION_MODE(enum.IntEnum):  # reference include/quatro.hpp:184-189
    PMC_EXACT = 0
    PMC_HEU = 1
    KCORE_HEU = 2
    NONE = 3


class ROTATION_ESTIMATION_ALGORITHM(enum.IntEnum):  # :172-175
    GNC_TLS = 0
    FGR = 1


class INLIER_GRAPH_FORMULATION(enum.IntEnum):  # :197-200
    CHAIN = 0
    COMPLETE = 1


@dataclass
class Params:
    """Quatro::Params (reference include/quatro.hpp:202-268), same field names and defaults."""
    reg_name: str = "Quatro"
    cote_mode: str = "median"
    using_rot_inliers_when_estimating_cote: bool = False
    noise_bound: float = 0.3
    cbar2: float = 1.0
    estimate_scaling: bool = True            # accepted, ignored (reference :361 forces scale = 1)
    rotation_estimation_algorithm: ROTATION_ESTIMATION_ALGORITHM = ROTATION_ESTIMATION_ALGORITHM.GNC_TLS
    rotation_gnc_factor: float = 1.4
    rotation_max_iterations: int = 100
    rotation_cost_threshold: float = 1e-6
    rotation_tim_graph: INLIER_GRAPH_FORMULATION = INLIER_GRAPH_FORMULATION.CHAIN
    inlier_selection_mode: INLIER_SELECTION_MODE = INLIER_SELECTION_MODE.PMC_HEU
    kcore_heuristic_threshold: float = 0.5
    use_max_clique: bool = True              # deprecated in the reference, unused
    max_clique_exact_solution: bool = True   # deprecated in the reference, unused
    max_clique_time_limit: float = 3600.0


@dataclass
class RegistrationSolution:  # reference include/quatro.hpp:161-168
    valid: bool = True
    scale: float = 1.0
    translation: np.ndarray = field(default_factory=lambda: np.zeros(3))
    rotation: np.ndarray = field(default_factory=lambda: np.eye(3))


_shared_handle = None


def _handle() -> "_ql.Handle":
    global _shared_handle
    if _shared_handle is None:
        _shared_handle = _ql.Handle(0)
    return _shared_handle


def _as_cloud(c) -> np.ndarray:
    a = np.asarray(c, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] not in (3, 4):
        raise ValueError("cloud must be [N,3] or [N,4]")
    if a.shape[1] == 3:
        a = np.concatenate([a, np.zeros((a.shape[0], 1), dtype=np.float32)], axis=1)
    return np.ascontiguousarray(a)


def voxelize(src, voxelSize: float, handle=None) -> np.ndarray:
    """voxelize<T>() (reference include/quatro.hpp:49-68): pcl::VoxelGrid centroid down-sampling."""
    return (handle or _handle()).voxelize(_as_cloud(src), float(voxelSize))


class PatchWork:
    """Reference include/patchwork.hpp:36-233 (ground segmentation on the concentric zone model).  The constructor
    takes the "/patchwork/..." parameters as keyword arguments (names of config/patchwork_params.yaml, e.g.
    sensor_height=1.723, czm={"num_zones": 4, ...}) instead of a ros::NodeHandle; unspecified ones keep the yaml values."""

    _SCALARS = {"sensor_height": "sensor_height", "num_iter": "num_iter", "num_lpr": "num_lpr",
                "num_min_pts": "num_min_pts", "th_seeds": "th_seeds", "th_dist": "th_dist", "max_r": "max_range",
                "min_r": "min_range", "uprightness_thr": "uprightness_thr",
                "adaptive_seed_selection_margin": "adaptive_seed_selection_margin",
                "using_global_elevation": "using_global_thr", "global_elevation_threshold": "global_elevation_thr"}

    def __init__(self, handle=None, czm: dict | None = None, **kw):
        p = _ql.pw_params()
        for k, v in kw.items():
            if k not in self._SCALARS:
                raise TypeError(f"unknown Patchwork parameter {k!r}")
            setattr(p, self._SCALARS[k], type(getattr(p, self._SCALARS[k]))(v))
        if czm:
            nz = int(czm.get("num_zones", p.num_zones))
            for key, field in (("num_sectors_each_zone", "num_sectors_each_zone"),
                               ("num_rings_each_zone", "num_rings_each_zone"),
                               ("min_ranges_each_zone", "min_ranges")):
                if key in czm:
                    if len(czm[key]) != nz:  # patchwork.hpp:598-604
                        raise ValueError("Some parameters are wrong! the size of parameters should be same")
                    arr = getattr(p, field)
                    for i in range(4):
                        arr[i] = czm[key][i] if i < nz else 0
            p.num_zones = nz
            if "elevation_thresholds" in czm or "flatness_thresholds" in czm:
                e, f = czm.get("elevation_thresholds", []), czm.get("flatness_thresholds", [])
                if len(e) != len(f) or len(e) > 8:  # :610
                    raise ValueError("Some parameters are wrong! Check the elevation/flatness_thresholds")
                p.num_thr = len(e)
                for i in range(len(e)):
                    p.elevation_thr[i], p.flatness_thr[i] = e[i], f[i]
        if p.min_range != p.min_ranges[0]:  # :606
            raise ValueError("Setting min. ranges are weired! The first term should be eqaul to min_range_")
        self.params = p
        self._h = handle

    def estimate_ground(self, cloudIn):
        """-> (cloudOut (ground), cloudNonground, time_taken [s]); (n, 4) float32 records in the reference's order."""
        import time
        t0 = time.perf_counter()
        r = (self._h or _handle()).patchwork(_as_cloud(cloudIn), self.params)
        return r["ground"], r["nonground"], time.perf_counter() - t0


class ImageProjection:
    """Reference include/imageProjection.hpp:31-581 (range-image projection + sub-cluster rejection, "Patchwork"
    ground mode): segmentCloud then getValidSegments / getOutliers."""

    def __init__(self, lidarType: str = "Velodyne-64-HDE", neighborSelectionMode: str = "4CrossNeighbor",
                 groundSegmentationMode: str = "Patchwork", numSubclusteringCriteria: int = 30, handle=None):
        try:
            self.params = _ql.ip_params(lidarType, neighborSelectionMode, numSubclusteringCriteria)
        except ValueError:
            try:
                _ql.ip_params(lidarType, "4Neighbor")
            except ValueError:
                raise ValueError("[ImageProjection]:Check your paramter. Lidar Type is wrong!") from None
            raise ValueError("[ImageProjection]:Check your paramter. Neighbor selection mode is wrong!") from None
        if groundSegmentationMode not in ("LeGO-LOAM", "Patchwork"):
            raise ValueError("[ImageProjection]: Check your paramter. Ground Segmentation mode is wrong!")
        if groundSegmentationMode == "LeGO-LOAM":
            raise ValueError("[ImageProjection]: the LeGO-LOAM ground removal is not part of the device path")
        self._h = handle
        self._r = None

    def segmentCloud(self, cloud):
        self._r = (self._h or _handle()).segment_cloud(_as_cloud(cloud), self.params)

    def getValidSegments(self) -> np.ndarray:
        """(n, 4) float32: x, y, z, segment label (pcl::PointXYZI view; drop the last column for PointXYZ)."""
        return self._r["valid"]

    def getOutliers(self) -> np.ndarray:
        return self._r["outliers"]

    def getGround(self) -> np.ndarray:
        return np.zeros((0, 4), dtype=np.float32)

    def getLabelMat(self) -> np.ndarray:
        return self._r["labels"]


class FPFHManager:
    """Reference include/fpfh_manager.hpp:25-238 (front-end orchestrator)."""

    def __init__(self, normal_radius: float = 0.5, fpfh_radius: float = 0.6, interval: int = 1, handle=None,
                 seed: int = 0):
        self.normal_radius_ = float(normal_radius)
        self.fpfh_radius_ = float(fpfh_radius)
        self.interval_ = interval
        self.is_initial_ = True
        self.is_odometry_test_ = False
        self.corr = np.zeros((0, 2), dtype=np.int32)
        self.src_cloud = self.tgt_cloud = None
        self._obj = self._scene = None
        self._src_normals = self._tgt_normals = None
        self.src_matched = self.tgt_matched = None
        self.tgt_normals = None
        self._h = handle
        self.seed = seed  # tuple-test RNG seed (the reference seeds from the clock)

    def flushAllFeatures(self):
        self.is_initial_ = True

    # matched-pair PCD cache (reference :91-96, 179-232): "%06d_to_%06d.pcd", source half then target half
    def setLoadDir(self, loaddir):
        self.loaddir_ = str(loaddir)

    def setSaveDir(self, savedir):
        self.savedir_ = str(savedir)

    def saveFeaturePair(self, src_idx: int, tgt_idx: int, verbose: bool = False):
        if not getattr(self, "savedir_", ""):
            raise ValueError("Save dir. is not set")
        name = "%s/%06d_to_%06d.pcd" % (self.savedir_, src_idx, tgt_idx)
        merge = np.concatenate([self.getSrcKps(), self.getTgtKps()])
        if verbose:
            print(f"[SAVER]: {name}")
        _ql.write_pcd_xyz(name, merge)

    def loadFeaturePair(self, src_idx: int, tgt_idx: int, verbose: bool = False):
        if not getattr(self, "loaddir_", ""):
            raise ValueError("Load dir. is not set")
        name = "%s/%06d_to_%06d.pcd" % (self.loaddir_, src_idx, tgt_idx)
        try:
            merge = _ql.read_pcd_xyz(name)
        except OSError:
            raise ValueError("[FPFHManager]: Load feature set failed.") from None
        half = merge.shape[0] // 2
        self._src_kps, self._tgt_kps = merge[:half].copy(), merge[half:].copy()
        self.src_matched = self._src_kps[:, :3].astype(np.float64).T.copy()
        self.tgt_matched = self._tgt_kps[:, :3].astype(np.float64).T.copy()
        if verbose:
            print(f"[LOADER]: Loaded data from {name}...=>{half} {merge.shape[0] - half}")


    def setParams(self, normal_radius, fpfh_radius, interval):
        self.normal_radius_, self.fpfh_radius_, self.interval_ = float(normal_radius), float(fpfh_radius), interval

    def clearInputs(self):
        self.is_initial_ = True
        self.src_cloud = self.tgt_cloud = self._obj = self._scene = None

    def swapTgt2Src(self):
        self.src_cloud, self._obj, self._src_normals = self.tgt_cloud, self._scene, self._tgt_normals

    def setFeaturePair(self, src, target):
        if self.normal_radius_ > self.fpfh_radius_:  # reference :99-102
            raise ValueError("[FPFHManager]: Normal should be lower than fpfh_radius!!!!")
        h = self._h or _handle()
        if self.is_initial_ and not self.is_odometry_test_:
            self.src_cloud = _as_cloud(src)
            self._src_normals, self._obj = h.fpfh(self.src_cloud, self.normal_radius_, self.fpfh_radius_)
            self.is_initial_ = False
        else:
            self.swapTgt2Src()
        self.tgt_cloud = _as_cloud(target)
        self._tgt_normals, self._scene = h.fpfh(self.tgt_cloud, self.normal_radius_, self.fpfh_radius_)
        fp = _ql.default_frontend_params(normal_radius=self.normal_radius_, fpfh_radius=self.fpfh_radius_,
                                         tuple_scale=0.95, use_crosscheck=1, use_tuple_test=1, seed=self.seed)
        self.corr = h.match(self.src_cloud, self._obj, self.tgt_cloud, self._scene, fp)
        self._src_kps = self._tgt_kps = None
        self.src_matched = self.src_cloud[self.corr[:, 0], :3].astype(np.float64).T.copy()  # 3 x L, as Eigen
        self.tgt_matched = self.tgt_cloud[self.corr[:, 1], :3].astype(np.float64).T.copy()
        self.tgt_normals = self._tgt_normals[self.corr[:, 1], :3].astype(np.float64).T.copy()

    def getSrcMatched(self):
        return self.src_matched

    def getTgtMatched(self):
        return self.tgt_matched

    def getTgtNormals(self):
        return self.tgt_normals

    def getObjDescriptor(self):
        return self._obj

    def getSceneDescriptor(self):
        return self._scene

    def getSrcKps(self) -> np.ndarray:
        if getattr(self, "_src_kps", None) is not None:  # loaded from the pair cache
            return self._src_kps
        return _as_cloud(self.src_cloud[self.corr[:, 0], :3])

    def getTgtKps(self) -> np.ndarray:
        if getattr(self, "_tgt_kps", None) is not None:
            return self._tgt_kps
        return _as_cloud(self.tgt_cloud[self.corr[:, 1], :3])

    def getCorrespondences(self):
        return [(int(a), int(b)) for a, b in self.corr]


class Quatro:
    """Reference include/quatro.hpp:70-1061 — the PCL-Registration-derived back-end surface."""

    def __init__(self, handle=None):
        self.reg_name_ = "Quatro"
        self.noise_bound_ = 0.3                       # public member, used by COTE (reference :115, :601)
        self.cost_ = float("inf")
        self.using_pre_estimated_RyRx_ = False
        self.estimated_RyRx_ = np.eye(3)
        self.solution_ = RegistrationSolution()
        self.params_ = Params()
        self.input_ = None
        self.target_ = None
        self.max_iterations_ = 0
        self._h = handle
        self._clear()

    def _clear(self):
        self.max_clique_ = np.zeros(0, dtype=np.int32)
        self.rotation_inliers_ = np.zeros(0, dtype=np.int32)
        self.final_inliers_ = np.zeros(0, dtype=np.int32)
        self.num_rot_inliers_ = 0
        self.num_maxclique_ = 0

    def getParams(self) -> Params:
        return self.params_

    def setParams(self, params: Params):
        self.params_ = params

    def setPreEstaimatedRyRx(self, estimated_RyRx):  # sic (reference :276-279)
        self.estimated_RyRx_ = np.asarray(estimated_RyRx, dtype=np.float64)[:3, :3].copy()
        self.using_pre_estimated_RyRx_ = True

    def setInputSource(self, cloud):
        self.input_ = _as_cloud(cloud)

    def setInputTarget(self, cloud):
        c = _as_cloud(cloud)
        if c.shape[0] == 0:  # reference :298-302: PCL_ERROR + return
            print("[pcl::Quatro::setInputSource] Invalid or empty point cloud dataset given!")
            return
        self.target_ = c

    def reset(self, params: Params):
        self.reg_name_ = params.reg_name
        self.params_ = params
        self._clear()

    def setMaximumIterations(self, nr_iterations: int):
        self.max_iterations_ = nr_iterations

    def _c_params(self) -> "_ql.Params":
        p = self.params_
        if p.cote_mode not in ("median", "weighted_mean"):
            raise ValueError("[COTE]: Wrong parameter comes!")  # reference :911
        if self.reg_name_ not in ("Quatro", "TEASER"):
            raise ValueError("[solveForRotation] The param is wrong! It should be 'TEASER' or 'Quatro'")  # :410
        if self.reg_name_ == "TEASER" and self.using_pre_estimated_RyRx_:
            raise ValueError("Wrong reg type name is coming!")  # :424-426
        cp = _ql.default_params()
        cp.reg_mode = _ql.REG_TEASER if self.reg_name_ == "TEASER" else _ql.REG_QUATRO
        cp.noise_bound = p.noise_bound
        cp.cbar2 = p.cbar2
        cp.rotation_gnc_factor = p.rotation_gnc_factor
        cp.rotation_cost_threshold = p.rotation_cost_threshold
        cp.kcore_heuristic_threshold = p.kcore_heuristic_threshold
        cp.cote_noise_bound = self.noise_bound_
        for i, v in enumerate(np.asarray(self.estimated_RyRx_, dtype=np.float64).reshape(-1)):
            cp.ryrx[i] = float(v)
        cp.rotation_max_iterations = int(p.rotation_max_iterations)
        cp.inlier_selection_mode = int(p.inlier_selection_mode)
        cp.cote_median = 1 if p.cote_mode == "median" else 0
        cp.using_rot_inliers_when_estimating_cote = int(bool(p.using_rot_inliers_when_estimating_cote))
        cp.using_pre_estimated_ryrx = int(bool(self.using_pre_estimated_RyRx_))
        return cp

    def computeTransformation(self, output=None):
        """computeTransformation(Eigen::Matrix4d& output) (reference :769-936).  Returns the 4x4; when a
        numpy array is passed it is overwritten in place — and left untouched if the clique is too small,
        as in the reference (:809-813)."""
        if self.input_ is None or self.target_ is None:
            raise ValueError("input clouds not set")
        if self.input_.shape[0] != self.target_.shape[0]:
            raise ValueError("source and target keypoint clouds must have equal length")
        h = self._h or _handle()
        cp = self._c_params()
        cp.max_clique_time_limit = float(self.params_.max_clique_time_limit)  # :800 (PMC_EXACT only)
        r = h.solve(self.input_, self.target_, cp)
        # the reference persists params_.noise_bound *= 2/scale for later calls (:850-852)
        self.params_.noise_bound = self.params_.noise_bound * 2.0
        self.max_clique_ = r["clique"]
        self.num_maxclique_ = int(r["clique"].size)
        if not r["valid"]:
            self.solution_.valid = False
            return output
        self.rotation_inliers_ = r["rot_inliers"]
        self.num_rot_inliers_ = int(r["rot_inliers"].size)
        self.final_inliers_ = r["final_inliers"]
        self.cost_ = r["cost"]
        self.solution_ = RegistrationSolution(True, 1.0, r["T"][:3, 3].copy(), r["T"][:3, :3].copy())
        if output is None:
            return r["T"].copy()
        output[...] = r["T"]
        return output

    def getMaxCliques(self):
        return self.input_[self.max_clique_], self.target_[self.max_clique_]

    def getFinalInliers(self):
        return self.input_[self.final_inliers_], self.target_[self.final_inliers_]

    def getFinalInliersIndices(self):
        return [int(i) for i in self.final_inliers_]

    def getNumRotaionInliers(self) -> int:  # sic
        return self.num_rot_inliers_

    def getNumMaxCliqueInliers(self) -> int:
        return self.num_maxclique_


class IterativeClosestPoint:
    """pcl::IterativeClosestPoint's surface (setInputSource / setInputTarget / the convergence knobs / align) over
    qtr_icp: the 6-DoF refinement that normally follows a global registration.  Point-to-plane by default
    (pcl::IterativeClosestPointWithNormals; target normals at normal_radius unless setTargetNormals gives them),
    point-to-point with method="point_to_point", plane-to-plane (Generalized ICP; setSourceNormals / setTargetNormals, or
    both normal sets at normal_radius) with method="plane_to_plane", its voxelised form (VGICP: the target as one Gaussian
    per voxel of side max_correspondence_distance, a lookup in place of the search; normals as for plane-to-plane) with
    method="voxel_plane_to_plane".  Everything numerical runs on the device."""

    def __init__(self, handle=None, method: str = "point_to_plane", normal_radius: float = 0.5):
        methods = {"point_to_plane": _ql.ICP_POINT_TO_PLANE, "point_to_point": _ql.ICP_POINT_TO_POINT,
                   "plane_to_plane": _ql.ICP_PLANE_TO_PLANE, "voxel_plane_to_plane": _ql.ICP_VOXEL_PLANE_TO_PLANE}
        if method not in methods:
            raise ValueError("method must be 'point_to_plane', 'point_to_point', 'plane_to_plane' or 'voxel_plane_to_plane'")
        self._h = handle
        self.params_ = _ql.default_icp_params(method=methods[method], normal_radius=float(normal_radius))
        self.input_ = None
        self.source_normals_ = None
        self.target_ = None
        self.target_normals_ = None
        self.final_transformation_ = np.eye(4)
        self.converged_ = False
        self.result_ = None

    def setInputSource(self, cloud):
        self.input_ = _as_cloud(cloud)
        self.source_normals_ = None

    def setInputTarget(self, cloud):
        self.target_ = _as_cloud(cloud)
        self.target_normals_ = None

    def setSourceNormals(self, normals):
        """plane-to-plane only: the source's normals (source frame); None = computed at normal_radius"""
        self.source_normals_ = None if normals is None else _as_cloud(normals)

    def setTargetNormals(self, normals):
        self.target_normals_ = None if normals is None else _as_cloud(normals)

    def setMaxCorrespondenceDistance(self, distance: float):
        self.params_.max_correspondence_distance = float(distance)

    def setMaximumIterations(self, nr_iterations: int):
        self.params_.max_iterations = int(nr_iterations)

    def setTransformationEpsilon(self, epsilon: float):
        self.params_.transformation_epsilon = float(epsilon)

    def setEuclideanFitnessEpsilon(self, epsilon: float):
        self.params_.euclidean_fitness_epsilon = float(epsilon)

    def getMaxCorrespondenceDistance(self) -> float:
        return self.params_.max_correspondence_distance

    def getMaximumIterations(self) -> int:
        return self.params_.max_iterations

    def align(self, guess=None):
        """Runs the loop from `guess` (4x4, default identity) and returns the source transformed by the final
        transformation, like pcl::Registration::align(output, guess)."""
        if self.input_ is None or self.target_ is None:
            raise ValueError("input clouds not set")
        h = self._h or _handle()
        g = np.eye(4) if guess is None else guess
        if self.params_.method in (_ql.ICP_PLANE_TO_PLANE, _ql.ICP_VOXEL_PLANE_TO_PLANE):
            r = h.gicp(self.input_, self.target_, self.source_normals_, self.target_normals_, g, self.params_)
        else:
            r = h.icp(self.input_, self.target_, self.target_normals_, g, self.params_)
        self.result_ = r
        self.final_transformation_ = r["T"]
        self.converged_ = r["converged"]
        T = r["T"]
        out = self.input_.copy()
        out[:, :3] = (self.input_[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        return out

    def hasConverged(self) -> bool:
        return bool(self.converged_)

    def getFitnessScore(self) -> float:
        """Mean squared distance of the last iteration's correspondences (DBL_MAX without any)."""
        return float(self.result_["fitness"]) if self.result_ else float(np.finfo(np.float64).max)

    def getFinalTransformation(self) -> np.ndarray:
        return self.final_transformation_.copy()


def refine_quatro(quatro: "Quatro", source_cloud, target_cloud, icp: IterativeClosestPoint | None = None):
    """Refines a Quatro result on the clouds themselves (the scans, typically voxelised): an IterativeClosestPoint on the
    same handle as `quatro`, started from its solution.  Returns the refined 4x4 (and leaves the ICP object's state
    readable: hasConverged, getFitnessScore)."""
    icp = icp or IterativeClosestPoint(handle=quatro._h)
    if icp._h is None:
        icp._h = quatro._h
    guess = np.eye(4)
    if quatro.solution_.valid:
        guess[:3, :3] = quatro.solution_.rotation
        guess[:3, 3] = quatro.solution_.translation
    icp.setInputSource(source_cloud)
    icp.setInputTarget(target_cloud)
    icp.align(guess)
    return icp.getFinalTransformation()


def best_candidate(records) -> int:
    """Index of the best registration record of a one-to-many job: the largest number of final inliers among the
    records with valid set, ties to the lowest index; -1 when no record is valid.  Host side only."""
    best, best_n = -1, -1
    for i, r in enumerate(records):
        if not r.get("valid"):
            continue
        n = int(r["n_final"]) if "n_final" in r else int(len(r["final_inliers"]))
        if n > best_n:
            best, best_n = i, n
    return best


def register_one_to_many(handle, query_kf, candidate_kfs, fp=None, params=None, icp=None, seeds=None):
    """Loop closing: one query keyframe (the source) against K candidate keyframes (the targets), as ONE batched job
    (Handle.register_batch_keyframes: K + 1 front ends were paid when the keyframes were made, none here).  seeds: one
    tuple-test seed per candidate (default: fp.seed for all).  Returns (records, best) — the per-candidate result dicts
    and best_candidate(records) — or with icp (records, refined, best)."""
    fp = fp or _ql.default_frontend_params()
    K = len(candidate_kfs)
    seeds = [int(fp.seed)] * K if seeds is None else [int(x) for x in seeds]
    assert len(seeds) == K
    out = handle.register_batch_keyframes([(query_kf, c, s) for c, s in zip(candidate_kfs, seeds)], fp, params, icp)
    if icp is None:
        return out, best_candidate(out)
    return out[0], out[1], best_candidate(out[0])


def evaluate_one_to_many(handle, query_kf, target_kfs, transforms, eval_params=None, slot=0):
    """Evaluates the query keyframe (the source) against K target keyframes under K transforms (4 x 4, query -> target
    frame) as ONE grouped job (Handle.evaluate_keyframes_batch; more than EVAL_MAX_PAIRS targets: several).  Returns one
    record dict per target: overlap, inlier_rmse, information, hessian_plane, ..."""
    assert len(target_kfs) == len(transforms)
    pairs = [(query_kf, t, T) for t, T in zip(target_kfs, transforms)]
    out = []
    for a in range(0, len(pairs), _ql.EVAL_MAX_PAIRS):
        out += handle.evaluate_keyframes_batch(pairs[a:a + _ql.EVAL_MAX_PAIRS], eval_params, slot)
    return out


def make_submap(handle, keyframes, poses, center, half_width, fp=None, id_lo=0, id_hi=None, slot=0):
    """The submap around keyframe `center`: the keyframes center - half_width .. center + half_width, clipped to
    [id_lo, id_hi) (id_hi = None: len(keyframes)), fused into one Keyframe by Handle.merge_keyframes.  Member i travels
    under inv(poses[center]) @ poses[i] (float64; poses[i]: 4 x 4, keyframe i's frame -> the map frame), so the submap lives
    in the centre keyframe's frame and a registration against it yields what one against the centre keyframe would.  fp
    belongs to the submap.  The caller closes the returned Keyframe."""
    id_hi = len(keyframes) if id_hi is None else min(int(id_hi), len(keyframes))
    lo, hi = max(int(center) - int(half_width), int(id_lo), 0), min(int(center) + int(half_width) + 1, id_hi)
    if not lo <= center < hi:
        raise ValueError(f"make_submap: centre {center} is outside the id range [{id_lo}, {id_hi})")
    inv_c = np.linalg.inv(np.asarray(poses[center], dtype=np.float64))
    rel = np.stack([inv_c @ np.asarray(poses[i], dtype=np.float64) for i in range(lo, hi)])
    return handle.merge_keyframes([keyframes[i] for i in range(lo, hi)], rel, fp, slot)


def build_map(handle, keyframes, poses, voxel_size=1.0, capacity=None, carve=None):
    """The global map: every keyframe inserted under its pose (4 x 4, keyframe frame -> map frame — what
    Handle.optimize_pose_graph returns) into a new VoxelMap of side voxel_size, in list order.  capacity None: the sum of
    the keyframes' voxel counts, which no map of them can exceed (at least 1).  The caller destroys the returned map; its
    fetch() is the map cloud.

    carve = CarveParams (lib.default_carve_params): after all inserts the map is carved with all keyframes under their poses
    (VoxelMap.carve_keyframes), in groups of 64 in list order, each group a vote of its own: what moved through the scene
    while it was mapped leaves the map.  Every group must hold at least carve.min_votes keyframes (ValueError before
    anything is built).  The keyframes should be made of raw sweeps (see VoxelMap.carve).  None: nothing is carved."""
    assert len(keyframes) == len(poses)
    if carve is not None:
        groups = [(a, min(a + _ql.CARVE_MAX_KEYFRAMES, len(keyframes))) for a in range(0, len(keyframes), _ql.CARVE_MAX_KEYFRAMES)]
        if any(b - a < carve.min_votes for a, b in groups):
            raise ValueError(f"build_map: carve.min_votes={carve.min_votes} exceeds a group of the {len(keyframes)} keyframes "
                             f"(groups of {_ql.CARVE_MAX_KEYFRAMES})")
    if capacity is None:
        capacity = max(1, sum(int(kf.info["n_voxels"]) for kf in keyframes))
    vmap = handle.voxel_map(voxel_size, capacity)
    try:
        for kf, pose in zip(keyframes, poses):
            vmap.insert_keyframe(kf, pose)
        if carve is not None:
            for a, b in groups:
                vmap.carve_keyframes(keyframes[a:b], np.asarray(poses, dtype=np.float64)[a:b], carve)
    except Exception:
        vmap.destroy()
        raise
    return vmap


def localize(handle, vmap, keyframe, guess, icp=None):
    """Localisation of a scan (a Keyframe) in a finished map: the voxelised plane-to-plane refinement of the keyframe
    against vmap from `guess` (4 x 4, keyframe frame -> map frame).  The map is only read.  Returns the ICP result dict; its T
    is the pose."""
    return vmap.register_keyframe(keyframe, guess, icp)


def pose_hypothesis(base, yaw, dx=0.0, dy=0.0):
    """qtr_vmap_hypothesis (include/qtr_vmap_batch_math.h) restated in Python floats: base . [Rz(yaw) | (dx, dy, 0)], cos
    and sin from libm, everything else in the header's order, so C, C++ and Python give the same bits.  Pure host code: no
    library is loaded."""
    b = [[float(x) for x in row] for row in np.asarray(base, dtype=np.float64).reshape(4, 4)]
    yaw, dx, dy = float(yaw), float(dx), float(dy)
    c, s = math.cos(yaw), math.sin(yaw)
    out = [[r[0] * c + r[1] * s, r[1] * c - r[0] * s, r[2], (r[0] * dx + r[1] * dy) + r[3]] for r in b[:3]]
    out.append([0.0, 0.0, 0.0, 1.0])
    return np.array(out, dtype=np.float64)


def pose_hypotheses(base, yaws, offsets):
    """The guesses around `base` (4 x 4, a frame -> the map frame): pose_hypothesis(base, yaw, dx, dy) for every yaw of
    `yaws` (radians, about base's z) and every (dx, dy) of `offsets` (metres, in base's xy plane), the yaws outermost.
    Returns [len(yaws) * len(offsets), 4, 4] float64."""
    out = [pose_hypothesis(base, yaw, dx, dy) for yaw in yaws for dx, dy in offsets]
    return np.stack(out) if out else np.zeros((0, 4, 4))


def best_hypothesis(results) -> int:
    """qtr_vmap_batch_best restated: among the ICP dicts with status 0 and valid, the largest n_corr; ties go to the smaller
    rmse, then to the smaller index; -1 when none qualifies."""
    best = -1
    for i, r in enumerate(results):
        if r.get("status", 0) != 0 or not r.get("valid"):
            continue
        if best < 0 or r["n_corr"] > results[best]["n_corr"] or (
                r["n_corr"] == results[best]["n_corr"] and float(r["rmse"]) < float(results[best]["rmse"])):
            best = i
    return best


def best_evaluation(evals) -> int:
    """qtr_vmap_eval_best (include/qtr_vmap_eval_math.h) restated: among the valid map evaluations the largest n_corr; ties
    go to the smaller rmse, then to the smaller index; -1 when none is valid."""
    best = -1
    for i, e in enumerate(evals):
        if not e.get("valid"):
            continue
        if best < 0 or e["n_corr"] > evals[best]["n_corr"] or (
                e["n_corr"] == evals[best]["n_corr"] and float(e["rmse"]) < float(evals[best]["rmse"])):
            best = i
    return best


def evaluation_order(evals) -> list:
    """The indices of the map evaluations sorted by best_evaluation's rule (more n_corr, then the smaller rmse, then the
    smaller index), the invalid ones last in index order: order[0] is best_evaluation(evals) when one is valid."""
    good = sorted((i for i, e in enumerate(evals) if e.get("valid")),
                  key=lambda i: (-int(evals[i]["n_corr"]), float(evals[i]["rmse"]), i))
    return good + [i for i, e in enumerate(evals) if not e.get("valid")]


def _scan_items(scan, guesses):
    scan = tuple(scan) if isinstance(scan, (tuple, list)) else (scan,)
    return [scan + (g,) for g in np.asarray(guesses, dtype=np.float64).reshape(-1, 4, 4)]


def score_hypotheses(handle, vmap, scan, guesses, slot=0):
    """One scan — a Keyframe, or a pair (xyz4, normals4) — evaluated against vmap under every pose of `guesses` ([G, 4, 4],
    scan frame -> map frame) by VoxelMap.evaluate_batch: one launch per 1024 poses, nothing is iterated.  Returns
    {"evaluations": the G evaluation dicts, "order": evaluation_order of them, "best": order[0] or -1 when none is valid}.
    The map is only read."""
    evals = vmap.evaluate_batch(_scan_items(scan, guesses), False, slot)
    order = evaluation_order(evals)
    return {"evaluations": evals, "order": order, "best": best_evaluation(evals)}


def relocalize(handle, vmap, keyframe, guesses, icp=None, slot=0, keep=None):
    """Localisation of a scan in a finished map without one good guess: the scan — a Keyframe, or a pair (xyz4, normals4) of
    a voxelised cloud with its normals — is registered against vmap from every guess of `guesses` ([G, 4, 4], scan frame ->
    map frame) by VoxelMap.register_batch — one chain of launches per 64 guesses — and best_hypothesis picks the winner.
    Returns {"best": its index (-1: no registration is valid), "T": its pose (None then), "results": the G ICP dicts}.
    keep = m: score_hypotheses first, then only the first m guesses of its order are registered (in index order; each is
    bit for bit what the full batch gives it); "results" holds None for the others and the output gains "scores".  Whether
    the eventual winner scores among the first m depends on the scene and on the grid's spacing.
    The map is only read."""
    guesses = np.asarray(guesses, dtype=np.float64).reshape(-1, 4, 4)
    items = _scan_items(keyframe, guesses)
    if keep is None:
        results = vmap.register_batch(items, icp, slot)
        best = best_hypothesis(results)
        return {"best": best, "T": results[best]["T"] if best >= 0 else None, "results": results}
    scores = score_hypotheses(handle, vmap, keyframe, guesses, slot)
    chosen = sorted(scores["order"][:max(int(keep), 0)])
    sub = vmap.register_batch([items[i] for i in chosen], icp, slot)
    results = [None] * len(items)
    for i, r in zip(chosen, sub):
        results[i] = r
    b = best_hypothesis(sub)
    best = chosen[b] if b >= 0 else -1
    return {"best": best, "T": results[best]["T"] if best >= 0 else None, "results": results, "scores": scores}


def relocalize_in_map(handle, index, poses, vmap, query_kf, k, yaws=(0.0,), offsets=((0.0, 0.0),), icp=None, id_lo=0,
                      id_hi=None, slot=0, keep=None):
    """Relocalisation from nothing: index.query(query_kf, k, id_lo, id_hi) names the k most similar entries with a yaw each
    (query -> entry); poses[id] (4 x 4, entry frame -> map frame) turned by that yaw is a guess for the query's pose in the
    map, and pose_hypotheses spreads `yaws` and `offsets` around it: len(matches) * len(yaws) * len(offsets) guesses,
    candidates outermost, registered by relocalize (keep: relocalize's).  Returns relocalize's dict plus "matches", "guesses"
    ([G, 4, 4]), "candidate" (per guess: its position in matches) and "best_id" (the index entry the winner came from, -1
    without one)."""
    matches = index.query(query_kf, k, id_lo, id_hi)
    guesses, cand = [], []
    for c, m in enumerate(matches):
        base = np.asarray(poses[m["id"]], dtype=np.float64).reshape(4, 4)
        hyp = pose_hypotheses(base, [float(m["yaw"]) + float(y) for y in yaws], offsets)
        guesses += list(hyp)
        cand += [c] * len(hyp)
    guesses = np.stack(guesses) if guesses else np.zeros((0, 4, 4))
    out = relocalize(handle, vmap, query_kf, guesses, icp, slot, keep)
    out.update(matches=matches, guesses=guesses, candidate=cand,
               best_id=matches[cand[out["best"]]]["id"] if out["best"] >= 0 else -1)
    return out


def degeneracy(evaluation):
    """How well a map evaluation's hessian (the registration's normal matrix at T: rotation first, then translation, in
    the map's frame) constrains the pose.  Host code only.  Returns {"eigenvalues": numpy.linalg.eigvalsh of the 6 x 6,
    ascending, "condition": largest / smallest (inf when the smallest is not positive), "translation_eigenvalues":
    eigvalsh of the translation block after the rotation is marginalised out (H_tt - H_tr H_rr^+ H_rt), ascending,
    "weakest_translation": the unit eigenvector of the smallest of them — along a corridor, in the plane of an open
    field}."""
    H = np.asarray(evaluation["hessian"], dtype=np.float64).reshape(6, 6)
    ev = np.linalg.eigvalsh(H)
    St = H[3:, 3:] - H[3:, :3] @ np.linalg.pinv(H[:3, :3]) @ H[:3, 3:]
    St = 0.5 * (St + St.T)
    tv, tvec = np.linalg.eigh(St)
    w = tvec[:, 0] / np.linalg.norm(tvec[:, 0])
    return {"eigenvalues": ev, "condition": float(ev[-1] / ev[0]) if ev[0] > 0.0 else float("inf"),
            "weakest_translation": w, "translation_eigenvalues": tv}


def constant_velocity_guess(T_prev2, T_prev1):
    """T_{k-1} (T_{k-2}^-1 T_{k-1}) for rigid 4 x 4 poses, in plain float64 arithmetic of a fixed order (the inverse is
    [R^T | -R^T t]), so every caller gets the same bits from the same poses."""
    A = [[float(x) for x in row] for row in np.asarray(T_prev2, dtype=np.float64).reshape(4, 4)]
    B = [[float(x) for x in row] for row in np.asarray(T_prev1, dtype=np.float64).reshape(4, 4)]
    inv = [[A[c][r] for c in range(3)] + [-((A[0][r] * A[0][3] + A[1][r] * A[1][3]) + A[2][r] * A[2][3])] for r in range(3)]
    inv.append([0.0, 0.0, 0.0, 1.0])

    def mul(X, Y):
        return [[((X[r][0] * Y[0][c] + X[r][1] * Y[1][c]) + X[r][2] * Y[2][c]) + X[r][3] * Y[3][c] for c in range(4)]
                for r in range(4)]

    G = mul(B, mul(inv, B))
    G[3] = [0.0, 0.0, 0.0, 1.0]
    return np.array(G, dtype=np.float64)


def constant_velocity_knots(T_prev2, T_prev1, period):
    """The knots of a sweep under the constant-velocity guess: ([0, period], [I, T_{k-2}^-1 T_{k-1}]) — the sensor moves during
    sweep k as it moved from pose k - 2 to pose k - 1, expressed in its own frame at the sweep's start — for Handle.deskew and
    Handle.keyframe(times=...).  The motion is computed in the fixed-order float64 arithmetic of constant_velocity_guess
    (the inverse is [R^T | -R^T t]), so every caller gets the same bits from the same poses."""
    A = [[float(x) for x in row] for row in np.asarray(T_prev2, dtype=np.float64).reshape(4, 4)]
    B = [[float(x) for x in row] for row in np.asarray(T_prev1, dtype=np.float64).reshape(4, 4)]
    inv = [[A[c][r] for c in range(3)] + [-((A[0][r] * A[0][3] + A[1][r] * A[1][3]) + A[2][r] * A[2][3])] for r in range(3)]
    inv.append([0.0, 0.0, 0.0, 1.0])
    M = [[((inv[r][0] * B[0][c] + inv[r][1] * B[1][c]) + inv[r][2] * B[2][c]) + inv[r][3] * B[3][c] for c in range(4)]
         for r in range(4)]
    M[3] = [0.0, 0.0, 0.0, 1.0]
    return np.array([0.0, float(period)], dtype=np.float64), np.stack([np.eye(4), np.array(M, dtype=np.float64)])


def sample_sweep(raw, times, leaf):
    """One RAW point of every voxel floor(p / leaf) of a sweep, on the host: the lowest-index finite point of each voxel, in
    ascending index, with its time.  A raw point and never a centroid, so its time is exact — what VoxelMap.register_ct needs.
    Returns (points [m, 4] float32, times [m] float32); the times are the input's, unaltered."""
    raw = np.ascontiguousarray(raw, dtype=np.float32).reshape(-1, 4)
    times = np.ascontiguousarray(times, dtype=np.float32).reshape(-1)
    if times.shape[0] != raw.shape[0]:
        raise ValueError(f"sample_sweep: {raw.shape[0]} points, {times.shape[0]} times")
    if not float(leaf) > 0.0:
        raise ValueError(f"sample_sweep: leaf={leaf} must be positive")
    idx = np.flatnonzero(np.isfinite(raw[:, :3]).all(axis=1))
    if idx.size == 0:
        return raw[:0].copy(), times[:0].copy()
    vox = np.floor(raw[idx, :3].astype(np.float64) / float(leaf)).astype(np.int64)
    _, first = np.unique(vox, axis=0, return_index=True)  # (the first occurrence of every voxel: the lowest index)
    keep = idx[np.sort(first)]
    return raw[keep].copy(), times[keep].copy()


def _scan_to_map_odometry_ct(handle, scans, fp, voxel_size, icp, capacity, window_radius, times, sweep_period, carve):
    """scan_to_map_odometry(continuous_time=True): see there."""
    period = float(sweep_period)
    knot_times = np.array([0.0, period], dtype=np.float64)
    vmap = handle.voxel_map(voxel_size, (1 << 20) if capacity is None else capacity)
    starts, end_prev = [], np.eye(4)
    try:
        for k, scan in enumerate(scans):
            if isinstance(scan, _ql.Keyframe):
                raise ValueError("scan_to_map_odometry: continuous_time needs raw sweeps (a keyframe's voxels carry no times)")
            begin = end_prev  # B_k = E_{k-1}; E_0 ends an identity motion
            if k == 0:
                end = np.eye(4)
            else:
                guess = constant_velocity_guess(starts[-1], begin)
                pts, ts = sample_sweep(scan, times[k], fp.voxel_size)
                normals, _ = handle.fpfh(pts, fp.normal_radius, fp.fpfh_radius)  # (the histograms are computed and not used)
                r = vmap.register_ct(pts, normals, ts, 0.0, period, begin, guess, icp)
                end = np.array(r["T"], dtype=np.float64) if r["valid"] else np.array(guess, dtype=np.float64)
            kf = handle.keyframe(scan, fp, times=times[k], knot_times=knot_times, knot_poses=np.stack([begin, end]), t_ref=0.0)
            try:
                vmap.insert_keyframe(kf, begin)
                if window_radius is not None:
                    vmap.evict(begin[:3, 3], window_radius)
                if carve is not None:
                    vmap.carve_keyframes([kf], begin[None], carve)
            finally:
                kf.close()
            starts.append(begin)
            end_prev = end
    except Exception:
        vmap.destroy()
        raise
    return (np.stack(starts) if starts else np.zeros((0, 4, 4))), vmap


def scan_to_map_odometry(handle, scans, fp=None, voxel_size=1.0, icp=None, capacity=None, window_radius=None, times=None,
                         sweep_period=None, carve=None, continuous_time=False):
    """Scan-to-map odometry: a keyframe of every scan (fp; a scan that already is a Keyframe is used as it is), the first
    inserted at the identity, every later one registered against the map from the constant-velocity guess
    T_{k-1} (T_{k-2}^-1 T_{k-1}) (the identity motion for the second scan) and inserted under the result.  A registration
    that is not valid keeps its guess as the pose.  Returns (poses [K, 4, 4], vmap); the caller destroys the map.  The
    keyframes made here are closed before the call returns.  capacity None: 1 << 20 voxels.

    window_radius = r (metres): a local map.  After each insert the map is evicted around the translation of the pose just
    inserted (VoxelMap.evict: voxels farther than floor(r / voxel_size) voxels from the pose's voxel leave), so `capacity`
    can be sized for the window, not for the trajectory, and scans are no longer registered against voxels folded from
    poses far behind.  None: nothing is evicted, the map of the whole trajectory.

    times = a list of per-scan float32 arrays (the time of every point since its sweep's start, seconds) with sweep_period
    (seconds per sweep): the scans are RAW sweeps of a moving sensor and every one is deskewed on the device on its way to
    its keyframe (Handle.keyframe(times=...), t_ref = 0): scan k >= 2 under constant_velocity_knots(T_{k-2}, T_{k-1},
    sweep_period), scans 0 and 1 under identity knots (no motion is known yet).  The poses are then the sensor's at the start
    of each sweep.  A scan that already is a Keyframe is used as it is.  None: the scans are taken as they are.

    carve = CarveParams (lib.default_carve_params): after each insert — and after its eviction where a window is set — the
    map is carved with that scan's keyframe under its pose (VoxelMap.carve_keyframes, one vote, so carve.min_votes must be
    1; ValueError before anything is built): voxels the scan saw through leave the map before the next registration.  The scans should be raw sweeps (see
    VoxelMap.carve).  None: nothing is carved.

    continuous_time = True (needs times and sweep_period; every scan a raw sweep): the deskew is the registration's result
    and no longer a guess made before it.  Sweep k >= 1 begins at B_k = E_{k-1}, the end pose of the sweep before it (E_0 = the
    identity: the first sweep is taken as unmoved).  One raw point per voxel of side fp.voxel_size is taken from the sweep
    with its time (sample_sweep), its normals come from Handle.fpfh (the histograms are wasted), and VoxelMap.register_ct
    fits the END pose E_k against the map from the constant-velocity end guess B_k (B_{k-1}^-1 B_k) with the begin pose held
    fixed, every point carried by the pose interpolated at its own time.  The sweep is then deskewed under the two knots
    (B_k, E_k) on its way to its keyframe and inserted under B_k.  A registration that is not valid keeps its guess as E_k.
    The returned poses stay the sweep STARTS, B_k.  False: everything above, unchanged."""
    fp = fp or _ql.default_frontend_params()
    if carve is not None and carve.min_votes != 1:
        raise ValueError(f"scan_to_map_odometry: carve.min_votes={carve.min_votes} (one scan votes per carve: it must be 1)")
    if continuous_time and times is None:
        raise ValueError("scan_to_map_odometry: continuous_time needs times and sweep_period (raw sweeps with per-point times)")
    if times is not None:
        if sweep_period is None or not float(sweep_period) > 0.0:
            raise ValueError("scan_to_map_odometry: times needs sweep_period > 0 (seconds per sweep)")
        if len(times) != len(scans):
            raise ValueError(f"scan_to_map_odometry: {len(scans)} scans, {len(times)} arrays of times")
    if continuous_time:
        return _scan_to_map_odometry_ct(handle, scans, fp, voxel_size, icp, capacity, window_radius, times, sweep_period, carve)
    vmap = handle.voxel_map(voxel_size, (1 << 20) if capacity is None else capacity)
    poses = []
    try:
        for k, scan in enumerate(scans):
            own = not isinstance(scan, _ql.Keyframe)
            if own and times is not None:
                kt, kp = (constant_velocity_knots(poses[-2], poses[-1], sweep_period) if k >= 2 else
                          (np.array([0.0, float(sweep_period)]), np.stack([np.eye(4), np.eye(4)])))
                kf = handle.keyframe(scan, fp, times=times[k], knot_times=kt, knot_poses=kp, t_ref=0.0)
            else:
                kf = handle.keyframe(scan, fp) if own else scan
            try:
                if k == 0:
                    T = np.eye(4)
                else:
                    guess = poses[-1] if k == 1 else constant_velocity_guess(poses[-2], poses[-1])
                    r = localize(handle, vmap, kf, guess, icp)
                    T = np.array(r["T"], dtype=np.float64) if r["valid"] else np.array(guess, dtype=np.float64)
                vmap.insert_keyframe(kf, T)
                if window_radius is not None:
                    vmap.evict(T[:3, 3], window_radius)
                if carve is not None:
                    vmap.carve_keyframes([kf], T[None], carve)
            finally:
                if own:
                    kf.close()
            poses.append(T)
    except Exception:
        vmap.destroy()
        raise
    return (np.stack(poses) if poses else np.zeros((0, 4, 4))), vmap


def close_loop(handle, index, keyframes, query_kf, k, id_lo=0, id_hi=None, fp=None, params=None, icp=None, poses=None,
               submap_half_width=0, evaluate=None, min_overlap=None):
    """Loop closing from the first link: index.query(query_kf) picks the k entries of [id_lo, id_hi) whose Scan Context
    descriptors are most similar (quatro_amd.lib.PlaceIndex), keyframes[id] are their keyframes, and register_one_to_many
    registers the query against exactly those, in the order the search returned them.  Returns a dict: "matches" (the
    search's dicts id / shift / distance / yaw), "records" (and "refined" with icp), "best" (best_candidate's index into
    them, -1 when no registration is valid) and "best_id" (the index entry of the winner, -1 likewise).  No candidate —
    an empty id range — registers nothing.  Host-side glue over existing calls.

    submap_half_width = n > 0 (poses required: one 4 x 4 per keyframe, its frame -> the map frame): every match `id` is
    registered as make_submap around id — the 2 n + 1 keyframes id - n .. id + n under their poses, clipped to the searched
    id range [id_lo, id_hi) — id_hi = None: the index's size — so the query's own neighbourhood is never fused.  The submaps are temporary: destroyed when the job is done.
    The transforms still map the query into keyframe id's frame.

    evaluate = an EvalParams (or True: the defaults): every valid record is evaluated (evaluate_one_to_many) at its refined T
    with icp, else at its registration T — against the submap where there is one — and the result gets "evaluations": one
    record per candidate, None where the registration was not valid.  min_overlap = x (implies evaluate): "best" / "best_id"
    are chosen among the records whose overlap reaches x, -1 when none does."""
    if min_overlap is not None and evaluate is None:
        evaluate = True
    if submap_half_width > 0 and poses is None:
        raise ValueError("close_loop: submap_half_width > 0 needs the keyframes' poses")
    matches = index.query(query_kf, k, id_lo, id_hi)
    out = {"matches": matches, "records": [], "best": -1, "best_id": -1}
    if icp is not None:
        out["refined"] = []
    if evaluate is not None:
        out["evaluations"] = []
    if not matches:
        return out
    submaps = []
    try:
        if submap_half_width > 0:
            hi = len(index) if id_hi is None else id_hi
            for m in matches:
                submaps.append(make_submap(handle, keyframes, poses, m["id"], submap_half_width, fp, id_lo, hi))
            targets = submaps
        else:
            targets = [keyframes[m["id"]] for m in matches]
        got = register_one_to_many(handle, query_kf, targets, fp, params, icp)
        if evaluate is not None:
            at = [i for i, r in enumerate(got[0]) if r.get("valid")]
            Ts = [got[1][i]["T"] if icp is not None and got[1][i].get("status") == 0 else got[0][i]["T"] for i in at]
            ev = evaluate_one_to_many(handle, query_kf, [targets[i] for i in at], Ts, None if evaluate is True else evaluate)
            out["evaluations"] = [None] * len(targets)
            for i, e in zip(at, ev):
                out["evaluations"][i] = e
    finally:
        for sm in submaps:
            sm.close()
    out["records"], out["best"] = got[0], got[-1]
    if icp is not None:
        out["refined"] = got[1]
    if min_overlap is not None:
        ev = out["evaluations"]
        out["best"] = best_candidate([r if ev[i] is not None and ev[i]["overlap"] >= min_overlap else {}
                                      for i, r in enumerate(out["records"])])
    if out["best"] >= 0:
        out["best_id"] = matches[out["best"]]["id"]
    return out


def find_loops(index, min_gap, k, max_distance=None, first=0, last=None):
    """Loop detection over a finished run: every entry i of [first, last) (last = None: the index's size) queries the entries
    [0, i - min_gap] of its own index, as grouped calls (PlaceIndex.query_batch, entry items read in place).  The entries are
    taken in chunks such that a call has at most PLACE_BATCH_MAX queries and PLACE_BATCH_MAX_PAIRS (query, entry) pairs of
    its union range [0, b - min_gap) — b the chunk's end.  Returns one list of match dicts per entry, in order; with
    max_distance only the matches whose distance is at most that are kept (filtered on the host: the search still
    returns the k best)."""
    if min_gap < 0:
        raise ValueError("find_loops: min_gap must be >= 0")
    size = len(index)
    last = size if last is None else min(int(last), size)
    first = max(int(first), 0)
    q_cap, pair_cap = int(_ql.PLACE_BATCH_MAX), int(_ql.PLACE_BATCH_MAX_PAIRS)
    out = []
    a = first
    while a < last:
        b = min(a + q_cap, last)
        while b - a > 1 and (b - a) * max(b - min_gap, 0) > pair_cap:
            b -= 1
        got = index.query_batch([(i, (0, i - min_gap + 1)) for i in range(a, b)], k)
        for ms in got:
            out.append(ms if max_distance is None else [m for m in ms if m["distance"] <= max_distance])
        a = b
    return out


def close_loops(handle, index, keyframes, queries, k, id_lo=0, id_hi=None, fp=None, params=None, icp=None):
    """close_loop for a group of queries: ONE index.query_batch picks every query's k entries, ONE
    Handle.register_batch_keyframes registers all (query, candidate) pairs, in the queries' order and, per query, in the
    order the search returned them.  queries: Keyframes, or (Keyframe, (id_lo, id_hi)) for a range of the query's own
    (default: [id_lo, id_hi) for all).  Returns per query what close_loop returns — "matches", "records" (and "refined"
    with icp), "best", "best_id" — without its submap and evaluate options."""
    fp = fp or _ql.default_frontend_params()
    kfs, items = [], []
    for q in queries:
        kf, rng = q if isinstance(q, tuple) else (q, (id_lo, id_hi))
        kfs.append(kf)
        items.append((kf, tuple(rng)))
    matches = index.query_batch(items, k) if items else []
    pairs = [(kf, keyframes[m["id"]], int(fp.seed)) for kf, ms in zip(kfs, matches) for m in ms]
    records, refined = [], []
    if pairs:
        got = handle.register_batch_keyframes(pairs, fp, params, icp)
        records, refined = (got, []) if icp is None else got
    outs, at = [], 0
    for ms in matches:
        o = {"matches": ms, "records": records[at:at + len(ms)], "best": -1, "best_id": -1}
        if icp is not None:
            o["refined"] = refined[at:at + len(ms)]
        at += len(ms)
        o["best"] = best_candidate(o["records"])
        if o["best"] >= 0:
            o["best_id"] = ms[o["best"]]["id"]
        outs.append(o)
    return outs


def default_line_process_weight(edges, max_correspondence_distance, preference_loop_closure=1.0):
    """Open3D's rule for the line process weight mu: preference_loop_closure x max_correspondence_distance^2 x the mean of
    information[5][5] over the UNCERTAIN edges (information[5][5] is n_corr in the evaluation's matrix).  edges: (s, t, T,
    information, uncertain) tuples.  0.0 without an uncertain edge (the line process is then off)."""
    n = [float(np.asarray(e[3], dtype=np.float64).reshape(6, 6)[5, 5]) for e in edges if e[4]]
    if not n:
        return 0.0
    return float(preference_loop_closure) * float(max_correspondence_distance) ** 2 * (sum(n) / len(n))


class PoseGraph:
    """A pose graph on the host: nodes (4 x 4 poses, keyframe frame -> map frame, what make_submap and close_loop(poses=)
    take) and edges (s, t, T, information, uncertain) with T mapping keyframe s's frame into keyframe t's — a registration's
    T with s the source / query and t the target / candidate — and information the 6 x 6 of the evaluation.  optimize()
    runs Handle.optimize_pose_graph (qtr_pgo_optimize) and writes the poses back."""

    def __init__(self):
        self.poses, self.fixed, self.edges = [], [], []

    def add_node(self, pose, fixed=False) -> int:
        self.poses.append(np.array(pose, dtype=np.float64).reshape(4, 4))
        self.fixed.append(bool(fixed))
        return len(self.poses) - 1

    def add_edge(self, s, t, T, information, uncertain=False) -> int:
        s, t = int(s), int(t)
        if not (0 <= s < len(self.poses) and 0 <= t < len(self.poses)) or s == t:
            raise ValueError(f"PoseGraph.add_edge: ({s}, {t}) does not join two different nodes of {len(self.poses)}")
        self.edges.append((s, t, np.array(T, dtype=np.float64).reshape(4, 4),
                           np.array(information, dtype=np.float64).reshape(6, 6), bool(uncertain)))
        return len(self.edges) - 1

    def add_odometry(self, s, t, record, evaluation) -> int:
        """A certain edge from a registration of keyframe s (source) against keyframe t (target): T from `record` (a
        registration or refinement record), information from `evaluation` (an evaluation record at that T)."""
        if not record.get("valid", True) or evaluation is None:
            raise ValueError("PoseGraph.add_odometry: the registration is not valid or was not evaluated")
        return self.add_edge(s, t, record["T"], evaluation["information"], False)

    def add_map_node(self) -> int:
        """A fixed node at the identity: a finished voxel map's frame.  Returns its id."""
        return self.add_node(np.eye(4), fixed=True)

    def add_localization(self, node, map_node, result, evaluation, which="information", uncertain=False) -> int:
        """The edge of a localisation in a map: s = node, t = map_node, T = result["T"] (a VoxelMap registration's pose, node
        frame -> map frame) and the 6 x 6 evaluation[which] of a map evaluation at that T; which: "information" (Open3D's
        form on the matched voxel means) or "hessian" (the registration's normal matrix).  The map node sits at the
        identity, X_t = I, so the optimiser's residual vee(X_t^-1 X_s Z^-1) vanishes at X_s = T; the matrix is formed on
        world points, and the world is the edge's target frame, which is the frame an edge's information is expressed in.
        Raises on an invalid result or evaluation."""
        if which not in ("information", "hessian"):
            raise ValueError(f"PoseGraph.add_localization: which={which!r} (\"information\" or \"hessian\")")
        if result is None or not result.get("valid") or result.get("status", 0) != 0:
            raise ValueError("PoseGraph.add_localization: the localisation is not valid")
        if evaluation is None or not evaluation.get("valid") or evaluation.get("status", 0) != 0:
            raise ValueError("PoseGraph.add_localization: the evaluation is not valid")
        return self.add_edge(node, map_node, result["T"], evaluation[which], uncertain)

    def add_loop(self, query_id, loop, use="best", uncertain=True) -> int:
        """The loop edge of a close_loop(..., evaluate=...) output: query_id -> the chosen candidate's index entry.  use:
        "best" or a candidate's position.  T is the refined one where the refinement ran (its status is QTR_OK), else the
        registration's; information comes from "evaluations".  Raises when close_loop ran without evaluate, or when the
        chosen candidate was not valid."""
        if "evaluations" not in loop:
            raise ValueError("PoseGraph.add_loop: close_loop was called without evaluate: there is no information matrix")
        i = int(loop["best"]) if use == "best" else int(use)
        if not 0 <= i < len(loop["records"]) or loop["evaluations"][i] is None:
            raise ValueError("PoseGraph.add_loop: no valid, evaluated candidate to take the edge from")
        ref = loop.get("refined")
        T = ref[i]["T"] if ref and ref[i].get("status") == 0 else loop["records"][i]["T"]
        return self.add_edge(query_id, loop["matches"][i]["id"], T, loop["evaluations"][i]["information"], uncertain)

    def optimize(self, handle, params=None, slot=0) -> dict:
        """Optimises, writes the poses back and returns the result dict with "weights" and "pruned" (the indices of the
        uncertain edges whose final weight is below params.edge_prune_threshold)."""
        prm = params or _ql.default_pgo_params()
        if not any(self.fixed) and self.fixed:
            fixed = None  # (node 0 is held)
        else:
            fixed = self.fixed
        X, w, res = handle.optimize_pose_graph(np.stack(self.poses), self.edges, fixed, prm, slot)
        self.poses = [X[i].copy() for i in range(X.shape[0])]
        res["weights"] = w
        res["pruned"] = [k for k, e in enumerate(self.edges) if e[4] and w[k] < prm.edge_prune_threshold]
        return res
