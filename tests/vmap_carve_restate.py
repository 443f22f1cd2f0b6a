"""The restatement of the voxel map's visibility carving (include/qtr_vmap_carve_math.h) in numpy: every binary64 operation
of the header written again, element-wise, in the header's order (numpy's + - * / sqrt floor on float64 are IEEE and nothing
is contracted), so the results can be compared with the header under g++ (tests/vmap_carve_ref/vmap_carve_ref.cpp, loaded by
ref()) and with the device bit for bit.  RefMap adds carve / carve_scans to vmap_keep_restate.RefMap (mirroring
quatro_amd.lib.VoxelMap.carve / carve_keyframes on clouds); build_map and odometry mirror quatro_amd.api's with carve=."""
import ctypes
import os
import subprocess
import tempfile
from dataclasses import dataclass

import numpy as np

import vmap_keep_restate as KR
import vmap_restate as M

ROOT = M.ROOT
PI, PI_2 = 3.14159265358979323846, 1.57079632679489661923
EMPTY = np.uint32(0xFFFFFFFF)
NO_VOTE, OCCUPIED, SEEN_THROUGH = 0, 1, 2
MAX_SCANS = 64
BadArgError = KR.BadArgError


@dataclass
class Params:
    """qtr_carve_params at its defaults."""
    rows: int = 64
    cols: int = 1024
    window: int = 2
    min_votes: int = 1
    fov_up_deg: float = 2.5
    fov_down_deg: float = -25.5
    margin_abs: float = 0.0
    margin_rel: float = 0.0
    min_range: float = 1.0
    max_range: float = 80.0

    def to_lib(self):
        from quatro_amd import lib as ql
        return ql.default_carve_params(**self.__dict__)


@dataclass
class Cfg:
    rows: int
    cols: int
    window: int
    min_votes: int
    fov_up: float
    fov_span: float
    margin_abs: float
    margin_rel: float
    min_range: float
    max_range: float


def cfg_make(p: Params, n_scans: int, voxel_size: float) -> Cfg:
    """qtr_carve_cfg_make: the checked parameters, or BadArgError(code)."""
    f = np.float64

    def fin(x):
        return bool(np.isfinite(f(x)))
    if p.rows < 1 or p.rows > 256:
        raise BadArgError(1)
    if p.cols < 8 or p.cols > 4096:
        raise BadArgError(2)
    if not fin(p.fov_up_deg) or not fin(p.fov_down_deg) or not p.fov_up_deg > p.fov_down_deg:
        raise BadArgError(3)
    if p.window < 0 or p.window > 3:
        raise BadArgError(4)
    if p.min_votes < 1 or p.min_votes > n_scans:
        raise BadArgError(5)
    if not fin(p.margin_abs) or not p.margin_abs >= 0.0 or not fin(p.margin_rel) or not p.margin_rel >= 0.0:
        raise BadArgError(6)
    if not fin(p.min_range) or not fin(p.max_range) or not p.min_range < p.max_range:
        raise BadArgError(7)
    up = (f(p.fov_up_deg) * f(PI)) / f(180.0)
    span = up - (f(p.fov_down_deg) * f(PI)) / f(180.0)
    if not span > 0.0:
        raise BadArgError(3)
    return Cfg(int(p.rows), int(p.cols), int(p.window), int(p.min_votes), float(up), float(span),
               float(voxel_size) if p.margin_abs == 0.0 else float(p.margin_abs), float(p.margin_rel), float(p.min_range),
               float(p.max_range))


def atan_pos(x):
    """qm_atan_pos on an array of finite or +inf x >= 0."""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        inv = x > 1.0
        t = np.where(inv, 1.0 / x, x)
        for _ in range(3):
            t = t / (1.0 + np.sqrt(1.0 + t * t))
        t2 = t * t
        s = np.full_like(t, 1.0 / 19.0)
        for k in (17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
            s = 1.0 / k - t2 * s
        s = 1.0 - t2 * s
        r = 8.0 * (t * s)
        return np.where(inv, PI_2 - r, r)


def atan2d(y, x):
    """qm_atan2d on arrays of finite, not-both-zero arguments."""
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        a = atan_pos(np.abs(y) / np.abs(x))
        a = np.where(x < 0, PI - a, a)
        out = np.copysign(a, y)
        out = np.where(x == 0.0, np.copysign(PI_2, y), out)
        out = np.where(y == 0.0, np.where(np.signbit(x), np.copysign(PI, y), np.copysign(0.0, y)), out)
    return out


def pixels(c: Cfg, xyz):
    """qtr_carve_pixel on [n, 3] float64: (ok [n] bool, r [n], row [n], col [n]); r, row, col mean nothing where not ok."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & ~((x == 0.0) & (y == 0.0))
        xs, ys, zs = np.where(ok, x, 1.0), np.where(ok, y, 1.0), np.where(ok, z, 1.0)
        h2 = xs * xs + ys * ys
        h = np.sqrt(h2)
        r = np.sqrt(h2 + zs * zs)
        el, az = atan2d(zs, h), atan2d(ys, xs)
        fr = np.floor(((c.fov_up - el) * np.float64(c.rows)) / c.fov_span)
        ok &= (fr >= 0.0) & (fr < float(c.rows))
        fc = np.floor(((az + PI) * np.float64(c.cols)) / (2.0 * PI))
        ok &= (fc >= 0.0) & (fc <= float(c.cols))
        ok &= (r >= c.min_range) & (r <= c.max_range)
    row = np.where(ok, fr, 0.0).astype(np.int64)
    col = np.where(ok, fc, 0.0).astype(np.int64)
    col = np.where(col == c.cols, 0, col)
    return ok, r, row, col


def image(c: Cfg, xyz4):
    """The range image (rows x cols uint32) of one scan, [n, 4] float32 in its own frame."""
    pts = np.asarray(xyz4, np.float32).reshape(-1, 4)
    ok, r, row, col = pixels(c, pts[:, :3].astype(np.float64))
    img = np.full(c.rows * c.cols, EMPTY, np.uint32)
    with np.errstate(all="ignore"):
        bits = r[ok].astype(np.float32).view(np.uint32)
    np.minimum.at(img, row[ok] * c.cols + col[ok], bits)
    return img.reshape(c.rows, c.cols)


def to_scan(P, mu):
    """qtr_carve_to_scan: [n, 3] voxel means in the frame of the scan taken at P (4 x 4)."""
    P = np.asarray(P, np.float64).reshape(16)
    mu = np.asarray(mu, np.float64).reshape(-1, 3)
    d0, d1, d2 = mu[:, 0] - P[3], mu[:, 1] - P[7], mu[:, 2] - P[11]
    return np.stack([(P[0] * d0 + P[4] * d1) + P[8] * d2, (P[1] * d0 + P[5] * d1) + P[9] * d2,
                     (P[2] * d0 + P[6] * d1) + P[10] * d2], axis=1)


def verdicts(c: Cfg, P, mu, img):
    """qtr_carve_verdict of one scan (pose P, image img) on [n, 3] voxel means: NO_VOTE / OCCUPIED / SEEN_THROUGH per voxel."""
    ok, rv, row, col = pixels(c, to_scan(P, mu))
    img = np.asarray(img, np.uint32).reshape(c.rows, c.cols)
    ok = ok & (img[row, col] != EMPTY)
    limit = (rv + c.margin_abs) + c.margin_rel * rv
    occupied = np.zeros(ok.shape, bool)
    for dr in range(-c.window, c.window + 1):
        rr = row + dr
        inside = (rr >= 0) & (rr < c.rows)
        rr = np.clip(rr, 0, c.rows - 1)
        for dc in range(-c.window, c.window + 1):
            v = img[rr, (col + dc) % c.cols]
            occupied |= inside & (v != EMPTY) & (v.view(np.float32).astype(np.float64) <= limit)
    return np.where(ok, np.where(occupied, OCCUPIED, SEEN_THROUGH), NO_VOTE).astype(np.int32)


def carve_votes(c: Cfg, clouds, poses, mu):
    """[n, B] verdicts of the B scans (clouds in their own frames, poses scan -> map) on the voxel means."""
    mu = np.asarray(mu, np.float64).reshape(-1, 3)
    out = np.zeros((mu.shape[0], len(clouds)), np.int32)
    for b, (cl, P) in enumerate(zip(clouds, poses)):
        out[:, b] = verdicts(c, P, mu, image(c, cl))
    return out


def _check_poses(poses):
    P = [np.eye(4) if p is None else np.asarray(p, np.float64).reshape(4, 4) for p in poses]
    for p in P:
        if not np.isfinite(p[:3]).all():
            raise BadArgError("pose")
    return P


class RefMap(KR.RefMap):
    def carve_scans(self, clouds, poses, params: Params | None = None) -> dict:
        """lib.VoxelMap.carve_keyframes on clouds: the keyframes' stored voxels (KF_VOX) with their poses."""
        clouds = [np.asarray(c, np.float32).reshape(-1, 4) for c in clouds]
        if len(clouds) > MAX_SCANS or len(clouds) != len(poses):
            raise BadArgError("scans")
        poses = _check_poses(poses)
        c = cfg_make(params or Params(), len(clouds) if clouds else MAX_SCANS, self.voxel_size)
        zero = {"n_kept": 0, "n_carved": 0, "n_tested": 0, "n_members_carved": 0}
        if not clouds or len(self) == 0:
            return zero
        f = self.fetch_all()
        votes = carve_votes(c, clouds, poses, f[M.RECORDS][:, :3])
        gone = (votes == SEEN_THROUGH).sum(axis=1) >= c.min_votes
        info = {"n_kept": int((~gone).sum()), "n_carved": int(gone.sum()), "n_tested": int((votes != NO_VOTE).any(axis=1).sum()),
                "n_members_carved": int(f[M.COUNT][gone].astype(np.int64).sum())}
        if gone.any():  # the kept rows as they are: moved, never recomputed
            n_inserts, n_members = self.n_inserts, self.n_members
            self.clear()
            self.restore(f[M.COORDS][~gone], f[M.COUNT][~gone], f[M.SUMS][~gone])
            self.n_inserts, self.n_members = n_inserts, n_members - info["n_members_carved"]
        return info

    def carve(self, xyz4, pose=None, params: Params | None = None) -> dict:
        """lib.VoxelMap.carve: one cloud, one vote."""
        return self.carve_scans([xyz4], [pose], params)


def build_map(clouds, normals, poses, voxel_size=1.0, capacity=None, carve: Params | None = None):
    """quatro_amd.api.build_map restated on the keyframes' fetched voxels and normals."""
    if capacity is None:
        capacity = max(1, sum(c.shape[0] for c in clouds))
    m = RefMap(voxel_size, capacity)
    for c, n, P in zip(clouds, normals, poses):
        m.insert(c, n, P)
    if carve is not None:
        for a in range(0, len(clouds), MAX_SCANS):
            m.carve_scans(clouds[a:a + MAX_SCANS], list(poses[a:a + MAX_SCANS]), carve)
    return m


def odometry(clouds, normals, voxel_size=1.0, capacity=1 << 20, window_radius=None, carve: Params | None = None, **icp):
    """quatro_amd.api.scan_to_map_odometry restated with its window and its carving on already voxelised clouds with their
    normals; returns (poses, RefMap, results, carved): carved[k] = the info of the carve after insert k."""
    m = RefMap(voxel_size, capacity)
    poses, results, carved = [], [], []
    for k, (c, n) in enumerate(zip(clouds, normals)):
        if k == 0:
            T = np.eye(4)
        else:
            guess = poses[-1] if k == 1 else M.constant_velocity_guess(poses[-2], poses[-1])
            r = m.register(c, n, guess, **icp)
            results.append(r)
            T = r["T"].copy() if r["valid"] else np.array(guess, np.float64)
        m.insert(c, n, T)
        if window_radius is not None:
            m.evict(T[:3, 3], window_radius)
        if carve is not None:
            carved.append(m.carve_scans([c], [T], carve))
        poses.append(T)
    return np.stack(poses), m, results, carved


# ---- the header itself under g++ ---------------------------------------------------------------------------------------
_ref = None


def ref():
    global _ref
    if _ref is None:
        out = os.path.join(tempfile.mkdtemp(prefix="vmap_carve_ref_"), "libvmap_carve_ref.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                               "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "vmap_carve_ref", "vmap_carve_ref.cpp"), "-o", out])
        lib = ctypes.CDLL(out)
        P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        lib.carve_ref_cfg.argtypes = [P, P, I, D, P]
        lib.carve_ref_pixels.restype = None
        lib.carve_ref_pixels.argtypes = [P, P, I, P, P, P, P]
        lib.carve_ref_image.restype = None
        lib.carve_ref_image.argtypes = [P, P, I, P]
        lib.carve_ref_verdicts.restype = None
        lib.carve_ref_verdicts.argtypes = [P, P, P, I, P, I, P]
        _ref = lib
    return _ref


class HeaderCfg:
    """The header's own QtrCarveCfg for (params, n_scans, voxel_size): .why is its refusal code, .cfg the restatement's Cfg
    read back from the struct's bytes (None where refused)."""

    def __init__(self, p: Params, n_scans: int, voxel_size: float):
        lib = ref()
        self.buf = ctypes.create_string_buffer(lib.carve_ref_cfg_bytes())
        ip = np.array([p.rows, p.cols, p.window, p.min_votes], np.int32)
        dp = np.array([p.fov_up_deg, p.fov_down_deg, p.margin_abs, p.margin_rel, p.min_range, p.max_range], np.float64)
        self.why = int(lib.carve_ref_cfg(ip.ctypes.data, dp.ctypes.data, int(n_scans), float(voxel_size), self.buf))
        self.cfg = None
        if self.why == 0:
            i4 = np.frombuffer(self.buf.raw[:16], np.int32)
            d6 = np.frombuffer(self.buf.raw[16:64], np.float64)
            self.cfg = Cfg(*map(int, i4), *map(float, d6))

    def pixels(self, xyz):
        xyz = np.ascontiguousarray(np.asarray(xyz, np.float64).reshape(-1, 3))
        n = xyz.shape[0]
        ok, r, row, col = np.zeros(n, np.int32), np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int32)
        ref().carve_ref_pixels(self.buf, xyz.ctypes.data, n, ok.ctypes.data, r.ctypes.data, row.ctypes.data, col.ctypes.data)
        return ok.astype(bool), r, row, col

    def image(self, xyz4):
        pts = np.ascontiguousarray(np.asarray(xyz4, np.float32).reshape(-1, 4))
        img = np.zeros((self.cfg.rows, self.cfg.cols), np.uint32)
        ref().carve_ref_image(self.buf, pts.ctypes.data, pts.shape[0], img.ctypes.data)
        return img

    def verdicts(self, poses, imgs, mu):
        P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
        imgs = np.ascontiguousarray(np.asarray(imgs, np.uint32).reshape(P.shape[0], self.cfg.rows, self.cfg.cols))
        mu = np.ascontiguousarray(np.asarray(mu, np.float64).reshape(-1, 3))
        votes = np.zeros((mu.shape[0], P.shape[0]), np.int32)
        ref().carve_ref_verdicts(self.buf, P.ctypes.data, imgs.ctypes.data, P.shape[0], mu.ctypes.data, mu.shape[0], votes.ctypes.data)
        return votes
