"""The host restatement of the voxel map's upkeep (tests/vmap_ref/vmap_keep_ref.cpp against include/qtr_vmap_keep_math.h),
compiled on first use with g++ -ffp-contract=off and driven through ctypes: RefMap adds evict and restore to
vmap_restate.RefMap (mirroring quatro_amd.lib.VoxelMap), odometry mirrors quatro_amd.api.scan_to_map_odometry with its
window.  Beside it an independent model in plain Python: DictMap, a dict keyed by coordinate triples whose window rule is
written with Python integers."""
import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np

import vmap_restate as M

ROOT = M.ROOT
BAD_ARG, CAPACITY = 2, 3  # QTR_ERR_BAD_ARG, QTR_ERR_CAPACITY
_lib = None


def load():
    global _lib
    if _lib is None:
        M.load()
        out = os.path.join(tempfile.mkdtemp(prefix="vmap_keep_ref_"), "libvmap_keep_ref.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                               "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "vmap_ref", "vmap_keep_ref.cpp"), "-o", out])
        lib = ctypes.CDLL(out)
        P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        lib.vmap_keep_window.argtypes = [P, D, D, P, P]
        lib.vmap_keep_verdict.argtypes = [P, D, D, P]
        lib.vmap_keep_evict.argtypes = [P, P, D, P, P]
        lib.vmap_keep_restore.argtypes = [P, P, P, P, I, P]
        _lib = lib
    return _lib


class BadArgError(ValueError):
    pass


def _c3(centre):
    return np.ascontiguousarray(np.asarray(centre, np.float64).reshape(3))


def window(centre, radius, side):
    """((Cx, Cy, Cz), R^2) of the header's window, or None where it is refused."""
    c, C3, R2 = _c3(centre), np.zeros(3, np.int32), ctypes.c_longlong(0)
    if not load().vmap_keep_window(c.ctypes.data, float(radius), float(side), C3.ctypes.data, ctypes.byref(R2)):
        return None
    return tuple(int(x) for x in C3), int(R2.value)


def verdict(centre, radius, side, coords):
    """The header's verdict on one voxel: True kept, False evicted, None the window is refused."""
    c, i = _c3(centre), np.ascontiguousarray(np.asarray(coords, np.int32).reshape(3))
    v = load().vmap_keep_verdict(c.ctypes.data, float(radius), float(side), i.ctypes.data)
    return None if v < 0 else bool(v)


class RefMap(M.RefMap):
    def evict(self, centre, radius) -> dict:
        c, info, members = _c3(centre), np.zeros(2, np.int32), ctypes.c_longlong(0)
        rc = load().vmap_keep_evict(self._m, c.ctypes.data, float(radius), info.ctypes.data, ctypes.byref(members))
        if rc != 0:
            raise BadArgError(f"window ({centre}, {radius}) refused")
        self.n_members -= int(members.value)
        return {"n_kept": int(info[0]), "n_evicted": int(info[1]), "n_members_evicted": int(members.value)}

    def restore(self, coords, count, sums) -> None:
        coords = np.ascontiguousarray(coords, np.int32).reshape(-1, 3)
        count = np.ascontiguousarray(count, np.int32).reshape(-1)
        sums = np.ascontiguousarray(sums, np.float64).reshape(-1, 9)
        assert coords.shape[0] == count.shape[0] == sums.shape[0]
        members = ctypes.c_longlong(0)
        was_empty = len(self) == 0
        rc = load().vmap_keep_restore(self._m, coords.ctypes.data, count.ctypes.data, sums.ctypes.data, coords.shape[0],
                                      ctypes.byref(members))
        if rc == CAPACITY:
            raise M.CapacityError(f"n={coords.shape[0]} exceeds capacity={self.capacity}")
        if rc != 0:
            if was_empty:
                self.n_members = 0
            raise BadArgError("restore refused")
        self.n_members, self.n_inserts = int(members.value), 0


# ---- an independent model: no shared header, Python integers --------------------------------------------------------------
def window_py(centre, radius, side):
    """The issue's window in Python: C_k = floor(c_k / side), R = floor(radius / side); None where it is refused."""
    c = [float(x) for x in np.asarray(centre, np.float64).reshape(3)]
    radius, side = float(radius), float(side)
    if not all(math.isfinite(x) for x in c) or not math.isfinite(radius) or radius < 0:
        return None
    C = [math.floor(x / side) for x in c]  # (an exact integer of the rounded quotient, as floor() of a double is)
    if not all(-(1 << 20) <= k < (1 << 20) for k in C):
        return None
    q = radius / side
    if not math.isfinite(q):
        return None
    R = math.floor(q)
    if R >= 1 << 22:
        return None
    return tuple(C), R * R


def kept_py(win, coords) -> bool:
    C, R2 = win
    return sum((int(i) - int(k)) ** 2 for i, k in zip(coords, C)) <= R2


class DictMap:
    """{(ix, iy, iz): (count, sums bytes)} built from fetched sections; evict by window_py / kept_py."""

    def __init__(self, side, sections=None):
        self.side, self.vox = float(side), {}
        if sections is not None:
            for c, n, s in zip(sections[M.COORDS], sections[M.COUNT], sections[M.SUMS]):
                self.vox[tuple(int(x) for x in c)] = (int(n), np.array(s, np.float64).tobytes())

    def evict(self, centre, radius):
        win = window_py(centre, radius, self.side)
        if win is None:
            raise BadArgError("refused")
        gone = [c for c in self.vox if not kept_py(win, c)]
        members = sum(self.vox[c][0] for c in gone)
        for c in gone:
            del self.vox[c]
        return {"n_kept": len(self.vox), "n_evicted": len(gone), "n_members_evicted": members}

    def sections(self):
        cs = sorted(self.vox, key=lambda c: (c[2], c[1], c[0]))  # ascending key
        return {M.COORDS: np.array(cs, np.int32).reshape(-1, 3), M.COUNT: np.array([self.vox[c][0] for c in cs], np.int32),
                M.SUMS: np.array([np.frombuffer(self.vox[c][1], np.float64) for c in cs], np.float64).reshape(-1, 9)}


def odometry(clouds, normals, voxel_size=1.0, capacity=1 << 20, window_radius=None, **icp):
    """quatro_amd.api.scan_to_map_odometry restated with its window on already voxelised clouds with their normals; returns
    (poses, RefMap, results, sizes): sizes[k] = the map's voxels after insert k, before its eviction (what capacity must hold)."""
    m = RefMap(voxel_size, capacity)
    poses, results, sizes = [], [], []
    for k, (c, n) in enumerate(zip(clouds, normals)):
        if k == 0:
            T = np.eye(4)
        else:
            guess = poses[-1] if k == 1 else M.constant_velocity_guess(poses[-2], poses[-1])
            r = m.register(c, n, guess, **icp)
            results.append(r)
            T = r["T"].copy() if r["valid"] else np.array(guess, np.float64)
        m.insert(c, n, T)
        sizes.append(len(m))
        if window_radius is not None:
            m.evict(T[:3, 3], window_radius)
        poses.append(T)
    return np.stack(poses), m, results, sizes
