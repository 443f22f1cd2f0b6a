"""The host restatement of the device voxel map (tests/vmap_ref/vmap_ref.cpp against include/qtr_vmap_math.h), compiled on
first use with g++ -ffp-contract=off and driven through ctypes: RefMap mirrors quatro_amd.lib.VoxelMap, odometry mirrors
quatro_amd.api.scan_to_map_odometry."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from icp_restate import f4

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CAPACITY = 3  # QTR_ERR_CAPACITY
COORDS, COUNT, SUMS, RECORDS, CLOUD = 1, 2, 3, 4, 5
_lib = None


def load():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="vmap_ref_"), "libvmap_ref.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                               "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "vmap_ref", "vmap_ref.cpp"),
                               "-o", out])
        lib = ctypes.CDLL(out)
        P, I, D, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_ulonglong
        lib.vmap_ref_new.restype = P
        lib.vmap_ref_new.argtypes = [D, I]
        lib.vmap_ref_free.restype = None
        lib.vmap_ref_free.argtypes = [P]
        lib.vmap_ref_clear.restype = None
        lib.vmap_ref_clear.argtypes = [P]
        lib.vmap_ref_size.argtypes = [P]
        lib.vmap_ref_hash.restype = U
        lib.vmap_ref_hash.argtypes = [U, U]
        lib.vmap_ref_key.restype = U
        lib.vmap_ref_key.argtypes = [I, I, I]
        lib.vmap_ref_coord.argtypes = [D, D, P]
        lib.vmap_ref_insert.argtypes = [P, P, P, I, P, P]
        lib.vmap_ref_fetch.restype = None
        lib.vmap_ref_fetch.argtypes = [P, P, P, P, P, P]
        lib.vmap_ref_register.restype = None
        lib.vmap_ref_register.argtypes = [P, P, I, P, P, D, D, I, I, P, P, P, P, P, I]
        _lib = lib
    return _lib


def coord(x: float, c: float):
    """The voxel coordinate of world coordinate x on a grid of side c, or None outside the grid."""
    i = ctypes.c_int(0)
    return i.value if load().vmap_ref_coord(float(x), float(c), ctypes.byref(i)) else None


def key(ix: int, iy: int, iz: int) -> int:
    return int(load().vmap_ref_key(int(ix), int(iy), int(iz)))


def hash_slot(k: int, n_slots: int) -> int:
    """Where key k's probe chain starts in a table of n_slots slots (a power of two)."""
    return int(load().vmap_ref_hash(int(k), int(n_slots) - 1))


def table_slots(capacity: int) -> int:
    """The device table's slot count for a capacity: the power of two >= max(64, 2 x capacity)."""
    s = 64
    while s < 2 * capacity:
        s <<= 1
    return s


class CapacityError(RuntimeError):
    pass


class RefMap:
    def __init__(self, voxel_size=1.0, capacity=1 << 20):
        self.voxel_size, self.capacity = float(voxel_size), int(capacity)
        self._m = ctypes.c_void_p(load().vmap_ref_new(self.voxel_size, self.capacity))
        self.n_inserts, self.n_members = 0, 0

    def __del__(self):
        if getattr(self, "_m", None):
            load().vmap_ref_free(self._m)
            self._m = None

    def __len__(self):
        return int(load().vmap_ref_size(self._m))

    def clear(self):
        load().vmap_ref_clear(self._m)
        self.n_inserts, self.n_members = 0, 0

    def insert(self, xyz4, normals4, pose=None) -> dict:
        pts, nrm = f4(xyz4), f4(normals4)
        assert pts.shape == nrm.shape
        P = None if pose is None else np.ascontiguousarray(np.asarray(pose, np.float64).reshape(16))
        info = np.zeros(4, np.int32)
        rc = load().vmap_ref_insert(self._m, pts.ctypes.data, nrm.ctypes.data, pts.shape[0],
                                    None if P is None else P.ctypes.data, info.ctypes.data)
        if rc != 0:
            raise CapacityError(f"{int(info[2])} new voxels on top of {len(self)} exceed capacity={self.capacity}")
        self.n_inserts += 1
        self.n_members += int(info[1])
        return dict(zip(("n_points", "n_members", "n_new_voxels", "n_touched_voxels"), map(int, info)))

    def fetch_all(self) -> dict:
        n = len(self)
        out = {COORDS: np.zeros((n, 3), np.int32), COUNT: np.zeros(n, np.int32), SUMS: np.zeros((n, 9)),
               RECORDS: np.zeros((n, 9)), CLOUD: np.zeros((n, 4), np.float32)}
        load().vmap_ref_fetch(self._m, *[out[k].ctypes.data for k in (COORDS, COUNT, SUMS, RECORDS, CLOUD)])
        return out

    def fetch(self, what=CLOUD) -> np.ndarray:
        return self.fetch_all()[what]

    def info(self) -> dict:
        return {"voxel_size": self.voxel_size, "capacity": self.capacity, "n_voxels": len(self),
                "n_inserts": self.n_inserts, "n_members": self.n_members}

    def register(self, src, src_nrm, guess=None, teps=1e-7, feps=1e-6, max_iter=30, min_corr=0, corr_iter=-1) -> dict:
        """The restated loop; a dict shaped like lib.VoxelMap.register's plus 'trace' (iterations x 18) and 'corr' (0 matched,
        -1 none, at evaluation corr_iter; < 0: the last)."""
        src, nrm = f4(src), f4(src_nrm)
        assert src.shape == nrm.shape
        g = np.ascontiguousarray(np.eye(4) if guess is None else np.asarray(guess, np.float64).reshape(4, 4))
        T, info, fr = np.zeros(16), np.zeros(5, np.int32), np.zeros(2)
        trace = np.zeros((max_iter, 18))
        corr = np.full(max(src.shape[0], 1), -1, np.int32)
        load().vmap_ref_register(self._m, src.ctypes.data, src.shape[0], nrm.ctypes.data, g.ctypes.data, teps, feps, max_iter,
                                 min_corr, T.ctypes.data, info.ctypes.data, fr.ctypes.data, trace.ctypes.data, corr.ctypes.data,
                                 corr_iter)
        it = int(info[0])
        return {"status": 0, "T": T.reshape(4, 4), "iterations": it, "stop_reason": int(info[1]), "valid": bool(info[2]),
                "converged": bool(info[3]), "n_corr": int(info[4]), "fitness": fr[0], "rmse": fr[1],
                "trace": trace[:it].copy(), "corr": corr[:src.shape[0]].copy()}


def constant_velocity_guess(T2, T1):
    """quatro_amd.api.constant_velocity_guess restated: T1 (T2^-1 T1), rigid inverse, fixed order, Python floats."""
    A = [[float(x) for x in r] for r in np.asarray(T2, np.float64).reshape(4, 4)]
    B = [[float(x) for x in r] for r in np.asarray(T1, np.float64).reshape(4, 4)]
    inv = [[A[c][r] for c in range(3)] + [-((A[0][r] * A[0][3] + A[1][r] * A[1][3]) + A[2][r] * A[2][3])] for r in range(3)]
    inv.append([0.0, 0.0, 0.0, 1.0])

    def mul(X, Y):
        return [[((X[r][0] * Y[0][c] + X[r][1] * Y[1][c]) + X[r][2] * Y[2][c]) + X[r][3] * Y[3][c] for c in range(4)]
                for r in range(4)]

    G = mul(B, mul(inv, B))
    G[3] = [0.0, 0.0, 0.0, 1.0]
    return np.array(G, np.float64)


def odometry(clouds, normals, voxel_size=1.0, capacity=1 << 20, **icp):
    """quatro_amd.api.scan_to_map_odometry restated on already voxelised clouds with their normals; returns
    (poses, RefMap, results)."""
    m = RefMap(voxel_size, capacity)
    poses, results = [], []
    for k, (c, n) in enumerate(zip(clouds, normals)):
        if k == 0:
            T = np.eye(4)
        else:
            guess = poses[-1] if k == 1 else constant_velocity_guess(poses[-2], poses[-1])
            r = m.register(c, n, guess, **icp)
            results.append(r)
            T = r["T"].copy() if r["valid"] else np.array(guess, np.float64)
        m.insert(c, n, T)
        poses.append(T)
    return np.stack(poses), m, results
