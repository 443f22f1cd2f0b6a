"""Named inputs of the grouped map registration (CPU and GPU tests share them).  Every case but the room stands on
vmap_cases.hand_built()'s map (three inserts on 0.5 m voxels inside [-3, 3]^3) and registers small clouds that lie on planes
through that region, with the planes' analytic normals.  A case is (items, icp) with items = [(xyz4, normals4, guess)] and
icp = RefMap.register's keywords where it does not take the defaults; each says what it is there for."""
import numpy as np

import icp_restate as R
import vmap_cases as K

FAR = R.rigid(np.eye(3), [50.0, -40.0, 30.0])  # a guess that puts every point where the map has no voxel


def plane_cloud(n, seed):
    """n points on three planes through the hand-built map's region (z = 0.3, x = -0.8, and the tilted plane through the
    origin with normal (1, 1, 1) / sqrt 3), round robin, with the planes' normals."""
    rng = np.random.default_rng(seed)
    uv = rng.random((n, 2)) * 5.0 - 2.5
    nd = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
    e1, e2 = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0), np.array([1.0, 1.0, -2.0]) / np.sqrt(6.0)
    pts, nrm = np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        u, v = uv[i]
        if i % 3 == 0:
            pts[i], nrm[i] = [u, v, 0.3], [0.0, 0.0, 1.0]
        elif i % 3 == 1:
            pts[i], nrm[i] = [-0.8, u, v], [1.0, 0.0, 0.0]
        else:
            pts[i], nrm[i] = u * e1 + v * e2, nd
    return R.f4(pts), R.f4(nrm)


def small(k):
    """The k-th of a family of small rigid offsets (a few hundredths of a radian and of a metre)."""
    rng = np.random.default_rng(100 + k)
    a, t = rng.uniform(-0.02, 0.02, 3), rng.uniform(-0.04, 0.04, 3)
    return R.rigid(R.rot(*a), t)


SIZES = (0, 1, 255, 256, 257, 700)


def sizes():
    """Item sizes 0, 1, 255, 256, 257 and 700 in one group: chunk edges (one chunk short by one, exactly one, one more than
    one, three with a short last one), an empty item, and the early return of the workgroups past an item's end (the grid is
    three chunks wide for every item)."""
    return [plane_cloud(n, 10 + j) + (small(j),) for j, n in enumerate(SIZES)], {}


def one_cloud_eight_guesses():
    """One cloud of 300 points (two chunks) under eight guesses: shared source arrays, separate states."""
    p, a = plane_cloud(300, 31)
    return [(p, a, small(20 + j)) for j in range(8)], {}


def invalid_beside_good():
    """A guess so far off that no point meets a voxel (n_corr = 0 stays below the minimum) between two good ones: an
    invalid stop inside a group."""
    p, a = plane_cloud(300, 32)
    q, b = plane_cloud(257, 33)
    return [(p, a, small(40)), (q, b, FAR), (q, b, small(41))], {}


def frozen():
    """Guesses of growing offset under transformation_epsilon = 1e-2: the items stop at different updates, and the ones that
    stopped must stay frozen while the others go on."""
    p, a = plane_cloud(700, 34)
    guesses = [np.eye(4), small(50), R.rigid(R.rot(0.0, 0.0, 0.05), [0.1, -0.08, 0.05]),
               R.rigid(R.rot(0.03, -0.04, 0.1), [0.2, 0.15, -0.1]), R.rigid(R.rot(-0.05, 0.05, -0.15), [-0.25, 0.2, 0.15])]
    return [(p, a, g) for g in guesses], {"teps": 1e-2}


CASES = {"sizes": sizes, "one_cloud_eight_guesses": one_cloud_eight_guesses, "invalid_beside_good": invalid_beside_good,
         "frozen": frozen}


def hand_map(make, side=K.SIDE, capacity=4096):
    """make(side, capacity) -> a map (RefMap or the device's) with the hand-built case's three inserts in it."""
    m = make(side, capacity)
    for p, n, pose in K.hand_built()[0]:
        m.insert(p, n, pose)
    return m


# ---- the room ----------------------------------------------------------------------------------------------------------
ROOM_SIDE = 1.0
ROOM_ORIGIN = np.array([0.41, 0.33, 0.37])  # (off the voxel faces, so that a surface's noise does not straddle two layers)


def _room_points(n, rng):
    """n points on the room's surfaces in the world frame with their normals: a 10 x 8 m floor, the walls x = 0 and y = 0
    (3 m high) and a 2 x 2 x 1.5 m box standing on the floor, all shifted by ROOM_ORIGIN; 1 cm of noise along the normal."""
    faces = [  # (origin, edge u, edge v, normal)
        ([0, 0, 0], [10, 0, 0], [0, 8, 0], [0, 0, 1]),
        ([0, 0, 0], [0, 8, 0], [0, 0, 3], [1, 0, 0]),
        ([0, 0, 0], [10, 0, 0], [0, 0, 3], [0, 1, 0]),
        ([6, 4, 1.5], [2, 0, 0], [0, 2, 0], [0, 0, 1]),
        ([6, 4, 0], [0, 2, 0], [0, 0, 1.5], [-1, 0, 0]),
        ([8, 4, 0], [0, 2, 0], [0, 0, 1.5], [1, 0, 0]),
        ([6, 4, 0], [2, 0, 0], [0, 0, 1.5], [0, -1, 0]),
        ([6, 6, 0], [2, 0, 0], [0, 0, 1.5], [0, 1, 0])]
    area = np.array([np.linalg.norm(np.cross(f[1], f[2])) for f in faces])
    which = rng.choice(len(faces), n, p=area / area.sum())
    uv = rng.random((n, 2))
    pts, nrm = np.zeros((n, 3)), np.zeros((n, 3))
    for i, f in enumerate(which):
        o, eu, ev, nn = (np.array(x, np.float64) for x in faces[f])
        pts[i] = o + uv[i, 0] * eu + uv[i, 1] * ev + rng.normal(scale=0.01) * nn
        nrm[i] = nn
    return pts + ROOM_ORIGIN, nrm


def _view(pose, n, seed):
    """What a sensor at `pose` (sensor frame -> world) holds of the room: n surface points and their normals in its frame."""
    pts, nrm = _room_points(n, np.random.default_rng(seed))
    Pi = np.linalg.inv(pose)
    return R.f4(pts @ Pi[:3, :3].T + Pi[:3, 3]), R.f4(nrm @ Pi[:3, :3].T)


ROOM_POSES = (R.rigid(R.rot(0.01, -0.02, 0.3), [3.0, 2.5, 1.2]), R.rigid(R.rot(-0.02, 0.01, -1.1), [6.5, 2.0, 1.3]),
              R.rigid(R.rot(0.015, 0.02, 2.4), [4.0, 6.0, 1.1]))
ROOM_TRUE = R.rigid(R.rot(0.02, -0.01, 0.8), [5.2, 3.4, 1.25])  # the query's pose
# where the search starts: the truth turned by 0.05 rad and moved by (0.45, -0.35) m in its own xy plane, so that no
# hypothesis of the grid below starts at the truth (the nearest one is 0.57 m off)
ROOM_YAWS = (-0.15, 0.0, 0.15)
ROOM_OFFSETS = tuple((dx * ROOM_SIDE, dy * ROOM_SIDE) for dx in (-1.0, 0.0, 1.0) for dy in (-1.0, 0.0, 1.0))


def room():
    """The room scene: inserts (three views of about 2 000 points under their poses), the query view (taken at ROOM_TRUE), and
    the 27 hypotheses = 3 yaws x 3 x 3 offsets one voxel side apart around a base that is off the truth.  Returns (inserts,
    (xyz4, normals4), hypotheses [27, 4, 4])."""
    from quatro_amd import api
    inserts = [_view(P, 2000, 70 + j) + (P,) for j, P in enumerate(ROOM_POSES)]
    query = _view(ROOM_TRUE, 2000, 77)
    base = api.pose_hypothesis(ROOM_TRUE, 0.05, 0.45, -0.35)
    return inserts, query, api.pose_hypotheses(base, ROOM_YAWS, ROOM_OFFSETS)


def room_map(make, capacity=4096):
    m = make(ROOM_SIDE, capacity)
    for p, n, pose in room()[0]:
        m.insert(p, n, pose)
    return m
