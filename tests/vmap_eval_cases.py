"""Named inputs of the evaluation of poses against the voxel map (CPU and GPU tests share them).  A case is a function that
returns (build, items): build(make) fills and returns a map made by make(side, capacity) — vmap_restate.RefMap or the
device's Handle.voxel_map — and items = [(xyz4, normals4, T)].  PREDICATES[name](items, evals) takes the restatement's
evaluations of the items and asserts the branch the case is there for."""
import numpy as np

import icp_restate as R
import vmap_batch_cases as BC
import vmap_cases as K
import vmap_restate as M


def _hand(make):
    return BC.hand_map(make)


# ---- sizes ---------------------------------------------------------------------------------------------------------------
def sizes():
    """Item sizes 0, 1, 255, 256, 257 and 700 in one group on the hand-built map: chunk counts 0, 1, 1, 1, 2, 3 under a grid
    three chunks wide — the grouped grid, the early return of the workgroups past an item's end, and the ticket."""
    return _hand, BC.sizes()[0]


def _p_sizes(items, evals):
    assert tuple(p.shape[0] for p, _, _ in items) == BC.SIZES
    assert [-(-p.shape[0] // 256) for p, _, _ in items] == [0, 1, 1, 1, 2, 3]
    assert not evals[0]["valid"] and evals[0]["n_source"] == 0 and not evals[0]["information"].any()
    assert all(e["n_source"] == p.shape[0] for e, (p, _, _) in zip(evals, items))
    assert all(e["valid"] and e["n_corr"] >= 40 for e in evals[2:]) and evals[5]["n_corr"] > evals[4]["n_corr"]


# ---- every kind of unmatched point -----------------------------------------------------------------------------------------
def _open_face_voxel():
    """A voxel of the hand-built map whose +x neighbour does not exist (the lowest key of those)."""
    have = {tuple(c) for c in BC.hand_map(M.RefMap).fetch(M.COORDS)}
    return next(c for c in sorted(have, key=lambda c: (c[2], c[1], c[0])) if (c[0] + 1, c[1], c[2]) not in have)


UNMATCHED_ROWS = ("non-finite point", "unusable normal", "voxel coordinate 2^20", "empty voxel", "on the face of a missing voxel",
                  "on the face of an existing voxel", "inside V300", "inside V65")


def unmatched_kinds():
    """One cloud at the identity on the hand-built map, one point per row of UNMATCHED_ROWS: a non-finite point (not
    considered), a finite point with a zero normal (considered, unmatched), q at voxel coordinate 2^20 (outside the grid), q in
    an empty voxel, q exactly on the face k c between an existing voxel and a missing one (it belongs to the missing one),
    q exactly on a face of an existing voxel (matched: a face belongs to the voxel above it), and two plainly matched points."""
    c = K.SIDE
    v = _open_face_voxel()
    pts = np.array([[np.nan, 0.25, 0.25],
                    [(K.V300[0] + 0.5) * c, (K.V300[1] + 0.5) * c, (K.V300[2] + 0.5) * c],
                    [float(1 << 20) * c, 0.25, 0.25],
                    [40.1, 40.2, 40.3],
                    [(v[0] + 1) * c, (v[1] + 0.5) * c, (v[2] + 0.5) * c],
                    [1.0, 0.25, 0.25],
                    [(K.V300[0] + 0.25) * c, (K.V300[1] + 0.5) * c, (K.V300[2] + 0.75) * c],
                    [(K.V65[0] + 0.5) * c, (K.V65[1] + 0.25) * c, (K.V65[2] + 0.5) * c]])
    nrm = np.tile([0.0, 0.6, 0.8], (len(pts), 1))
    nrm[1] = 0.0
    return _hand, [(R.f4(pts), R.f4(nrm), np.eye(4))]


def _p_unmatched(items, evals):
    e = evals[0]
    assert (e["n_source"], e["n_corr"]) == (7, 3), (e["n_source"], e["n_corr"])
    assert list(e["corr"]) == [-1, -1, -1, -1, -1, 0, 0, 0]
    assert np.all(e["point"][:5] == 0.0) and np.all(e["point"][5:, 1] > 0.0)
    assert e["point"][6, 1] == 300.0 and e["point"][7, 1] == 65.0  # (the weight is the voxel's member count)


# ---- nothing matched, everything matched -------------------------------------------------------------------------------
AWAY = R.rigid(np.eye(3), [70.0, 0.0, 0.0])


def all_unmatched():
    """A 300-point cloud under a pose 70 m away: valid is 0 and the record is all zeros but n_source."""
    p, a = BC.plane_cloud(300, 61)
    return _hand, [(p, a, AWAY)]


def _p_all_unmatched(items, evals):
    e = evals[0]
    assert not e["valid"] and e["n_source"] == 300 and e["n_corr"] == 0 and np.all(e["corr"] == -1)
    assert all(not np.any(e[k]) for k in ("overlap", "sum_d2", "inlier_rmse", "sum_w", "chi2", "rmse", "information", "hessian", "gradient"))
    assert e["S"][41] == 300.0 and not e["S"][:41].any()


def all_matched():
    """The map's own voxel means (those whose binary32 image lies clearly inside its voxel) at the identity: every point is
    matched, overlap is exactly 1."""
    cloud = BC.hand_map(M.RefMap).fetch(M.CLOUD)[:, :3].astype(np.float64)
    f = cloud / K.SIDE - np.floor(cloud / K.SIDE)
    pts = cloud[((f > 0.01) & (f < 0.99)).all(axis=1)]
    return _hand, [(R.f4(pts), R.f4(np.tile([0.0, 0.0, 1.0], (len(pts), 1))), np.eye(4))]


def _p_all_matched(items, evals):
    e, n = evals[0], items[0][0].shape[0]
    assert n > 256 and e["valid"] and e["n_source"] == n and e["n_corr"] == n and e["overlap"] == 1.0 and np.all(e["corr"] == 0)
    assert e["inlier_rmse"] < 1e-6 and e["information"][5, 5] == n


# ---- the room ------------------------------------------------------------------------------------------------------------
def room():
    """The room of vmap_batch_cases: the query view under the 27 hypotheses, and under its true pose (item 27)."""
    _, (q, qa), hyp = BC.room()
    return BC.room_map, [(q, qa, g) for g in hyp] + [(q, qa, BC.ROOM_TRUE)]


def room_rank(evals, results):
    """Where the full registration batch's winner stands in the order of the 27 scores (1 = first)."""
    from quatro_amd import api
    return api.evaluation_order(evals[:27]).index(api.best_hypothesis(results)) + 1


ROOM_KEEP_LIMIT = 13  # relocalize(keep=) is only worth having when the winner stands no worse than this among 27
ROOM_RANK = 8         # where it stands (test_vmap_eval_cpu.test_room_winner_stands_among_the_first_scores holds it there)
ROOM_KEEP = 9         # ... rounded up to the next multiple of 3: what the GPU test passes as keep


def _p_room(items, evals):
    assert len(items) == 28 and all(it[0] is items[0][0] for it in items)
    true = evals[27]
    assert true["valid"] and true["overlap"] > 0.9 and true["inlier_rmse"] < 0.5
    assert all(e["n_corr"] <= true["n_corr"] for e in evals[:27])  # no hypothesis explains more of the scan than the truth
    assert len({e["n_corr"] for e in evals[:27]}) > 5  # and the scores do tell them apart


# ---- the corridor --------------------------------------------------------------------------------------------------------
COR_SIDE = 1.0
COR_ORIGIN = np.array([0.41, 0.33, 0.37])
COR_POSES = (R.rigid(R.rot(0.01, -0.01, 0.05), [4.0, 2.0, 1.2]), R.rigid(R.rot(-0.01, 0.02, -0.08), [10.0, 1.8, 1.3]),
             R.rigid(R.rot(0.02, 0.01, 3.1), [16.0, 2.2, 1.1]))
COR_TRUE = R.rigid(R.rot(0.015, -0.02, 0.1), [8.5, 2.1, 1.25])


def _corridor_view(pose, n, seed):
    """n points of a corridor along x (a 20 x 4 m floor and the walls y = 0 and y = 4, 3 m high, shifted by COR_ORIGIN; 1 cm
    of noise along the normal) with their normals, in the frame of a sensor at `pose`."""
    rng = np.random.default_rng(seed)
    faces = [([0, 0, 0], [20, 0, 0], [0, 4, 0], [0, 0, 1]), ([0, 0, 0], [20, 0, 0], [0, 0, 3], [0, 1, 0]),
             ([0, 4, 0], [20, 0, 0], [0, 0, 3], [0, -1, 0])]
    area = np.array([np.linalg.norm(np.cross(f[1], f[2])) for f in faces])
    which = rng.choice(len(faces), n, p=area / area.sum())
    uv = rng.random((n, 2))
    pts, nrm = np.zeros((n, 3)), np.zeros((n, 3))
    for i, f in enumerate(which):
        o, eu, ev, nn = (np.array(x, np.float64) for x in faces[f])
        pts[i] = o + uv[i, 0] * eu + uv[i, 1] * ev + rng.normal(scale=0.01) * nn
        nrm[i] = nn
    pts = pts + COR_ORIGIN
    Pi = np.linalg.inv(pose)
    return R.f4(pts @ Pi[:3, :3].T + Pi[:3, 3]), R.f4(nrm @ Pi[:3, :3].T)


def corridor_map(make, capacity=4096):
    m = make(COR_SIDE, capacity)
    for j, P in enumerate(COR_POSES):
        p, a = _corridor_view(P, 2000, 80 + j)
        m.insert(p, a, P)
    return m


def corridor():
    """A floor and two parallel walls along x: a map of three views and a query view at its true pose.  Nothing in the scene
    fixes x, and the registration's normal matrix must say so."""
    return corridor_map, [_corridor_view(COR_TRUE, 1500, 87) + (COR_TRUE,)]


def _p_corridor(items, evals):
    from quatro_amd import api
    e = evals[0]
    assert e["valid"] and e["overlap"] > 0.9
    d = api.degeneracy(e)
    w, tv = d["weakest_translation"], d["translation_eigenvalues"]
    ang = np.degrees(np.arccos(min(1.0, abs(float(w[0])))))
    print(f"corridor: weakest translation {w}, {ang:.3f} deg off x; translation eigenvalues {tv}; condition {d['condition']:.3g}")
    assert ang < 5.0 and tv[0] < 0.1 * tv[1]
    assert abs(np.linalg.norm(w) - 1.0) < 1e-12 and d["eigenvalues"].shape == (6,) and np.all(np.diff(d["eigenvalues"]) >= 0)


# ---- the crowded table -----------------------------------------------------------------------------------------------------
def _crowded_map(make):
    coords, _ = K.crowded(64, 62)
    m = make(1.0, 64)
    m.insert(*K.cloud_of_voxels(coords, 1.0))
    return m


def crowded():
    """A capacity-64 map whose 62 voxels all start their probe chains in the table's last six slots, so the chains are long
    and wrap; the cloud has points in every second of them and in four voxels with the same home slots that are not in the
    map: lookups at chain ends, and misses that walk to an empty slot."""
    coords, extra = K.crowded(64, 62)
    s, sn = K.cloud_of_voxels(np.concatenate([coords[::2], extra]), 1.0, per_voxel=(3,), seed=8)
    return _crowded_map, [(s, sn, R.rigid(np.eye(3), [0.01, 0.02, -0.01]))]  # (a shift that keeps every point in its voxel)


def _p_crowded(items, evals):
    coords, extra = K.crowded(64, 62)
    S = M.table_slots(64)
    assert S == 128 and all(M.hash_slot(M.key(*c), S) >= S - 6 for c in np.concatenate([coords, extra]))
    e = evals[0]
    assert e["n_source"] == 3 * (31 + len(extra)) and e["n_corr"] == 3 * 31  # (the extra voxels' points find no voxel)
    assert (e["corr"] == -1).sum() == 3 * len(extra)


CASES = {"sizes": sizes, "unmatched_kinds": unmatched_kinds, "all_unmatched": all_unmatched, "all_matched": all_matched,
         "room": room, "corridor": corridor, "crowded": crowded}
PREDICATES = {"sizes": _p_sizes, "unmatched_kinds": _p_unmatched, "all_unmatched": _p_all_unmatched,
              "all_matched": _p_all_matched, "room": _p_room, "corridor": _p_corridor, "crowded": _p_crowded}
