"""Inputs the voxel-map tests share (CPU and GPU): the hand-built three-insert case, the crowded table, the positive-octant
clouds on which the map must reproduce method 3, and an independent numpy implementation of the map and its registration."""
import numpy as np

import icp_restate as R
import vmap_restate as M

SIDE = 0.5  # the hand-built case's voxel side: faces k / 2 are exact in binary32
# insert 0 travels under an EXACT pose (a quarter turn about z and an integer shift), so world coordinates on faces and at
# the ends of the grid are what the case says; the other two are general rigid poses
POSES = (R.rigid(np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), [2.0, -3.0, 1.0]),
         R.rigid(R.rot(0.03, -0.05, 0.7), [1.5, -0.25, 0.4]),
         R.rigid(R.rot(-0.4, 0.2, -1.9), [-2.0, 3.0, -0.7]))
V1, V65, V300, VALL = (3, -2, 1), (-4, 5, 0), (2, 2, -3), (-1, -1, 2)
LO, HI = -(1 << 20), (1 << 20) - 1


def _local(P, world):
    """The float32 cloud-frame points whose image under P is (close to) `world`."""
    Pi = np.linalg.inv(P)
    return (np.asarray(world, np.float64) @ Pi[:3, :3].T + Pi[:3, 3]).astype(np.float32)


def hand_built():
    """Three inserts (xyz4, normals4, pose) of 150 + 420 + 130 = 700 points in random storage order on 0.5 m voxels, and 300
    sources.  World voxel V1 gets 1 member (insert 0), V65 65 (insert 1: one wave plus one), V300 300 (insert 1: more than a
    workgroup; 6 more of its points carry unusable normals and are not members), VALL 7 + 9 + 5 from the three inserts; the
    rest is spread over [-3, 3]^3, negative coordinates included.  Insert 0 (exact pose) also carries points on voxel faces,
    one at voxel coordinate -2^20 (exactly on the grid's lowest face) and one at 2^20 - 1, one just outside either end,
    non-finite points and unusable normals.  Returns (inserts, src4, src_normals4)."""
    rng = np.random.default_rng(11)

    def inside(v, n):
        return (np.array(v) + 0.0625 + 0.875 * rng.random((n, 3))) * SIDE

    def spread(n):
        return rng.random((n, 3)) * 6.0 - 3.0

    faces = np.array([[1.0, 0.25, 0.25], [-1.5, -0.5, 0.25], [0.0, 0.0, 0.0], [-0.0, 2.5, -2.0], [0.5, 0.5, 0.5],
                      [-2.0, -2.0, -2.0]])
    ends = np.array([[LO * SIDE, 0.25, 0.25], [0.25, HI * SIDE + 0.25, 0.25], [0.25, 0.25, (HI + 1) * SIDE],
                     [(LO - 1) * SIDE, 0.25, 0.25]])
    world = [np.concatenate([inside(V1, 1), inside(VALL, 7), faces, ends, spread(150 - 1 - 7 - 6 - 4)]),
             np.concatenate([inside(V65, 65), inside(V300, 306), inside(VALL, 9), spread(420 - 65 - 306 - 9)]),
             np.concatenate([inside(VALL, 5), spread(125)])]
    inserts = []
    for j, (W, P) in enumerate(zip(world, POSES)):
        p = _local(P, W)
        n = rng.normal(size=p.shape)
        if j == 0:
            n[8:14] = [0.0, 0.0, 1.0]     # (the face points: members)
            p[20] = [np.nan, 0.0, 0.0]    # non-finite points
            p[21] = [0.0, np.inf, 0.0]
            p[22] = [3e38, 3e38, 3e38]    # finite, but its world position is not
            n[23] = 0.0                   # unusable normals
            n[24] = [np.nan, 1.0, 0.0]
            n[25] = [1.0, -np.inf, 0.0]
        if j == 1:
            n[65 + 300:65 + 306] = 0.0    # V300's six non-members
        if j == 2:
            n[7::31] = 0.0
            p[9] = np.nan
        perm = rng.permutation(p.shape[0])
        inserts.append((R.f4(p[perm]), R.f4(n[perm]), P))
    assert sum(c[0].shape[0] for c in inserts) == 700
    # sources: map points seen from a slightly wrong frame, some on faces, some far from every voxel, some unusable
    allw = np.concatenate([w[np.isfinite(w).all(axis=1)] for w in world])
    allw = allw[np.abs(allw).max(axis=1) < 100.0]
    s = allw[rng.choice(allw.shape[0], 300, replace=True)] + rng.normal(scale=0.02, size=(300, 3))
    s[:5] = [[1.0, 0.25, 0.25], [0.0, 0.0, 0.0], [-1.5, -0.5, 0.25], [0.5, 0.5, 0.5], [-2.0, -2.0, -2.0]]
    s[5:12] = rng.random((7, 3)) * 5.0 + 40.0   # no voxel there
    s[12] = [np.nan, 1.0, 1.0]
    s[13] = [1e30, 1.0, 1.0]
    s[14] = [LO * SIDE, 0.25, 0.25]
    sn = rng.normal(size=(300, 3))
    sn[:5] = [0.0, 0.0, 1.0]
    sn[15::19] = 0.0
    sn[16::23, 2] = np.inf
    return inserts, R.f4(s), R.f4(sn)


GUESS = R.rigid(R.rot(0.01, -0.02, 0.015), [0.03, -0.02, 0.025])


def crowded(capacity=64, n_keys=62, seed=3):
    """n_keys distinct voxel coordinates whose probe chains all start in the last six slots of the device table for this
    capacity (vmap_restate.table_slots): the chains are long and wrap past the table's end.  Found by drawing coordinates
    and keeping those the contract's hash sends there; one more such coordinate for the refused insert and a spare."""
    S = M.table_slots(capacity)
    rng = np.random.default_rng(seed)
    got, seen = [], set()
    while len(got) < n_keys + 4:
        c = tuple(int(x) for x in rng.integers(-200, 200, 3))
        if c in seen:
            continue
        seen.add(c)
        if M.hash_slot(M.key(*c), S) >= S - 6:
            got.append(c)
    return np.array(got[:n_keys]), np.array(got[n_keys:])


def cloud_of_voxels(coords, side, per_voxel=(1, 2, 3), seed=0):
    """Points (and normals) inside the given voxels, per_voxel[k % len] of them in voxel k, in random storage order."""
    rng = np.random.default_rng(seed)
    pts = np.concatenate([(np.array(c) + 0.125 + 0.75 * rng.random((per_voxel[k % len(per_voxel)], 3))) * side
                          for k, c in enumerate(coords)])
    nrm = rng.normal(size=pts.shape)
    perm = rng.permutation(pts.shape[0])
    return R.f4(pts[perm]), R.f4(nrm[perm])


def octant_hand_built():
    """The hand-built positive-octant pair on which the map must reproduce method 3: 500 targets in [0, 6]^3 with one point
    exactly at the origin (the box's minimum: method 3's grid origin is then (0, 0, 0)), a non-finite one and unusable
    normals; 300 sources around them, some outside the box, on faces, unusable.  Side 1.0."""
    rng = np.random.default_rng(21)
    t = rng.random((500, 3)) * 6.0
    t[0] = 0.0
    t[1] = [6.0, 6.0, 6.0]
    t[7] = np.nan
    tn = rng.normal(size=(500, 3))
    tn[3::17] = 0.0
    tn[4::29, 0] = np.nan
    perm = rng.permutation(500)
    s = t[rng.choice(500, 300)] + rng.normal(scale=0.05, size=(300, 3))
    s[:4] = [[1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [6.5, 1.0, 1.0], [-0.25, 3.0, 3.0]]
    s[4] = np.nan
    sn = rng.normal(size=(300, 3))
    sn[5::21] = 0.0
    return R.f4(s), R.f4(sn), R.f4(t[perm]), R.f4(tn[perm])


def into_octant(src4, tgt4):
    """Both clouds shifted by a whole number of metres so that every finite target coordinate is >= 1, then one target
    point exactly at the origin appended (its normal is the caller's to append).  The shift is integral and small, so it is
    applied in binary32 as it stands."""
    t = np.asarray(tgt4, np.float32)
    fin = np.isfinite(t[:, :3]).all(axis=1)
    shift = (1.0 - np.floor(t[fin, :3].min(axis=0))).astype(np.float32)
    s2, t2 = np.array(src4, np.float32), t.copy()
    s2[:, :3] += shift
    t2[:, :3] += shift
    t2 = np.concatenate([t2, np.zeros((1, 4), np.float32)])
    assert t2[np.isfinite(t2[:, :3]).all(axis=1), :3].min() == 0.0
    return R.f4(s2), R.f4(t2)


# ---- an independent numpy implementation (no shared header, no fixed summation order) ---------------------------------
EPS = 1e-3


class NumpyMap:
    """dict keyed by voxel coordinates -> [n, sum X, sum m m^T]; means by np.add.at; inverses by np.linalg.inv."""

    def __init__(self, side):
        self.side, self.vox = float(side), {}

    def insert(self, xyz4, normals4, pose=None):
        P = np.eye(4) if pose is None else np.asarray(pose, np.float64).reshape(4, 4)
        p, a = np.asarray(xyz4, np.float64)[:, :3], np.asarray(normals4, np.float64)[:, :3]
        with np.errstate(all="ignore"):
            la = np.linalg.norm(a, axis=1)
            X = p @ P[:3, :3].T + P[:3, 3]
            ok = np.isfinite(p).all(axis=1) & np.isfinite(a).all(axis=1) & (la > 0) & np.isfinite(X).all(axis=1)
            idx = np.floor(X / self.side)
            ok &= ((idx >= -(1 << 20)) & (idx < (1 << 20))).all(axis=1)
        X, idx = X[ok], idx[ok].astype(np.int64)
        m = (a[ok] / la[ok, None]) @ P[:3, :3].T
        uniq, inv = np.unique(idx, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        n = np.zeros(len(uniq))
        sx = np.zeros((len(uniq), 3))
        smm = np.zeros((len(uniq), 3, 3))
        np.add.at(n, inv, 1.0)
        np.add.at(sx, inv, X)
        np.add.at(smm, inv, m[:, :, None] * m[:, None, :])
        for k, c in enumerate(map(tuple, uniq)):
            old = self.vox.get(c, [0.0, np.zeros(3), np.zeros((3, 3))])
            self.vox[c] = [old[0] + n[k], old[1] + sx[k], old[2] + smm[k]]

    def records(self):
        """coords (sorted by z, y, x: ascending key), counts, means, C_b (3 x 3)."""
        cs = sorted(self.vox, key=lambda c: (c[2], c[1], c[0]))
        n = np.array([self.vox[c][0] for c in cs])
        mu = np.array([self.vox[c][1] / self.vox[c][0] for c in cs])
        Cb = np.array([np.eye(3) - (1 - EPS) * self.vox[c][2] / self.vox[c][0] for c in cs])
        return np.array(cs), n, mu, Cb

    def register(self, src4, src_normals4, guess, iters):
        """`iters` Gauss-Newton iterations of the weighted voxel cost; returns the list of T after each."""
        p, a = np.asarray(src4, np.float64)[:, :3], np.asarray(src_normals4, np.float64)[:, :3]
        with np.errstate(all="ignore"):
            la = np.linalg.norm(a, axis=1)
            use = np.isfinite(p).all(axis=1) & np.isfinite(a).all(axis=1) & (la > 0)
        p, a = p[use], a[use] / la[use, None]
        T = np.asarray(guess, np.float64).reshape(4, 4).copy()
        out = []
        for _ in range(iters):
            Rm, t = T[:3, :3], T[:3, 3]
            q = p @ Rm.T + t
            H, b = np.zeros((6, 6)), np.zeros(6)
            for qi, ai in zip(q, a):
                c = tuple(int(v) for v in np.floor(qi / self.side))
                if c not in self.vox:
                    continue
                N, sx, smm = self.vox[c]
                m = Rm @ ai
                Sigma = (np.eye(3) - (1 - EPS) * smm / N) + (np.eye(3) - (1 - EPS) * np.outer(m, m))
                Mi = np.linalg.inv(Sigma)
                d = qi - sx / N
                K = np.array([[0, -qi[2], qi[1]], [qi[2], 0, -qi[0]], [-qi[1], qi[0], 0]])
                J = np.hstack([-K, np.eye(3)])
                H += N * J.T @ Mi @ J
                b += N * J.T @ Mi @ d
            x = np.linalg.solve(H, -b)
            qv = np.array([1.0, 0.5 * x[0], 0.5 * x[1], 0.5 * x[2]])
            qv /= np.linalg.norm(qv)
            w, xq, yq, zq = qv
            dR = np.array([[1 - 2 * (yq * yq + zq * zq), 2 * (xq * yq - w * zq), 2 * (xq * zq + w * yq)],
                           [2 * (xq * yq + w * zq), 1 - 2 * (xq * xq + zq * zq), 2 * (yq * zq - w * xq)],
                           [2 * (xq * zq - w * yq), 2 * (yq * zq + w * xq), 1 - 2 * (xq * xq + yq * yq)]])
            D = np.eye(4)
            D[:3, :3], D[:3, 3] = dR, x[3:]
            T = D @ T
            out.append(T.copy())
        return out
