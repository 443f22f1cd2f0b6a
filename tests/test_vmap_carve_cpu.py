"""The contract of the voxel map's visibility carving (include/qtr_vmap_carve_math.h) on the host: the header under g++
(tests/vmap_carve_ref/vmap_carve_ref.cpp) against the numpy restatement (tests/vmap_carve_restate.py) bit for bit on the
named cases, the pixel function against an independent numpy model (np.arctan2, np.hypot), the named edge cases, the
refusals, what a carve does to a map, the quality of the rule on a scene with a moving box, and the header's entry points in
the extension library's symbol table."""
import numpy as np
import pytest

import icp_restate as R
import vmap_carve_cases as CC
import vmap_carve_restate as CR
import vmap_cases as K
import vmap_restate as M

SECTIONS = (M.COORDS, M.COUNT, M.SUMS, M.RECORDS, M.CLOUD)
F32 = np.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_sections(fa, fb, what=""):
    for k in SECTIONS:
        assert fa[k].shape == fb[k].shape and np.array_equal(_bits(fa[k]), _bits(fb[k])), (what, k)


def _hand_map(capacity=4096):
    inserts, _, _ = K.hand_built()
    m = CR.RefMap(K.SIDE, capacity)
    for c in inserts:
        m.insert(*c)
    return m


def _same_pixels(a, b, what=""):
    (ok_a, r_a, row_a, col_a), (ok_b, r_b, row_b, col_b) = a, b
    assert np.array_equal(ok_a, ok_b), what
    assert np.array_equal(_bits(r_a[ok_a]), _bits(r_b[ok_a])), what
    assert np.array_equal(row_a[ok_a], row_b[ok_a]) and np.array_equal(col_a[ok_a], col_b[ok_a]), what


PARAM_SETS = (CR.Params(), CR.Params(**CC.WIDE), CR.Params(**CC.TINY), CR.Params(rows=1, cols=8, window=0),
              CR.Params(rows=256, cols=4096, window=3, fov_up_deg=15.0, fov_down_deg=-24.8, margin_abs=0.3, margin_rel=0.01),
              CR.Params(rows=37, cols=1001, window=1, min_range=0.0, max_range=1e6))


def test_header_and_restatement_agree_bit_for_bit():
    rng = np.random.default_rng(3)
    hand = _hand_map().fetch_all()
    mu = hand[M.RECORDS][:, :3]
    for p in PARAM_SETS:
        h = CR.HeaderCfg(p, 3, K.SIDE)
        c = CR.cfg_make(p, 3, K.SIDE)
        assert h.why == 0 and h.cfg == c, p                      # the checked parameters, every double the same bits
        pts = np.concatenate([rng.normal(scale=s, size=(4000, 3)) for s in (0.5, 5.0, 50.0)])
        pts[::97] = np.round(pts[::97])                           # axes, planes, exact diagonals
        pts[::89, 2] = 0.0
        pts[::83, 1] = 0.0
        pts[::101, :2] = 0.0
        pts[5] = [np.nan, 1, 1]
        pts[6] = [1, -np.inf, 1]
        _same_pixels(h.pixels(pts), CR.pixels(c, pts), p)
        pts32 = pts.astype(F32).astype(np.float64)
        _same_pixels(h.pixels(pts32), CR.pixels(c, pts32), p)
        clouds, poses = CC.hand_scans(hand[M.CLOUD], n_scans=3)
        clouds.append(CC.raster_scan(p, 9, r_lo=1.5, r_hi=12.0))
        poses = np.concatenate([poses, R.rigid(R.rot(0.01, 0.02, 1.0), [0.2, 0.1, 0.0])[None]])
        imgs = np.stack([CR.image(c, cl) for cl in clouds])
        assert np.array_equal(imgs, np.stack([h.image(cl) for cl in clouds])), p
        votes = CR.carve_votes(c, clouds, poses, mu)
        assert np.array_equal(votes, h.verdicts(poses, imgs, mu)), p
        if p.rows >= 16:
            assert all((votes == v).sum() > 0 for v in (CR.NO_VOTE, CR.OCCUPIED, CR.SEEN_THROUGH)), (p, np.bincount(votes.ravel()))


def test_pixel_function_against_an_independent_model():
    """np.arctan2 / np.hypot / np.floor in the obvious formula.  Rows and columns may differ from the contract's only where the
    model's own angle lies within EDGE (1e-9 of a pixel) of a pixel edge; the share of such points is printed and bounded."""
    EDGE = 1e-9
    rng = np.random.default_rng(8)
    n_all = n_near = 0
    for p in PARAM_SETS:
        c = CR.cfg_make(p, 1, 1.0)
        pts = np.concatenate([rng.normal(scale=s, size=(20000, 3)) for s in (1.0, 10.0, 40.0)]).astype(F32).astype(np.float64)
        ok, r, row, col = CR.pixels(c, pts)
        up, down = np.deg2rad(p.fov_up_deg), np.deg2rad(p.fov_down_deg)
        rm = np.sqrt((pts ** 2).sum(axis=1))
        fr = (up - np.arctan2(pts[:, 2], np.hypot(pts[:, 0], pts[:, 1]))) * p.rows / (up - down)
        fc = (np.arctan2(pts[:, 1], pts[:, 0]) + np.pi) * p.cols / (2 * np.pi)
        near = (np.abs(fr - np.round(fr)) < EDGE) | (np.abs(fc - np.round(fc)) < EDGE) | \
               (np.abs(rm - p.min_range) < 1e-9) | (np.abs(rm - p.max_range) < 1e-9)
        ok_m = (np.floor(fr) >= 0) & (np.floor(fr) < p.rows) & (rm >= p.min_range) & (rm <= p.max_range)
        far = ~near
        assert np.array_equal(ok[far], ok_m[far]), p
        both = far & ok
        assert np.array_equal(row[both], np.floor(fr[both]).astype(int)), p
        assert np.array_equal(col[both], np.floor(fc[both]).astype(int) % p.cols), p
        assert np.abs(r[ok] - rm[ok]).max() < 1e-12 * max(1.0, rm[ok].max())
        n_all += pts.shape[0]
        n_near += int(near.sum())
    print(f"pixel model: {n_near} of {n_all} points lie within {EDGE} of a pixel or range edge of the model")
    assert n_near <= n_all * 1e-5


def test_named_edge_cases():
    p = CR.Params(rows=8, cols=16, fov_up_deg=40.0, fov_down_deg=-40.0, window=1, margin_abs=2.5)
    c, h = CR.cfg_make(p, 1, 0.5), CR.HeaderCfg(p, 1, 0.5)

    def px(x, y, z):
        a, b = CR.pixels(c, [[x, y, z]]), h.pixels([[x, y, z]])
        _same_pixels(a, b, (x, y, z))
        return (int(a[2][0]), int(a[3][0])) if a[0][0] else None
    # az = pi from y = +0 and az = -pi from y = -0: both the first column
    assert px(-5.0, 0.0, 0.0) == (4, 0) and px(-5.0, -0.0, 0.0) == (4, 0)
    assert px(-5.0, -1e-9, 0.0) == (4, 0) and px(-5.0, 1e-9, 0.0) == (4, 15)
    assert px(5.0, 0.0, 0.0) == (4, 8) and px(5.0, -0.0, 0.0) == (4, 8) and px(0.0, 5.0, 0.0) == (4, 12)
    # the z axis has no pixel; a hair off it has one
    assert px(0.0, 0.0, 3.0) is None and px(0.0, -0.0, -3.0) is None and px(1e-3, 0.0, 3.0) is None  # (89.98 degrees: row -5)
    # rows -1 and `rows`: just above the top and at / below the bottom edge
    up = np.deg2rad(40.0)
    for el, want in ((up + 1e-9, None), (up - 1e-9, 0), (-up + 1e-9, 7), (-up - 1e-9, None), (0.0, 4), (1e-12, 3)):
        got = px(5 * np.cos(el), 0.0, 5 * np.sin(el))
        assert (got is None and want is None) or got[0] == want, (el, got, want)
    # ranges: the ends belong to the interval
    assert px(1.0, 0.0, 0.0) == (4, 8) and px(np.nextafter(1.0, 0), 0.0, 0.0) is None
    assert px(80.0, 0.0, 0.0) == (4, 8) and px(np.nextafter(80.0, 100), 0.0, 0.0) is None
    for bad in (np.nan, np.inf, -np.inf):
        assert px(bad, 1.0, 1.0) is None and px(1.0, bad, 1.0) is None and px(1.0, 1.0, bad) is None

    # verdicts on hand-made images: the voxel mean (3, 4, 0) seen from the identity has r_v = 5 exactly, limit 7.5
    mu, I = np.array([[3.0, 4.0, 0.0]]), np.eye(4)[None]
    row, col = px(3.0, 4.0, 0.0)
    assert (row, col) == (4, 10)

    def verdict(img, cfg=c, hdr=h, pose=I, m=mu):
        v = CR.verdicts(cfg, pose[0], m, img)
        assert np.array_equal(v, hdr.verdicts(pose, img[None], m)[:, 0])
        return int(v[0])

    def blank(cfg=c):
        return np.full((cfg.rows, cfg.cols), CR.EMPTY, np.uint32)

    def f32bits(x):
        return np.array([x], F32).view(np.uint32)[0]
    img = blank()
    assert verdict(img) == CR.NO_VOTE
    img[row - 1:row + 2, col - 1:col + 2] = f32bits(3.0)
    img[row, col] = CR.EMPTY
    assert verdict(img) == CR.NO_VOTE                      # an empty centre with filled neighbours: no vote
    img = blank()
    img[row, col] = f32bits(7.5)
    assert verdict(img) == CR.OCCUPIED                     # exactly at r_v + margin: kept
    img[row, col] = f32bits(np.nextafter(F32(7.5), F32(8)))
    assert verdict(img) == CR.SEEN_THROUGH                 # one float above: seen through
    img[row + 1, col - 1] = f32bits(7.5)
    assert verdict(img) == CR.OCCUPIED                     # ... unless a neighbour is at the limit
    img[row + 1, col - 1] = CR.EMPTY
    img[row + 2, col] = f32bits(1.0)
    img[row, col + 2] = f32bits(1.0)
    assert verdict(img) == CR.SEEN_THROUGH                 # outside the window: not looked at
    # the window across the column wrap: a voxel in column 0, its near neighbour in the last column
    mu0 = np.array([[-5.0, -1e-9, 0.0]])
    img = blank()
    img[4, 0] = f32bits(30.0)
    assert verdict(img, m=mu0) == CR.SEEN_THROUGH
    img[5, 15] = f32bits(6.0)
    assert verdict(img, m=mu0) == CR.OCCUPIED
    img[5, 15] = CR.EMPTY
    img[3, 1] = f32bits(6.0)
    assert verdict(img, m=mu0) == CR.OCCUPIED
    mu15 = np.array([[-5.0, 1e-9, 0.0]])                   # ... and from the last column into column 0
    img = blank()
    img[4, 15] = f32bits(30.0)
    assert verdict(img, m=mu15) == CR.SEEN_THROUGH
    img[4, 0] = f32bits(7.5)
    assert verdict(img, m=mu15) == CR.OCCUPIED
    # clamped at the first and the last row: the rows outside are neutral
    for el, r0 in ((up - 1e-3, 0), (-up + 1e-3, 7)):
        m_edge = np.array([[5 * np.cos(el), 0.0, 5 * np.sin(el)]])
        img = blank()
        img[r0, 8] = f32bits(40.0)
        assert verdict(img, m=m_edge) == CR.SEEN_THROUGH
        img[r0 + (1 if r0 == 0 else -1), 9] = f32bits(5.0)
        assert verdict(img, m=m_edge) == CR.OCCUPIED
        img[r0 + (1 if r0 == 0 else -1), 9] = CR.EMPTY
        img[7 - r0, 8] = f32bits(5.0)                      # (the row a wrapped index would reach)
        assert verdict(img, m=m_edge) == CR.SEEN_THROUGH
    # a window of 0 looks at the centre alone; margin_rel scales with the range
    p0 = CR.Params(rows=8, cols=16, fov_up_deg=40.0, fov_down_deg=-40.0, window=0, margin_abs=0.5, margin_rel=0.25)
    c0, h0 = CR.cfg_make(p0, 1, 0.5), CR.HeaderCfg(p0, 1, 0.5)
    img = blank()
    img[row, col] = f32bits(6.75)                          # (5 + 0.5) + 0.25 x 5
    img[row, col + 1] = f32bits(1.0)
    assert verdict(img, c0, h0) == CR.OCCUPIED
    img[row, col] = f32bits(np.nextafter(F32(6.75), F32(7)))
    assert verdict(img, c0, h0) == CR.SEEN_THROUGH
    # margin_abs = 0 means the voxel side
    pz = CR.Params(rows=8, cols=16, fov_up_deg=40.0, fov_down_deg=-40.0, window=0)
    assert CR.cfg_make(pz, 1, 0.75).margin_abs == 0.75 == CR.HeaderCfg(pz, 1, 0.75).cfg.margin_abs
    # the image keeps the minimum, whatever the order, and skips what has no pixel
    cloud = R.f4(np.array([[4.5, 6.0, 0.0], [3.0, 4.0, 0.0], [6.0, 8.0, 0.0], [np.nan, 0, 0], [0, 0, 2.0], [0.1, 0.1, 0.0]]))
    for perm in ([0, 1, 2, 3, 4, 5], [2, 4, 1, 5, 0, 3]):
        img = CR.image(c, cloud[perm])
        assert np.array_equal(img, h.image(cloud[perm]))
        assert img[4, 10] == f32bits(5.0) and (img != CR.EMPTY).sum() == 1


def test_named_edge_cases_as_clouds():
    """The clouds the GPU test runs (vmap_carve_cases.edge_clouds) give the verdicts they are named for."""
    p = CR.Params(**CC.EDGE_IMAGE)
    up = np.zeros((1, 4), F32)
    up[0, 2] = 1.0
    for name, pts, scan, carved in CC.edge_clouds():
        m = CR.RefMap(0.5, 64)
        m.insert(pts, up)
        assert len(m) == 1 and np.array_equal(m.fetch(M.RECORDS)[0, :3], pts[0, :3].astype(np.float64)), name
        got = m.carve(scan, None, p)
        assert got["n_carved"] == int(carved) and got["n_tested"] == (0 if name in ("empty", "skipped") else 1), (name, got)


def test_votes_and_what_a_carve_does_to_a_map():
    m = _hand_map()
    before, info0 = m.fetch_all(), m.info()
    n = len(m)
    clouds, poses = CC.hand_scans(before[M.CLOUD], n_scans=3)
    p = CR.Params(**CC.WIDE, window=1, min_votes=2)
    c = CR.cfg_make(p, 3, K.SIDE)
    votes = CR.carve_votes(c, clouds, poses, before[M.RECORDS][:, :3])
    through = (votes == CR.SEEN_THROUGH).sum(axis=1)
    assert all((through == k).sum() > 0 for k in (0, 1, 2, 3)), np.bincount(through)
    # a voxel seen through by one scan and occupied in another: one vote, which min_votes = 1 takes and min_votes = 2 does not
    mixed = (through == 1) & (votes == CR.OCCUPIED).any(axis=1)
    assert mixed.sum() > 0
    for min_votes in (1, 2, 3):                                  # reached exactly and missed by one
        mm = _hand_map()
        pp = CR.Params(**CC.WIDE, window=1, min_votes=min_votes)
        info = mm.carve_scans(clouds, poses, pp)
        gone = through >= min_votes
        assert 0 < gone.sum() < n
        assert info == {"n_kept": int((~gone).sum()), "n_carved": int(gone.sum()),
                        "n_tested": int((votes != CR.NO_VOTE).any(axis=1).sum()),
                        "n_members_carved": int(before[M.COUNT][gone].sum())}
        assert (gone[mixed]).all() == (min_votes == 1)
        _same_sections(mm.fetch_all(), {k: before[k][~gone] for k in SECTIONS}, min_votes)     # the kept rows, bit for bit
        i = mm.info()
        assert (i["n_voxels"], i["n_inserts"], i["n_members"]) == (n - int(gone.sum()), info0["n_inserts"],
                                                                   info0["n_members"] - info["n_members_carved"])
        again = mm.carve_scans(clouds, poses, pp)               # the same call again carves nothing
        assert again["n_carved"] == 0 and again["n_kept"] == len(mm)
    # one cloud = one scan; kept voxels go on, carved ones start anew
    mm, whole = _hand_map(), _hand_map()
    info = mm.carve(clouds[0], poses[0], CR.Params(**CC.WIDE, window=1))
    assert info["n_carved"] == int((votes[:, 0] == CR.SEEN_THROUGH).sum()) > 0
    kept = {tuple(x) for x in mm.fetch(M.COORDS)}
    more, more_n = K.cloud_of_voxels(before[M.COORDS][::5], K.SIDE, per_voxel=(2,), seed=5)
    alone = CR.RefMap(K.SIDE, 4096)
    for x in (mm, whole, alone):
        x.insert(more, more_n)
    fw, fa, fm = whole.fetch_all(), alone.fetch_all(), mm.fetch_all()
    iw = {tuple(x): j for j, x in enumerate(fw[M.COORDS])}
    ia = {tuple(x): j for j, x in enumerate(fa[M.COORDS])}
    n_cont = n_new = 0
    for j, x in enumerate(map(tuple, fm[M.COORDS])):
        src, row = (fw, iw[x]) if x in kept else (fa, ia[x])
        for k in SECTIONS:
            assert np.array_equal(_bits(fm[k][j]), _bits(src[k][row])), (x, k)
        n_cont += x in kept and x in ia
        n_new += x not in kept
    assert n_cont > 0 and n_new > 0
    # no scan, no voxel, no point
    assert _hand_map().carve_scans([], [], CR.Params()) == {"n_kept": 0, "n_carved": 0, "n_tested": 0, "n_members_carved": 0}
    assert CR.RefMap(1.0, 8).carve(clouds[0]) == {"n_kept": 0, "n_carved": 0, "n_tested": 0, "n_members_carved": 0}
    assert _hand_map().carve(clouds[0][:0], None, CR.Params(**CC.WIDE)) == {"n_kept": n, "n_carved": 0, "n_tested": 0,
                                                                            "n_members_carved": 0}


def test_every_refusal_in_both():
    for name, value, code in CC.BAD_PARAMS:
        p = CR.Params(**{name: value})
        assert CR.HeaderCfg(p, 2, 1.0).why == code, (name, value)
        with pytest.raises(CR.BadArgError) as ei:
            CR.cfg_make(p, 2, 1.0)
        assert ei.value.args[0] == code, (name, value)
    for name, value in (("rows", 1), ("rows", 256), ("cols", 8), ("cols", 4096), ("window", 0), ("window", 3), ("min_votes", 2),
                        ("margin_abs", 0.0), ("margin_rel", 0.0), ("min_range", -1.0)):
        p = CR.Params(**{name: value})
        assert CR.HeaderCfg(p, 2, 1.0).why == 0 and CR.HeaderCfg(p, 2, 1.0).cfg == CR.cfg_make(p, 2, 1.0)
    m = _hand_map()
    before = m.fetch_all()
    clouds, poses = CC.hand_scans(before[M.CLOUD], n_scans=2)
    bad_pose = poses.copy()
    bad_pose[1, 2, 3] = np.nan
    with pytest.raises(CR.BadArgError):
        m.carve_scans(clouds, bad_pose, CR.Params(**CC.WIDE))
    with pytest.raises(CR.BadArgError):
        m.carve_scans(clouds, poses, CR.Params(**CC.WIDE, min_votes=3))
    with pytest.raises(CR.BadArgError):
        m.carve_scans([clouds[0]] * 65, [poses[0]] * 65, CR.Params(**CC.WIDE))
    _same_sections(m.fetch_all(), before)


# ---- quality -----------------------------------------------------------------------------------------------------------
# The restatement's own figures on the two scenes, carved with all eight scans at the defaults except
# min_votes = 2: (ghosts carved, ghosts, static carved, static).
QUALITY = {False: (399, 399, 0, 19604), True: (395, 396, 294, 36832)}


@pytest.mark.parametrize("vegetation", (False, True))
def test_quality_on_a_scene_with_a_moving_box(vegetation):
    """Eight scans 1.5 m apart of synth._scene (with and without KITTI16K's vegetation), ground kept, and a 4 x 2 x 1.5 m box
    that moves 3 m per scan, inserted into a 0.5 m map: a voxel of which more than half the members are box returns is a
    ghost.  Carved with all eight scans, window 2, min_votes 2, 64 x 1024: at least 80 % of the ghosts and at most 1 % of the
    static voxels leave; and the figures stay where they were measured (the static share within a factor 2: it is a count of
    tens to hundreds of voxels, and the margin is for a changed seed)."""
    from collections import Counter
    scans, poses, is_box = CC.moving_box_scans(vegetation)
    m = CR.RefMap(0.5, 1 << 20)
    up = np.zeros((max(s.shape[0] for s in scans), 4), F32)
    up[:, 2] = 1.0
    for s, P in zip(scans, poses):
        m.insert(s, up[:s.shape[0]], P)
    f = m.fetch_all()
    tot, box = Counter(), Counter()
    for s, P, b in zip(scans, poses, is_box):
        coords = np.floor((s[:, :3].astype(np.float64) + P[:3, 3]) / 0.5).astype(np.int64)
        u, inv = np.unique(coords, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        nt, nb = np.bincount(inv, minlength=len(u)), np.bincount(inv, weights=b.astype(np.float64), minlength=len(u))
        for k, c in enumerate(map(tuple, u)):
            tot[c] += int(nt[k])
            box[c] += int(nb[k])
    coords = [tuple(int(x) for x in c) for c in f[M.COORDS]]
    assert all(tot[c] == n for c, n in zip(coords, f[M.COUNT]))          # the labels are of the map's own members
    ghost = np.array([2 * box[c] > tot[c] for c in coords])
    p = CR.Params(min_votes=2)
    info = m.carve_scans(scans, poses, p)
    left = {tuple(int(x) for x in c) for c in m.fetch(M.COORDS)}
    gone = np.array([c not in left for c in coords])
    got = (int((gone & ghost).sum()), int(ghost.sum()), int((gone & ~ghost).sum()), int((~ghost).sum()))
    print(f"vegetation={vegetation}: ghosts carved {got[0]} of {got[1]}, static voxels carved {got[2]} of {got[3]}; {info}")
    assert info["n_carved"] == int(gone.sum())
    assert got[0] >= 0.8 * got[1] and got[2] <= 0.01 * got[3]
    g0, gn, s0, sn = QUALITY[vegetation]
    assert got[1] == gn and got[3] == sn and got[0] >= g0 - 4 and got[2] <= 2 * max(s0, 10)


def test_the_three_entry_points_are_declared_exported_and_bound():
    """The entry points of include/quatro_voxelmap_carve.h are three of libquatro_ext.so's exports, they have their ctypes
    signatures, libquatro_hip.so exports none of them, the structs are their ctypes mirrors and the defaults are the
    documented ones."""
    import ctypes
    import os
    import subprocess
    import tempfile
    import ext_abi
    from quatro_amd import lib as ql
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    assert ext_abi.check_header("quatro_voxelmap_carve.h") == {"qtr_default_carve_params", "qtr_voxel_map_carve",
                                                               "qtr_voxel_map_carve_keyframes"}
    src = r"""
#include <stdio.h>
#include <stddef.h>
#include "quatro_voxelmap_carve.h"
#define O(f) offsetof(qtr_carve_params, f)
#define I(f) offsetof(qtr_voxel_map_carve_info, f)
int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(qtr_carve_params), O(rows), O(cols), O(window),
  O(min_votes), O(fov_up_deg), O(fov_down_deg), O(margin_abs), O(margin_rel), O(min_range), O(max_range), O(reserved));
  printf("%zu %zu %zu %zu %zu\n", sizeof(qtr_voxel_map_carve_info), I(n_kept), I(n_carved), I(n_tested), I(n_members_carved));
  return 0;}
"""
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), c, "-o", os.path.join(d, "s")])
        got = list(map(int, subprocess.check_output([os.path.join(d, "s")]).split()))
    P, E = ql.CarveParams, ql.VoxelMapCarveInfo
    assert got[:12] == [ctypes.sizeof(P)] + [getattr(P, n).offset for n, _ in P._fields_] == [96, 0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64]
    assert got[12:] == [ctypes.sizeof(E), E.n_kept.offset, E.n_carved.offset, E.n_tested.offset, E.n_members_carved.offset] == [24, 0, 4, 8, 16]
    d = ql.default_carve_params()
    want = CR.Params()
    assert all(getattr(d, k) == v for k, v in want.__dict__.items()) and not any(d.reserved)
    assert ql.default_carve_params(window=3, margin_rel=0.5).window == 3
    with pytest.raises(TypeError):
        ql.default_carve_params(nothing=1)
