"""Named edge inputs for the two stages every raw-scan registration passes through first: Patchwork ground segmentation
(quatro_amd/csrc/patchwork.hip: k_pw_keys, k_pw_bin, k_pw_bounds, k_pw_patch, k_pw_scan, k_pw_emit) and the range image
with sub-cluster rejection (quatro_amd/csrc/segment.hip: k_ip_project, k_ip_init, k_ip_merge, k_ip_flatten,
k_ip_flatten_agg, k_ip_classify, k_ip_blockscan, k_ip_rootrank, k_ip_compact).  A plain module: deterministic numpy
generators, no fixtures, no GPU work.  Used by tests/test_scan_cases_cpu.py (the oracle against the independent
references below, every case against what it claims) and tests/test_gpu_scan_cases.py (the device against the oracle,
bit for bit).

    pw_case(name) -> PwCase(cloud, params_mutation, claims)
    ip_case(name) -> IpCase(cloud, ip_fields, claims)

cloud is [P, 4] binary32 and its w column is the point's input index, so that every output row names the input point it
is a copy of.  params_mutation is a dict of qtr_pw_params fields laid over PW_DEFAULT (pw_apply writes it into either
ctypes structure); ip_fields is the whole qtr_ip_params as a dict (ip_apply).  claims says what the case is there for;
the CPU test asserts every entry.

The references share no code with oracle/:

  * pw_structure: Patchwork's binning in binary64 numpy -> patch id per point, every patch's list in stable height
    order, the low-point prefix and the seed mean, and each point's distance from the nearest bin boundary;
  * pw_planefit: the region-wise plane fit in binary64 (two-pass covariance, np.linalg.eigh, the same iteration count
    and status rule) -> the two output lists, and the smallest distance of any residual from its threshold.  It is the
    expected answer only where that distance is at least RES_MARGIN: there the binary32 single-pass moments of the
    oracle and of the device cannot change a decision;
  * ip_pixels: the pixel arithmetic of ImageProjection::projectPointCloud mirrored step by step in binary32 numpy;
  * ip_label: connected components by union-find over the occupied pixels, the validity rule (rows holding a pixel other
    than the component's first), labels numbered by first pixels in row-major order, outputs in row-major order.
"""
from collections import namedtuple

import numpy as np

f32 = np.float32
f64 = np.float64

PwCase = namedtuple("PwCase", "cloud params_mutation claims")
IpCase = namedtuple("IpCase", "cloud ip_fields claims")

# ---------------------------------------------------------------------------------------------- mirrored constants
PW_DEFAULT = dict(  # config/patchwork_params.yaml of the reference; the CPU test holds it to the oracle's pw_params()
    sensor_height=1.723, num_iter=3, num_lpr=20, num_min_pts=80, th_seeds=0.25, th_dist=0.125, max_range=80.0,
    min_range=2.7, uprightness_thr=0.707, adaptive_seed_selection_margin=-1.1, using_global_thr=0,
    global_elevation_thr=-0.5, num_zones=4, num_sectors_each_zone=[16, 32, 54, 32], num_rings_each_zone=[2, 4, 4, 4],
    min_ranges=[2.7, 12.3625, 22.025, 41.35], num_thr=4, elevation_thr=[-1.2, -0.9984, -0.851, -0.605, 0, 0, 0, 0],
    flatness_thr=[0.0001, 0.000125, 0.000185, 0.000185, 0, 0, 0, 0])
PW_MAX_PATCHES = 1024   # k_pw_scan: one 1024-thread workgroup; pw_begin refuses more
PW_REFUSAL = "Some parameters are wrong! the size of parameters should be same"
PW_WG = 256             # k_pw_patch / k_pw_emit: positions per round
BIN_MARGIN = 1e-4       # metres: every point not named as a boundary point is at least this far inside its bin
RES_MARGIN = 0.05       # metres: binary64 residuals and seed heights stay this far from their thresholds
IP_BLOCK = 1024         # pixels per workgroup of k_ip_classify / k_ip_rootrank / k_ip_compact
IP_OUTLIER = 999999
MODES = {"4Neighbor": 0, "8Neighbor": 1, "4CrossNeighbor": 2}
THETA = float(f32(60.0 / 180.0 * np.pi))
ANGLE_MARGIN_DEG = 5.0  # every pair of neighbouring pixels gives an angle at least this far from segment_theta


def pw_fields(mutation=None):
    f = {k: (list(v) if isinstance(v, list) else v) for k, v in PW_DEFAULT.items()}
    for k, v in (mutation or {}).items():
        assert k in f, k
        f[k] = list(v) if isinstance(v, (list, tuple)) else v
    return f


def pw_apply(p, mutation=None):
    """write PW_DEFAULT + mutation into a ctypes qtr_pw_params (the oracle's or the library's) and return it"""
    for k, v in pw_fields(mutation).items():
        if isinstance(v, list):
            arr = getattr(p, k)
            for i in range(len(arr)):
                arr[i] = v[i] if i < len(v) else 0
        else:
            setattr(p, k, v)
    return p


def ip_apply(p, fields):
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _seed(name):
    return [ord(c) for c in name]


def _finish(xyz, rng=None):
    """[n, 3] binary64 -> [n, 4] binary32 in a shuffled order, w = input index"""
    xyz = np.asarray(xyz, dtype=f64).reshape(-1, 3)
    if rng is not None:
        xyz = xyz[rng.permutation(xyz.shape[0])]
    c = np.zeros((xyz.shape[0], 4), dtype=f32)
    with np.errstate(over="ignore", invalid="ignore"):
        c[:, :3] = xyz.astype(f32)
    c[:, 3] = np.arange(xyz.shape[0], dtype=f32)
    return c


# ============================================================================================== Patchwork references
def _pw_layout(F):
    nz = F["num_zones"]
    nsec, nring, mr = F["num_sectors_each_zone"][:nz], F["num_rings_each_zone"][:nz], F["min_ranges"][:nz]
    base = [0]
    for k in range(nz):
        base.append(base[-1] + nsec[k] * nring[k])
    hi = [mr[k + 1] if k + 1 < nz else F["max_range"] for k in range(nz)]
    ring_size = [(hi[k] - mr[k]) / nring[k] for k in range(nz)]
    sector_size = [2 * np.pi / nsec[k] for k in range(nz)]
    return nz, nsec, nring, mr, base, ring_size, sector_size


def pw_margin_height(F):
    return -0.1 if F["sensor_height"] == 0.0 else F["adaptive_seed_selection_margin"] * F["sensor_height"]


def pw_patch_id(F, zone, ring, sector):
    nz, nsec, nring, mr, base, _, _ = _pw_layout(F)
    return base[zone] + ring * nsec[zone] + sector


def pw_patch_zrs(F, pid):
    nz, nsec, nring, mr, base, _, _ = _pw_layout(F)
    k = max(z for z in range(nz) if pid >= base[z])
    return k, (pid - base[k]) // nsec[k], (pid - base[k]) % nsec[k]


def pw_structure(cloud, F):
    """Binning in binary64.  -> dict(patch [P] (-1: in no patch), lists {pid: input indices in stable height order},
    prefix {pid: low-point prefix length}, seed_mean {pid: binary64 mean of the seed heights}, margin [P]: distance in
    metres from the nearest boundary of the point's bin (inf for points in no patch))"""
    nz, nsec, nring, mr, base, ring_size, sector_size = _pw_layout(F)
    P = cloud.shape[0]
    x, y, z = (cloud[:, i].astype(f64) for i in range(3))
    patch = np.full(P, -1, dtype=np.int64)
    margin = np.full(P, np.inf)
    for i in range(P):
        if not (np.isfinite(x[i]) and np.isfinite(y[i]) and np.isfinite(z[i])):
            continue
        if z[i] < -1.8 * F["sensor_height"]:
            continue
        r = np.sqrt(x[i] * x[i] + y[i] * y[i])
        if not (r <= F["max_range"] and r > F["min_range"]):
            continue
        at = np.arctan2(y[i], x[i])
        theta = at if at > 0 else at + 2 * np.pi
        k = nz - 1
        for zz in range(1, nz):
            if r < mr[zz]:
                k = zz - 1
                break
        fr, fs = (r - mr[k]) / ring_size[k], theta / sector_size[k]
        ring, sector = min(int(fr), nring[k] - 1), min(int(fs), nsec[k] - 1)
        patch[i] = base[k] + ring * nsec[k] + sector
        m = min(r - F["min_range"], F["max_range"] - r, z[i] + 1.8 * F["sensor_height"])
        m = min(m, (fr - ring) * ring_size[k], (ring + 1 - fr) * ring_size[k] if fr < nring[k] else np.inf)
        m = min(m, (fs - sector) * sector_size[k] * r, (sector + 1 - fs) * sector_size[k] * r)
        margin[i] = m
    lists, prefix, seed_mean = {}, {}, {}
    order = np.argsort(cloud[:, 2], kind="stable")  # -0.0 == +0.0: input order decides; non-finite never used
    low = pw_margin_height(F)
    for pid in np.unique(patch[patch >= 0]):
        ids = order[patch[order] == pid]
        lists[int(pid)] = ids
        zone = max(q for q in range(nz) if pid >= base[q])
        init = 0
        if zone == 0:
            while init < ids.size and z[ids[init]] < low:
                init += 1
        cnt, s = min(F["num_lpr"], ids.size - init), 0.0
        for t in range(init, init + cnt):
            s += z[ids[t]]
        prefix[int(pid)] = init
        seed_mean[int(pid)] = s / cnt if cnt else 0.0
    return dict(patch=patch, lists=lists, prefix=prefix, seed_mean=seed_mean, margin=margin)


def pw_processed(F, S):
    """patch ids the reference processes (more than num_min_pts points), in its zone / ring / sector order"""
    return [p for p in sorted(S["lists"]) if S["lists"][p].size > F["num_min_pts"]]


def pw_planefit(cloud, F, S):
    """Region-wise ground plane fit in binary64.  -> dict(ground, nonground: input indices in output order,
    res_margin: smallest |residual - threshold| (seed heights against the seed threshold included), status_margin:
    smallest distance of a status comparison from its threshold (uprightness absolute; elevation absolute; flatness as
    |log10| of the ratio), per_patch {pid: (reject_all, n_ground)})"""
    xyz = cloud[:, :3].astype(f64)
    nz, nsec, nring, mr, base, _, _ = _pw_layout(F)
    ring_base = np.concatenate([[0], np.cumsum(nring)])
    ground, nonground, per = [], [], {}
    res_margin, status_margin = np.inf, np.inf
    for pid in pw_processed(F, S):
        ids = S["lists"][pid]
        p = xyz[ids]
        seed_thr = S["seed_mean"][pid] + F["th_seeds"]
        member = p[:, 2] < seed_thr
        res_margin = min(res_margin, np.abs(p[:, 2] - seed_thr).min())
        for _ in range(F["num_iter"]):
            q = p[member]
            mean = q.mean(axis=0)
            d = q - mean
            cov = d.T @ d / q.shape[0]
            w, v = np.linalg.eigh(cov)
            n = v[:, 0]
            if n[2] < 0:
                n = -n
            thr = F["th_dist"] + n @ mean
            res = p @ n
            member = res < thr
            res_margin = min(res_margin, np.abs(res - thr).min())
        sv = np.sort(np.abs(w))[::-1]
        k, ring, _ = pw_patch_zrs(F, pid)
        ci = ring_base[k] + ring
        reject = False
        status_margin = min(status_margin, abs(abs(n[2]) - F["uprightness_thr"]))
        if abs(n[2]) < F["uprightness_thr"]:
            reject = True
        elif ci < F["num_thr"]:
            ti = ring + 2 * k
            status_margin = min(status_margin, abs(mean[2] - F["elevation_thr"][ti]))
            if mean[2] > F["elevation_thr"][ti]:
                surface = sv[2] / sv.sum()
                ft = F["flatness_thr"][ti]
                if ft > 0:
                    status_margin = min(status_margin, abs(np.log10(max(surface, 1e-300) / ft)))
                reject = not (ft > surface)
        elif F["using_global_thr"]:
            status_margin = min(status_margin, abs(mean[2] - F["global_elevation_thr"]))
            reject = mean[2] > F["global_elevation_thr"]
        (nonground if reject else ground).extend(ids[member].tolist())
        nonground.extend(ids[~member].tolist())
        per[pid] = (bool(reject), int(member.sum()))
    return dict(ground=np.array(ground, dtype=np.int64), nonground=np.array(nonground, dtype=np.int64),
                res_margin=float(res_margin), status_margin=float(status_margin), per_patch=per)


# ============================================================================================== Patchwork builders
def _box(F, zone, ring, sector):
    nz, nsec, nring, mr, base, ring_size, sector_size = _pw_layout(F)
    return (mr[zone] + ring * ring_size[zone], mr[zone] + (ring + 1) * ring_size[zone], sector * sector_size[zone],
            (sector + 1) * sector_size[zone])


def _xy(F, rng, zone, ring, sector, n, r_span=None):
    """n points well inside a patch: the middle 60 % of its ring (or r_span metres about its middle), 80 % of its sector"""
    r0, r1, t0, t1 = _box(F, zone, ring, sector)
    half = 0.3 * (r1 - r0) if r_span is None else 0.5 * r_span
    r = 0.5 * (r0 + r1) + rng.uniform(-half, half, n)
    t = 0.5 * (t0 + t1) + rng.uniform(-0.4, 0.4, n) * (t1 - t0)
    return r * np.cos(t), r * np.sin(t)


def _patch(F, rng, zone, ring, sector, n_ground, n_obj=0, n_low=0, n_probe=0, z_probe=0.0, heavy=(), tilt=0.0,
           obj_dz=2.5, low_dz=0.2, ground_z=None, noise=0.01):
    """One patch as populations: a ground plane with at most `noise` metres of height noise (tilted by `tilt` along the
    sector's middle direction when asked), objects obj_dz .. obj_dz + 1 m above it, low points low_dz below it, a probe
    level at height z_probe, single heavy heights.  -> [n, 3]"""
    gz = -F["sensor_height"] if ground_z is None else ground_z
    n = n_ground + n_obj + n_low + n_probe + len(heavy)
    x, y = _xy(F, rng, zone, ring, sector, n, r_span=0.4 if tilt else None)
    _, _, t0, t1 = _box(F, zone, ring, sector)
    tc = 0.5 * (t0 + t1)
    u = x * np.cos(tc) + y * np.sin(tc)
    plane = gz + tilt * (u - u.min())
    z = plane.copy()
    a, b = n_ground, n_ground + n_obj
    z[:a] += rng.uniform(0, noise, a) if noise else 0.0
    if a and not tilt:
        z[0] = gz  # the lowest ground height is the plane's own
    z[a:b] += obj_dz + rng.uniform(0, 1.0, n_obj)
    z[b:b + n_low] -= low_dz
    z[b + n_low:b + n_low + n_probe] = z_probe
    z[b + n_low + n_probe:] = np.asarray(heavy, dtype=f64)
    return np.stack([x, y, z], axis=1)


_PLAIN = dict(num_min_pts=10, num_thr=0)  # small patches; no elevation / flatness table unless the case is about it
# the binary64 plane fit stands for the binary32 one only near the sensor (single-pass moments lose digits with the
# square of the range): every patch it is applied to lies within PLANE_FIT_RANGE.  Cases that need the outer zones
# pull the whole layout in
PLANE_FIT_RANGE = 20.0
_NEAR = dict(min_ranges=[2.7, 6.0, 10.0, 14.0], max_range=20.0)
SIZES = [10, 11, 63, 64, 65, 255, 256, 257, 511, 512, 513]
PREFIXES = [0, 1, 255, 256, 257, 512, "n"]
BLOCK64_IDS = sorted(set([0, 63, 64, 511, 512, 959, 1023] + [64 * b + o for b in range(16) for o in (5, 37)]))


def _sizes(name, tilt):
    rng = np.random.default_rng(_seed(name))
    mut = dict(_PLAIN, th_seeds=3.0)
    F = pw_fields(mut)
    parts, want = [], {}
    for j, n in enumerate(SIZES):  # one patch each: zone 0 or 1 by turns, ring 1, sector j
        zone, ring, sector = j % 2, 1, j
        n_obj = max(1, n // 8)
        parts.append(_patch(F, rng, zone, ring, sector, n - n_obj, n_obj, tilt=tilt, obj_dz=6.0,
                            noise=0.0 if tilt else 0.01))
        want[pw_patch_id(F, zone, ring, sector)] = n
    claims = dict(two_population=True, patch_sizes=want, all_rejected=bool(tilt), none_rejected=not tilt)
    return PwCase(_finish(np.concatenate(parts), rng), mut, claims)


def _prefix(name, zone):
    """ground at -h (its lowest height exactly), `prefix` low points 0.2 m below it, as many probes as ground points
    0.9 m above it; num_lpr = 1 and one iteration.  In zone 0 the seed height is the first height past the prefix (-h),
    the seed threshold -h + 1 and the probes are seeds, so the one plane runs between ground and probes (at most 0.67 m
    under the probes) and both are ground; a prefix counted one short puts the seed height 0.2 m lower and the probes
    out, 0.9 m and more above the plane.  In zone 1 nothing is skipped and the probes are no seeds (but for the patch
    without low points).  Two rings per zone, the second of zone 0 or the first of zone 1: the patch is metres wide, so
    the smallest spread of ground + probes is the vertical one."""
    rng = np.random.default_rng(_seed(name))
    mut = dict(_PLAIN, num_lpr=1, num_iter=1, th_seeds=1.0, th_dist=0.8, num_rings_each_zone=[2, 2, 4, 4])
    F = pw_fields(mut)
    h = F["sensor_height"]
    parts, want, probes = [], {}, {}
    ring = 1 if zone == 0 else 0
    for j, pre in enumerate(PREFIXES):
        sector = 2 * j
        if pre == "n":
            parts.append(_patch(F, rng, zone, ring, sector, 0, n_low=40, noise=0.0))
            want[pw_patch_id(F, zone, ring, sector)] = 40 if zone == 0 else 0
        else:
            g = max(40, pre)
            parts.append(_patch(F, rng, zone, ring, sector, g, n_low=pre, n_probe=g, z_probe=-h + 0.9))
            want[pw_patch_id(F, zone, ring, sector)] = pre if zone == 0 else 0
            probes[pw_patch_id(F, zone, ring, sector)] = zone == 0 or pre == 0
    claims = dict(two_population=True, prefix=want, probes_are_ground=probes)
    return PwCase(_finish(np.concatenate(parts), rng), mut, claims)


def _num_lpr(name, L):
    """A patch longer than num_lpr whose seed window ends on a heavy height: ground at -h, probes, then heights of 0.2 L.
    The window is all of ground and probes plus one heavy height at window position L - 1 (for 257 the first of the
    second 256-chunk), so a sum that loses it puts the seed threshold 0.2 m lower.  The probes (about 1.2 m above the
    ground) sit 0.1 m under the right threshold.  One iteration: probes that are seeds pull the plane half way up and
    stay ground (0.6 m from it, th_dist 0.9); probes that are not are 1.2 m above it.  A patch shorter than num_lpr (its
    window is the whole patch) is a plain ground + objects one.  Zone 0, ring 1: patches metres wide (no height here is
    under the margin height, so nothing is skipped)."""
    rng = np.random.default_rng(_seed(name))
    mut = dict(_PLAIN, num_lpr=L, num_iter=1, th_seeds=0.5)
    F = pw_fields(mut)
    h = F["sensor_height"]
    parts = []
    if L == 1:
        g = 40
        parts.append(_patch(F, rng, 0, 1, 0, g, n_obj=8))
        longer, shorter = pw_patch_id(F, 0, 1, 0), None
        zp = None
    else:
        heavy = 0.2 * L
        g = (L - 1) // 2
        pn = L - 1 - g
        a = g * (-h + 0.005) + heavy
        zp = (a / L + 0.4) / (1 - pn / L)
        mut["th_dist"] = 0.9
        parts.append(_patch(F, rng, 0, 1, 0, g, n_probe=pn, z_probe=zp, heavy=[heavy] * 8))
        parts.append(_patch(F, rng, 0, 1, 4, min(L - 6, 90), n_obj=5, obj_dz=8.0))
        longer, shorter = pw_patch_id(F, 0, 1, 0), pw_patch_id(F, 0, 1, 4)
    claims = dict(two_population=True, longer=longer, shorter=shorter, num_lpr=L, probe_height=zp)
    return PwCase(_finish(np.concatenate(parts), rng), mut, claims)


_EXACT = dict(_PLAIN, sensor_height=1.25, adaptive_seed_selection_margin=-1.0, min_range=2.5, max_range=20.0,
              min_ranges=[2.5, 5.0, 10.0, 15.0], th_seeds=0.5, th_dist=0.3)  # every ring 1.25 m


def _bin_boundaries(name):
    """one point on every comparison of k_pw_bin, with exactly representable coordinates (3-4-5 triples scaled by powers
    of two, axis points with signed zeros), each inside a patch of 40 ordinary ground points"""
    rng = np.random.default_rng(_seed(name))
    F = pw_fields(_EXACT)
    h = F["sensor_height"]
    pts, want = [], []  # want: (x, y, z, expected patch id or -1)

    def put(x, y, z, zone=None, ring=None, sector=None):
        pid = -1 if zone is None else pw_patch_id(F, zone, ring, sector)
        want.append((x, y, z, pid))
        if pid >= 0:
            pts.append(_patch(F, rng, zone, ring, sector, 40))

    put(12.0, 16.0, -h, 3, 3, 4)        # r == max_range: kept, the ring index 4 clamps to 3; atan2(4, 3) = 53.1 deg
    put(1.5, 2.0, -h)                   # r == min_range: dropped
    put(3.0, 4.0, -h, 1, 0, 4)          # r == min_ranges[1]: zone 1, ring 0
    put(6.0, 8.0, -h, 2, 0, 7)          # r == min_ranges[2]: zone 2 (54 sectors: 53.13 / 6.67 = 7.97)
    put(9.0, 12.0, -h, 3, 0, 4)         # r == min_ranges[3]
    put(3.75, 5.0, -h, 1, 1, 4)         # r on the ring boundary 6.25 of zone 1: the upper ring
    put(4.0, 0.0, -h, 0, 1, 15)         # atan2 == +0: theta = 2 pi, the last sector
    put(4.0, -0.0, -h, 0, 1, 15)        # atan2 == -0: the same
    put(-4.0, 0.0, -h, 0, 1, 8)         # atan2 == +pi: exactly on the boundary of sector 8
    put(-4.0, -0.0, -h, 0, 1, 8)        # atan2 == -pi -> pi
    put(0.0, 4.0, -h, 0, 1, 4)          # pi / 2: exactly on the boundary of sector 4
    put(-0.0, -4.0, -h, 0, 1, 12)       # -pi / 2 -> 3 pi / 2: sector 12
    put(0.0, 8.0, -h, 1, 2, 8)          # the same in the 32-sector zone: sector 8, ring (8 - 5) / 1.25 = 2
    put(2.5, 1.875, -1.8 * h, 0, 0, 1)  # z == -1.8 sensor_height: kept (and a low point of zone 0); r = 3.125
    put(2.5, 1.875, float(f32(-1.8 * h) - f32(2.0 ** -20)))  # one step below: dropped
    xyz = np.concatenate(pts + [np.array([w[:3] for w in want])])
    n_bulk = xyz.shape[0] - len(want)
    cloud = _finish(xyz)  # (not shuffled: the boundary points are the last rows)
    claims = dict(two_population=True, boundary=[(n_bulk + i, w[3]) for i, w in enumerate(want)])
    return PwCase(cloud, dict(_EXACT), claims)


def _margin_heights(name):
    """The low-point skip of zone 0 is `z < margin`, strictly.  sensor_height 1.25 and a margin factor of -1 make the
    margin height -1.25, a binary32 number.  One patch: 3 low points at -1.45, 40 ground points at exactly -1.25, 40
    points 0.6 m above them and 40 probes 1.3 m above them; num_lpr = 1, one iteration.  The seed height is the first
    height that is not skipped: -1.25, so the seed threshold is -0.25, the probes (+0.05) are no seeds, the plane runs
    0.3 m over the ground and the probes, 1 m over it, are non-ground (th_dist 0.85).  A skip that takes `<=` also
    drops the 40 ground heights: the seed height becomes -0.65, the threshold +0.35, the probes seeds and, 0.67 m over
    a plane through all three levels, ground."""
    rng = np.random.default_rng(_seed(name))
    mut = dict(_PLAIN, sensor_height=1.25, adaptive_seed_selection_margin=-1.0, num_lpr=1, num_iter=1, th_seeds=1.0,
               th_dist=0.85)
    F = pw_fields(mut)
    xyz = _patch(F, rng, 0, 1, 5, 40, n_low=3, n_probe=40, z_probe=-0.65, heavy=[0.05] * 40, noise=0.0)
    claims = dict(two_population=True, margin_block=40, prefix_len=3, level_above=-0.65, probe_height=0.05,
                  patch=pw_patch_id(F, 0, 1, 5))
    return PwCase(_finish(xyz, rng), mut, claims)


def _many_patches(name):
    rng = np.random.default_rng(_seed(name))
    mut = dict(_PLAIN, num_sectors_each_zone=[64] * 4, num_rings_each_zone=[4] * 4, **_NEAR)
    F = pw_fields(mut)
    parts = []
    for pid in BLOCK64_IDS:
        zone, ring, sector = pw_patch_zrs(F, pid)
        parts.append(_patch(F, rng, zone, ring, sector, 10 + pid % 3, n_obj=2 + pid % 2))
    claims = dict(two_population=True, npatch=1024, populated=BLOCK64_IDS)
    return PwCase(_finish(np.concatenate(parts), rng), mut, claims)


def _nonfinite_rows(n):
    return [0, n // 2, n - 1]


def _pw_nonfinite(name, value, coord):
    rng = np.random.default_rng(_seed("pw_nonfinite"))
    F = pw_fields(_PLAIN)
    parts = [_patch(F, rng, z, r, s_, 30, n_obj=6) for z, r, s_ in [(0, 1, 1), (1, 0, 4), (1, 1, 7), (1, 2, 10)]]
    cloud = _finish(np.concatenate(parts), rng)
    rows = _nonfinite_rows(cloud.shape[0])
    was = pw_structure(cloud, F)["patch"][rows]
    cloud[rows, coord] = value
    return PwCase(cloud, dict(_PLAIN), dict(two_population=True, nonfinite_rows=rows, were_in_patches=was.tolist()))


_NONFINITE = {"nan": np.nan, "pinf": np.inf, "ninf": -np.inf}


def pw_case(name):
    rng = np.random.default_rng(_seed(name))
    F = pw_fields(_PLAIN)
    h = F["sensor_height"]
    if name == "signed_zero_heights":
        # the ground plane is z = 0 and every height is +0.0 or -0.0, in an input order that alternates in runs
        mut = dict(_PLAIN, th_seeds=1.0)
        xyz = np.concatenate([_patch(F, rng, 0, 1, 3, 300, n_obj=20, ground_z=0.0, noise=0.0),
                              _patch(F, rng, 1, 1, 7, 40, n_obj=5, ground_z=0.0, noise=0.0)])
        cloud = _finish(xyz, rng)
        flat = np.nonzero(cloud[:, 2] == 0)[0]
        cloud[flat[rng.random(flat.size) < 0.5], 2] = f32(-0.0)
        return PwCase(cloud, mut, dict(two_population=True, signed_zeros=True))
    if name == "equal_heights_many":
        mut = dict(_PLAIN, th_seeds=1.0)
        xyz = _patch(F, rng, 1, 2, 9, 600, n_obj=30, noise=0.0)
        return PwCase(_finish(xyz, rng), mut, dict(two_population=True, equal_heights=600))
    if name == "patch_sizes":
        return _sizes(name, 0.0)
    if name == "patch_sizes_rejected":
        return _sizes(name, 2.0)
    if name == "low_prefix_zone0":
        return _prefix(name, 0)
    if name == "low_prefix_zone1":
        return _prefix(name, 1)
    if name.startswith("num_lpr_"):
        return _num_lpr(name, int(name[8:]))
    if name == "bin_boundaries":
        return _bin_boundaries(name)
    if name == "margin_equal_heights":
        return _margin_heights(name)
    if name == "patches_1024":
        return _many_patches(name)
    if name == "patches_1025":
        mut = dict(_PLAIN, num_sectors_each_zone=[64, 64, 64, 257], num_rings_each_zone=[4, 4, 4, 1])
        return PwCase(_finish(_patch(pw_fields(mut), rng, 0, 0, 0, 20), rng), mut, dict(npatch=1025, refused=PW_REFUSAL))
    if name == "threshold_table":
        # ring + 2 zone against the concentric index: zone 2 ring 0 is concentric 6 and reads entry 4, zone 2 ring 1 is
        # concentric 7 and reads entry 5; entries 4 and 7 reject every elevated patch (flatness 0), 5 and 6 none
        # (elevation +10); entry 1 (zone 0 ring 1) is decided by flatness: elevated, yet flat enough
        ev = [-5.0, -5.0, 10.0, 10.0, -5.0, 10.0, 10.0, -5.0]
        fl = [0.0, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
        mut = dict(num_min_pts=10, num_thr=8, elevation_thr=ev, flatness_thr=fl, **_NEAR)
        F = pw_fields(mut)
        where = [(2, 0, 3), (2, 1, 5), (1, 2, 7), (0, 1, 2), (0, 0, 6), (3, 1, 1)]
        xyz = np.concatenate([_patch(F, rng, z, r, s, 30, n_obj=5) for z, r, s in where])
        want = {pw_patch_id(F, 2, 0, 3): True, pw_patch_id(F, 2, 1, 5): False, pw_patch_id(F, 1, 2, 7): True,
                pw_patch_id(F, 0, 1, 2): False, pw_patch_id(F, 0, 0, 6): True, pw_patch_id(F, 3, 1, 1): False}
        return PwCase(_finish(xyz, rng), mut, dict(two_population=True, rejected=want))
    if name == "global_threshold":
        mut = dict(num_min_pts=10, using_global_thr=1, global_elevation_thr=-5.0, **_NEAR)
        F = pw_fields(mut)
        xyz = np.concatenate([_patch(F, rng, 2, 0, 3, 30, n_obj=5), _patch(F, rng, 0, 0, 3, 30, n_obj=5)])
        want = {pw_patch_id(F, 2, 0, 3): True, pw_patch_id(F, 0, 0, 3): False}
        return PwCase(_finish(xyz, rng), mut, dict(two_population=True, rejected=want))
    if name.startswith("points_"):
        P = int(name[7:])
        n_obj = P // 8
        xyz = _patch(F, rng, 1, 1, 5, P - n_obj, n_obj=n_obj)
        return PwCase(_finish(xyz, rng), dict(_PLAIN), dict(two_population=True, points=P))
    if name == "all_dropped":
        n = 300
        t = rng.uniform(0, 2 * np.pi, n)
        r = np.where(np.arange(n) % 3 == 0, rng.uniform(0.1, 2.6, n), rng.uniform(80.5, 200.0, n))
        z = np.full(n, -h)
        r[np.arange(n) % 3 == 2] = 20.0
        z[np.arange(n) % 3 == 2] = -1.8 * h - 0.5
        return PwCase(_finish(np.stack([r * np.cos(t), r * np.sin(t), z], axis=1)), dict(_PLAIN), dict(all_dropped=True))
    if name == "one_patch_survives":
        parts = [_patch(F, rng, z, 0, 2 * z + 1, 10) for z in range(4)] + [_patch(F, rng, 1, 2, 20, 9, n_obj=2)]
        return PwCase(_finish(np.concatenate(parts), rng), dict(_PLAIN),
                      dict(two_population=True, survivor=pw_patch_id(F, 1, 2, 20)))
    if name == "empty_seed_set":
        mut = dict(_PLAIN, th_seeds=-5.0)
        parts = [_patch(F, rng, z, 1, 3 * z, 30, n_obj=6) for z in range(4)]
        return PwCase(_finish(np.concatenate(parts), rng), mut, dict(all_nonground=True))
    if name.startswith("nonfinite_"):
        _, v, c = name.split("_")
        return _pw_nonfinite(name, _NONFINITE[v], "xyz".index(c))
    raise KeyError(name)


PW_NONFINITE_NAMES = [f"nonfinite_{v}_{c}" for v in _NONFINITE for c in "xyz"]
PW_NAMES = (["signed_zero_heights", "equal_heights_many", "patch_sizes", "patch_sizes_rejected", "low_prefix_zone0",
             "low_prefix_zone1", "num_lpr_1", "num_lpr_256", "num_lpr_257", "num_lpr_600", "bin_boundaries", "margin_equal_heights",
             "patches_1024", "threshold_table", "global_threshold", "points_1", "points_255", "points_256",
             "points_257", "all_dropped", "one_patch_survives", "empty_seed_set"] + PW_NONFINITE_NAMES)
PW_REFUSED_NAMES = ["patches_1025"]


# ============================================================================================== range-image references
def ip_fields(H=100, n_scan=8, mode="4Neighbor", num_min_pts=30):
    ry = 2.0 if n_scan <= 16 else 1.0
    return dict(n_scan=n_scan, horizon_scan=H, ang_res_x=float(f32(360.0) / f32(H)), ang_res_y=ry,
                ang_bottom=float(f32(ry * n_scan / 2)), neighbor_mode=MODES[mode], num_min_pts=num_min_pts,
                segment_theta=THETA, valid_point_num=5, valid_line_num=3)


def pixel_point(ip, row, col, rng):
    """a point at the centre of pixel (row, col)'s angular cell, at range rng"""
    H = ip["horizon_scan"]
    va = np.deg2rad((row + 0.5) * ip["ang_res_y"] - ip["ang_bottom"])
    ha = 90.0 + (H // 2 - col) * ip["ang_res_x"]  # column = -round((ha - 90) / res_x) + H / 2, wrapped at H
    if ha > 180.0:
        ha -= 360.0
    ha = np.deg2rad(ha)
    return np.array([rng * np.cos(va) * np.sin(ha), rng * np.cos(va) * np.cos(ha), rng * np.sin(va)])


def _atan2f(y, x):
    with np.errstate(invalid="ignore"):
        return np.arctan2(y.astype(f64), x.astype(f64)).astype(f32)


def _deg(a):
    return ((a * f32(180)).astype(f64) / np.pi).astype(f32)


def _trunc_ll(v):
    """(long long) of a double the way x86-64 converts: NaN and anything out of range -> the most negative value"""
    v = np.asarray(v, dtype=f64)
    bad = ~np.isfinite(v) | (np.abs(v) >= 2.0 ** 63)
    return np.where(bad, -2 ** 63, np.trunc(np.where(bad, 0, v))).astype(np.int64)


def ip_pixels(cloud, ip):
    """projectPointCloud's arithmetic, step by step in binary32 (binary64 where the reference uses it).
    -> dict(pixel [P] (row * H + col, -1: no pixel), range [P] binary32, rf [P], column_raw [P] (before the wrap))"""
    H, NS = ip["horizon_scan"], ip["n_scan"]
    x, y, z = (np.ascontiguousarray(cloud[:, i], dtype=f32) for i in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        va = _deg(_atan2f(z, np.sqrt(x * x + y * y)))
        rf = (va + f32(ip["ang_bottom"])) / f32(ip["ang_res_y"])
        r = _trunc_ll(rf)
        ha = _deg(_atan2f(x, y))
        q = (ha.astype(f64) - 90.0) / f64(f32(ip["ang_res_x"]))
        rq = np.sign(q) * np.floor(np.abs(q) + 0.5)  # C's round(): halves away from zero
        cd = -rq + f64(H // 2)
        c0 = _trunc_ll(cd)
        c = np.where(c0 >= H, c0 - H, c0)
        rg = np.sqrt(x * x + y * y + z * z)
        ok = (r >= 0) & (r < NS) & (c0 >= 0) & (c >= 0) & (c < H) & ~(rg.astype(f64) < 0.1)
        ok &= ~(np.isnan(x) | np.isnan(y) | np.isnan(z))
    return dict(pixel=np.where(ok, r * H + c, -1), range=rg, rf=rf, column_raw=c0)


def ip_trig(ip):
    out = []
    for res in (ip["ang_res_x"], ip["ang_res_y"]):
        a = f64(f32(f64(f32(res)) / 180.0 * np.pi))
        out += [f32(np.sin(a)), f32(np.cos(a))]
    return out  # sx, cx, sy, cy


def _edge_angle(ra, rb, sn, cs):
    d1, d2 = (ra, rb) if ra > rb else (rb, ra)
    with np.errstate(invalid="ignore", over="ignore"):
        return f32(np.arctan2(f64(f32(d2 * sn)), f64(f32(d1 - f32(d2 * cs)))))


_FORWARD = {0: [(0, 1), (1, 0)], 1: [(0, 1), (1, 0), (1, 1), (1, -1)], 2: [(1, 1), (1, -1)]}


def ip_label(cloud, ip, wrap=True):
    """-> dict(labels [n_scan, H] (-1 empty, 999999 outlier, 1.. valid), valid [nv, 4], outliers [no, 4], n_segments,
    components: list of (first pixel, size, rows counted, valid) in row-major order of first pixels, angle_margin_deg:
    smallest distance of a neighbouring pair's angle from segment_theta, in degrees)"""
    H, NS = ip["horizon_scan"], ip["n_scan"]
    px = ip_pixels(cloud, ip)
    owner = {}
    for i in np.nonzero(px["pixel"] >= 0)[0]:
        owner[int(px["pixel"][i])] = int(i)  # ascending i: the last writer wins
    sx, cx, sy, cy = ip_trig(ip)
    parent = {p: p for p in owner}

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    theta, margin = f32(ip["segment_theta"]), np.inf
    for p in sorted(owner):
        r, c = divmod(p, H)
        for dr, dc in _FORWARD[ip["neighbor_mode"]]:
            rr, cc = r + dr, c + dc
            if rr >= NS:
                continue
            if cc < 0 or cc >= H:
                if not wrap:
                    continue
                cc = H - 1 if cc < 0 else 0
            q = rr * H + cc
            if q not in owner or q == p:
                continue
            ang = _edge_angle(px["range"][owner[p]], px["range"][owner[q]], sx if dr == 0 else sy, cx if dr == 0 else cy)
            if not np.isnan(ang):
                margin = min(margin, abs(np.rad2deg(f64(ang)) - np.rad2deg(f64(theta))))
            if ang > theta:
                a, b = find(p), find(q)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    comps = {}
    for p in sorted(owner):
        comps.setdefault(find(p), []).append(p)
    labels = np.full(NS * H, -1, dtype=np.int32)
    components, n_seg = [], 0
    for first in sorted(comps):
        mem = comps[first]
        assert first == mem[0]
        rows = len({p // H for p in mem[1:]})
        ok = len(mem) >= ip["num_min_pts"] or (len(mem) >= ip["valid_point_num"] and rows >= ip["valid_line_num"])
        if ok:
            n_seg += 1
        labels[mem] = n_seg if ok else IP_OUTLIER
        components.append((first, len(mem), rows, ok))
    valid, outl = [], []
    for p in sorted(owner):
        q = cloud[owner[p]].copy()
        if labels[p] == IP_OUTLIER:
            q[3] = f32(p // H) + f32(p % H) / f32(10000.0)
            outl.append(q)
        else:
            q[3] = f32(labels[p])
            valid.append(q)
    as4 = lambda rows_: np.array(rows_, dtype=f32).reshape(-1, 4)
    return dict(labels=labels.reshape(NS, H), valid=as4(valid), outliers=as4(outl), n_segments=n_seg,
                components=components, angle_margin_deg=float(margin), pixels=px, owner=owner)


# ============================================================================================== range-image builders
def _from_image(ip, img, rng=None):
    """img {(row, col): range} -> cloud of pixel-centre points (shuffled when rng is given)"""
    pts = [pixel_point(ip, r, c, g) for (r, c), g in sorted(img.items())]
    return _finish(np.array(pts).reshape(-1, 3), rng)


def _random_levels(ip, rng, fill=0.7):
    return {(r, c): (10.0 if rng.random() < 0.6 else 20.0) for r in range(ip["n_scan"]) for c in range(ip["horizon_scan"])
            if rng.random() < fill}


def _shape(shape, ip):
    H, NS = ip["horizon_scan"], ip["n_scan"]
    if shape == "whole":      # one range everywhere
        return {(r, c): 10.0 for r in range(NS) for c in range(H)}
    if shape == "snake_axis":  # down a column, across the bottom / top row to the column after next, back up, ...
        img, c, down = {}, 0, True
        while c < H - 2:
            for r in range(NS):
                img[(r, c)] = 10.0
            img[(NS - 1 if down else 0, c + 1)] = 10.0
            c, down = c + 2, not down
        return img
    if shape == "snake_diag":  # one pixel per column, the row a triangle wave: every step is a diagonal one
        per = 2 * (NS - 1)
        return {((t % per) if (t % per) < NS else per - (t % per), t): 10.0 for t in range(H)}
    if shape == "seam_axis":   # joined only by the horizontal step from column H - 1 to column 0
        return {(2, H - 2): 10.0, (2, H - 1): 10.0, (2, 0): 10.0, (2, 1): 10.0}
    if shape == "seam_diag":   # joined only by the diagonal step across the seam
        return {(1, H - 2): 10.0, (2, H - 1): 10.0, (3, 0): 10.0, (4, 1): 10.0}
    if shape == "singletons":  # four range levels by (row, column) parity: no two neighbours share one
        lev = [10.0, 20.0, 40.0, 80.0]
        return {(r, c): lev[(r % 2) * 2 + c % 2] for r in range(NS) for c in range(H)}
    raise KeyError(shape)


# (shape, mode) -> number of components the case claims.  A shape in a mode that does not connect it falls apart: the
# diagonal snake and the seam shapes into single pixels; the axis snake in the cross mode keeps only the turns (a connector
# and the last-but-one pixel of the one or two columns beside it): 441 pixels less two for each of 48 connectors, one for
# the last
SHAPES = {("snake_axis", "4CrossNeighbor"): 344, ("snake_diag", "4Neighbor"): 100, ("seam_axis", "4CrossNeighbor"): 4,
          ("seam_diag", "4Neighbor"): 4, ("whole", "4Neighbor"): 1, ("whole", "8Neighbor"): 1, ("whole", "4CrossNeighbor"): 2,
          ("snake_axis", "4Neighbor"): 1, ("snake_axis", "8Neighbor"): 1, ("snake_diag", "8Neighbor"): 1,
          ("snake_diag", "4CrossNeighbor"): 1, ("seam_axis", "4Neighbor"): 1, ("seam_axis", "8Neighbor"): 1,
          ("seam_diag", "8Neighbor"): 1, ("seam_diag", "4CrossNeighbor"): 1, ("singletons", "4Neighbor"): 800,
          ("singletons", "8Neighbor"): 800, ("singletons", "4CrossNeighbor"): 800}


def _corners(ip):
    img = {}
    for c in range(29):
        img[(0, 2 + c)] = 10.0                                   # 29 in one row: one short of num_min_pts = 30
    for c in range(30):
        img[(0, 40 + c)] = 10.0                                  # 30 in one row
    for rc in [(2, 5), (3, 5), (3, 6), (4, 5), (4, 6)]:
        img[rc] = 10.0        # 5 over three rows, the first row holding only the first pixel: 2 rows counted
    for rc in [(2, 15), (2, 16), (3, 15), (4, 15), (4, 16)]:
        img[rc] = 10.0        # 5 over three rows, a second pixel in the first row: 3 rows counted
    for r in range(4):
        img[(2 + r, 25)] = 10.0                                  # 4 over four rows
    for r in range(5):
        img[(2 + r, 35)] = 10.0                                  # 5 over five rows: 4 counted
    return img


def _big_image(ip, rng):
    H = ip["horizon_scan"]
    img, blocks = {}, [0, 63, 64, 127, 128, 255, 256, 511]
    for b in blocks:  # 8 blocks of 1024 pixels to a row
        r, c0 = divmod(b * IP_BLOCK, H)
        for c in range(30):
            img[(r, c0 + 100 + c)] = 10.0   # a valid run whose first pixel (the root) is inside the block
        img[(r, c0 + 500)] = 10.0            # an outlier
        img[(r, c0 + 700)] = 20.0            # another, at the other level
    for c in range(2000):
        img[(40, 3000 + c)] = 10.0           # one long component across two blocks
    used_rows = {divmod(b * IP_BLOCK, H)[0] for b in blocks} | {40}
    for _ in range(1500):                    # sparse singletons: rows and columns two apart, away from the rows above
        r, c = 2 * int(rng.integers(1, 31)), 2 * int(rng.integers(0, H // 2))
        if not ({r - 1, r, r + 1} & used_rows):
            img[(r, c)] = 10.0
    return img, blocks


def ip_case(name):
    rng = np.random.default_rng(_seed(name))
    if name.startswith("width_"):
        H = int(name[6:])
        ip = ip_fields(H=H, mode="8Neighbor", num_min_pts=12)
        return IpCase(_from_image(ip, _random_levels(ip, rng), rng), ip, dict(width=H))
    if name.startswith("rows_"):
        NS = int(name[5:])
        ip = ip_fields(H=100, n_scan=NS, mode="4Neighbor", num_min_pts=30)
        img = _random_levels(ip, rng, fill=0.5)
        for r in range(NS):
            img[(r, 7)] = 40.0  # a column at a level of its own: one component through every row, the last included
        claims = dict(rows=NS, column=7)
        if NS == 64:
            # two components of 5 at a level of their own whose verdict hangs on row 63: the first row holds the first
            # pixel and one more, so rows 61, 62, 63 are counted, three, and without row 63 two.  At H = 100 the wave of
            # k_ip_flatten_agg that holds (63, 10) starts in row 62 (the bit comes from its second row), the wave that
            # holds (63, 50) lies in row 63
            for c0 in (10, 50):
                for rc in [(61, c0), (61, c0 + 1), (62, c0), (63, c0), (63, c0 + 1)]:
                    img[rc] = 80.0
            claims["hang_on_row_63"] = [(61 * 100 + 10, True), (61 * 100 + 50, False)]  # (first pixel, wave straddles)
        return IpCase(_from_image(ip, img, rng), ip, claims)
    if name == "pixels_1016":
        ip = ip_fields(H=127, mode="4CrossNeighbor", num_min_pts=10)
        return IpCase(_from_image(ip, _random_levels(ip, rng), rng), ip, dict(np=1016))
    if name.startswith("shape_"):
        shape, mode = name[6:].rsplit("_", 1)
        ip = ip_fields(mode=mode)
        return IpCase(_from_image(ip, _shape(shape, ip), rng), ip,
                      dict(components=SHAPES[(shape, mode)], seam=shape.startswith("seam") and SHAPES[(shape, mode)] == 1))
    if name == "parity_odd_width":
        ip = ip_fields(H=101, mode="4CrossNeighbor")
        return IpCase(_from_image(ip, _shape("whole", ip), rng), ip, dict(components=1))
    if name in ("validity_corners", "validity_corners_min1"):
        ip = ip_fields(num_min_pts=30 if name == "validity_corners" else 1)
        want = [(29, 1, False), (30, 1, True), (5, 2, False), (5, 3, True), (4, 3, False), (5, 4, True)]
        if ip["num_min_pts"] == 1:
            want = [(s, r, True) for s, r, _ in want]
        # row-major order of first pixels: the two runs of row 0, then the four blobs of row 2 by column
        return IpCase(_from_image(ip, _corners(ip), rng), ip, dict(corner_components=want))
    if name == "last_writer":
        # 500 returns in pixel (3, 50) at ranges 10 .. 11 in no order, the last of them at 20; its neighbours: (3, 51) at
        # 20 (joined only if the last return owns the pixel) and (3, 49) at 10.5 (joined if any other does)
        ip = ip_fields(num_min_pts=2)
        rg = 10.0 + rng.random(500)
        rg[-1] = 20.0
        pts = [pixel_point(ip, 3, 49, 10.5), pixel_point(ip, 3, 51, 20.0)] + [pixel_point(ip, 3, 50, g) for g in rg]
        return IpCase(_finish(np.array(pts)), ip, dict(owner_pixel=3 * 100 + 50, owner_index=501, joined=(3, 51)))
    if name == "axes_signed_zero":
        ip = ip_fields(num_min_pts=1)
        xy = [(8.0, 0.0), (8.0, -0.0), (-8.0, 0.0), (-8.0, -0.0), (0.0, 8.0), (-0.0, 8.0), (0.0, -8.0), (-0.0, -8.0)]
        pts = [(x, y, -1.0 + 0.28 * i) for i, (x, y) in enumerate(xy)]  # point i lands in row i
        cols = [50, 50, 0, 0, 75, 75, 25, 25]
        return IpCase(_finish(np.array(pts)), ip, dict(columns=cols, wrapped=[2, 3, 7]))
    if name == "row_fraction_and_range":
        ip = ip_fields(num_min_pts=1)
        below = pixel_point(ip, 0, 20, 10.0)
        va = np.deg2rad(-ip["ang_bottom"] - 0.25 * ip["ang_res_y"])  # rf = -0.25: truncates to row 0
        below[:2] *= np.cos(va) / np.hypot(below[0], below[1]) * 10.0
        below[2] = 10.0 * np.sin(va)
        under = pixel_point(ip, 0, 30, 10.0)
        va = np.deg2rad(-ip["ang_bottom"] - 1.5 * ip["ang_res_y"])   # rf = -1.5: row -1, no pixel
        under[:2] *= np.cos(va) / np.hypot(under[0], under[1]) * 10.0
        under[2] = 10.0 * np.sin(va)
        pts = [below, under, pixel_point(ip, 4, 60, 0.0999), pixel_point(ip, 4, 70, 0.1001)]
        return IpCase(_finish(np.array(pts)), ip, dict(pixels=[20, -1, -1, 4 * 100 + 70]))
    if name == "big_image":
        ip = ip_fields(H=8192, n_scan=64, num_min_pts=30)
        img, blocks = _big_image(ip, rng)
        return IpCase(_from_image(ip, img, rng), ip, dict(blocks=blocks, long_component=2000))
    if name.startswith("nonfinite_"):
        _, v, c = name.split("_")
        ip = ip_fields(mode="8Neighbor", num_min_pts=10)
        g = np.random.default_rng(_seed("ip_nonfinite"))
        img = _random_levels(ip, g)
        for c0 in range(3):
            img.pop((0, c0), None)  # nothing near pixel (0, 0): a point that lands there by mistake shows
            img.pop((1, c0), None)
        cloud = _from_image(ip, img, g)
        rows = _nonfinite_rows(cloud.shape[0])
        cloud[rows, "xyz".index(c)] = _NONFINITE[v]
        return IpCase(cloud, ip, dict(nonfinite_rows=rows, nan=(v == "nan")))
    raise KeyError(name)


IP_NONFINITE_NAMES = [f"nonfinite_{v}_{c}" for v in _NONFINITE for c in "xyz"]
IP_SMALL_NAMES = ([f"width_{H}" for H in (4, 63, 64, 65, 127, 128)] + [f"rows_{n}" for n in (1, 3, 64)] +
                  ["pixels_1016"] + [f"shape_{s}_{m}" for s, m in SHAPES] +
                  ["parity_odd_width", "validity_corners", "validity_corners_min1", "last_writer", "axes_signed_zero",
                   "row_fraction_and_range"] + IP_NONFINITE_NAMES)
IP_NAMES = IP_SMALL_NAMES + ["big_image"]
