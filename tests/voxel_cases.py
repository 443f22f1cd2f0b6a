"""Named clouds for the voxel grid of quatro_amd/csrc/frontend.hip (k2_minmax, k2_keys_hist, k2_radix_scatter,
k2_vox_centroids), each placed at a constant the kernels branch on: the centroid kernel's window (a tile of 256 or 1024
sorted points plus a halo of 512), the radix tile of 1024 keys, the 8 / 16 / 24-bit borders of the adaptive sort, the
grid stride of the bounding-box kernel, and the int32 edge of pcl::VoxelGrid's index arithmetic.  A plain module:
deterministic numpy generators with fixed seeds, no fixtures, no GPU work.  Used by tests/test_voxel_cases_cpu.py (the
oracle against the restatement below, every cloud against what it claims, every cloud against the wrong variants it
was built to catch) and tests/test_gpu_voxel_cases.py (the device against the oracle, bit for bit, on every route that
runs the voxel stage).

    case(name) -> (cloud float32 [P, 4], leaf, claims dict)

The stage is bit-exact by contract: nothing here has a tolerance.

voxelize_numpy() restates the operation independently of the oracle's C++: bounding box, the overflow verdict from the
TRUNCATED extents `(long)((max - min) * inv) + 1`, pass-through when their product exceeds INT32_MAX, cell indices
`floor(p * inv) - floor(min * inv)` in binary32, the linear index in int32 with explicit two's-complement wrap, order by
(index as uint32, point number), centroids summed in binary32 in that order.  Its `variant` argument names deliberately
wrong forms of the same operation; the CPU test asserts that each changes the output bits of the cases built for it.
"""
from collections import namedtuple

import numpy as np

f32 = np.float32

# ---------------------------------------------------------------------------------------------- mirrored constants
VOX_TILES = (256, 1024)   # frontend.hip: VOX_TILE_SINGLE (one cloud or pair at a time), VOX_TILE_BATCH (qtr_submit_batch)
VOX_HALO = 512            # sorted points a tile stages behind its own; a longer run goes on from global memory
RADIX_TILE = 1024         # keys per workgroup of a radix pass
MM_STRIDE = 128 * 256     # MM_MAX_PARTS workgroups of 256 threads: points per grid-stride round of k2_minmax
INT32_MAX = 2 ** 31 - 1

LAYOUT_LEAF = 1.0
LAYOUT_ORIGIN = 4096.0    # sums of a few values near 4096 round in binary32: their order shows in the bits
DIGITS_LEAF = 0.25


def _seed(name):
    return [ord(c) for c in name]


def _pack(xyz):
    c = np.zeros((xyz.shape[0], 4), dtype=f32)
    c[:, :3] = xyz
    return c


def _bits(cells):
    """significant bits of the largest linear index: what CNT_SORT_BITS must say (1 for one cell, 32 for a wrapped grid)"""
    return 1 if cells <= 1 else min(32, int(cells - 1).bit_length())


# ---------------------------------------------------------------------------------------------- the restatement
def _wrap32(x):
    return ((np.asarray(x, dtype=np.int64) + 2 ** 31) & 0xffffffff) - 2 ** 31


Grid = namedtuple("Grid", "passed trunc dims bits keys")

VARIANTS = ("reversed", "ties_descending", "truncate_window", "lose_last", "gain_next", "heads_per_tile",
            "sort_8_bits", "sort_16_bits", "sort_24_bits", "keys_int64", "keys_signed", "verdict_floor")


def grid(cloud, leaf, variant=None):
    """-> Grid(passed, truncated extents, floor-difference dimensions, key bits, keys int64 [P] in the order domain).
    The keys are the uint32 view of the wrapped int32 index; variant keys_int64: the index without any wrap;
    keys_signed: the wrapped index compared as int32; verdict_floor: pass-through decided by the floor-difference
    dimensions, which make the keys, instead of the truncated extents."""
    p = np.ascontiguousarray(cloud[:, :3], dtype=f32)
    inv = f32(1.0) / f32(leaf)
    mn, mx = p.min(0), p.max(0)
    trunc = [int(np.trunc(f32(f32(mx[a] - mn[a]) * inv))) + 1 for a in range(3)]
    minb = [int(np.floor(f32(mn[a] * inv))) for a in range(3)]
    maxb = [int(np.floor(f32(mx[a] * inv))) for a in range(3)]
    dims = [maxb[a] - minb[a] + 1 for a in range(3)]
    verdict = dims if variant == "verdict_floor" else trunc
    passed = verdict[0] * verdict[1] * verdict[2] > INT32_MAX
    bits = 32 if passed else _bits(dims[0] * dims[1] * dims[2])
    if passed:
        return Grid(True, trunc, dims, bits, None)
    ijk = (np.floor(p * inv) - np.array(minb, dtype=f32)).astype(f32).astype(np.int64)
    if variant == "keys_int64":
        keys = ijk[:, 0] + ijk[:, 1] * dims[0] + ijk[:, 2] * (dims[0] * dims[1])
    else:
        mul1 = _wrap32(dims[0])
        mul2 = _wrap32(mul1 * _wrap32(dims[1]))
        idx = _wrap32(_wrap32(ijk[:, 0] + _wrap32(ijk[:, 1] * mul1)) + _wrap32(ijk[:, 2] * mul2))
        keys = idx if variant == "keys_signed" else idx & 0xffffffff
    return Grid(False, trunc, dims, bits, keys)


Plan = namedtuple("Plan", "passed bits order keys starts lengths")


def plan(cloud, leaf):
    """the sorted keys of the right operation and their runs: what the claims are checked on"""
    g = grid(cloud, leaf)
    if g.passed:
        return Plan(True, g.bits, None, None, None, None)
    order = np.lexsort((np.arange(g.keys.size), g.keys))
    ks = g.keys[order]
    starts = np.nonzero(np.r_[True, ks[1:] != ks[:-1]])[0]
    return Plan(False, g.bits, order, ks, starts, np.diff(np.r_[starts, ks.size]))


def voxelize_numpy(cloud, leaf, variant=None, tile=None):
    """-> [n, 4] float32 (w = 0), or the cloud itself when the grid overflows int32.  `tile` (one of VOX_TILES) is what the
    window variants need: the window of a run that starts at sorted position i ends at (i // tile) * tile + tile + VOX_HALO.
      reversed          the points of a voxel are added up in descending order
      ties_descending   the sort breaks ties between equal keys by descending point number
      truncate_window   a run ends where its tile's window ends
      lose_last         a run that reaches its window's end (ends there or beyond) loses its last point
      gain_next         ... gains the first point of the next voxel
      heads_per_tile    a tile takes its first element for a run's head without looking at the key in front of it
      sort_N_bits       the keys are sorted on their lowest N bits only
      keys_int64, keys_signed, verdict_floor   see grid()"""
    assert variant is None or variant in VARIANTS
    cloud = np.ascontiguousarray(cloud, dtype=f32)
    g = grid(cloud, leaf, variant)
    if g.passed:
        return cloud.copy()
    P = cloud.shape[0]
    number = np.arange(P)
    by = g.keys & ((1 << int(variant.split("_")[1])) - 1) if variant and variant.startswith("sort_") else g.keys
    order = np.lexsort((-number if variant == "ties_descending" else number, by))
    ks = g.keys[order]
    change = np.r_[True, ks[1:] != ks[:-1]]
    head = change.copy()
    if variant == "heads_per_tile":
        head[::tile] = True
    starts = np.nonzero(head)[0]
    run_first = np.nonzero(change)[0]
    run_end = np.r_[run_first[1:], P]
    ends = run_end[np.searchsorted(run_first, starts, side="right") - 1]  # a run's sum follows the keys, not the heads
    if variant in ("truncate_window", "lose_last", "gain_next"):
        wend = (starts // tile) * tile + tile + VOX_HALO
        if variant == "truncate_window":
            ends = np.minimum(ends, wend)
        elif variant == "lose_last":
            ends = np.where(ends >= wend, ends - 1, ends)
        else:
            ends = np.where((ends >= wend) & (ends < P), ends + 1, ends)
    lengths = ends - starts
    pts = cloud[order, :3]
    acc = np.zeros((starts.size, 3), dtype=f32)
    longest_first = np.argsort(-lengths, kind="stable")
    sorted_len = lengths[longest_first]
    for k in range(int(lengths.max())):
        live = longest_first[:np.searchsorted(-sorted_len, -k, side="left")]  # the runs longer than k
        at = ends[live] - 1 - k if variant == "reversed" else starts[live] + k
        acc[live] = acc[live] + pts[at]
    out = np.zeros((starts.size, 4), dtype=f32)
    out[:, :3] = acc / lengths.astype(f32)[:, None]
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=f32), np.ascontiguousarray(b, dtype=f32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


# ---------------------------------------------------------------------------------------------- family `layout`
def _layout_cloud(seed, lengths):
    """One voxel per entry of `lengths`, in a row along x at leaf 1: voxel c holds lengths[c] points 4096 + c + u in x and
    4096 + u in y and z, u in [0.05, 0.95).  The input order is a fixed random permutation of all points."""
    rng = np.random.default_rng(seed)
    cell = np.repeat(np.arange(len(lengths)), lengths)
    xyz = rng.uniform(0.05, 0.95, (cell.size, 3)) + LAYOUT_ORIGIN
    xyz[:, 0] += cell
    return _pack(xyz.astype(f32)[rng.permutation(cell.size)])


def must_change(variant, start, n, tile, P):
    """whether a wrong variant must change the centroid of the run of n points at sorted position `start`: the order
    variants every run of three or more (a + b = b + a), the window variants the runs at their window's end.  Used to
    choose the seeds only: tests/test_voxel_cases_cpu.py asserts with a predicate of its own (_expected, written from
    how far a run ends behind its window), on purpose — a slip here would otherwise choose seeds that agree with it."""
    if variant in ("reversed", "ties_descending"):
        return n >= 3
    end, wend = start + n, (start // tile) * tile + tile + VOX_HALO if tile else P + 1
    return {"truncate_window": end > wend, "lose_last": end >= wend, "gain_next": end >= wend and end < P}[variant]


def _tells(cloud, lengths, named, tile):
    """the seed's test: every named run's centroid changes under exactly the variants that must change it (a mean of
    1500 values near 4096 can round to the same binary32 with one point less)"""
    right = voxelize_numpy(cloud, LAYOUT_LEAF)
    first = np.cumsum(np.r_[0, lengths])
    for variant in ("reversed", "truncate_window", "lose_last", "gain_next"):
        if tile is None and variant != "reversed":
            continue
        wrong = voxelize_numpy(cloud, LAYOUT_LEAF, variant, tile)
        for start, n in named:
            row = int(np.searchsorted(first, start))
            if same_bits(wrong[row], right[row]) == must_change(variant, start, n, tile, cloud.shape[0]):
                return False
    return True


def _place(T, spec, lead=(), trail=0):
    """run lengths in voxel order: the runs of `lead`, then every (s, length) of spec behind as much singleton filler as
    puts its start at offset s of a tile (a whole tile of it where none would be needed between two named runs), then
    `trail` singletons -> (lengths, [(start, length)] of the named runs)"""
    lengths, named, pos = list(lead), [], sum(lead)
    for s, n in spec:
        fill = (s - pos) % T
        if fill == 0 and named:
            fill = T
        lengths += [1] * fill
        pos += fill
        named.append((pos, n))
        lengths.append(n)
        pos += n
    return lengths + [1] * trail, named


def _layout_spec(group, T):
    H, W = VOX_HALO, T + VOX_HALO
    if group == "from_start":    # the last LDS element, then the first, eighth and ninth element from global memory
        return _place(T, [(0, n) for n in (W - 1, W, W + 1, W + 7, W + 8, W + 9)], trail=3)
    if group == "tile_last":     # a run that starts on a tile's last element; H + 1 ends exactly at the window's end
        return _place(T, [(T - 1, n) for n in (1, 2, H, H + 1, H + 2, H + 9, H + 10)], trail=3)
    if group == "scalar_rest":   # W - s = H + 4: the scalar loop behind the 8-wide one takes the window's last 4
        return _place(T, [(T - 4, n) for n in (H + 3, H + 4, H + 5)], trail=3)
    if group == "headless":      # whole tiles without a head (at T = 256 the run also goes on from global memory)
        return _place(T, [(T // 2, 3 * T)], trail=3)
    if group == "last_global":   # the cloud's last run ends at P inside an 8-wide round of global loads
        return _place(T, [(5, W + 3)], lead=(3, 1, 2))  # (8 elements behind the window: the round after them lies wholly past P)
    if group == "last_global_mid":  # ... 4 elements behind the window: P falls in the middle of a round
        return _place(T, [(5, W - 1)], lead=(3, 1, 2, 2))
    if group == "last_single":   # the cloud's last run is one point: P = k T + 1
        return _place(T, [(0, 1)], lead=(3, 1, 2) + (1,) * (2 * T - 6))
    if group == "last_full":     # the cloud's last run ends exactly at a tile's end: P = k T
        return _place(T, [(T - 7, 7)], lead=(3, 1, 2) + (1,) * T)
    if group == "singles_3t":
        return [1] * (3 * T), []
    if group == "singles_3t1":
        return [1] * (3 * T + 1), []
    raise KeyError(group)


LAYOUT_GROUPS = ("from_start", "tile_last", "scalar_rest", "headless", "last_global", "last_global_mid", "last_single",
                 "last_full", "singles_3t", "singles_3t1")
WINDOW_EDGE_GROUPS = ("from_start", "tile_last", "scalar_rest", "headless", "last_global", "last_global_mid")
TINY = {"tiny_1": [1], "tiny_2_one_voxel": [2], "tiny_2_two_voxels": [1, 1]}
for _n in (255, 256, 257):
    TINY[f"tiny_{_n}_one_run"] = [_n]
    TINY[f"tiny_{_n}_singletons"] = [1] * _n


def layout_names(T):
    return tuple(f"{g}_t{T}" for g in LAYOUT_GROUPS)


def window_edge_names(T):
    return tuple(f"{g}_t{T}" for g in WINDOW_EDGE_GROUPS)


TINY_NAMES = tuple(TINY)
LAYOUT_NAMES = layout_names(256) + layout_names(1024) + TINY_NAMES
WINDOW_EDGE_NAMES = window_edge_names(256) + window_edge_names(1024)


def _layout(name):
    if name in TINY:
        T, lengths = None, TINY[name]
        named = [(0, lengths[0])] if len(lengths) == 1 else []
    else:
        group, t = name.rsplit("_t", 1)
        T = int(t)
        lengths, named = _layout_spec(group, T)
    # The first seed of the name's row whose named runs tell every wrong variant from the right one.  The generator thus
    # depends on the variants being what they say: the CPU test's run-by-run assertions against the oracle are what holds
    # them to it (a variant that changed nothing, or everything, would fail there for every seed).
    for attempt in range(32):
        cloud = _layout_cloud(_seed(name) + [attempt], lengths)
        if _tells(cloud, lengths, named, T):
            break
    else:
        raise AssertionError(name)
    # runs: (sorted position of the run's first point, length) of every named run; a named run starts at
    # `start % tile` of its tile and its window ends at (start // tile) * tile + tile + VOX_HALO
    return cloud, LAYOUT_LEAF, dict(tile=T, runs=named, n_voxels=len(lengths), key_bits=_bits(len(lengths)), passed=False)


# ---------------------------------------------------------------------------------------------- family `digits`
DIGITS = {  # name: (cell dimensions, P)
    "bits_1": ((1, 1, 1), 1025),
    "bits_8": ((256, 1, 1), 3 * 1024 + 1),
    "bits_16": ((256, 256, 1), 3 * 1024 + 1),
    "bits_24": ((256, 256, 256), 3 * 1024 + 1),
    "bits_25": ((257, 256, 256), 3 * 1024 + 1),
    "few_digits": ((256, 40, 1), 4 * 1024 + 1),
    "tiles_33": ((256, 256, 1), 32 * 1024 + 1),
}
for _p in (1023, 1024, 1025):
    DIGITS[f"bits_9_p{_p}"] = ((257, 1, 1), _p)
    DIGITS[f"bits_17_p{_p}"] = ((257, 256, 1), _p)
DIGITS_NAMES = tuple(DIGITS)
DIGITS_ORIGIN = np.array([-100, 37, -3])  # cell coordinates of the box's minimum cell: the box spans zero in x and z
# the cases just above each border of the adaptive sort: what a sort on only that many bits must get wrong
JUST_ABOVE = {8: tuple(n for n in DIGITS if n.startswith("bits_9_")), 16: tuple(n for n in DIGITS if n.startswith("bits_17_")),
              24: ("bits_25",)}
BITS_SEQUENCE_NAMES = {1: "bits_1", 8: "bits_8", 9: "bits_9_p1025", 16: "bits_16", 17: "bits_17_p1025", 24: "bits_24",
                       25: "bits_25"}


def _digits(name):
    """The box's corners are pinned by one point in the minimum cell (u = 0.02 on every axis) and one in the maximum cell
    (u = 0.98): they alone hold the box's extremes, and their keys are 0 and cells - 1.  The fill lies at u in [0.1, 0.9) of
    random cells, about 30 % of the points in a voxel that holds another one."""
    dims, P = DIGITS[name]
    dims = np.array(dims)
    cells = int(dims.prod())
    rng = np.random.default_rng(_seed(name))
    n = P - 2
    if name == "few_digits":  # the lowest digit takes three values: whole 64-lane groups agree on it
        ix, iy = rng.choice([0, 1, 255], n), rng.integers(0, dims[1], n)
        ijk = np.stack([ix, iy, np.zeros(n, dtype=np.int64)], axis=1)
    else:
        own = np.unique(rng.integers(0, cells, int(0.85 * n)))
        ids = rng.permutation(np.concatenate([own, rng.choice(own, n - own.size)]))
        ijk = np.stack([ids % dims[0], (ids // dims[0]) % dims[1], ids // (dims[0] * dims[1])], axis=1)
    xyz = ((DIGITS_ORIGIN + ijk + rng.uniform(0.1, 0.9, (n, 3))) * DIGITS_LEAF).astype(f32)
    lo = ((DIGITS_ORIGIN + 0.02) * DIGITS_LEAF).astype(f32)
    hi = ((DIGITS_ORIGIN + dims - 1 + 0.98) * DIGITS_LEAF).astype(f32)
    # tiles_33: the minimum is the only point of the second grid-stride round of k2_minmax, the maximum the last of the first
    at_lo, at_hi = (MM_STRIDE, MM_STRIDE - 1) if name == "tiles_33" else sorted(rng.choice(P, 2, replace=False))[::-1]
    cloud = np.zeros((P, 3), dtype=f32)
    rest = np.ones(P, dtype=bool)
    rest[[at_lo, at_hi]] = False
    cloud[rest], cloud[at_lo], cloud[at_hi] = xyz, lo, hi
    claims = dict(dims=tuple(int(d) for d in dims), key_bits=_bits(cells), key_max=cells - 1, min_at=int(at_lo), max_at=int(at_hi),
                  passed=False)
    if name == "few_digits":
        claims["digit0"] = (0, 1, 255)
    return _pack(cloud), DIGITS_LEAF, claims


# ---------------------------------------------------------------------------------------------- family `box`
BOX_NAMES = ("box_spans_zero", "box_signed_zero", "box_leaf_0.3", "box_leaf_0.1", "box_last_extreme")


def _box(name):
    rng = np.random.default_rng(_seed(name))
    if name == "box_spans_zero":
        return _pack(rng.uniform(-3.3, 2.9, (1500, 3)).astype(f32)), 0.25, dict(negative_on_all_axes=True, passed=False)
    if name == "box_signed_zero":  # -0.0 and +0.0 together hold the minimum of every axis
        xyz = rng.uniform(0.01, 4.0, (600, 3)).astype(f32)
        for a in range(3):
            xyz[10 + 7 * a, a], xyz[400 + 11 * a, a] = f32(-0.0), f32(0.0)
        return _pack(xyz), 0.5, dict(signed_zero_minimum=True, passed=False)
    if name.startswith("box_leaf_"):  # the rounding of p * inv at binary32 k * leaf and one ulp to either side of it
        leaf = f32(float(name[9:]))
        k = np.arange(-40, 41).astype(f32) * leaf
        v = np.concatenate([np.nextafter(k, f32(-np.inf)), k, np.nextafter(k, f32(np.inf))]).astype(f32)
        xyz = np.stack([v, rng.permutation(v), rng.permutation(v)], axis=1)
        return _pack(xyz), float(leaf), dict(borders=81, passed=False)
    if name == "box_last_extreme":  # the maximum of every axis is held by the last point alone, in a partial radix tile
        xyz = rng.uniform(0.0, 10.0, (1500, 3)).astype(f32)
        xyz[-1] = (25.3, 31.7, 12.2)
        return _pack(xyz), 0.5, dict(max_at=1499, passed=False)
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------- family `int32_edge`
INT32_EDGE_NAMES = ("line_31_bits", "line_overflow", "cube_wrap", "slab_wrap", "slab_wrap_2x2")
WRAP_NAMES = ("cube_wrap", "slab_wrap")   # the index wraps int32 and stays below 2^32
WRAP_PAST_U32_NAMES = ("slab_wrap_2x2",)  # 2 x 2 x 2147483522 key cells: the index wraps past uint32 and voxels 2^30 apart in z merge


def _whole(rng, n, top):
    """n whole numbers below `top` that binary32 holds: half of every magnitude, half spread evenly"""
    v = np.concatenate([np.exp(rng.uniform(0.0, np.log(top), n // 2)), rng.uniform(0.0, top, n - n // 2)])
    return np.floor(v).astype(f32).astype(np.float64)


def _int32_edge(name):
    rng = np.random.default_rng(_seed(name))
    if name in ("line_31_bits", "line_overflow"):
        top = 2147483520.0 if name == "line_31_bits" else 2147483648.0
        far = _whole(rng, 150, 2.0 ** 31 - 200)
        x = np.concatenate([[0.0, top], far, rng.choice(far, 60),               # voxels shared at large indices
                            rng.integers(1, 6, 88) + rng.uniform(0.1, 0.9, 88)])  # and next to the origin
        xyz = np.stack([x, rng.uniform(0.1, 0.9, x.size), rng.uniform(0.1, 0.9, x.size)], axis=1)
        trunc = int(top) + 1
        claims = dict(trunc=(trunc, 1, 1), dims=(trunc, 1, 1), passed=trunc > INT32_MAX, key_bits=32 if trunc > INT32_MAX else 31)
        return _pack(rng.permutation(xyz).astype(f32)), 1.0, claims
    if name == "cube_wrap":  # truncated extents 1290^3 fit; the keys are made with 1291 per axis, and 1291^3 > 2^31
        n = 130
        z = np.concatenate([rng.uniform(-0.5, 3.0, n), rng.uniform(1286.0, 1289.4, n), rng.uniform(3.0, 1286.0, n // 2)])
        xy = rng.uniform(-0.5, 1289.4, (z.size, 2))
        xyz = np.concatenate([np.stack([xy[:, 0], xy[:, 1], z], axis=1)] * 2)
        xyz[z.size:] = np.floor(xyz[z.size:]) + rng.uniform(0.05, 0.95, (z.size, 3))  # a second point in the voxel of each
        xyz = np.concatenate([[[-0.5] * 3, [1289.4] * 3], np.clip(xyz, -0.5, 1289.4)])
        claims = dict(trunc=(1290,) * 3, dims=(1291,) * 3, passed=False, key_bits=32, keys_above_int32=True)
        return _pack(rng.permutation(xyz).astype(f32)), 1.0, claims
    if name == "slab_wrap":  # 1 x 1 x 2147483521 by the truncated extents, 1 x 2 x 2147483522 by the floors
        far = _whole(rng, 150, 2.0 ** 31 - 200)
        z = np.concatenate([[-0.1, 2147483520.0], far, rng.choice(far, 60), rng.integers(0, 5, 88) + rng.uniform(0.1, 0.9, 88)])
        xyz = np.stack([rng.uniform(0.0, 0.5, z.size), rng.choice([-0.1, 0.1], z.size), z], axis=1)
        xyz[0, :2], xyz[1, :2] = (0.0, -0.1), (0.5, 0.1)
        claims = dict(trunc=(1, 1, 2147483521), dims=(1, 2, 2147483522), passed=False, key_bits=32, keys_above_int32=True)
        return _pack(rng.permutation(xyz).astype(f32)), 1.0, claims
    if name == "slab_wrap_2x2":  # the same slab with two cells in x as well: more than 2^32 key cells, CNT_SORT_BITS above 32
        m = rng.choice(2 ** 23 - 1, 60, replace=False) + 1
        near, far = 128.0 * m - 1 + rng.uniform(0.1, 0.9, 60), 2.0 ** 30 + 128.0 * m  # i2 = 128 m and 2^30 + 128 m: one key
        z = np.concatenate([[-0.1, 2147483520.0], near, far, _whole(rng, 120, 2.0 ** 31 - 200), rng.integers(0, 5, 58) + rng.uniform(0.1, 0.9, 58)])
        xyz = np.stack([rng.choice([-0.1, 0.1], z.size), rng.choice([-0.1, 0.1], z.size), z], axis=1)
        xyz[0, :2], xyz[1, :2] = (-0.1, -0.1), (0.1, 0.1)
        xyz[62:122, :2] = xyz[2:62, :2]
        claims = dict(trunc=(1, 1, 2147483521), dims=(2, 2, 2147483522), passed=False, key_bits=32, merged_pairs=50)  # (at least: binary32 rounds a few of the 60 apart)
        return _pack(rng.permutation(xyz).astype(f32)), 1.0, claims
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------- the table
NAMES = LAYOUT_NAMES + DIGITS_NAMES + BOX_NAMES + INT32_EDGE_NAMES
MAX_POINTS = 32 * 1024 + 1  # tiles_33, the largest cloud of the file

_cache = {}


def case(name):
    """(cached: the cloud is shared and read-only)"""
    if name not in _cache:
        if name in LAYOUT_NAMES:
            c = _layout(name)
        elif name in DIGITS:
            c = _digits(name)
        elif name in BOX_NAMES:
            c = _box(name)
        elif name in INT32_EDGE_NAMES:
            c = _int32_edge(name)
        else:
            raise KeyError(name)
        assert c[0].dtype == f32 and c[0].shape[0] <= MAX_POINTS and np.all(np.isfinite(c[0]))
        c[0].setflags(write=False)
        _cache[name] = c
    return _cache[name]
