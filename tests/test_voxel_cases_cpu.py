"""No-GPU checks of tests/voxel_cases.py, the inputs of tests/test_gpu_voxel_cases.py:

  * the oracle (qo.voxelize, what the device is held to) equals the numpy restatement on every case, bit for bit — the
    two `*_wrap` clouds included, whose linear index overflows int32 in the oracle's C++ as it does in pcl::VoxelGrid: they
    are cases because the wrap-explicit restatement and the oracle agree here;
  * every cloud is where it claims to be: each named run of a `layout` cloud at its sorted position and length (so at its
    offset of a tile, and this far from its window's end), the key bits, the voxel count, pass-through or not, the digit
    census of few_digits, the points that hold the extremes;
  * every cloud can catch what it was built for: deliberately wrong variants of the restatement change the output bits
    of the cases named for them — and only where the fault lies, run by run for the `layout` family.

Two entries of the variant table are what arithmetic allows rather than what one might wish:
  * a run of one or two points has one order of summation in binary32 (a + b = b + a), so the two order variants change
    every named run of three or more points and leave the named runs of 1 and 2 alone;
  * keys_int64 (no wrap at all) cannot change cube_wrap and slab_wrap: both grids have fewer than 2^32 key cells, so
    the unwrapped index IS the uint32 view of the wrapped one, and keys_int64 is asserted EQUAL there.  What the wrap can
    break in them is a SIGNED comparison of the wrapped index — keys_signed, which changes both.  slab_wrap_2x2 is the
    cloud that keys_int64 does change: 2 x 2 x 2147483522 key cells under accepted extents of 1 x 1 x 2147483521, the
    index wraps past uint32 and voxels 2^30 cells apart share a key.
"""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_cases as vc  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32
H = vc.VOX_HALO
_outs = {}


def _want(qo, name):
    """the oracle's answer, computed once"""
    if name not in _outs:
        cloud, leaf, _ = vc.case(name)
        _outs[name] = qo.voxelize(cloud, leaf)
    return _outs[name]


def _b(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _changed_rows(a, b):
    assert a.shape == b.shape
    return set(np.nonzero(np.any(_b(a) != _b(b), axis=1))[0].tolist())


def test_mirrored_constants():
    src = open(os.path.join(ROOT, "quatro_amd", "csrc", "frontend.hip")).read()
    hdr = open(os.path.join(ROOT, "quatro_amd", "csrc", "frontend.h")).read()
    define = lambda text, name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert (define(src, "VOX_TILE_SINGLE"), define(src, "VOX_TILE_BATCH")) == vc.VOX_TILES
    assert define(src, "VOX_HALO") == vc.VOX_HALO
    assert define(hdr, "RADIX_TILE") == vc.RADIX_TILE
    assert define(src, "MM_MAX_PARTS") * 256 == vc.MM_STRIDE
    assert re.search(r"constexpr int RIF = 8;", src)  # eight rows of four tiles: a second round above 32 radix tiles
    assert set(vc.NAMES) == set(vc.LAYOUT_NAMES) | set(vc.DIGITS_NAMES) | set(vc.BOX_NAMES) | set(vc.INT32_EDGE_NAMES)
    assert len(set(vc.NAMES)) == len(vc.NAMES)
    assert max(vc.case(n)[0].shape[0] for n in vc.NAMES) == vc.MAX_POINTS


@pytest.mark.parametrize("name", vc.NAMES)
def test_oracle_equals_the_restatement(qo, name):
    cloud, leaf, claims = vc.case(name)
    want = _want(qo, name)
    got = vc.voxelize_numpy(cloud, leaf)
    assert got.shape == want.shape and np.array_equal(_b(got), _b(want))
    p = vc.plan(cloud, leaf)
    assert p.passed == claims["passed"]
    if p.passed:
        assert want.shape[0] == cloud.shape[0] and np.array_equal(_b(want), _b(cloud))  # the input's bits, w included
    else:
        assert want.shape[0] == p.starts.size and not np.any(_b(want[:, 3]))
    if "key_bits" in claims:
        assert p.bits == claims["key_bits"]


# ---------------------------------------------------------------------------------------------- the claims
# how far every named run ends behind (+) or in front of (-) its window's end, per group: what the group is there for
BEYOND = {
    "from_start": lambda T: (-1, 0, 1, 7, 8, 9),
    "tile_last": lambda T: (-H - 1 + 1, -H - 1 + 2, -1, 0, 1, 8, 9),
    "scalar_rest": lambda T: (-1, 0, 1),
    "headless": lambda T: (3 * T - T // 2 - H,),
    "last_global": lambda T: (8,),
    "last_global_mid": lambda T: (4,),
    "last_single": lambda T: (1 - T - H,),
    "last_full": lambda T: (7 - 7 - H,),
}
OFFSET = {"from_start": lambda T: 0, "tile_last": lambda T: T - 1, "scalar_rest": lambda T: T - 4, "headless": lambda T: T // 2,
          "last_global": lambda T: 5, "last_global_mid": lambda T: 5, "last_single": lambda T: 0, "last_full": lambda T: T - 7}


@pytest.mark.parametrize("name", vc.LAYOUT_NAMES)
def test_layout_clouds_are_where_they_claim(name):
    cloud, leaf, claims = vc.case(name)
    assert leaf == vc.LAYOUT_LEAF
    p = vc.plan(cloud, leaf)
    P, T = cloud.shape[0], claims["tile"]
    assert not p.passed and p.starts.size == claims["n_voxels"]
    assert np.array_equal(p.keys[p.starts], np.arange(p.starts.size))  # one row of voxels: voxel order is x order
    runs = dict(zip(p.starts.tolist(), p.lengths.tolist()))
    for start, n in claims["runs"]:
        assert runs[start] == n, (name, start, n)
    if name in vc.TINY:
        assert P == sum(vc.TINY[name]) and p.lengths.tolist() == vc.TINY[name]
        return
    # the input order interleaves every voxel's points with everyone else's: only a stable sort restores them
    for start, n in claims["runs"]:
        number = p.order[start:start + n]
        assert np.all(np.diff(number) > 0) and (n == 1 or number[-1] - number[0] >= n)
    group = name.rsplit("_t", 1)[0]
    assert T in vc.VOX_TILES and name in vc.layout_names(T)
    if group.startswith("singles"):
        assert claims["runs"] == [] and np.all(p.lengths == 1) and P == 3 * T + (group == "singles_3t1")
        return
    named = claims["runs"]
    assert all(start % T == OFFSET[group](T) for start, _ in named)
    assert tuple(start + n - ((start // T) * T + T + H) for start, n in named) == BEYOND[group](T)
    others = np.delete(p.lengths, np.searchsorted(p.starts, [s for s, _ in named]))
    assert others.max() <= 3 and (others == 1).sum() >= others.size - 3  # singleton filler (and the three runs in front)
    if group == "scalar_rest":
        assert (T + H - OFFSET[group](T)) % 8 == 4  # the 8-wide loop stops four short of the window's end
    if group.startswith("last_"):
        start, n = named[-1]
        assert start + n == P  # the cloud's last run
        assert P % T == {"last_single": 1, "last_full": 0}.get(group, P % T)
    if group == "last_global":
        assert (P - ((named[0][0] // T) * T + T + H)) % 8 == 0  # whole rounds: the next one lies wholly past P
    if group == "last_global_mid":
        assert (P - ((named[0][0] // T) * T + T + H)) % 8 == 4  # P inside a round
    if group == "headless":
        start, n = named[0]
        assert (start + n) // T - start // T >= 3  # two whole tiles without a head in between


def test_batch_clouds_have_distinct_voxel_counts():
    counts = [vc.case(n)[2]["n_voxels"] for n in vc.layout_names(1024)]
    assert len(set(counts)) == len(counts)


@pytest.mark.parametrize("name", vc.DIGITS_NAMES)
def test_digits_clouds_are_where_they_claim(name):
    cloud, leaf, claims = vc.case(name)
    dims, P = vc.DIGITS[name]
    p = vc.plan(cloud, leaf)
    g = vc.grid(cloud, leaf)
    assert leaf == vc.DIGITS_LEAF and cloud.shape[0] == P and not p.passed
    assert tuple(g.dims) == tuple(g.trunc) == dims == claims["dims"]
    cells = dims[0] * dims[1] * dims[2]
    assert p.bits == claims["key_bits"] == (1 if cells == 1 else int(cells - 1).bit_length())
    # the corners alone hold the box: keys 0 and cells - 1, digit 0 and the top digit in every pass that runs
    xyz = cloud[:, :3]
    for a in range(3):
        assert np.nonzero(xyz[:, a] == xyz[:, a].min())[0].tolist() == [claims["min_at"]]
        assert np.nonzero(xyz[:, a] == xyz[:, a].max())[0].tolist() == [claims["max_at"]]
    assert g.keys[claims["min_at"]] == 0 and g.keys[claims["max_at"]] == cells - 1 == claims["key_max"]
    if cells > 1 and name != "few_digits":
        shared = np.repeat(p.lengths, p.lengths) > 1
        assert 0.15 < shared.mean() <= 1.0  # (every point shares where there are fewer cells than points)
    if name == "few_digits":
        assert tuple(np.unique(g.keys & 255).tolist()) == claims["digit0"] == (0, 1, 255)
        assert (p.bits + 7) // 8 == 2 and np.unique((g.keys >> 8) & 255).size == dims[1]
        # groups of 64 sorted neighbours that agree on both digits and straddle a radix tile after the first pass
        first = np.lexsort((np.arange(P), g.keys & 255))
        assert any((g.keys[first][t - 1] & 255) == (g.keys[first][t] & 255) for t in range(vc.RADIX_TILE, P, vc.RADIX_TILE))
    if name == "tiles_33":
        assert P == 32 * vc.RADIX_TILE + 1 and (P + vc.RADIX_TILE - 1) // vc.RADIX_TILE == 33
        assert (claims["min_at"], claims["max_at"]) == (vc.MM_STRIDE, vc.MM_STRIDE - 1)  # the second grid-stride round owns the minimum
    if name.startswith(("bits_9_", "bits_17_")):
        assert P in (1023, 1024, 1025)


@pytest.mark.parametrize("name", vc.BOX_NAMES)
def test_box_clouds_are_where_they_claim(name):
    cloud, leaf, claims = vc.case(name)
    xyz = cloud[:, :3]
    g = vc.grid(cloud, leaf)
    assert not g.passed
    if "negative_on_all_axes" in claims:
        assert np.all(xyz.min(0) < -1) and np.all(xyz.max(0) > 1) and np.all(np.floor(xyz.min(0) / f32(leaf)) < -1)
    if "signed_zero_minimum" in claims:
        for a in range(3):
            zero = xyz[xyz[:, a] == 0, a]
            assert xyz[:, a].min() == 0 and set(np.signbit(zero).tolist()) == {True, False}
    if "borders" in claims:
        inv = f32(1.0) / f32(leaf)
        k = np.arange(-40, 41)
        at = (k.astype(f32) * f32(leaf)).astype(f32)
        assert np.all(np.isin(at, xyz[:, 0])) and claims["borders"] == k.size
        lo, hi = np.nextafter(at, f32(-np.inf)), np.nextafter(at, f32(np.inf))
        assert np.all(np.isin(lo, xyz[:, 0])) and np.all(np.isin(hi, xyz[:, 0]))
        # the cell of a border value is whatever the binary32 product p * inv says: it is k for some, k - 1 for others
        cell = np.floor(at * inv).astype(int)
        assert np.all((cell == k) | (cell == k - 1)) and np.all(np.floor(hi * inv) >= cell) and np.all(np.floor(lo * inv) <= cell)
        if name == "box_leaf_0.3":
            assert np.any(np.floor(lo * inv).astype(int) == k) or np.any(cell == k - 1)  # the rounding shows at 0.3
    if "max_at" in claims:
        for a in range(3):
            assert np.nonzero(xyz[:, a] == xyz[:, a].max())[0].tolist() == [claims["max_at"]] == [cloud.shape[0] - 1]
        assert cloud.shape[0] % vc.RADIX_TILE not in (0, 1)


@pytest.mark.parametrize("name", vc.INT32_EDGE_NAMES)
def test_int32_edge_clouds_are_where_they_claim(qo, name):
    cloud, leaf, claims = vc.case(name)
    g = vc.grid(cloud, leaf)
    assert leaf == 1.0 and 200 <= cloud.shape[0] <= 700
    assert tuple(g.trunc) == claims["trunc"] and tuple(g.dims) == claims["dims"]
    product = g.trunc[0] * g.trunc[1] * g.trunc[2]
    assert g.passed == claims["passed"] == (product > vc.INT32_MAX) and g.bits == claims["key_bits"]
    want = _want(qo, name)
    if name == "line_31_bits":
        assert product == 2147483521 and (g.bits + 7) // 8 == 4
        assert all(np.unique((g.keys >> s) & 255).size > 8 for s in (0, 8, 16, 24))  # every pass has digits to sort
        assert want.shape[0] < cloud.shape[0]
    if name == "line_overflow":
        assert product == 2147483649 and want.shape[0] == cloud.shape[0] and np.array_equal(_b(want), _b(cloud))
    if name in vc.WRAP_NAMES:
        cells = g.dims[0] * g.dims[1] * g.dims[2]
        assert product <= vc.INT32_MAX < cells < 2 ** 32 and claims["keys_above_int32"]
        assert 10 < (g.keys > vc.INT32_MAX).sum() < cloud.shape[0] - 10  # the index wraps for some points, not for all
        assert want.shape[0] < cloud.shape[0]
    if name == "cube_wrap":
        assert product == 2146689000 and cells == 2151685171
    if name == "slab_wrap":
        assert product == 2147483521 and cells == 4294967044
    if name == "slab_wrap_2x2":
        cells = g.dims[0] * g.dims[1] * g.dims[2]
        assert product == 2147483521 <= vc.INT32_MAX and cells > 2 ** 32  # (the device's counter says 34 bits: four passes all the same)
        # voxels 2^30 cells apart in z share a key: the oracle, like pcl::VoxelGrid, merges them
        ijk = np.floor(cloud[:, :3]).astype(np.int64) + 1
        apart = {}
        for (i, j, k), key in zip(ijk.tolist(), g.keys.tolist()):
            apart.setdefault(key, set()).add((i, j, k))
        assert sum(len(v) > 1 for v in apart.values()) >= claims["merged_pairs"]


# ---------------------------------------------------------------------------------------------- the wrong variants
ROW_VARIANTS = ("reversed", "ties_descending", "truncate_window", "lose_last", "gain_next")


def _expected(variant, start, n, T, P):
    """whether the variant must change the centroid of the named run (start, n), from how far it ends behind its window.
    Written a second time on purpose: voxel_cases.must_change chooses the seeds, this one judges them."""
    if variant in ("reversed", "ties_descending"):
        return n >= 3
    beyond = start + n - ((start // T) * T + T + H)
    return beyond > 0 if variant == "truncate_window" else beyond >= 0 and (variant == "lose_last" or start + n < P)


# (a tiny cloud belongs to no tile size: the window variants run on the tiled clouds)
@pytest.mark.parametrize("name,variant", [(n, v) for n in vc.LAYOUT_NAMES if vc.case(n)[2]["runs"] for v in ROW_VARIANTS
                                          if vc.case(n)[2]["tile"] or v in ("reversed", "ties_descending")])
def test_a_wrong_variant_changes_exactly_the_named_runs_it_must(qo, name, variant):
    cloud, leaf, claims = vc.case(name)
    T, P = claims["tile"], cloud.shape[0]
    want = _want(qo, name)
    wrong = vc.voxelize_numpy(cloud, leaf, variant, tile=T)
    changed = _changed_rows(wrong, want)
    p = vc.plan(cloud, leaf)
    rows = {start: int(np.searchsorted(p.starts, start)) for start, _ in claims["runs"]}
    for start, n in claims["runs"]:
        assert (rows[start] in changed) == _expected(variant, start, n, T, P), (name, variant, start, n)
    if variant not in ("reversed", "ties_descending"):
        assert changed <= set(rows.values())  # the filler never reaches a window's end


def test_the_window_variants_change_every_window_edge_cloud(qo):
    """... and leave the clouds without a run at a window's end alone.  gain_next has nothing to gain where the run at the
    window's end is the cloud's last: last_global and last_global_mid are unchanged by it, and are asserted so."""
    for T in vc.VOX_TILES:
        for name in vc.layout_names(T):
            cloud, leaf, _ = vc.case(name)
            want = _want(qo, name)
            edge = name in vc.WINDOW_EDGE_NAMES
            for variant in ("truncate_window", "lose_last", "gain_next", "heads_per_tile"):
                wrong = vc.voxelize_numpy(cloud, leaf, variant, tile=T)
                must = edge and not (variant == "gain_next" and name.startswith("last_global"))
                assert vc.same_bits(wrong, want) != must, (name, variant)


def test_heads_per_tile_splits_the_runs_that_cross_a_tile(qo):
    for T in vc.VOX_TILES:
        for name in vc.window_edge_names(T):
            cloud, leaf, claims = vc.case(name)
            crossings = sum((start + n - 1) // T - start // T for start, n in claims["runs"])
            wrong = vc.voxelize_numpy(cloud, leaf, "heads_per_tile", tile=T)
            assert crossings >= 1 and wrong.shape[0] == _want(qo, name).shape[0] + crossings


@pytest.mark.parametrize("nbits", [8, 16, 24])
def test_a_sort_on_too_few_bits_changes_the_cases_just_above(qo, nbits):
    variant = f"sort_{nbits}_bits"
    for name in vc.DIGITS_NAMES:
        cloud, leaf, claims = vc.case(name)
        wrong = vc.voxelize_numpy(cloud, leaf, variant)
        if name in vc.JUST_ABOVE[nbits]:
            assert claims["key_bits"] == nbits + 1 and not vc.same_bits(wrong, _want(qo, name)), name
        elif claims["key_bits"] <= nbits:
            assert vc.same_bits(wrong, _want(qo, name)), name


@pytest.mark.parametrize("name", vc.WRAP_NAMES + vc.WRAP_PAST_U32_NAMES)
def test_the_wrap_clouds_catch_a_signed_order_and_the_other_verdict(qo, name):
    cloud, leaf, _ = vc.case(name)
    want = _want(qo, name)
    assert not vc.same_bits(vc.voxelize_numpy(cloud, leaf, "keys_signed"), want)
    floor_verdict = vc.voxelize_numpy(cloud, leaf, "verdict_floor")
    assert np.array_equal(_b(floor_verdict), _b(cloud)) and not vc.same_bits(floor_verdict, want)  # it would pass through
    # fewer than 2^32 key cells: the index without any wrap is the uint32 view of the wrapped one (see the module's text);
    # more than 2^32: keys that never wrap keep the voxels apart that the wrap merges
    assert vc.same_bits(vc.voxelize_numpy(cloud, leaf, "keys_int64"), want) == (name in vc.WRAP_NAMES)


def test_the_wrap_variants_leave_a_grid_below_int32_alone(qo):
    cloud, leaf, _ = vc.case("line_31_bits")
    for variant in ("keys_signed", "keys_int64", "verdict_floor"):
        assert vc.same_bits(vc.voxelize_numpy(cloud, leaf, variant), _want(qo, "line_31_bits"))
