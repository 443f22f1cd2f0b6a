"""The CPU oracle's Patchwork and range-image stages on the named inputs of tests/scan_cases.py, against the independent
references of that module, and every case against what it claims.  No GPU.  Outputs are copies of input points (their w
column is the input index), so they are compared as bits.

  * every Patchwork case: the oracle's patch id per point equals the binary64 binning; every point that is not a named
    boundary point lies BIN_MARGIN inside its bin; the outputs hold exactly the points of the processed patches, patch
    after patch in the reference's order, each patch's ground and non-ground parts in stable height order;
  * the two-population cases: the oracle's two output lists equal the binary64 plane fit's, and every binary64 residual
    (and seed height) stays RES_MARGIN = 0.05 m from its threshold in every iteration;
  * every range-image case: labels, valid segments, outliers and the segment count equal the union-find labeller's, and
    every neighbouring pair's angle stays ANGLE_MARGIN_DEG from segment_theta.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_cases as sc  # noqa: E402


def _b(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_pw = {}


def _pw_run(qo, name):
    """(case, fields, structure reference, oracle result), computed once per case"""
    if name not in _pw:
        c = sc.pw_case(name)
        F = sc.pw_fields(c.params_mutation)
        _pw[name] = (c, F, sc.pw_structure(c.cloud, F), qo.patchwork(c.cloud, sc.pw_apply(qo.PwParams(), c.params_mutation)))
    return _pw[name]


def _ids(out, cloud):
    """input indices of output rows; the rows are bit copies of those input rows"""
    ids = out[:, 3].astype(np.int64)
    assert np.array_equal(_b(out), _b(cloud[ids]))
    return ids


def test_mirrored_defaults_are_the_oracles(qo):
    p = qo.pw_params()
    for k, v in sc.PW_DEFAULT.items():
        got = getattr(p, k)
        assert (list(got) == list(v)) if isinstance(v, list) else (got == v), k
    q = qo.ip_params()
    assert q.segment_theta == sc.THETA and (q.valid_point_num, q.valid_line_num) == (5, 3)
    assert sc.PW_NAMES == sorted(set(sc.PW_NAMES), key=sc.PW_NAMES.index) and len(set(sc.IP_NAMES)) == len(sc.IP_NAMES)


@pytest.mark.parametrize("name", sc.PW_NAMES)
def test_patchwork_oracle_equals_the_structure_reference(qo, name):
    c, F, S, o = _pw_run(qo, name)
    assert c.cloud.shape[0] <= 6000
    assert np.array_equal(o["patch"], S["patch"])
    named = {i for i, _ in c.claims.get("boundary", [])}
    rest = np.array([i not in named for i in range(c.cloud.shape[0])])
    assert S["margin"][rest].min(initial=np.inf) >= sc.BIN_MARGIN
    g, n = _ids(o["ground"], c.cloud), _ids(o["nonground"], c.cloud)
    done = sc.pw_processed(F, S)
    emitted = np.concatenate([S["lists"][p] for p in done]) if done else np.zeros(0, np.int64)
    assert np.array_equal(np.sort(np.concatenate([g, n])), np.sort(emitted))
    # patch after patch; inside a patch both parts keep the stable height order
    for out in (g, n):
        pids = S["patch"][out]
        rank = {p: r for r, p in enumerate(done)}
        assert np.all(np.diff([rank[p] for p in pids]) >= 0)
    pos = np.zeros(c.cloud.shape[0], dtype=np.int64)
    for p in done:
        pos[S["lists"][p]] = np.arange(S["lists"][p].size)
        gp, np_ = g[S["patch"][g] == p], n[S["patch"][n] == p]
        assert np.all(np.diff(pos[gp]) > 0)
        # (a rejected patch puts its ground-classified part in front of the rest: at most one descent)
        assert np.sum(np.diff(pos[np_]) < 0) <= 1


@pytest.mark.parametrize("name", sc.PW_NAMES)
def test_patchwork_oracle_equals_the_binary64_plane_fit(qo, name):
    c, F, S, o = _pw_run(qo, name)
    if not c.claims.get("two_population"):
        assert name in ("all_dropped", "empty_seed_set")
        return
    R = sc.pw_planefit(c.cloud, F, S)
    for p in sc.pw_processed(F, S):  # the plane-fit reference is used near the sensor only
        xy = c.cloud[S["lists"][p], :2].astype(np.float64)
        assert np.hypot(xy[:, 0], xy[:, 1]).max() <= sc.PLANE_FIT_RANGE
    assert R["res_margin"] >= sc.RES_MARGIN, R["res_margin"]
    assert R["status_margin"] >= 0.01, R["status_margin"]
    assert np.array_equal(_ids(o["ground"], c.cloud), R["ground"])
    assert np.array_equal(_ids(o["nonground"], c.cloud), R["nonground"])


@pytest.mark.parametrize("name", sc.PW_NAMES)
def test_patchwork_case_claims(qo, name):
    c, F, S, o = _pw_run(qo, name)
    cl, z = c.claims, c.cloud[:, 2]
    sizes = {p: ids.size for p, ids in S["lists"].items()}
    R = sc.pw_planefit(c.cloud, F, S) if cl.get("two_population") else None
    if cl.get("signed_zeros"):
        for p, ids in S["lists"].items():
            zz = z[ids]
            flat = ids[zz == 0]
            neg = np.signbit(c.cloud[flat, 2])
            assert neg.any() and (~neg).any()
            # a +0.0 stands in front of a -0.0 in input order: a key that tells the zeros apart reorders them
            assert np.any(~neg[:-1] & neg[1:]) and np.all(np.diff(flat) > 0)
    if "equal_heights" in cl:
        (ids,) = S["lists"].values()
        assert np.sum(z[ids] == z[ids[0]]) == cl["equal_heights"] and np.all(np.diff(ids[:cl["equal_heights"]]) > 0)
    if "patch_sizes" in cl:
        assert sizes == cl["patch_sizes"] and sorted(sizes.values()) == sc.SIZES
        rej = [R["per_patch"][p][0] for p in sc.pw_processed(F, S)]
        assert all(rej) if cl["all_rejected"] else not any(rej)
        assert sorted(sc.pw_processed(F, S)) == sorted(p for p, n in sizes.items() if n > 10)
        # both output parts of a patch are non-empty, so k_pw_emit compacts two interleaved streams
        assert all(0 < R["per_patch"][p][1] < sizes[p] for p in R["per_patch"])
    if "prefix" in cl:
        assert S["prefix"] == cl["prefix"]
        low = sc.pw_margin_height(F)
        want = sorted(v if v != "n" else 40 for v in sc.PREFIXES)
        assert sorted(int(np.sum(z[ids] < low)) for ids in S["lists"].values()) == want
        for p, are_ground in cl["probes_are_ground"].items():
            probes = S["lists"][p][np.isclose(z[S["lists"][p]], -F["sensor_height"] + 0.9)]
            assert probes.size >= 40 and np.isin(probes, R["ground"]).all() == are_ground
            assert np.isin(probes, R["nonground"]).all() == (not are_ground)
    if "num_lpr" in cl:
        L = cl["num_lpr"]
        assert sizes[cl["longer"]] > L and (cl["shorter"] is None or 10 < sizes[cl["shorter"]] < L)
        if cl["probe_height"] is not None:
            ids = S["lists"][cl["longer"]]
            zp = np.float32(cl["probe_height"])
            thr = S["seed_mean"][cl["longer"]] + F["th_seeds"]
            # the window's last height is a heavy one; without it the probes are no seeds
            assert z[ids[L - 1]] == np.float32(0.2 * L) and z[ids[L - 2]] == zp
            short = (S["seed_mean"][cl["longer"]] * L - float(z[ids[L - 1]])) / L + F["th_seeds"]
            assert short + sc.RES_MARGIN < zp < thr - sc.RES_MARGIN
            assert np.isin(ids[z[ids] == zp], R["ground"]).all()
    if "boundary" in cl:
        for i, pid in cl["boundary"]:
            assert S["patch"][i] == pid, (i, c.cloud[i], S["patch"][i], pid)
        assert np.any(z.astype(np.float64) == -1.8 * F["sensor_height"])
    if "margin_block" in cl:
        p, low = cl["patch"], sc.pw_margin_height(F)
        ids = S["lists"][p]
        z64 = z[ids].astype(np.float64)
        assert low == -1.25 and int(np.sum(z64 == low)) == cl["margin_block"] and int(np.sum(z64 < low)) == cl["prefix_len"]
        assert S["prefix"][p] == cl["prefix_len"] and S["seed_mean"][p] == low
        probes = ids[z[ids] == np.float32(cl["probe_height"])]
        # the strict skip: the probes are no seeds and come out non-ground; a skip that also took the heights ON the
        # margin would start from the level above, and the probes would be seeds by a wide margin
        thr, thr_le = low + F["th_seeds"], float(np.float32(cl["level_above"])) + F["th_seeds"]
        assert thr + sc.RES_MARGIN < cl["probe_height"] < thr_le - sc.RES_MARGIN
        assert probes.size == 40 and np.isin(probes, R["nonground"]).all() and not np.isin(probes, R["ground"]).any()
        got_n = o["nonground"][:, 3].astype(np.int64)
        assert np.isin(probes, got_n).all()
        # what `<=` would give, by the same reference: the probes ground
        S2 = dict(S, prefix={p: cl["prefix_len"] + cl["margin_block"]}, seed_mean={p: float(np.float32(cl["level_above"]))})
        assert np.isin(probes, sc.pw_planefit(c.cloud, F, S2)["ground"]).all()
    if "npatch" in cl:
        nz, nsec, nring, mr, base, _, _ = sc._pw_layout(F)
        assert base[-1] == cl["npatch"]
    if "populated" in cl:
        assert sorted(sizes) == cl["populated"] == sc.pw_processed(F, S)
        assert all(sum(1 for p in sizes if p // 64 == b) >= 2 for b in range(16))
    if "rejected" in cl:
        assert {p: r for p, (r, _) in R["per_patch"].items()} == cl["rejected"]
    if "points" in cl:
        assert c.cloud.shape[0] == cl["points"]
    if cl.get("all_dropped"):
        assert (S["patch"] == -1).all() and o["ground"].shape[0] == 0 and o["nonground"].shape[0] == 0
    if "survivor" in cl:
        assert sc.pw_processed(F, S) == [cl["survivor"]] and len(sizes) == 5
    if cl.get("all_nonground"):
        done = sc.pw_processed(F, S)
        assert len(done) == 4 and o["ground"].shape[0] == 0
        assert np.array_equal(_ids(o["nonground"], c.cloud), np.concatenate([S["lists"][p] for p in done]))
    if "nonfinite_rows" in cl:
        rows = cl["nonfinite_rows"]
        assert rows == [0, c.cloud.shape[0] // 2, c.cloud.shape[0] - 1] and all(p >= 0 for p in cl["were_in_patches"])
        assert not np.isfinite(c.cloud[rows, :3]).all(axis=1).any()
        assert (S["patch"][rows] == -1).all()
        out = np.concatenate([o["ground"][:, 3], o["nonground"][:, 3]]).astype(np.int64)
        assert not np.isin(rows, out).any() and np.isfinite(np.concatenate([o["ground"], o["nonground"]])).all()


def test_patchwork_layout_past_the_scan_width(qo):
    c = sc.pw_case("patches_1025")
    nz, nsec, nring, mr, base, _, _ = sc._pw_layout(sc.pw_fields(c.params_mutation))
    assert base[-1] == c.claims["npatch"] == sc.PW_MAX_PATCHES + 1 and c.claims["refused"] == sc.PW_REFUSAL


# ---------------------------------------------------------------------------------------------- range image
_ip = {}


def _ip_run(qo, name):
    if name not in _ip:
        c = sc.ip_case(name)
        _ip[name] = (c, sc.ip_label(c.cloud, c.ip_fields), qo.segment_cloud(c.cloud, sc.ip_apply(qo.IpParams(), c.ip_fields)))
    return _ip[name]


@pytest.mark.parametrize("name", sc.IP_NAMES)
def test_segment_oracle_equals_the_labeller(qo, name):
    c, L, o = _ip_run(qo, name)
    assert L["angle_margin_deg"] >= sc.ANGLE_MARGIN_DEG
    assert np.array_equal(o["labels"], L["labels"])
    assert np.array_equal(_b(o["valid"]), _b(L["valid"]))
    assert np.array_equal(_b(o["outliers"]), _b(L["outliers"]))
    assert o["labels"][(o["labels"] > 0) & (o["labels"] < sc.IP_OUTLIER)].max(initial=0) == L["n_segments"]
    want = np.full(o["ranges"].size, np.finfo(np.float32).max, dtype=np.float32)
    for p, i in L["owner"].items():
        want[p] = L["pixels"]["range"][i]
    assert np.array_equal(_b(o["ranges"].ravel()), _b(want))


@pytest.mark.parametrize("name", sc.IP_NAMES)
def test_segment_case_claims(qo, name):
    c, L, o = _ip_run(qo, name)
    cl, ip = c.claims, c.ip_fields
    H, NS = ip["horizon_scan"], ip["n_scan"]
    comps = L["components"]
    if "width" in cl:
        assert H == cl["width"] and len(comps) > 1 and any(v for *_, v in comps) and any(not v for *_, v in comps)
    if "hang_on_row_63" in cl:
        assert NS == 64 and ip["valid_line_num"] == 3
        for first, straddles in cl["hang_on_row_63"]:
            (k,) = [k for k in comps if k[0] == first]
            mem = np.nonzero(L["labels"].ravel() == L["labels"].ravel()[first])[0]
            assert k[1] == mem.size == 5 < ip["num_min_pts"] and k[2] == 3 and k[3]
            counted = {int(q) // H for q in mem if q != first}
            assert counted == {61, 62, 63} and len(counted - {63}) < ip["valid_line_num"]  # an outlier without row 63
            last = max(int(q) for q in mem)
            assert ((last // 64) * 64) // H == (62 if straddles else 63)  # the row its wave starts in
    if "rows" in cl:
        col = [k for k in comps if k[0] == cl["column"]]
        assert NS == cl["rows"] and len(col) == 1 and col[0][1] == NS and col[0][2] == NS - 1
        assert L["labels"][NS - 1, cl["column"]] == L["labels"][0, cl["column"]]
    if "np" in cl:
        assert NS * H == cl["np"] and all(cl["np"] % m for m in (64, 256, 1024))
    if "components" in cl:
        assert len(comps) == cl["components"]
        if cl.get("seam"):
            assert len(sc.ip_label(c.cloud, ip, wrap=False)["components"]) == 2
        if name.startswith("shape_snake") and cl["components"] == 1:
            assert comps[0][2] >= NS - 1 and set(np.nonzero((L["labels"] > 0).any(axis=1))[0]) == set(range(NS))
        if name == "shape_whole_4CrossNeighbor":
            lab = L["labels"]
            assert np.array_equal(lab, 1 + (np.add.outer(np.arange(NS), np.arange(H)) % 2))
    if "corner_components" in cl:
        assert [(s, r, v) for _, s, r, v in comps] == cl["corner_components"]
    if "owner_pixel" in cl:
        assert L["owner"][cl["owner_pixel"]] == cl["owner_index"] == c.cloud.shape[0] - 1
        assert int(np.sum(L["pixels"]["pixel"] == cl["owner_pixel"])) == 500
        rg = L["pixels"]["range"][L["pixels"]["pixel"] == cl["owner_pixel"]]
        assert rg.argmax() == 499 and np.any(np.diff(rg[:-1]) < 0)
        r, cc = cl["joined"]
        assert L["labels"][r, cc] == L["labels"][r, cc - 1] == 1 and L["labels"][r, cc - 2] == sc.IP_OUTLIER
    if "columns" in cl:
        px = L["pixels"]
        assert [int(p) // H for p in px["pixel"]] == list(range(8)) and [int(p) % H for p in px["pixel"]] == cl["columns"]
        assert list(np.nonzero(px["column_raw"] >= H)[0]) == cl["wrapped"]
        assert np.signbit(c.cloud[[1, 3], 1]).all() and np.signbit(c.cloud[[5, 7], 0]).all()
    if "pixels" in cl:
        px = L["pixels"]
        assert [int(p) for p in px["pixel"]] == cl["pixels"]
        assert -1 < px["rf"][0] < 0 and -2 < px["rf"][1] < -1 and px["range"][2] < 0.1 < px["range"][3]
    if "blocks" in cl:
        assert c.cloud.shape[0] <= 5000 and NS * H == 512 * sc.IP_BLOCK
        lab = L["labels"].ravel()
        roots = {k[0] for k in comps if k[3]}
        for b in cl["blocks"]:
            blk = lab[b * sc.IP_BLOCK:(b + 1) * sc.IP_BLOCK]
            assert np.any((blk > 0) & (blk < sc.IP_OUTLIER)) and np.any(blk == sc.IP_OUTLIER)
            assert any(b * sc.IP_BLOCK <= r < (b + 1) * sc.IP_BLOCK for r in roots)
        assert max(k[1] for k in comps) == cl["long_component"] and sum(1 for k in comps if k[1] == 1) > 500
    if "nonfinite_rows" in cl:
        rows = cl["nonfinite_rows"]
        assert not np.isfinite(c.cloud[rows, :3]).all(axis=1).any()
        if cl["nan"]:
            assert (L["pixels"]["pixel"][rows] == -1).all() and L["labels"][0, 0] == -1
        assert not np.isnan(np.concatenate([o["valid"], o["outliers"]])).any()
