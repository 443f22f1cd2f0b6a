"""The kernels of quatro_amd/csrc/patchwork.hip and quatro_amd/csrc/segment.hip on the named inputs of
tests/scan_cases.py, against the CPU oracle, bit for bit: `ground` and `nonground` for Patchwork; `labels`, `valid`,
`outliers` and `n_segments` for the range image.  tests/test_scan_cases_cpu.py holds the oracle to independent
references on the same inputs and asserts that every input is on the branch it is named after.

Every Patchwork case and every small image case runs twice on one handle with another case in between: whatever a call
leaves in first / last / info / offs or in owner / cnt / rowmask must not reach the next one.
"""
import os
import sys

import numpy as np
import pytest

from quatro_amd import lib as ql

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu
_want = {}


def _b(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and bool(np.array_equal(_b(got), _b(want)))


@pytest.fixture(scope="module")
def h():
    hd = ql.Handle(0, max_points=8192, max_voxels=4096, max_corr=1024)
    yield hd
    hd.close()


def _pw_oracle(qo, name):
    if ("pw", name) not in _want:
        c = sc.pw_case(name)
        _want[("pw", name)] = qo.patchwork(c.cloud, sc.pw_apply(qo.PwParams(), c.params_mutation))
    return _want[("pw", name)]


def _ip_oracle(qo, name):
    if ("ip", name) not in _want:
        c = sc.ip_case(name)
        _want[("ip", name)] = qo.segment_cloud(c.cloud, sc.ip_apply(qo.IpParams(), c.ip_fields))
    return _want[("ip", name)]


def _call(fn, *args):
    """a device error ends the run: nothing else is started on a device that has reported one"""
    try:
        return fn(*args)
    except ql.QuatroHipError as e:
        if e.code == ql.QTR_ERR_HIP:
            pytest.exit(f"device error, nothing more is run: {e}", returncode=3)
        raise


def _pw_device(hd, name):
    c = sc.pw_case(name)
    return _call(hd.patchwork, c.cloud, sc.pw_apply(ql.PwParams(), c.params_mutation))


def _ip_device(hd, name):
    c = sc.ip_case(name)
    return _call(hd.segment_cloud, c.cloud, sc.ip_apply(ql.IpParams(), c.ip_fields))


def _pw_equal(g, o):
    return _same(g["ground"], o["ground"]) and _same(g["nonground"], o["nonground"])


def _ip_equal(g, o):
    n_seg = int(o["labels"][(o["labels"] > 0) & (o["labels"] < sc.IP_OUTLIER)].max(initial=0))
    return (np.array_equal(g["labels"], o["labels"]) and _same(g["valid"], o["valid"]) and
            _same(g["outliers"], o["outliers"]) and g["n_segments"] == n_seg)


@pytest.mark.parametrize("name", sc.PW_NAMES)
def test_patchwork_equals_the_oracle_twice_on_one_handle(h, qo, name):
    other = sc.PW_NAMES[(sc.PW_NAMES.index(name) + 5) % len(sc.PW_NAMES)]
    assert _pw_equal(_pw_device(h, name), _pw_oracle(qo, name))
    _pw_device(h, other)  # (judged under its own name)
    assert _pw_equal(_pw_device(h, name), _pw_oracle(qo, name))


def test_patchwork_refuses_more_patches_than_the_scan_serves(h):
    c = sc.pw_case("patches_1025")
    with pytest.raises(ql.QuatroHipError) as e:
        h.patchwork(c.cloud, sc.pw_apply(ql.PwParams(), c.params_mutation))
    assert e.value.code == ql.QTR_ERR_BAD_ARG and c.claims["refused"] in str(e.value)


@pytest.mark.parametrize("name", sc.IP_SMALL_NAMES)
def test_segment_equals_the_oracle_twice_on_one_handle(h, qo, name):
    other = sc.IP_SMALL_NAMES[(sc.IP_SMALL_NAMES.index(name) + 7) % len(sc.IP_SMALL_NAMES)]
    assert _ip_equal(_ip_device(h, name), _ip_oracle(qo, name))
    _ip_device(h, other)  # (judged under its own name)
    assert _ip_equal(_ip_device(h, name), _ip_oracle(qo, name))


def test_segment_big_image_equals_the_oracle(h, qo):
    """n_scan = 64, H = 8192: 512 blocks of 1024 pixels, the first and the last block of several waves of k_ip_blockscan
    holding valid pixels, outliers and a valid root; then a small image on the arena the big one has left behind"""
    assert _ip_equal(_ip_device(h, "big_image"), _ip_oracle(qo, "big_image"))
    assert _ip_equal(_ip_device(h, "validity_corners"), _ip_oracle(qo, "validity_corners"))


def _records_equal(got, want):
    for g, w in zip(got, want):
        assert (g["status"], g["n_src"], g["n_tgt"], g["L"]) == (w["status"], w["n_src"], w["n_tgt"], w["L"])
        assert g["n_src"] > 0 and g["n_tgt"] > 0 and np.array_equal(g["T"], w["T"])


def test_batch_preprocessing_equals_the_single_calls(h, qo):
    """Patchwork and the range image as the raw-sweep batch enqueues them (pw_begin on the pair's host scans, seg_begin
    on the non-ground cloud where Patchwork left it on the device, one slot per scan) against the same two stages
    called one by one.  The batch hands out registration records only, so that is what is compared: the records on the
    raw scans equal the records of the same handle, its pre-processing switched off, on the single calls' valid
    segments, which in turn equal the oracle's.

      * a Patchwork case: the patch-size cloud and its copy in which every patch is rejected share one parameter set;
        every non-ground pixel of a 64 x 1024 image is kept (num_min_pts = 1);
      * an image case: width_128 and width_65 under their own image parameters, behind a Patchwork that keeps every
        point as non-ground (no minimum patch size, an empty seed set: the case empty_seed_set pins that answer).  Every
        pixel of these images has one return, so the order in which Patchwork hands the points on cannot change the
        image, and the valid segments are the named case's own."""
    a, b = sc.pw_case("patch_sizes_rejected"), sc.pw_case("patch_sizes")
    assert a.params_mutation == b.params_mutation
    ipf = sc.ip_fields(H=1024, n_scan=64, mode="8Neighbor", num_min_pts=1)
    pw, ip = sc.pw_apply(ql.PwParams(), a.params_mutation), sc.ip_apply(ql.IpParams(), ipf)
    single = [_call(h.segment_cloud, _call(h.patchwork, c.cloud, pw)["nonground"], ip)["valid"] for c in (a, b)]
    want = [qo.segment_cloud(qo.patchwork(c.cloud, sc.pw_apply(qo.PwParams(), a.params_mutation))["nonground"],
                             sc.ip_apply(qo.IpParams(), ipf))["valid"] for c in (a, b)]
    assert all(_same(s_, w) for s_, w in zip(single, want))
    assert single[0].shape[0] > 500 and single[1].shape[0] > 50
    keep_all = dict(num_min_pts=0, num_thr=0, th_seeds=-5.0)
    u, v = sc.ip_case("width_128"), sc.ip_case("width_65")
    pw2 = sc.pw_apply(ql.PwParams(), keep_all)
    ips = [sc.ip_apply(ql.IpParams(), c.ip_fields) for c in (u, v)]
    single2 = []
    for c, ipp in zip((u, v), ips):
        ng = _call(h.patchwork, c.cloud, pw2)
        assert ng["ground"].shape[0] == 0 and ng["nonground"].shape[0] == c.cloud.shape[0]
        single2.append(_call(h.segment_cloud, ng["nonground"], ipp)["valid"])
        assert _same(single2[-1], _ip_oracle(qo, "width_128" if c is u else "width_65")["valid"])
    hb = ql.Handle(0, n_slots=2, max_points=8192, max_voxels=4096, max_corr=1024)
    try:
        hb.set_batch_preprocess(pw, ip)
        got = _call(hb.register_batch, [(a.cloud, b.cloud, 3), (b.cloud, a.cloud, 4)])
        got2 = []
        for c, ipp in zip((u, v), ips):
            hb.set_batch_preprocess(pw2, ipp)
            got2 += _call(hb.register_batch, [(c.cloud, c.cloud[::-1].copy(), 5)])
        hb.set_batch_preprocess(on=False)
        plain = _call(hb.register_batch, [(single[0], single[1], 3), (single[1], single[0], 4)])
        plain2 = _call(hb.register_batch, [(s_, s_, 5) for s_ in single2])
    finally:
        hb.close()
    _records_equal(got, plain)
    _records_equal(got2, plain2)
