"""qtr_get_stage_times per call shape: WHICH fields of qtr_stage_times a call fills and which it leaves at zero (the table
of quatro_amd/csrc/stage_times.h), with the stage events on and off, with and without the nearest-neighbour event pairs,
and after a call of another shape on the same slot.  No duration is a pass condition: only > 0 / == 0 and, where the
stages follow one another on one stream, total >= every stage."""
import contextlib
import os

import numpy as np
import pytest

from quatro_amd import lib as ql
from quatro_amd import synth

pytestmark = pytest.mark.gpu
LIMITS = dict(max_points=65536, max_voxels=16384, max_corr=8192)
STAGES = ("voxelize", "fpfh", "match", "graph", "clique", "solve")
FRONT, BACK = ("voxelize", "fpfh", "match"), ("graph", "clique", "solve")
# shape -> (the stage fields it fills, whether it runs a matcher: nn_kernel / nn_launches)
SHAPES = {
    "solve": (BACK, False),
    "register_pair": (STAGES, True),
    "feature_pair": (FRONT, True),
    "register_keyframes": (("match",) + BACK, True),  # no voxel grid, no FPFH chain; match = load + matcher
    "register_pair_corr": (STAGES, True),
}


@contextlib.contextmanager
def _env(**kv):
    """environment variables the library reads at qtr_create, set around a handle's creation and restored afterwards"""
    keep = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _handle(overlap=True, events=True):
    with _env(QTR_CORR_OVERLAP=None if overlap else "0", QTR_STAGE_EVENTS=None if events else "0"):
        return ql.Handle(0, **LIMITS)


@pytest.fixture(scope="module")
def inputs():
    """the `tiny` scans of tests/test_gpu_corr_overlap.py (250 points on a 0.8 m patch and their moved copy) and 300
    correspondences"""
    g = np.random.default_rng(3)
    g.uniform(0, 5.0, 2000), g.uniform(0, 5.0, 2000), g.normal(0, 0.01, 2000)
    e = np.zeros((250, 4), dtype=np.float32)
    e[:, 0], e[:, 1] = g.uniform(0, 0.8, 250), g.uniform(0, 0.8, 250)
    e[:, 2] = 0.1 * np.sin(5.0 * e[:, 0]) * np.cos(4.0 * e[:, 1]) + g.normal(0, 0.002, 250)
    f = e.copy()
    f[:, :3] = (e[:, :3].astype(np.float64) @ synth.yaw_matrix(0.2).T + np.asarray((0.05, -0.03, 0.01))).astype(np.float32)
    f[:, :3] += np.random.default_rng(13).normal(0, 0.0005, (250, 3)).astype(np.float32)
    cs, ct = synth.correspondences(300, 0.1, 7, noise=0.1)[:2]
    return {"scans": (e, f), "corr": (cs, ct), "fp": ql.default_frontend_params(seed=2)}


def _call(h, shape, inputs, kfs=None):
    s, t = inputs["scans"]
    fp = inputs["fp"]
    if shape == "solve":
        h.solve(*inputs["corr"])
    elif shape == "register_pair":
        h.register_pair(s, t, fp)
    elif shape == "feature_pair":
        h.feature_pair(s, t, fp)
    elif shape == "register_keyframes":
        h.register_keyframes(*kfs, fp)
    else:
        h.register_pair_corr(s, t, *inputs["corr"], fp)
    return h.stage_times()


def _check(st, shape, nn=True, events=True, ordered=True):
    filled, matcher = SHAPES[shape]
    print(shape, {k: v for k, v in st.items()})
    for k in STAGES + ("total",):
        assert np.isfinite(st[k])
        if events and (k in filled or k == "total"):
            assert st[k] > 0, (shape, k, st)
        else:
            assert st[k] == 0, (shape, k, st)
    assert st["graph_kernel"] == 0, (shape, st)
    if matcher and nn:
        assert st["nn_kernel"] > 0 and st["nn_launches"] == 2, (shape, st)
        assert st["nn_dir1"] > 0 and st["nn_dir2"] > 0, (shape, st)
    else:
        assert st["nn_kernel"] == 0 and st["nn_launches"] == 0, (shape, st)
    if events and ordered:
        assert st["total"] >= max(st[k] for k in STAGES), (shape, st)


@pytest.mark.parametrize("overlap", [True, False])
def test_fields_per_shape_with_events_on(inputs, overlap):
    """every shape on a handle of its own slot history: a fresh slot per shape would hide nothing, so they share one — in an
    order in which every call follows one of ANOTHER shape (the stale-event case: the later shape's pattern is reported)"""
    h = _handle(overlap=overlap)
    try:
        with h.keyframe(inputs["scans"][0], inputs["fp"]) as ks, h.keyframe(inputs["scans"][1], inputs["fp"]) as kt:
            order = ("solve", "register_pair", "solve", "feature_pair", "register_keyframes", "register_pair_corr", "solve",
                     "register_pair_corr", "feature_pair", "register_pair", "register_keyframes", "solve")
            for shape in order:
                st = _call(h, shape, inputs, (ks, kt))
                # the overlapped call measures graph / clique / solve on the third stream WHILE the front end runs
                _check(st, shape, ordered=not (overlap and shape == "register_pair_corr"))
                assert st == h.stage_times()  # (read twice: the second read finds nothing pending and the same record)
    finally:
        h.close()


def test_nn_fields_follow_the_event_stride(inputs):
    h = _handle()
    try:
        with h.keyframe(inputs["scans"][0], inputs["fp"]) as ks, h.keyframe(inputs["scans"][1], inputs["fp"]) as kt:
            h.set_nn_event_stride(0)
            for shape in SHAPES:
                _check(_call(h, shape, inputs, (ks, kt)), shape, nn=False, ordered=shape != "register_pair_corr")
            h.set_nn_event_stride(2)  # the first match after the call is a timed one, the second is not
            _check(_call(h, "register_pair", inputs), "register_pair", nn=True)
            _check(_call(h, "feature_pair", inputs), "feature_pair", nn=False)
            _check(_call(h, "register_keyframes", inputs, (ks, kt)), "register_keyframes", nn=True)
            _check(_call(h, "solve", inputs), "solve")
    finally:
        h.close()


@pytest.mark.parametrize("overlap", [True, False])
def test_every_field_reads_zero_with_events_off(inputs, overlap):
    h = _handle(overlap=overlap, events=False)
    try:
        with h.keyframe(inputs["scans"][0], inputs["fp"]) as ks, h.keyframe(inputs["scans"][1], inputs["fp"]) as kt:
            h.set_nn_event_stride(0)
            for shape in SHAPES:
                _check(_call(h, shape, inputs, (ks, kt)), shape, nn=False, events=False)
            h.set_nn_event_stride(1)  # the nearest-neighbour launches keep their own event pairs
            for shape in SHAPES:
                if SHAPES[shape][1]:
                    _check(_call(h, shape, inputs, (ks, kt)), shape, nn=True, events=False)
            h.set_stage_events(True)  # and back on, on the same slot
            _check(_call(h, "register_pair", inputs), "register_pair")
            _check(_call(h, "solve", inputs), "solve")
    finally:
        h.close()
