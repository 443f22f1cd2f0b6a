"""The grouped map registration without a GPU: the header's entry points against the binding and the extension
library's symbol table (tests/ext_abi.py), the two host-side helpers of include/qtr_vmap_batch_math.h compiled with g++
against their Python restatement bit for bit, and the named cases of tests/vmap_batch_cases.py: each makes the branch it
claims, shown with the single call's restatement (vmap_restate.RefMap.register), which is the reference of every item."""
import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import ext_abi
import icp_restate as R
import vmap_batch_cases as BC
import vmap_restate as M

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TWO = {"qtr_voxel_map_register_batch", "qtr_voxel_map_batch_fetch"}
STOP_MAX, STOP_TEPS, STOP_FEPS, STOP_TOO_FEW = 1, 2, 3, 4


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


@pytest.fixture(scope="module")
def ref_lib():
    from quatro_amd import lib as ql
    out = os.path.join(tempfile.mkdtemp(prefix="vmap_batch_ref_"), "libvmap_batch_ref.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "vmap_batch_ref", "vmap_batch_ref.cpp"),
                           "-o", out])
    lib = ctypes.CDLL(out)
    lib.vmap_batch_ref_hypothesis.restype = None
    lib.vmap_batch_ref_hypothesis.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]
    lib.vmap_batch_ref_best.argtypes = [ctypes.POINTER(ql.IcpResult), ctypes.c_int]
    lib.vmap_batch_ref_layout.restype = None
    lib.vmap_batch_ref_layout.argtypes = [ctypes.c_void_p]
    return lib


def test_the_two_entry_points_are_declared_exported_and_bound(ref_lib):
    """The entry points of include/quatro_voxelmap_batch.h are two of libquatro_ext.so's exports; header and binding name the
    same two; libquatro_hip.so exports neither; the item and the constants are their ctypes mirrors."""
    from quatro_amd import lib as ql
    assert ext_abi.check_header("quatro_voxelmap_batch.h") == TWO
    got = np.zeros(12, np.int32)
    ref_lib.vmap_batch_ref_layout(got.ctypes.data)
    I = ql.VmapRegItem
    assert list(got) == [ctypes.sizeof(ql.IcpResult), ctypes.sizeof(I), I.kf.offset, I.src4.offset, I.src_normals4.offset,
                         I.n.offset, I.mem.offset, I.guess.offset, ql.VMAP_BATCH_MAX, ql.VMAP_BATCH_TRACE, ql.VMAP_BATCH_CORR,
                         ql.VMAP_BATCH_TIMES]
    assert (int(got[1]), int(got[8])) == (160, 64)


def test_hypothesis_equals_its_python_restatement_bit_for_bit(ref_lib):
    from quatro_amd import api
    rng = np.random.default_rng(5)
    bases = [np.eye(4), R.rigid(R.rot(0.1, -0.2, 2.5), [10.0, -20.0, 1.5]), R.rigid(R.rot(-0.03, 0.02, -0.7), [-3.25, 7.5, 0.1])]
    bases += [R.rigid(R.rot(*rng.uniform(-3, 3, 3)), rng.uniform(-100, 100, 3)) for _ in range(5)]
    yaws = [0.0, -0.0, math.pi, -math.pi, math.pi / 2, 1e-9, 0.05, -2.9] + list(rng.uniform(-math.pi, math.pi, 8))
    yaws += [float(np.float32(1.2345))]  # (a place match's yaw is a float32)
    offs = [(0.0, 0.0), (1.0, -1.0), (0.45, -0.35), (-123.456, 7e-3)]
    for b in bases:
        for yaw in yaws:
            for dx, dy in offs:
                want = np.zeros(16)
                bb = np.ascontiguousarray(b.reshape(16))
                ref_lib.vmap_batch_ref_hypothesis(bb.ctypes.data, yaw, dx, dy, want.ctypes.data)
                got = api.pose_hypothesis(b, yaw, dx, dy)
                assert np.array_equal(_bits(got.reshape(16)), _bits(want)), (yaw, dx, dy)
                assert np.array_equal(got[3], [0.0, 0.0, 0.0, 1.0])
    # what the rule means: base . [Rz(yaw) | (dx, dy, 0)]; yaw 0 and no offset give the base's rows 0 - 2 back bit for bit
    b = bases[1]
    assert np.array_equal(_bits(api.pose_hypothesis(b, 0.0, 0.0, 0.0)[:3]), _bits(b[:3]))
    assert np.array_equal(_bits(api.pose_hypothesis(np.eye(4), 0.0)), _bits(np.eye(4)))
    assert np.allclose(api.pose_hypothesis(b, 0.3, 0.5, -0.25), b @ R.rigid(R.rot(0.0, 0.0, 0.3), [0.5, -0.25, 0.0]), atol=1e-12)
    assert np.allclose(api.pose_hypothesis(b, math.pi)[:3, :2], -b[:3, :2], atol=1e-14)
    # a row 3 that is not (0 0 0 1) is not read
    junk = b.copy()
    junk[3] = [1.0, 2.0, 3.0, 4.0]
    assert np.array_equal(_bits(api.pose_hypothesis(junk, 0.3, 1.0, 2.0)), _bits(api.pose_hypothesis(b, 0.3, 1.0, 2.0)))
    H = api.pose_hypotheses(b, (-0.1, 0.2), ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0)))
    assert H.shape == (6, 4, 4) and np.array_equal(_bits(H[4]), _bits(api.pose_hypothesis(b, 0.2, 1.0, 0.0)))
    assert api.pose_hypotheses(b, (), ((0.0, 0.0),)).shape == (0, 4, 4)


def test_best_equals_its_python_restatement(ref_lib):
    from quatro_amd import api
    from quatro_amd import lib as ql

    def both(rows):
        """rows: (status, valid, n_corr, rmse)"""
        arr = (ql.IcpResult * max(len(rows), 1))()
        for a, (st, v, n, e) in zip(arr, rows):
            a.status, a.valid, a.n_corr, a.rmse = st, v, n, e
        c = ref_lib.vmap_batch_ref_best(arr, len(rows))
        p = api.best_hypothesis([ql._icp_dict(arr[i]) for i in range(len(rows))])
        assert c == p, (rows, c, p)
        return c

    assert both([]) == -1                                                    # B = 0
    assert both([(0, 0, 100, 0.1), (7, 1, 500, 0.1), (1, 1, 9, 0.0)]) == -1    # all invalid or not run
    assert both([(0, 1, 10, 0.5), (0, 1, 30, 0.9), (0, 1, 20, 0.1)]) == 1      # the largest n_corr
    assert both([(0, 1, 30, 0.5), (0, 1, 30, 0.25), (0, 1, 30, 0.75)]) == 1    # ties in n_corr: the smaller rmse
    assert both([(0, 1, 30, 0.5), (0, 1, 30, 0.5), (0, 1, 30, 0.5)]) == 0      # ties in rmse: the smaller index
    assert both([(0, 0, 99, 0.0), (0, 1, 30, 0.5), (0, 1, 30, 0.5)]) == 1
    assert both([(0, 1, 30, 0.5), (7, 1, 99, 0.0), (0, 0, 99, 0.0), (0, 1, 31, 9.0)]) == 3
    rng = np.random.default_rng(9)
    for _ in range(200):
        B = int(rng.integers(1, 65))
        both([(int(rng.choice([0, 0, 0, 7])), int(rng.integers(0, 2)), int(rng.integers(0, 4)), float(rng.integers(0, 3)) / 4)
              for _ in range(B)])


@pytest.fixture(scope="module")
def hand_ref():
    return BC.hand_map(M.RefMap)


def _run(ref, case):
    items, icp = BC.CASES[case]()
    return items, [ref.register(p, a, g, **icp) for p, a, g in items]


def test_sizes_case_covers_the_chunk_edges(hand_ref):
    items, res = _run(hand_ref, "sizes")
    assert tuple(p.shape[0] for p, _, _ in items) == (0, 1, 255, 256, 257, 700)
    chunks = [-(-p.shape[0] // 256) for p, _, _ in items]
    assert chunks == [0, 1, 1, 1, 2, 3]  # every item but the last ends before the grid does
    assert not res[0]["valid"] and res[0]["stop_reason"] == STOP_TOO_FEW and np.array_equal(res[0]["T"], items[0][2])
    assert not res[1]["valid"] and res[1]["stop_reason"] == STOP_TOO_FEW and res[1]["iterations"] == 0
    assert all(r["valid"] and r["iterations"] >= 3 and r["n_corr"] >= 40 for r in res[2:])
    assert len({r["iterations"] for r in res[2:]}) >= 2  # at the defaults they also stop at different updates


def test_eight_guesses_case_gives_eight_different_runs(hand_ref):
    items, res = _run(hand_ref, "one_cloud_eight_guesses")
    assert len(items) == 8 and all(it[0] is items[0][0] and it[1] is items[0][1] for it in items)
    assert items[0][0].shape[0] == 300
    assert all(r["valid"] and r["iterations"] >= 3 for r in res)
    first = [hand_ref.register(p, a, g, teps=0.0, feps=0.0, max_iter=1)["T"].tobytes() for p, a, g in items]
    assert len(set(first)) == 8  # separate states: no two guesses share a first update


def test_invalid_case_really_ends_invalid_beside_good_ones(hand_ref):
    items, res = _run(hand_ref, "invalid_beside_good")
    assert res[0]["valid"] and res[2]["valid"] and res[0]["iterations"] >= 3 and res[2]["iterations"] >= 3
    bad = res[1]
    assert not bad["valid"] and not bad["converged"] and bad["stop_reason"] == STOP_TOO_FEW and bad["n_corr"] == 0
    assert bad["iterations"] == 0 and np.array_equal(bad["T"], BC.FAR) and np.all(bad["corr"] == -1)
    # the same cloud under a good guess is fine: it is the guess that fails
    assert items[1][0] is items[2][0]


def test_frozen_case_stops_at_different_updates(hand_ref):
    items, res = _run(hand_ref, "frozen")
    its = [r["iterations"] for r in res]
    print("frozen: iterations", its)
    assert all(r["valid"] and r["stop_reason"] == STOP_TEPS for r in res)
    assert len(set(its)) >= 3 and max(its) < 30 and max(its) - min(its) >= 4
    # a blocked loop of 4 launches per block has a short last block at 10 fixed updates, and at the epsilon's stops the host
    # leaves the loop between the first item's stop and the last one's
    assert min(its) > 4 and (min(its) - 1) // 4 < (max(its) - 1) // 4


def test_room_scene_meets_its_conditions():
    """The fixture's conditions (not measurements): the restatement's winner among the 27 hypotheses lies within half a
    voxel side of the truth, and nearer to it than every starting hypothesis."""
    from quatro_amd import api
    inserts, (q, qa), hyp = BC.room()
    assert len(inserts) == 3 and all(1900 <= p.shape[0] <= 2100 for p, _, _ in inserts) and hyp.shape == (27, 4, 4)
    ref = BC.room_map(M.RefMap)
    res = [ref.register(q, qa, g) for g in hyp]
    best = api.best_hypothesis(res)
    start = [float(np.linalg.norm(g[:3, 3] - BC.ROOM_TRUE[:3, 3])) for g in hyp]
    end = float(np.linalg.norm(res[best]["T"][:3, 3] - BC.ROOM_TRUE[:3, 3]))
    print(f"room: {len(ref)} voxels; winner {best} ends {end:.4f} m from the truth, the hypotheses start {min(start):.3f} .. "
          f"{max(start):.3f} m away; valid {sum(r['valid'] for r in res)} of 27")
    assert best >= 0 and res[best]["valid"]
    assert end < 0.5 * BC.ROOM_SIDE and end < min(start)
    assert min(start) > 0.5 * BC.ROOM_SIDE  # no hypothesis starts where the winner must end
    # one voxel side apart
    d = np.linalg.norm(hyp[1, :3, 3] - hyp[0, :3, 3])
    assert abs(d - BC.ROOM_SIDE) < 1e-12
