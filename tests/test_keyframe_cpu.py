"""No-GPU checks of the keyframe entry points: the ctypes mirrors of the two new structs have the C sizes and field
offsets, every new entry refuses NULL arguments before it touches a device, and register_one_to_many's ranking rule."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

NEW_ENTRIES = ("qtr_keyframe_create", "qtr_keyframe_get_info", "qtr_keyframe_fetch", "qtr_keyframe_destroy",
               "qtr_register_keyframes", "qtr_submit_batch_keyframes")


@pytest.fixture(scope="module")
def lib():
    from quatro_amd import build as qbuild
    qbuild.build(force=False, verbose=False)
    from quatro_amd import lib as ql
    return ql.load()


def test_new_entries_are_exported_and_bound(lib):
    from quatro_amd import lib as ql
    for n in NEW_ENTRIES:
        assert n in ql.EXPORTS and hasattr(lib, n), n
        assert getattr(lib, n).argtypes is not None, n


def test_keyframe_struct_layouts_match_header(lib):
    """sizeof and the offset of every field, from a C program compiled against the header."""
    from quatro_amd import lib as ql
    info_f = [n for n, _ in ql.KeyframeInfo._fields_]
    desc_f = [n for n, _ in ql.KfPairDesc._fields_]
    prints = ['printf("%zu %zu\\n", sizeof(qtr_keyframe_info), sizeof(qtr_kf_pair_desc));']
    prints += [f'printf("%zu\\n", offsetof(qtr_keyframe_info, {f}));' for f in info_f]
    prints += [f'printf("%zu\\n", offsetof(qtr_kf_pair_desc, {f}));' for f in desc_f]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "quatro_hip.h"\nint main(void){' + "".join(prints) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = list(map(int, subprocess.check_output([exe]).split()))
    want = [C.sizeof(ql.KeyframeInfo), C.sizeof(ql.KfPairDesc)]
    want += [getattr(ql.KeyframeInfo, f).offset for f in info_f] + [getattr(ql.KfPairDesc, f).offset for f in desc_f]
    assert got == want


def test_null_arguments_are_refused_without_a_device(lib):
    from quatro_amd import lib as ql
    fp, prm, icp = ql.default_frontend_params(), ql.demo_params(), ql.default_icp_params()
    res, ires, info = ql.Result(), ql.IcpResult(), ql.KeyframeInfo()
    scan = np.zeros((8, 4), dtype=np.float32)
    kf = C.c_void_p()
    bad = ql.QTR_ERR_BAD_ARG
    assert lib.qtr_keyframe_create(None, 0, scan.ctypes.data, 8, C.byref(fp), ql.MEM_HOST, C.byref(kf)) == bad and not kf
    assert lib.qtr_keyframe_create(None, 0, scan.ctypes.data, 8, C.byref(fp), ql.MEM_HOST, None) == bad
    assert lib.qtr_keyframe_get_info(None, C.byref(info)) == bad
    assert lib.qtr_keyframe_fetch(None, None, ql.KF_VOX, None, 0) < 0
    lib.qtr_keyframe_destroy(None, None)  # (a no-op)
    assert lib.qtr_register_keyframes(None, 0, None, None, C.byref(fp), C.byref(prm), C.byref(res), None, None, 0) == bad
    descs = (ql.KfPairDesc * 1)()
    assert lib.qtr_submit_batch_keyframes(None, descs, 1, C.byref(fp), C.byref(prm), None, C.byref(res), None) == bad
    assert lib.qtr_submit_batch_keyframes(None, descs, 1, C.byref(fp), C.byref(prm), C.byref(icp), C.byref(res),
                                          C.byref(ires)) == bad


def test_one_to_many_ranking_rule():
    from quatro_amd import api
    rec = lambda valid, n: {"valid": valid, "n_final": n}  # noqa: E731
    assert api.best_candidate([rec(True, 5), rec(True, 9), rec(True, 7)]) == 1
    assert api.best_candidate([rec(True, 9), rec(True, 9), rec(True, 3)]) == 0  # ties: the lowest index
    assert api.best_candidate([rec(False, 99), rec(True, 2), rec(True, 2)]) == 1  # an invalid record never wins
    assert api.best_candidate([rec(False, 4), rec(False, 8)]) == -1
    assert api.best_candidate([]) == -1
    # records that carry the inlier list instead of its length (register_pair's dicts)
    lists = [{"valid": True, "final_inliers": np.arange(3)}, {"valid": True, "final_inliers": np.arange(6)},
             {"valid": False, "final_inliers": np.arange(60)}]
    assert api.best_candidate(lists) == 1


def test_one_to_many_pairs_the_query_with_every_candidate():
    """register_one_to_many is host-side glue: K pairs (query, candidate k, seed k) in candidate order, one batched job."""
    from quatro_amd import api
    from quatro_amd import lib as ql

    class FakeHandle:
        def register_batch_keyframes(self, pairs, fp, params, icp):
            self.pairs = pairs
            out = [{"valid": k != 0, "n_final": 10 + k} for k in range(len(pairs))]
            return out if icp is None else (out, [{"status": 0}] * len(pairs))

    h = FakeHandle()
    fp = ql.FrontendParams(0.3, 0.5, 0.75, 0.95, 1, 1, 7)
    recs, best = api.register_one_to_many(h, "q", ["a", "b", "c"], fp)
    assert h.pairs == [("q", "a", 7), ("q", "b", 7), ("q", "c", 7)] and best == 2 and len(recs) == 3
    recs, refined, best = api.register_one_to_many(h, "q", ["a", "b"], fp, icp=object(), seeds=[1, 2])
    assert h.pairs == [("q", "a", 1), ("q", "b", 2)] and best == 1 and len(refined) == 2
