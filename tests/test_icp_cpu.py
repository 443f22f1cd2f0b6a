"""No-GPU checks of the ICP refinement (qtr_icp / qtr_refine_pair): the ctypes mirrors against the header, the host
restatement of the device loop (tests/icp_ref/icp_ref.cpp over include/qtr_icp_math.h) on exact data, and the
restatement against an independent scipy cKDTree ICP."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import icp_restate as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_icp_structs_match_the_header_layout(tmp_path):
    from quatro_amd import lib as ql
    pairs = {"qtr_icp_params": ql.IcpParams, "qtr_icp_result": ql.IcpResult}
    hdr = open(os.path.join(ROOT, "include", "quatro_hip.h")).read()
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "quatro_hip.h"', "int main(void) {"]
    for cname, cls in pairs.items():
        body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", hdr, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            head, *rest = [p.strip() for p in decl.split(",")]
            names.append(re.sub(r"\[.*?\]", "", head.split()[-1]))
            names += [re.sub(r"\[.*?\]", "", p) for p in rest]
        assert names == [n for n, _ in cls._fields_], (cname, names)
        lines.append(f'  printf("{cname} %zu", sizeof({cname}));')
        lines += [f'  printf(" %zu", offsetof({cname}, {n}));' for n in names]
        lines.append('  printf("\\n");')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n"):
        if not line.strip():
            continue
        w = line.split()
        cls = pairs[w[0]]
        assert int(w[1]) == ctypes.sizeof(cls), w[0]
        assert [int(v) for v in w[2:]] == [getattr(cls, n).offset for n, _ in cls._fields_], w[0]


def test_icp_defaults_and_entry_points_are_bound():
    from quatro_amd import lib as ql
    p = ql.default_icp_params()
    assert (p.max_correspondence_distance, p.transformation_epsilon, p.euclidean_fitness_epsilon) == (1.0, 1e-7, 1e-6)
    assert (p.max_iterations, p.method, p.min_correspondences) == (30, ql.ICP_POINT_TO_PLANE, 0)
    assert abs(p.normal_radius - 0.5) < 1e-7
    lib = ql.load()
    for n in ("qtr_default_icp_params", "qtr_icp", "qtr_refine_pair"):
        assert n in ql.EXPORTS and getattr(lib, n).argtypes is not None, n


def _exact_pair():
    s, n = R.box_scene()
    s[:, :3] = np.round(s[:, :3] * 64) / 64  # dyadic coordinates: the rigid copy below is exact in float32
    T = np.array([[0, -1, 0, 0.25], [1, 0, 0, -0.5], [0, 0, 1, 0.125], [0, 0, 0, 1.0]])
    tgt = R.apply(T, s)
    nt = n.copy()
    nt[:, :3] = n[:, :3] @ T[:3, :3].T
    assert np.array_equal(R.apply(np.linalg.inv(T), tgt)[:, :3], s[:, :3])
    return s, tgt, nt, T


@pytest.mark.parametrize("method", [0, 1])
def test_restatement_recovers_an_exact_rigid_copy(method):
    s, tgt, nt, T = _exact_pair()
    guess = T @ R.rigid(R.rot(0.02, -0.015, 0.03), [0.3, -0.2, 0.1])
    o = R.run(s, tgt, nt, guess, max_d=1.5, method=method, max_iter=60, teps=1e-12, feps=0.0)
    assert o["valid"] and o["converged"]
    assert np.abs(o["T"] - T).max() <= 1e-9
    assert o["fitness"] < 1e-20 and o["n_corr"] == s.shape[0]
    # the trace holds every update; the last row is the final transform
    assert o["trace"].shape == (o["iterations"], 18) and np.array_equal(o["trace"][-1, :16].reshape(4, 4), o["T"])


def test_restatement_stops_on_a_single_plane_and_far_guesses():
    rng = np.random.default_rng(3)
    plane = R.f4(np.c_[rng.random((2000, 2)) * 10, np.zeros(2000)])
    nrm = R.f4(np.tile([0.0, 0.0, 1.0], (2000, 1)))
    o = R.run(plane, plane, nrm, R.rigid(np.eye(3), [0.1, 0.1, 0.05]), method=0)
    assert o["stop_reason"] == 5 and not o["valid"] and np.isfinite(o["T"]).all()
    far = R.rigid(np.eye(3), [5000.0, 0, 0])
    s, tgt, nt, _ = _exact_pair()
    o = R.run(s, tgt, nt, far, method=0)
    assert o["stop_reason"] == 4 and not o["valid"] and o["iterations"] == 0 and np.array_equal(o["T"], far)


def _scipy_icp(src, tgt, nrm, T, max_d, method, iters):
    """Independent float64 ICP: cKDTree nearest neighbours, numpy least squares / SVD, the same number of updates."""
    from scipy.spatial import cKDTree
    tree = cKDTree(tgt[:, :3].astype(np.float64))
    p = src[:, :3].astype(np.float64)
    for _ in range(iters):
        q = p @ T[:3, :3].T + T[:3, 3]
        d, j = tree.query(q, distance_upper_bound=max_d)
        ok = np.isfinite(d)
        q, t = q[ok], tgt[j[ok], :3].astype(np.float64)
        if method == 0:
            n = nrm[j[ok], :3].astype(np.float64)
            J = np.c_[np.cross(q, n), n]
            r = ((q - t) * n).sum(1)
            x = np.linalg.solve(J.T @ J, -J.T @ r)
            w = x[:3] / 2
            qq = np.r_[1.0, w] / np.linalg.norm(np.r_[1.0, w])
            a, b, c, e = qq
            dR = np.array([[a * a + b * b - c * c - e * e, 2 * (b * c - a * e), 2 * (b * e + a * c)],
                           [2 * (b * c + a * e), a * a - b * b + c * c - e * e, 2 * (c * e - a * b)],
                           [2 * (b * e - a * c), 2 * (c * e + a * b), a * a - b * b - c * c + e * e]])
            dt = x[3:]
        else:
            mq, mt = q.mean(0), t.mean(0)
            U, _, Vt = np.linalg.svd((q - mq).T @ (t - mt))
            D = np.diag([1, 1, np.sign(np.linalg.det(Vt.T @ U.T))])
            dR = Vt.T @ D @ U.T
            dt = mt - dR @ mq
        T = R.rigid(dR, dt) @ T
    return T


@pytest.mark.parametrize("method", [0, 1])
def test_restatement_agrees_with_an_independent_scipy_icp(method):
    pytest.importorskip("scipy")
    rng = np.random.default_rng(7)
    s, n = R.box_scene(seed=5)
    Tt = R.rigid(R.rot(0.03, -0.02, 0.05), [0.4, -0.3, 0.2])
    tgt = R.apply(Tt, s)
    tgt[:, :3] += rng.normal(0, 0.01, (tgt.shape[0], 3)).astype(np.float32)  # sensor noise: no exact fixed point
    nt = n.copy()
    nt[:, :3] = n[:, :3] @ Tt[:3, :3].T
    o = R.run(s, tgt, nt, np.eye(4), max_d=1.0, method=method, max_iter=12, teps=0.0, feps=0.0)
    assert o["iterations"] == 12 and o["stop_reason"] == 1
    Ts = _scipy_icp(s, tgt, nt, np.eye(4), 1.0, method, 12)
    assert np.abs(o["T"] - Ts).max() < 1e-9
    assert R.rot_err_deg(o["T"], Tt) < 0.05 and np.abs(o["T"][:3, 3] - Tt[:3, 3]).max() < 0.02
