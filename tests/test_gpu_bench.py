"""bench.py's plain line (no --full): the contract's keys and nothing measured beside them, and --dump-outputs writing what
the timed entry point returned for the LAST timed step — equal to a direct qtr_register_pair_corr call on pool pair
(K - 1) % 4 for K = 7 and K = 6 (which also pins --steps as the number of timed steps), and identical from run to run,
since the inputs are seeded.  Once in one process, once as a two-rank launch on the one GPU (QTR_BENCH_ONE_DEVICE, gloo)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIELDS = ("status", "valid", "T", "cost", "gnc_iters", "n_clique", "n_rot_inliers", "n_final", "max_core", "n_edges",
          "n_card", "n_src", "n_tgt", "n_corr")


def _line(p):
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def _dumped(d):
    assert sorted(os.listdir(d)) == sorted(f + ".npy" for f in FIELDS)
    a = {f: np.load(os.path.join(d, f + ".npy")) for f in FIELDS}
    for f, v in a.items():
        assert v.dtype == np.float64 and np.isfinite(v).all(), f
    # a GNC cost is never negative: -1 stands for the record's +inf, GNC-TLS stopped at its first iteration
    assert a["cost"][0] >= 0 or (a["cost"][0] == -1 and a["gnc_iters"][0] == 1), (a["cost"], a["gnc_iters"])
    return a


@pytest.fixture(scope="module")
def direct():
    """pool pair `pid` of bench.py (the same seeded scans, correspondences, parameters and handle limits) through ONE host
    call of the timed entry point, as the dump's fields (cost +inf written as -1, like the dump)"""
    from quatro_amd import lib as ql
    from quatro_amd import synth
    h = ql.Handle(0, max_points=131072, max_voxels=32768, max_corr=8192)

    def run(pid):
        s, t, _ = synth.kitti64_pair_16k(pid)
        cs, ct, _, _ = synth.correspondences(5000, 0.05, seed=pid, noise=0.1)
        r = h.register_pair_corr(s, t, cs, ct, ql.default_frontend_params(seed=pid), ql.demo_params())
        return {"status": r["status"], "valid": int(r["valid"]), "T": r["T"],
                "cost": -1.0 if np.isposinf(r["cost"]) else r["cost"], "gnc_iters": r["gnc_iters"],
                "n_clique": r["clique"].size, "n_rot_inliers": r["n_rot_inliers"],
                "n_final": r["final_inliers"].size, "max_core": r["max_core"], "n_edges": r["n_edges"], "n_card": r["n_card"],
                "n_src": r["n_src"], "n_tgt": r["n_tgt"], "n_corr": r["L"]}
    yield run
    h.close()


def _same_record(a, want):
    for f in FIELDS:
        assert np.array_equal(a[f].ravel(), np.asarray(want[f], dtype=np.float64).ravel()), (f, a[f], want[f])


def _plain(tmp_path, tag, steps):
    d = str(tmp_path / tag)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
                        "--dump-outputs", d], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    return _line(p), _dumped(d)


def test_plain_line_and_dumped_outputs(tmp_path, direct):
    out, a = _plain(tmp_path, "a", 7)
    assert out["steps"] == 7 and out["warmup"] == 2 and out["n_gpus"] == 1
    assert out["metric"].startswith("scan-pair registrations/sec") and out["unit"] == "registrations/s"
    assert out["higher_is_better"] is True and out["dtype"].startswith("f32")
    assert out["ms_per_step"] > 0 and abs(out["value"] - 1e3 / out["ms_per_step"]) < 1e-6 * out["value"]
    for extra in ("roofline", "cpu_baseline", "parity_vs_oracle", "repeat_regions", "stage_ms", "batch256_leg"):
        assert extra not in out
    assert len(json.dumps(out)) < 1500
    assert a["T"].shape == (4, 4) and a["n_card"].shape == (3,)
    assert a["valid"][0] == 1 and a["status"][0] == 0 and a["n_corr"][0] == 5000 and a["n_clique"][0] > 0
    assert np.allclose(a["T"][3], [0, 0, 0, 1]) and np.allclose(a["T"][:3, :3] @ a["T"][:3, :3].T, np.eye(3), atol=1e-9)
    # the last of 7 timed steps registers pool pair (7 - 1) % 4 = 2, the last of 6 pair 1: the dump is that step's record
    p2, p1 = direct(2), direct(1)
    assert not np.array_equal(p2["T"], p1["T"])  # (the two pairs tell the step counts apart)
    _same_record(a, p2)
    out6, c = _plain(tmp_path, "c", 6)
    assert out6["steps"] == 6
    _same_record(c, p1)
    _, b = _plain(tmp_path, "b", 7)
    for f in FIELDS:
        assert np.array_equal(a[f], b[f]), f


def test_plain_line_of_a_two_rank_launch(tmp_path, direct):
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", QTR_BENCH_ONE_DEVICE="1", MASTER_ADDR="127.0.0.1")
    d = str(tmp_path / "r")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--dump-outputs", d]
    out = _line(subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                               timeout=600))
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["scaling"] == "weak" and out["value"] > 0
    assert "roofline" not in out and "sharded_leg" not in out
    _same_record(_dumped(d), direct(2))  # rank 0 times pair ids [0, 3): its last step is pair 2
