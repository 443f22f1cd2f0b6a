"""Time of a registration on raw scans against the same registration on pre-built keyframes, one handle, same process.

  (a) register_pair on raw scans            (b) register_keyframes on keyframes made beforehand
over kitti64_pair_16k(0..15), alternating (a, b, a, b ...) after a warm-up of both, the host clock around calls that end
in a synchronise; per repetition the mean time of a registration over the pool, reported as median [min - max] of the
repetitions.  Also: qtr_keyframe_create per scan, a 64-pair batch on 16 slots both ways, and a 1-versus-16 loop-closing
job against 16 register_pair calls.  Writes one JSON object (--out) and prints it.

  python tests/probe/keyframe_time.py [--reps 5] [--rounds 13] [--out profiles/keyframe_time.json]
  python tests/probe/keyframe_time.py --trace    # a short run for a kernel trace (load / pack kernel durations)
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))


def _mmm(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=13, help="passes over the 16 pairs per repetition (13 x 16 = 208 registrations)")
    ap.add_argument("--out", default="")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    import numpy as np
    from quatro_amd import lib as ql
    from quatro_amd import api, synth

    pool = [synth.kitti64_pair_16k(k) for k in range(16)]
    fps = [ql.default_frontend_params(seed=k) for k in range(16)]
    prm = ql.demo_params()
    h = ql.Handle(0, n_slots=16)
    h.set_stage_events(False)  # (as the drop-in classes run: no event markers in either path)
    out = {"pool": "kitti64_pair_16k(0..15)", "unit": "ms"}

    t_create = []
    kfs = []
    for s, t, _ in pool:
        for c in (s, t):
            t0 = time.perf_counter()
            kfs.append(h.keyframe(c))
            t_create.append((time.perf_counter() - t0) * 1e3)
    src, tgt = kfs[0::2], kfs[1::2]
    out["n_voxels"] = _mmm([k.info["n_voxels"] for k in kfs])
    out["device_bytes"] = _mmm([k.info["device_bytes"] for k in kfs])
    if a.trace:
        for k in range(16):
            h.register_pair(pool[k][0], pool[k][1], fps[k], prm)
            h.register_keyframes(src[k], tgt[k], fps[k], prm)
        h.register_batch_keyframes([(src[k], tgt[k], k) for k in range(16)], fps[0], prm, want_lists=False)
        h.close()
        return
    # creation again, warm (the first pass above includes first-use costs)
    t_create = []
    for s, t, _ in pool:
        t0 = time.perf_counter()
        h.keyframe(s).close()
        t_create.append((time.perf_counter() - t0) * 1e3)
    out["keyframe_create_per_scan"] = _mmm(t_create)

    def one_a(k):
        t0 = time.perf_counter()
        r = h.register_pair(pool[k][0], pool[k][1], fps[k], prm)
        return (time.perf_counter() - t0) * 1e3, r

    def one_b(k):
        t0 = time.perf_counter()
        r = h.register_keyframes(src[k], tgt[k], fps[k], prm)
        return (time.perf_counter() - t0) * 1e3, r

    for k in range(16):  # warm-up of both, and the bits
        ra, rb = one_a(k)[1], one_b(k)[1]
        assert np.array_equal(ra["T"].view(np.uint64), rb["T"].view(np.uint64)), k
    rep_a, rep_b = [], []
    for _ in range(a.reps):
        ta = tb = 0.0
        for _ in range(a.rounds):
            for k in range(16):
                ta += one_a(k)[0]
                tb += one_b(k)[0]
        rep_a.append(ta / (16 * a.rounds))
        rep_b.append(tb / (16 * a.rounds))
    out["register_pair_raw"] = _mmm(rep_a)
    out["register_keyframes"] = _mmm(rep_b)
    out["registrations_per_repetition"] = 16 * a.rounds
    out["single_ratio_raw_over_keyframes"] = statistics.median(rep_a) / statistics.median(rep_b)
    out["single_keyframes_max_below_raw_min"] = max(rep_b) < min(rep_a)

    raw64 = [(pool[k % 16][0], pool[k % 16][1], k) for k in range(64)]
    kf64 = [(src[k % 16], tgt[k % 16], k) for k in range(64)]
    h.register_batch(raw64, fps[0], prm, want_lists=False)
    h.register_batch_keyframes(kf64, fps[0], prm, want_lists=False)
    ba, bb = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        h.register_batch(raw64, fps[0], prm, want_lists=False)
        ba.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        h.register_batch_keyframes(kf64, fps[0], prm, want_lists=False)
        bb.append((time.perf_counter() - t0) * 1e3)
    out["batch64_raw"] = _mmm(ba)
    out["batch64_keyframes"] = _mmm(bb)
    out["batch_ratio_raw_over_keyframes"] = statistics.median(ba) / statistics.median(bb)

    la, lb = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        for k in range(16):
            h.register_pair(pool[2][0], pool[k][1], fps[2], prm)
        la.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        api.register_one_to_many(h, src[2], tgt, fps[2], prm)
        lb.append((time.perf_counter() - t0) * 1e3)
    out["loop_closing_1v16_raw_calls"] = _mmm(la)
    out["loop_closing_1v16_keyframe_job"] = _mmm(lb)
    out["loop_closing_ratio"] = statistics.median(la) / statistics.median(lb)
    h.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
