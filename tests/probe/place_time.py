"""Times of the place index (a diagnostic, not a test): add per keyframe, query at 1 000 / 10 000 / 50 000 entries (filled
through add_desc with rolled and rescaled copies of real descriptors), k = 10, the host clock around calls that end in
their one synchronise; close_loop with k = 16 beside the 16-candidate one-to-many job it contains; and the same search in
the numpy restatement on the host CPU for scale.  Every figure is the median [min - max] of --reps repetitions, a
repetition being the mean over --calls calls.  Writes one JSON object (--out) and prints it.

  python tests/probe/place_time.py [--reps 5] [--calls 50] [--out profiles/place_time.json]
  python tests/probe/place_time.py --trace 10000    # a short run for a kernel trace: 20 queries at that size, nothing else
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))


def _mmm(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def _fill(ix, base, n, rng, np):
    while len(ix) < n:
        i = len(ix)
        d = np.roll(base[i % len(base)], i // len(base), axis=1) * rng.uniform(0.6, 1.4, (base[0].shape[0], 1))
        ix.add_desc(d.astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--no-cpu", action="store_true", help="skip the numpy restatement's search")
    a = ap.parse_args()
    import numpy as np
    from quatro_amd import lib as ql
    from quatro_amd import api, synth

    rng = np.random.default_rng(1)
    pool = [synth.kitti64_pair_16k(k) for k in range(16)]
    h = ql.Handle(0, n_slots=16)
    h.set_stage_events(False)
    src = [h.keyframe(p[0]) for p in pool]
    tgt = [h.keyframe(p[1]) for p in pool]
    small = h.place_index(16)
    for kf in tgt:
        small.add(kf)
    base = [small.fetch(i) for i in range(16)]
    qdesc = small.describe(src[2].fetch(ql.KF_VOX))

    if a.trace:
        ix = h.place_index(a.trace)
        _fill(ix, base, a.trace, rng, np)
        for _ in range(20):
            ix.query_desc(qdesc, 10)
            ix.query(src[2], 10)
        h.close()
        return

    out = {"unit": "ms", "shape": [20, 60], "k": 10, "calls_per_repetition": a.calls,
           "n_voxels": _mmm([k.info["n_voxels"] for k in src + tgt])}
    # add per keyframe (into a scratch index, warm)
    rep = []
    for _ in range(a.reps + 1):
        with h.place_index(16) as ix:
            t0 = time.perf_counter()
            for kf in tgt:
                ix.add(kf)
            rep.append((time.perf_counter() - t0) * 1e3 / 16)
    out["add_per_keyframe"] = _mmm(rep[1:])

    ix = h.place_index(50000)
    for n in (1000, 10000, 50000):
        before, t0 = len(ix), time.perf_counter()
        _fill(ix, base, n, rng, np)
        out[f"add_desc_per_entry_up_to_{n}"] = (time.perf_counter() - t0) * 1e3 / (n - before)  # (includes making the copy)
        for name, call in (("query_desc", lambda: ix.query_desc(qdesc, 10)), ("query_keyframe", lambda: ix.query(src[2], 10))):
            call()
            rep = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    call()
                rep.append((time.perf_counter() - t0) * 1e3 / a.calls)
            out[f"{name}_{n}"] = _mmm(rep)
        if n == 10000:
            rep = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    ix.query_desc(qdesc, 64)
                rep.append((time.perf_counter() - t0) * 1e3 / a.calls)
            out["query_desc_10000_k64"] = _mmm(rep)
    want = ix.query_desc(qdesc, 10)

    # close_loop with k = 16 beside the one-to-many job over the same 16 candidates
    fp, prm = ql.default_frontend_params(seed=2), ql.demo_params()
    cand = [tgt[m["id"]] for m in small.query(src[2], 16)]
    api.close_loop(h, small, tgt, src[2], 16, fp=fp, params=prm)
    api.register_one_to_many(h, src[2], cand, fp, prm)
    ra, rb, rq = [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        api.register_one_to_many(h, src[2], cand, fp, prm)
        ra.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        api.close_loop(h, small, tgt, src[2], 16, fp=fp, params=prm)
        rb.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        small.query(src[2], 16)
        rq.append((time.perf_counter() - t0) * 1e3)
    out["one_to_many_16"] = _mmm(ra)
    out["close_loop_k16_index_of_16"] = _mmm(rb)
    out["query_keyframe_16_entries_k16"] = _mmm(rq)

    if not a.no_cpu:
        import place_restate as pr
        E = np.stack([ix.fetch(i) for i in range(1000)])
        rep = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            got = pr.query(qdesc, E, 10)
            rep.append((time.perf_counter() - t0) * 1e3)
        out["numpy_restatement_search_1000"] = _mmm(rep)
        assert [g[0] for g in got] == [m["id"] for m in ix.query_desc(qdesc, 10, 0, 1000)]
    out["top10_of_50000"] = [[m["id"], m["shift"], float(m["distance"])] for m in want]
    h.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
