"""Times of the grouped place query (a diagnostic, not a test): Q queries against N entries, k = 10, 20 x 60, as
  arm A   Q single qtr_place_query_desc calls on device-resident descriptors (one wait each), and
  arm B   one qtr_place_query_batch, with the same descriptors as entry items (read in place) and as device-descriptor items,
for Q in {16, 256, 1024} and N in {1000, 10 000}.  The host clock runs around calls that end in their own wait; the arms
alternate inside each of --reps repetitions and every figure is the median [min - max] over them, per whole group of Q.  The
queries are entries of the index (entry q N / Q), so both arms answer the same questions; their records are compared in
the run.  Writes one JSON object (--out) and prints it.

  python tests/probe/place_batch_time.py [--reps 10] [--out profiles/place_batch_time.json]
  python tests/probe/place_batch_time.py --trace    # a short run for a kernel trace: 20 batches of 256 x 10 000, nothing else
"""
import argparse
import ctypes as C
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    from quatro_amd import lib as ql
    from quatro_amd import synth

    rng = np.random.default_rng(1)
    h = ql.Handle(0)
    h.set_stage_events(False)
    lib, lib2 = h._lib, ql.load_ext()
    kfs = [h.keyframe(s) for k in range(8) for s in synth.kitti64_pair(k)[:2]]
    with h.place_index(16) as small:
        for kf in kfs:
            small.add(kf)
        base = [small.fetch(i) for i in range(16)]
    N_MAX, K = 10000, 10
    ix = h.place_index(N_MAX)
    E = np.zeros((N_MAX, 20, 60), np.float32)
    ident = C.c_int(-1)
    for i in range(N_MAX):
        E[i] = np.roll(base[i % 16], i // 16, axis=1) * rng.uniform(0.6, 1.4, (20, 1))
        assert lib.qtr_place_index_add_desc(h._h, 0, ix._ix, E[i].ctypes.data, ql.MEM_HOST, C.byref(ident)) == 0
    dev = torch.from_numpy(E).cuda().contiguous()  # the same descriptors as caller-owned device memory
    torch.cuda.synchronize()

    def items_for(Q, N, kind):
        arr = (ql.PlaceQueryItem * Q)()
        for q in range(Q):
            e = (q * N) // Q
            arr[q].id_lo, arr[q].id_hi, arr[q].entry = 0, N, -1
            if kind == "entry":
                arr[q].entry = e
            else:
                arr[q].desc, arr[q].mem = dev.data_ptr() + e * 4800, ql.MEM_DEVICE
        return arr

    def arm_a(Q, N, out, n):
        one, po = C.c_int(0), out.ctypes.data
        for q in range(Q):
            e = (q * N) // Q
            rc = lib.qtr_place_query_desc(h._h, 0, ix._ix, dev.data_ptr() + e * 4800, ql.MEM_DEVICE, 0, N, K,
                                          C.cast(po + q * K * 16, C.POINTER(ql.PlaceMatch)), C.byref(one))
            assert rc == 0
            n[q] = one.value

    def arm_b(Q, items, out, n):
        assert lib2.qtr_place_query_batch(h._h, 0, ix._ix, items, Q, K, out.ctypes.data, n.ctypes.data) == 0

    if a.trace:
        items = items_for(256, N_MAX, "entry")
        out, n = np.zeros((256, K), ql.PLACE_MATCH_DTYPE), np.zeros(256, np.int32)
        for _ in range(20):
            arm_b(256, items, out, n)
        h.close()
        return

    res = {"unit": "ms per group of Q queries", "shape": [20, 60], "k": K, "repetitions": a.reps, "cases": []}
    for N in (1000, 10000):
        for Q in (16, 256, 1024):
            it_e, it_d = items_for(Q, N, "entry"), items_for(Q, N, "device")
            outs = [np.zeros((Q, K), ql.PLACE_MATCH_DTYPE) for _ in range(3)]
            ns = [np.zeros(Q, np.int32) for _ in range(3)]
            arm_a(Q, N, outs[0], ns[0])  # (warm: the arenas are grown here)
            arm_b(Q, it_e, outs[1], ns[1])
            arm_b(Q, it_d, outs[2], ns[2])
            same = all(np.array_equal(outs[0].view(np.uint8), o.view(np.uint8)) and np.array_equal(ns[0], m)
                       for o, m in zip(outs[1:], ns[1:]))
            assert same and (ns[0] == K).all(), (Q, N)
            ta, te, td = [], [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                arm_a(Q, N, outs[0], ns[0])
                t1 = time.perf_counter()
                arm_b(Q, it_e, outs[1], ns[1])
                t2 = time.perf_counter()
                arm_b(Q, it_d, outs[2], ns[2])
                t3 = time.perf_counter()
                ta.append((t1 - t0) * 1e3)
                te.append((t2 - t1) * 1e3)
                td.append((t3 - t2) * 1e3)
            res["cases"].append({"Q": Q, "N": N, "records_equal": bool(same), "A_single_calls": _mmm(ta),
                                 "B_batch_entry_items": _mmm(te), "B_batch_device_descriptors": _mmm(td),
                                 "A_over_B_entry_median": statistics.median(ta) / statistics.median(te),
                                 "A_over_B_device_median": statistics.median(ta) / statistics.median(td)})
    h.close()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
