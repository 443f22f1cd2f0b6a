"""One call of each front-end path, for a kernel trace with per-kernel call counts (a profiler's kernel trace around
`python tests/probe/front_paths_trace.py`): one register_pair, one keyframe pair created and registered, one 4-pair batch
with refinement.  Two commits whose host code enqueues the same launches give the same counts.  Synthetic scans only."""
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))

import torch  # noqa: E402,F401  (first: one HIP runtime per process)

from quatro_amd import lib as ql  # noqa: E402
from quatro_amd import synth  # noqa: E402


def main():
    pairs = [synth.kitti64_pair(i)[:2] for i in range(4)]
    fp = ql.default_frontend_params(seed=1)
    h = ql.Handle(0, max_points=131072, max_voxels=32768, max_corr=8192, n_slots=4)
    try:
        r = h.register_pair(*pairs[0], fp)
        with h.keyframe(pairs[0][0], fp) as ks, h.keyframe(pairs[0][1], fp) as kt:
            k = h.register_keyframes(ks, kt, fp)
        res, ref = h.register_batch_refine([(s, t, 1) for s, t in pairs], fp)
    finally:
        h.close()
    print("pair", r["n_src"], r["n_tgt"], r["L"], r["clique"].size, "| keyframes", k["L"], k["clique"].size,
          "| batch", [(b["L"], b["clique"].size, q["iterations"]) for b, q in zip(res, ref)])


if __name__ == "__main__":
    main()
