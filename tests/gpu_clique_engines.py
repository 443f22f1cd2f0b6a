"""The comparison engines of the clique stage on the named graphs of tests/clique_cases.py.  The product library has one
path; this script loads the -DQTR_TEST_ENGINES build, where QTR_KCORE=peel (the peeling workgroup for every size),
QTR_KCORE=sweeps (h-index sweeps, one launch each), QTR_RANK_QUADRATIC=1 (the quadratic ranking and its own core-number
launch) and QTR_CLIQUE_ROUND0=1 (round 0 of the clique search in a launch of its own) select the older chains.  The
library reads these variables once, so tests/test_gpu_clique_cases.py starts one process per setting.  Every case of at
most 4097 vertices — and, under `peel`, the path of 16385 vertices, whose queue does not fit LDS — must give the oracle's
clique, largest core, core numbers and (core, id) order, exactly as the product route does.
usage: QTR_KCORE=peel python tests/gpu_clique_engines.py QTR_KCORE=peel"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
from quatro_amd import lib as ql  # noqa: E402
from oracle import oracle as qo  # noqa: E402
import clique_cases as cc  # noqa: E402
from test_gpu_clique_cases import MODES, check_case  # noqa: E402


def main():
    setting = sys.argv[1] if len(sys.argv) > 1 else ""
    if setting:
        var, value = setting.split("=", 1)
        assert os.environ.get(var) == value, f"{var} is not set to {value} in this process"
    names = [n for n in cc.NAMES if cc.size_of(n) <= 4097]
    if setting == "QTR_KCORE=peel":
        names.append("path_16385")
    h = ql.Handle(0, lib_path=ql.TEST_ENGINES_LIB_PATH)
    lines = []
    for n in names:
        c = cc.case(n)
        bm = cc.case(n[6:] if n.startswith("dirty_") else n).bitmap  # (the oracle reads the bits as they are)
        core, _, mc = qo.kcore(bm)
        ref = {"core": np.asarray(core), "max_core": int(mc)}
        for mode, thr in MODES:
            ref[(mode, thr)] = qo.max_clique(bm, mode, thr)
        check_case(h, c, ref, say=lines.append)
    h.close()
    print("\n".join(lines[-4:]))
    print(f"{setting or 'no setting'}: {len(names)} cases")
    print("CLIQUE_ENGINES_OK")


if __name__ == "__main__":
    main()
