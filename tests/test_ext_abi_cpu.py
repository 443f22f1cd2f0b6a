"""The two dynamic symbol tables, whole: libquatro_ext.so is the 25 entry points of the six extension headers, named one
by one in csrc/exports_ext.map, and libquatro_hip.so is the 75 of include/quatro_hip.h.  What each header declares is checked
beside its layouts in its own *_cpu.py test (tests/ext_abi.check_header)."""
import itertools
import os
import re

import ext_abi


def test_the_extension_library_exports_the_six_headers_and_the_product_library_its_own():
    from quatro_amd import lib as ql
    lists = [getattr(ql, attr) for attr, _ in ext_abi.HEADERS.values()]
    assert [len(names) for names in lists] == [count for _, count in ext_abi.HEADERS.values()] == [10, 2, 3, 3, 2, 5]
    for a, b in itertools.combinations(lists + [ql.EXPORTS], 2):
        assert not (set(a) & set(b))
    union = set().union(*lists)
    assert len(union) == 25 and list(ql.EXT_EXPORTS) == [n for names in lists for n in names]
    hip, ext = ext_abi.libraries()
    assert ext_abi.table(ext) == union
    assert ext_abi.table(hip) == set(ql.EXPORTS) and len(set(ql.EXPORTS)) == 75
    emap = open(os.path.join(ext_abi.ROOT, "quatro_amd", "csrc", "exports_ext.map")).read()
    assert set(re.findall(r"\b(qtr_[a-z_0-9]+)\s*;", emap)) == union
    assert emap.count("*") == 1 and re.search(r"\blocal:\s*\*;", emap)  # no wildcard among the globals
    elib = ql.load_ext()
    assert all(getattr(elib, n).argtypes is not None for n in union)
