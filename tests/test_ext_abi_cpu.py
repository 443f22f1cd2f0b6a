"""The two dynamic symbol tables, whole: libquatro_ext.so is the entry points of the extension headers — the 29 of the eight
in ext_abi.HEADERS and those of any header added since —, named one by one in csrc/exports_ext.map, and libquatro_hip.so is the
75 of include/quatro_hip.h, named one by one in csrc/exports.map; both carry the same device code.  What each header declares
is checked beside its layouts in its own *_cpu.py test (tests/ext_abi.check_header)."""
import itertools
import os
import re

import ext_abi


def _map_names(name):
    text = open(os.path.join(ext_abi.ROOT, "quatro_amd", "csrc", name)).read()
    assert text.count("*") == 1 and re.search(r"\blocal:\s*\*;", text)  # no wildcard among the globals
    return set(re.findall(r"\b(qtr_[a-z_0-9]+)\s*;", text))


def test_the_extension_library_exports_its_headers_and_the_product_library_its_own():
    from quatro_amd import lib as ql
    known = [getattr(ql, attr) for attr, _ in ext_abi.HEADERS.values()]
    assert [len(names) for names in known] == [count for _, count in ext_abi.HEADERS.values()] == [10, 2, 3, 3, 2, 5, 2, 2]
    assert len(set().union(*known)) == 29 and list(ql.EXT_EXPORTS)[:29] == [n for names in known for n in names]
    # every header that declares with QTR_EXT_API, the eight and whatever came later: nothing undeclared, nothing unlisted
    headers = ext_abi.extension_headers()
    lists = [getattr(ql, ext_abi.list_name(h)) for h in headers]
    assert lists[:len(known)] == known
    for header, names in zip(headers, lists):
        assert ext_abi.check_names(header) == set(names), header
    for a, b in itertools.combinations(lists + [ql.EXPORTS], 2):
        assert not (set(a) & set(b))
    union = set().union(*lists)
    assert set(ql.EXT_EXPORTS) == union and len(ql.EXT_EXPORTS) == len(union)
    hip, ext = ext_abi.libraries()
    assert ext_abi.table(ext) == union
    assert ext_abi.table(hip) == set(ql.EXPORTS) and len(set(ql.EXPORTS)) == 75
    assert _map_names("exports_ext.map") == union
    assert _map_names("exports.map") == set(ql.EXPORTS)
    elib = ql.load_ext()
    assert all(getattr(elib, n).argtypes is not None for n in union)
    # both libraries come from the same build: they carry the same device code, byte for byte
    code = ext_abi.fatbin(hip)
    assert len(code) > 1 << 20 and code == ext_abi.fatbin(ext)
