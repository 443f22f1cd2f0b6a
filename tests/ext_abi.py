"""What the symbol-table tests of the six extension headers share: libquatro_ext.so exports the entry points of
include/quatro_voxelmap.h, _keep.h, _carve.h, _batch.h, _eval.h and quatro_deskew.h and nothing else, and libquatro_hip.so's
table stays include/quatro_hip.h's.  Each header's own *_cpu.py test calls check_header beside its layout checks;
tests/test_ext_abi_cpu.py checks the two tables whole."""
import os
import re
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
# header -> (its list in quatro_amd.lib, how many entry points it declares)
HEADERS = {"quatro_voxelmap.h": ("VOXELMAP_EXPORTS", 10), "quatro_voxelmap_keep.h": ("VOXELMAP_KEEP_EXPORTS", 2),
           "quatro_deskew.h": ("DESKEW_EXPORTS", 3), "quatro_voxelmap_carve.h": ("VOXELMAP_CARVE_EXPORTS", 3),
           "quatro_voxelmap_batch.h": ("VOXELMAP_BATCH_EXPORTS", 2), "quatro_voxelmap_eval.h": ("VOXELMAP_EVAL_EXPORTS", 5)}


def table(path):
    """The dynamic symbol table of a library."""
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def libraries():
    """(libquatro_hip.so, libquatro_ext.so), built where they are stale."""
    from quatro_amd import build as qbuild
    ext = qbuild.build_ext(force=False, verbose=False)
    return qbuild.LIB, ext


def check_header(header):
    """The names the header declares with QTR_EXT_API at line start are all its qtr_...( names and quatro_amd.lib's list for
    it, as many as HEADERS says; libquatro_ext.so exports them and has their ctypes signatures, libquatro_hip.so and its
    list have none of them.  Returns the names."""
    from quatro_amd import lib as ql
    attr, count = HEADERS[header]
    hdr = open(os.path.join(ROOT, "include", header)).read()
    declared = set(re.findall(r"^QTR_EXT_API [^\n(]*?\b(qtr_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    assert declared == set(re.findall(r"\b(qtr_[a-z_0-9]+)\s*\(", hdr)) == set(getattr(ql, attr))
    assert len(declared) == len(getattr(ql, attr)) == count
    hip, ext = libraries()
    assert declared <= table(ext)
    assert not (table(hip) & declared) and not (set(ql.EXPORTS) & declared)
    elib = ql.load_ext()
    assert all(getattr(elib, n).argtypes is not None for n in declared)
    return declared
