"""What the symbol-table tests of the extension headers share: libquatro_ext.so exports the entry points of the eight headers
of HEADERS (include/quatro_voxelmap.h, _keep.h, _carve.h, _batch.h, _eval.h, _ct.h, quatro_deskew.h and quatro_place_batch.h),
of every later include/quatro_*.h that declares with QTR_EXT_API, and nothing else, and libquatro_hip.so's table stays
include/quatro_hip.h's.  Each header's own *_cpu.py test calls check_header beside its layout checks;
tests/test_ext_abi_cpu.py checks the two tables whole.

A header that is not in HEADERS needs no line here.  Its list in quatro_amd.lib is named after the file,
include/quatro_<name>.h -> <NAME>_EXPORTS (list_name), and check_names holds it to what check_header asks of the eight,
less the literal count."""
import glob
import os
import re
import subprocess
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
# header -> (its list in quatro_amd.lib, how many entry points it declares)
HEADERS = {"quatro_voxelmap.h": ("VOXELMAP_EXPORTS", 10), "quatro_voxelmap_keep.h": ("VOXELMAP_KEEP_EXPORTS", 2),
           "quatro_deskew.h": ("DESKEW_EXPORTS", 3), "quatro_voxelmap_carve.h": ("VOXELMAP_CARVE_EXPORTS", 3),
           "quatro_voxelmap_batch.h": ("VOXELMAP_BATCH_EXPORTS", 2), "quatro_voxelmap_eval.h": ("VOXELMAP_EVAL_EXPORTS", 5),
           "quatro_place_batch.h": ("PLACE_BATCH_EXPORTS", 2), "quatro_voxelmap_ct.h": ("VMAP_CT_EXPORTS", 2)}
DECLARATION = r"^QTR_EXT_API [^\n(]*?\b(qtr_[a-z_0-9]+)\s*\("


def table(path):
    """The dynamic symbol table of a library."""
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def fatbin(path):
    """The device code a library carries: its .hip_fatbin section."""
    with tempfile.TemporaryDirectory(prefix="fatbin_") as tmp:
        out = os.path.join(tmp, "fatbin")
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", path, out])
        return open(out, "rb").read()


def libraries():
    """(libquatro_hip.so, libquatro_ext.so), built where they are stale."""
    from quatro_amd import build as qbuild
    ext = qbuild.build_ext(force=False, verbose=False)
    return qbuild.LIB, ext


def extension_headers():
    """The eight of HEADERS in their order, then every other include/quatro_*.h that declares with QTR_EXT_API."""
    found = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "quatro_*.h"))
                   if re.search(DECLARATION, open(p).read(), flags=re.M))
    assert set(HEADERS) <= set(found)
    return list(HEADERS) + [h for h in found if h not in HEADERS]


def list_name(header):
    """The name of the header's list in quatro_amd.lib."""
    return HEADERS[header][0] if header in HEADERS else header[len("quatro_"):-len(".h")].upper() + "_EXPORTS"


def check_names(header):
    """The names the header declares with QTR_EXT_API at line start are all its qtr_...( names and quatro_amd.lib's list for
    it, each once.  Returns the names."""
    from quatro_amd import lib as ql
    names = getattr(ql, list_name(header))
    hdr = open(os.path.join(ROOT, "include", header)).read()
    declared = set(re.findall(DECLARATION, hdr, flags=re.M))
    assert declared == set(re.findall(r"\b(qtr_[a-z_0-9]+)\s*\(", hdr)) == set(names)
    assert len(declared) == len(names)
    return declared


def check_header(header):
    """check_names, as many names as HEADERS says; libquatro_ext.so exports them and has their ctypes signatures,
    libquatro_hip.so and its list have none of them.  Returns the names."""
    from quatro_amd import lib as ql
    declared = check_names(header)
    assert len(declared) == HEADERS[header][1]
    hip, ext = libraries()
    assert declared <= table(ext)
    assert not (table(hip) & declared) and not (set(ql.EXPORTS) & declared)
    elib = ql.load_ext()
    assert all(getattr(elib, n).argtypes is not None for n in declared)
    return declared
