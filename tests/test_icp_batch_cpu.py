"""No-GPU checks of the batched refinement entry (qtr_submit_batch_refine): declared in the header, exported by the built
library, bound in quatro_amd.lib with argtypes, and the ctypes mirrors of the records it reads and writes have the C
layout's sizes."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_submit_batch_refine_is_declared_exported_and_bound():
    from quatro_amd import lib as ql
    hdr = open(os.path.join(ROOT, "include", "quatro_hip.h")).read()
    decl = re.search(r"QTR_API int qtr_submit_batch_refine\((.*?)\);", hdr, flags=re.S)
    assert decl, "qtr_submit_batch_refine is not declared with QTR_API"
    assert len(decl.group(1).split(",")) == 9
    out = subprocess.run(["nm", "-D", "--defined-only", ql.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT qtr_submit_batch_refine$", out, flags=re.M), "not exported by the built library"
    assert "qtr_submit_batch_refine" in ql.EXPORTS
    lib = ql.load()
    at = lib.qtr_submit_batch_refine.argtypes
    assert at is not None and len(at) == 9
    assert at[1] is ctypes.POINTER(ql.PairDesc) and at[5] is ctypes.POINTER(ql.IcpParams)
    assert at[6] is ctypes.POINTER(ql.Result) and at[7] is ctypes.POINTER(ql.IcpResult)
    h = ql.Handle.__new__(ql.Handle)  # (the Python entry points exist without a device)
    assert callable(getattr(h, "register_batch_refine")) and callable(getattr(h, "register_batch_dev_refine"))


def test_batch_refine_records_have_the_header_sizes(tmp_path):
    from quatro_amd import lib as ql
    mirrors = {"qtr_icp_params": ql.IcpParams, "qtr_icp_result": ql.IcpResult, "qtr_pair_desc": ql.PairDesc}
    lines = ['#include <stdio.h>', '#include "quatro_hip.h"', "int main(void) {"]
    lines += [f'  printf("{c} %zu\\n", sizeof({c}));' for c in mirrors]
    lines += ["  return 0;", "}"]
    src = tmp_path / "sizes.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
               if line.strip())
    for c, cls in mirrors.items():
        assert int(got[c]) == ctypes.sizeof(cls), c
