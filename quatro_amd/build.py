"""Builds quatro_amd/libquatro_hip.so for gfx950 with hipcc (cross-compiles without a GPU).

Flags that matter for parity with the CPU oracle:
  -ffp-contract=off                          no FMA contraction: float/double expressions round exactly as written
  -fhip-fp32-correctly-rounded-divide-sqrt   IEEE fp32 division / sqrt (the default, stated explicitly)
  no -ffast-math, denormals preserved (hipcc default)
"""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libquatro_hip.so")
# the product library above has ONE path; the comparison engines of the test-suite (all-exact / f32-MFMA nearest-neighbour
# search, one-workgroup matcher tails, peeling / sweep core numbers, quadratic ranking) and the knobs that select them
# live in a second build with -DQTR_TEST_ENGINES that only tests load (quatro_amd.lib.Handle(lib_path=...))
TEST_LIB = os.path.join(HERE, "libquatro_hip_testengines.so")
# every entry point added after include/quatro_hip.h (the six extension headers: voxel map, its upkeep, carving, grouped
# registration and evaluation, sweep deskew) is exported by ONE extension library over the same sources, -DQTR_EXT_LIB with
# exports_ext.map: libquatro_hip.so's dynamic symbol table stays the C ABI of include/quatro_hip.h
EXT_LIB = os.path.join(HERE, "libquatro_ext.so")
# both tables above are pinned by the test-suite, so what is added after them (include/quatro_place_batch.h onwards) is
# exported by a second extension library over the same sources, -DQTR_EXT2_LIB with exports_ext2.map
EXT2_LIB = os.path.join(HERE, "libquatro_ext2.so")
# that table is pinned too, so what is added after it (include/quatro_voxelmap_ct.h onwards) is exported by a third extension
# library over the same sources, -DQTR_EXT3_LIB with exports_ext3.map
EXT3_LIB = os.path.join(HERE, "libquatro_ext3.so")
INCLUDE = os.path.join(HERE, "..", "include")
SOURCES = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".inc", ".map"))) + sorted(
    os.path.join("..", "..", "include", f) for f in os.listdir(INCLUDE)
    if f.endswith(".h") and (f.startswith("quatro_") or (f.startswith("qtr_") and f.endswith("math.h"))))


def is_stale(lib: str = LIB) -> bool:
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    return any(os.path.getmtime(os.path.join(CSRC, s)) > t for s in SOURCES)


def build_test_engines(force: bool = False, verbose: bool = True) -> str:
    return build(force, verbose, lib=TEST_LIB, defines=("-DQTR_TEST_ENGINES",))


def build_ext(force: bool = False, verbose: bool = True) -> str:
    build(False, verbose)  # (the two libraries come from the same sources: the product library, where it is stale)
    return build(force, verbose, lib=EXT_LIB, defines=("-DQTR_EXT_LIB",), exports="exports_ext.map")


def build_ext2(force: bool = False, verbose: bool = True) -> str:
    build(False, verbose)  # (as build_ext: the product library, where it is stale)
    return build(force, verbose, lib=EXT2_LIB, defines=("-DQTR_EXT2_LIB",), exports="exports_ext2.map")


def build_ext3(force: bool = False, verbose: bool = True) -> str:
    build(False, verbose)  # (as build_ext: the product library, where it is stale)
    return build(force, verbose, lib=EXT3_LIB, defines=("-DQTR_EXT3_LIB",), exports="exports_ext3.map")


def build(force: bool = False, verbose: bool = True, lib: str = LIB, defines=(), exports: str = "exports.map") -> str:
    if not force and not is_stale(lib):
        return lib
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, *defines, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-Wno-unused-value", "-fvisibility=hidden",
           "-Wl,--version-script=" + os.path.join(CSRC, exports),
           os.path.join(CSRC, "unity.hip"), "-ldl", "-o", lib]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return lib


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    build_ext(force="--force" in sys.argv)
    build_ext2(force="--force" in sys.argv)
    build_ext3(force="--force" in sys.argv)
    build_test_engines(force="--force" in sys.argv)
