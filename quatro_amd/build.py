"""Builds quatro_amd/libquatro_hip.so and libquatro_ext.so for gfx950 with hipcc (cross-compiles without a GPU).

Flags that matter for parity with the CPU oracle:
  -ffp-contract=off                          no FMA contraction: float/double expressions round exactly as written
  -fhip-fp32-correctly-rounded-divide-sqrt   IEEE fp32 division / sqrt (the default, stated explicitly)
  no -ffast-math, denormals preserved (hipcc default)

csrc/unity.hip is compiled ONCE to an object, and that object is linked twice: with csrc/exports.map into the product
library, whose dynamic symbol table is the C ABI of include/quatro_hip.h, and with csrc/exports_ext.map into the extension
library, whose table is the C ABI of every extension header (include/quatro_voxelmap.h onwards).  The version script alone
decides a table, and the two libraries cannot come from different builds.
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libquatro_hip.so")
EXT_LIB = os.path.join(HERE, "libquatro_ext.so")
# the product library above has ONE path; the comparison engines of the test-suite (all-exact / f32-MFMA nearest-neighbour
# search, one-workgroup matcher tails, peeling / sweep core numbers, quadratic ranking) and the knobs that select them
# live in a second compile with -DQTR_TEST_ENGINES that only tests load (quatro_amd.lib.Handle(lib_path=...))
TEST_LIB = os.path.join(HERE, "libquatro_hip_testengines.so")
OBJ = os.path.join(HERE, "unity.o")
TEST_OBJ = os.path.join(HERE, "unity_testengines.o")
INCLUDE = os.path.join(HERE, "..", "include")
SOURCES = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".inc"))) + sorted(
    os.path.join("..", "..", "include", f) for f in os.listdir(INCLUDE)
    if f.endswith(".h") and (f.startswith("quatro_") or (f.startswith("qtr_") and f.endswith("math.h"))))


def _hipcc(args, verbose: bool) -> None:
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *args]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def _compile(force: bool, verbose: bool, obj: str, defines=()) -> None:
    """unity.hip -> obj, where obj is missing or a source is newer than it."""
    if not force and os.path.exists(obj):
        t = os.path.getmtime(obj)
        if not any(os.path.getmtime(os.path.join(CSRC, s)) > t for s in SOURCES):
            return
    _hipcc([*defines, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
            "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-Wno-unused-value", "-fvisibility=hidden",
            "-c", os.path.join(CSRC, "unity.hip"), "-o", obj], verbose)


def _link(verbose: bool, obj: str, lib: str, exports: str) -> str:
    """obj -> lib under the version script `exports`, where lib is missing or older than obj or the script."""
    script = os.path.join(CSRC, exports)
    if os.path.exists(lib) and os.path.getmtime(lib) >= max(os.path.getmtime(obj), os.path.getmtime(script)):
        return lib
    _hipcc(["--hip-link", "--offload-arch=gfx950", "-fPIC", "-shared", "-Wl,--version-script=" + script, obj, "-ldl", "-o", lib],
           verbose)
    return lib


def build(force: bool = False, verbose: bool = True) -> str:
    """Both libraries of the one object (a forced or stale compile makes both stale); returns the product library."""
    _compile(force, verbose, OBJ)
    _link(verbose, OBJ, EXT_LIB, "exports_ext.map")
    return _link(verbose, OBJ, LIB, "exports.map")


def build_ext(force: bool = False, verbose: bool = True) -> str:
    build(force, verbose)
    return EXT_LIB


def build_test_engines(force: bool = False, verbose: bool = True) -> str:
    _compile(force, verbose, TEST_OBJ, defines=("-DQTR_TEST_ENGINES",))
    return _link(verbose, TEST_OBJ, TEST_LIB, "exports.map")


def build_all(force: bool = False, verbose: bool = True) -> tuple:
    """(LIB, EXT_LIB, TEST_LIB); the two compiles are independent and run side by side."""
    with ThreadPoolExecutor(max_workers=2) as pool:
        jobs = [pool.submit(f, force, verbose) for f in (build, build_test_engines)]
        lib, test_lib = (j.result() for j in jobs)
    return lib, EXT_LIB, test_lib


if __name__ == "__main__":
    build_all(force="--force" in sys.argv)
