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
# the voxel map's entry points (include/quatro_voxelmap.h) are a library of their own over the same sources: libquatro_hip.so's
# dynamic symbol table stays the C ABI of include/quatro_hip.h
VOXELMAP_LIB = os.path.join(HERE, "libquatro_voxelmap.so")
# ... and so are the map's upkeep entry points (include/quatro_voxelmap_keep.h): the other two tables stay what they were
VOXELMAP_KEEP_LIB = os.path.join(HERE, "libquatro_voxelmap_keep.so")
# ... and sweep deskew (include/quatro_deskew.h), a fourth
DESKEW_LIB = os.path.join(HERE, "libquatro_deskew.so")
# ... and the map's visibility carving (include/quatro_voxelmap_carve.h), a fifth
VOXELMAP_CARVE_LIB = os.path.join(HERE, "libquatro_voxelmap_carve.so")
# ... and the grouped map registration (include/quatro_voxelmap_batch.h), a sixth
VOXELMAP_BATCH_LIB = os.path.join(HERE, "libquatro_voxelmap_batch.so")
# ... and the evaluation of poses against the map (include/quatro_voxelmap_eval.h), a seventh
VOXELMAP_EVAL_LIB = os.path.join(HERE, "libquatro_voxelmap_eval.so")
SOURCES = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".inc", ".map"))) + [
    os.path.join("..", "..", "include", "qtr_math.h"), os.path.join("..", "..", "include", "qtr_icp_math.h"),
    os.path.join("..", "..", "include", "qtr_place_math.h"),
    os.path.join("..", "..", "include", "qtr_submap_math.h"), os.path.join("..", "..", "include", "qtr_eval_math.h"),
    os.path.join("..", "..", "include", "qtr_pgo_math.h"), os.path.join("..", "..", "include", "qtr_vmap_math.h"), os.path.join("..", "..", "include", "quatro_voxelmap.h"),
    os.path.join("..", "..", "include", "qtr_vmap_keep_math.h"), os.path.join("..", "..", "include", "quatro_voxelmap_keep.h"),
    os.path.join("..", "..", "include", "qtr_deskew_math.h"), os.path.join("..", "..", "include", "quatro_deskew.h"),
    os.path.join("..", "..", "include", "qtr_vmap_carve_math.h"), os.path.join("..", "..", "include", "quatro_voxelmap_carve.h"),
    os.path.join("..", "..", "include", "qtr_vmap_batch_math.h"), os.path.join("..", "..", "include", "quatro_voxelmap_batch.h"),
    os.path.join("..", "..", "include", "qtr_vmap_eval_math.h"), os.path.join("..", "..", "include", "quatro_voxelmap_eval.h"),
    os.path.join("..", "..", "include", "quatro_hip.h")]


def is_stale(lib: str = LIB) -> bool:
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    return any(os.path.getmtime(os.path.join(CSRC, s)) > t for s in SOURCES)


def build_test_engines(force: bool = False, verbose: bool = True) -> str:
    return build(force, verbose, lib=TEST_LIB, defines=("-DQTR_TEST_ENGINES",))


def build_voxelmap(force: bool = False, verbose: bool = True) -> str:
    build(force, verbose)  # (the two libraries come from the same sources)
    return build(force, verbose, lib=VOXELMAP_LIB, defines=("-DQTR_VOXELMAP_LIB",), exports="exports_voxelmap.map")


def build_voxelmap_keep(force: bool = False, verbose: bool = True) -> str:
    build_voxelmap(False, verbose)  # (the three libraries come from the same sources: the other two, where they are stale)
    return build(force, verbose, lib=VOXELMAP_KEEP_LIB, defines=("-DQTR_VOXELMAP_KEEP_LIB",),
                 exports="exports_voxelmap_keep.map")


def build_deskew(force: bool = False, verbose: bool = True) -> str:
    build_voxelmap_keep(False, verbose)  # (the four libraries come from the same sources: the other three, where they are stale)
    return build(force, verbose, lib=DESKEW_LIB, defines=("-DQTR_DESKEW_LIB",), exports="exports_deskew.map")


def build_voxelmap_carve(force: bool = False, verbose: bool = True) -> str:
    build_deskew(False, verbose)  # (the five libraries come from the same sources: the other four, where they are stale)
    return build(force, verbose, lib=VOXELMAP_CARVE_LIB, defines=("-DQTR_VOXELMAP_CARVE_LIB",),
                 exports="exports_voxelmap_carve.map")


def build_voxelmap_batch(force: bool = False, verbose: bool = True) -> str:
    build_voxelmap_carve(False, verbose)  # (the six libraries come from the same sources: the other five, where they are stale)
    return build(force, verbose, lib=VOXELMAP_BATCH_LIB, defines=("-DQTR_VOXELMAP_BATCH_LIB",),
                 exports="exports_voxelmap_batch.map")


def build_voxelmap_eval(force: bool = False, verbose: bool = True) -> str:
    build_voxelmap_batch(False, verbose)  # (the seven libraries come from the same sources: the other six, where they are stale)
    return build(force, verbose, lib=VOXELMAP_EVAL_LIB, defines=("-DQTR_VOXELMAP_EVAL_LIB",),
                 exports="exports_voxelmap_eval.map")


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
    build_voxelmap(force="--force" in sys.argv)
    build_voxelmap_keep(force="--force" in sys.argv)
    build_deskew(force="--force" in sys.argv)
    build_voxelmap_carve(force="--force" in sys.argv)
    build_voxelmap_batch(force="--force" in sys.argv)
    build_voxelmap_eval(force="--force" in sys.argv)
    build_test_engines(force="--force" in sys.argv)
