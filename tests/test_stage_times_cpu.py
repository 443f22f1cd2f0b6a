"""No-GPU: which fields of qtr_stage_times each shape of call reports, and between which of a slot's events
(quatro_amd/csrc/stage_times.h: plain data), compiled into a stand-alone program under ASan + UBSan."""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "quatro_amd", "csrc", "stage_times.h")

# event k is given the time 2^k: 0 begin, 1 voxel stage done (qtr_solve: correspondences staged), 2 graph, 3 clique, 4 solve,
# 5 the second stream's join (no stage time), 6 FPFH chain, 7 matcher, 8 the overlapped back end's start, 9 the overlapped
# call's end
T = [2 ** k for k in range(10)]
# shape -> (event synchronised first, nn fields filled, voxelize, fpfh, match, graph, clique, solve, total): what
# qtr_get_stage_times reports per shape of call (include/quatro_hip.h, DESIGN.md "Stage times"), written out by hand
WANT = {
    0: (-1, 0, 0, 0, 0, 0, 0, 0, 0),                                                                      # nothing pending
    1: (-1, 1, 0, 0, 0, 0, 0, 0, 0),                                                                      # stage events off
    2: (4, 0, 0, 0, 0, T[2] - T[1], T[3] - T[2], T[4] - T[3], T[4] - T[0]),                               # qtr_solve
    3: (4, 1, T[1] - T[0], T[6] - T[1], T[7] - T[6], T[2] - T[7], T[3] - T[2], T[4] - T[3], T[4] - T[0]),  # qtr_register_pair
    4: (7, 1, T[1] - T[0], T[6] - T[1], T[7] - T[6], 0, 0, 0, T[7] - T[0]),                               # qtr_feature_pair
    5: (4, 1, 0, 0, T[7] - T[0], T[2] - T[7], T[3] - T[2], T[4] - T[3], T[4] - T[0]),                     # qtr_register_keyframes
    6: (9, 1, T[1] - T[0], T[6] - T[1], T[7] - T[6], T[2] - T[8], T[3] - T[2], T[4] - T[3], T[9] - T[0]),  # back end beside the front end
}


def test_header_has_no_hip():
    txt = open(HEADER).read()
    assert "#include" not in txt and "__device__" not in txt and "hip" not in txt.replace("capi.hip", "")


def test_rows_of_every_shape(tmp_path):
    exe = str(tmp_path / "stage_times_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "quatro_amd", "csrc"),
                           os.path.join(ROOT, "tests", "stage_times", "stage_times_demo.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-800:]
    got = {}
    for ln in p.stdout.strip().splitlines():
        v = [int(x) for x in ln.split()]
        got[v[0]] = tuple(v[1:])
    assert got == WANT
