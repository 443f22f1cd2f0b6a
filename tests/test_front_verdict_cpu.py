"""No-GPU: the decisions the front-end drivers of quatro_amd/csrc/capi.hip take from a cloud's device counters
(quatro_amd/csrc/front_verdict.h: plain functions of integers), compiled into a stand-alone program under ASan + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

OK, TIMEOUT, PASS_TOO_LARGE, TOO_MANY, EMPTY = range(5)  # enum VoxReason
LISTS_OK, TILE_ERROR, CAPACITY, NEED_LONG = range(4)     # enum ListsVerdict


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("front_verdict") / "front_verdict_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "quatro_amd", "csrc"),
                           os.path.join(ROOT, "tests", "front_verdict", "front_verdict_demo.cpp"), "-o", exe])

    def call(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr[-800:]
        out = [tuple(int(x) for x in ln.split()) for ln in p.stdout.strip().splitlines()]
        assert len(out) == len(lines)
        return out
    return call


def test_header_has_no_hip():
    txt = open(os.path.join(ROOT, "quatro_amd", "csrc", "front_verdict.h")).read()
    assert "#include" not in txt and "__device__" not in txt and "hip" not in txt.replace("capi.hip", "")


def test_vox_verdict_full_table(run):
    M = 64  # max_voxels
    # (NVOX, overflow flag, P) -> (n, passed, reason)
    table = {
        # a tile never published its count: nothing else is looked at
        (-1, 0, 1): (0, 0, TIMEOUT), (-1, 0, M): (0, 0, TIMEOUT), (-1, 0, M + 1): (0, 0, TIMEOUT),
        (-1, 1, 1): (0, 0, TIMEOUT), (-1, 1, M): (0, 0, TIMEOUT), (-1, 1, M + 1): (0, 0, TIMEOUT),
        # a voxel grid: the count decides, whatever P
        (0, 0, 1): (0, 0, EMPTY), (0, 0, M): (0, 0, EMPTY), (0, 0, M + 1): (0, 0, EMPTY),
        (1, 0, 1): (1, 0, OK), (1, 0, M): (1, 0, OK), (1, 0, M + 1): (1, 0, OK),
        (M, 0, 1): (M, 0, OK), (M, 0, M): (M, 0, OK), (M, 0, M + 1): (M, 0, OK),
        (M + 1, 0, 1): (M + 1, 0, TOO_MANY), (M + 1, 0, M): (M + 1, 0, TOO_MANY), (M + 1, 0, M + 1): (M + 1, 0, TOO_MANY),
        # pass-through: n = P, whatever the count word holds
        (0, 1, 1): (1, 1, OK), (0, 1, M): (M, 1, OK), (0, 1, M + 1): (M + 1, 1, PASS_TOO_LARGE),
        (1, 1, 1): (1, 1, OK), (1, 1, M): (M, 1, OK), (1, 1, M + 1): (M + 1, 1, PASS_TOO_LARGE),
        (M, 1, 1): (1, 1, OK), (M, 1, M): (M, 1, OK), (M, 1, M + 1): (M + 1, 1, PASS_TOO_LARGE),
        (M + 1, 1, 1): (1, 1, OK), (M + 1, 1, M): (M, 1, OK), (M + 1, 1, M + 1): (M + 1, 1, PASS_TOO_LARGE),
    }
    assert len(table) == 5 * 2 * 3
    keys = sorted(table)
    got = run([f"v {nvox} {ovf} {P} {M}" for nvox, ovf, P in keys])
    for k, g in zip(keys, got):
        assert g == table[k], (k, g, table[k])


def _passes(run, state, bits, launched, attempt):
    (rerun, passes, fewer), = run([f"p {state[0]} {state[1]} {bits} {launched} {attempt}"])
    return rerun, (passes, fewer)


def test_first_call_that_under_launches_reruns_with_four_passes_exactly_once(run):
    state = (2, 3)  # the slot's last calls needed 2 passes; this one needs 3 (17 .. 24 bits)
    rerun, state = _passes(run, state, 20, launched=2, attempt=0)
    assert rerun == 1 and state == (4, 0)
    rerun, state = _passes(run, state, 20, launched=4, attempt=1)  # the second run: enough, and one call towards stepping down
    assert rerun == 0 and state == (4, 1)


def test_attempt_one_never_reruns(run):
    for bits in (0, 8, 9, 20, 32, 33):
        for launched in (1, 2, 3, 4):
            rerun, _ = _passes(run, (launched, 0), bits, launched, attempt=1)
            assert rerun == 0, (bits, launched)
    rerun, state = _passes(run, (1, 2), 32, launched=1, attempt=1)  # still under-launched: no third run, no step
    assert rerun == 0 and state == (1, 0)


def test_four_agreeing_calls_step_down_on_the_fourth(run):
    state = (4, 0)
    for call in range(1, 5):
        rerun, state = _passes(run, state, 20, launched=state[0], attempt=0)  # 20 bits: 3 passes would do
        assert rerun == 0
        assert state == ((4, call) if call < 4 else (3, 0)), (call, state)
    rerun, state = _passes(run, state, 20, launched=3, attempt=0)  # exactly what it needs from now on
    assert rerun == 0 and state == (3, 0)


def test_alternating_needs_never_step_down(run):
    state = (4, 0)
    for call in range(12):
        rerun, state = _passes(run, state, 20 if call % 2 == 0 else 30, launched=state[0], attempt=0)
        assert rerun == 0 and state[0] == 4 and state[1] == (1 if call % 2 == 0 else 0), (call, state)


def test_sort_bits_clamp_to_one_and_four_passes(run):
    # 0 bits need 1 pass, not 0: a launch of 1 is enough, and four calls at 2 step down to 1
    assert _passes(run, (1, 0), 0, launched=1, attempt=0) == (0, (1, 0))
    state = (2, 0)
    for _ in range(4):
        rerun, state = _passes(run, state, 0, launched=2, attempt=0)
        assert rerun == 0
    assert state == (1, 0)
    # 33 bits need 4 passes, not 5: a launch of 4 is never under-launched
    assert _passes(run, (4, 2), 33, launched=4, attempt=0) == (0, (4, 0))
    assert _passes(run, (3, 0), 33, launched=3, attempt=0) == (1, (4, 0))


def test_lists_verdict_precedence(run):
    cases = []  # (long_lists, lines, tail0, cap0, ovf0, tail1, cap1, ovf1) -> verdict
    for lines in (1, 2):
        for ll in (0, 1):
            for where in range(lines):  # which counter line carries the words
                def line(t, c, o):
                    w = [0, 0, 0, 0, 0, 0]
                    w[3 * where:3 * where + 3] = [t, c, o]
                    return (ll, lines, *w)
                cases += [
                    (line(0, 0, 0), LISTS_OK),
                    (line(1, 0, 0), TILE_ERROR), (line(1, 1, 0), TILE_ERROR), (line(1, 0, 1), TILE_ERROR),
                    (line(1, 1, 1), TILE_ERROR),                       # tile error before capacity before overflow
                    (line(0, 1, 0), CAPACITY), (line(0, 1, 1), CAPACITY),
                    (line(0, 0, 1), LISTS_OK if ll else NEED_LONG),     # an overflow is served when the chain had long lists
                ]
    # the words of the two lines are OR-ed: the higher verdict wins wherever it stands
    cases += [((0, 2, 0, 0, 1, 1, 0, 0), TILE_ERROR), ((0, 2, 0, 1, 0, 1, 0, 0), TILE_ERROR),
              ((0, 2, 0, 0, 1, 0, 1, 0), CAPACITY), ((1, 2, 0, 0, 1, 0, 0, 1), LISTS_OK),
              ((0, 2, 0, 0, 1, 0, 0, 1), NEED_LONG)]
    # with ONE line the second is not read
    cases += [((0, 1, 0, 0, 0, 1, 1, 1), LISTS_OK)]
    got = run(["l " + " ".join(str(x) for x in c) for c, _ in cases])
    for (c, want), g in zip(cases, got):
        assert g == (want,), (c, g, want)
