"""No-GPU: where a group of clouds goes in a slot's arena (quatro_amd/csrc/vmap_group_plan.h: the 256-byte line, the
arena's cursor and which host clouds are staged once — plain functions of pointers and sizes), compiled into a
stand-alone program under ASan + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEAD = (3 * 200, 3 * 64, 0)      # head sections of a call (the last one empty)
A, AN, B_, BN = 0x10000, 0x20000, 0x30000, 0x40000  # addresses of clouds and normals (never read)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vmap_group_plan") / "vmap_group_plan_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "quatro_amd", "csrc"),
                           os.path.join(ROOT, "tests", "vmap_group_plan", "vmap_group_plan_demo.cpp"), "-o", exe])

    def call(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr[-800:]
        out = [[int(x) for x in ln.split()] for ln in p.stdout.strip().splitlines()]
        assert len(out) == len(lines)
        return out
    return call


def plan(run, items, head=HEAD, own=lambda n: (n * 4, 0)):
    """items: (host, src, nrm, n).  Lays the group out and checks what holds for every group: offsets are multiples of 256,
    the sections (a zero-byte one as one line) are pairwise disjoint, and the need is the end of the last one.  Returns
    [(same_as, o_src, o_nrm)] and the number of staged copies."""
    M = len(own(0))
    words = [f"g {len(head)} {len(items)} {M}"] + [str(b) for b in head]
    for host, src, nrm, n in items:
        words += [str(int(host)), str(src), str(nrm), str(n)] + [str(b) for b in own(n)]
    (out,) = run([" ".join(words)])
    need, out = out[0], out[1:]
    sections = list(zip(out[:len(head)], head))
    out, got = out[len(head):], []
    for i, (host, src, nrm, n) in enumerate(items):
        row = out[i * (M + 3):(i + 1) * (M + 3)]
        sections += list(zip(row[:M], own(n)))
        same_as, o_src, o_nrm = row[M:]
        got.append((same_as, o_src, o_nrm))
        if host and n > 0:
            if same_as < 0:
                sections += [(o_src, n * 16), (o_nrm, n * 16)]
            else:  # the first earlier host item with the same pointers and size, and its copy
                first = min(j for j in range(i) if items[j] == items[i])
                assert same_as == first and (o_src, o_nrm) == got[first][1:], (i, row)
        else:
            assert (same_as, o_src, o_nrm) == (-1, -1, -1), (i, row)
    spans = sorted((at, at + max(256, -(-size // 256) * 256)) for at, size in sections)
    assert all(at % 256 == 0 for at, _ in spans), spans
    assert spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:])), spans  # disjoint, and no gap either
    assert need == spans[-1][1], (need, spans[-1])
    copies = sum(1 for (host, _, _, n), g in zip(items, got) if host and n > 0 and g[0] < 0)
    return got, copies


def test_header_has_no_hip():
    txt = open(os.path.join(ROOT, "quatro_amd", "csrc", "vmap_group_plan.h")).read()
    assert "__device__" not in txt and "hip" not in txt.replace("voxelmap_group.hip", "") and "float4" not in txt


def test_round_up_and_empty_section(run):
    got = run([f"u {b}" for b in (0, 1, 255, 256, 257, 4096, (1 << 40) + 1)])
    assert [g[0] for g in got] == [0, 256, 256, 256, 512, 4096, (1 << 40) + 256]
    (out,) = run(["g 3 0 0 0 0 1"])  # three head sections, two of them empty: one line each
    assert out == [768, 0, 256, 512]


def test_smallest_group(run):
    for item in ((True, A, AN, 1), (False, A, AN, 1), (True, A, AN, 0)):
        got, copies = plan(run, [item])
        assert got[0][0] == -1 and copies == (1 if item[0] and item[3] else 0)


def test_device_items_are_never_staged(run):
    got, copies = plan(run, [(False, A, AN, 300), (False, A, AN, 300), (False, B_, BN, 257), (False, A, AN, 0)])
    assert copies == 0 and all(g == (-1, -1, -1) for g in got)


def test_empty_host_item_has_no_copy_and_no_same_as(run):
    got, copies = plan(run, [(True, A, AN, 0), (True, A, AN, 0), (True, A, AN, 5), (True, A, AN, 0)])
    assert copies == 1 and [g[0] for g in got] == [-1, -1, -1, -1] and got[0] == got[1] == got[3] == (-1, -1, -1)


def test_same_host_pointers_and_size_share_the_first_item_s_copy(run):
    got, copies = plan(run, [(True, A, AN, 257)] * 3)
    assert copies == 1 and [g[0] for g in got] == [-1, 0, 0] and got[1][1:] == got[2][1:] == got[0][1:]
    # ... with other items between them, and a second shared cloud
    got, copies = plan(run, [(True, A, AN, 257), (True, B_, BN, 257), (False, A, AN, 257), (True, A, AN, 257), (True, B_, BN, 257)])
    assert copies == 2 and [g[0] for g in got] == [-1, -1, -1, 0, 1]


def test_what_is_not_shared(run):
    for other in ((True, A, AN, 256),      # same pointers, another size
                  (True, A, BN, 257),      # same points, other normals
                  (True, B_, AN, 257),     # other points, same normals
                  (False, A, AN, 257)):    # the same pointers as a device item
        got, copies = plan(run, [(True, A, AN, 257), other])
        assert [g[0] for g in got] == [-1, -1] and copies == (2 if other[0] else 1), other
        got, copies = plan(run, [other, (True, A, AN, 257)])
        assert [g[0] for g in got] == [-1, -1] and copies == (2 if other[0] else 1), other


def test_1024_items_of_one_host_cloud_have_one_staged_copy(run):
    got, copies = plan(run, [(True, A, AN, 300)] * 1024, own=lambda n: (2 * 43 * 8,))
    assert copies == 1 and got[0][0] == -1 and all(g == (0,) + got[0][1:] for g in got[1:])
