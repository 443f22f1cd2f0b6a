"""The pose-graph optimisation's named cases (tests/pgo_cases.py) hold themselves, without a GPU: on every case
include/qtr_pgo_math.h compiled by g++ (tests/pgo_host.py) equals the numpy restatement (tests/pgo_restate.py) on every field
pgo_restate.differences checks — poses, weights, the result record, the trace — and on the first solve's residuals, and the
case's `wants` predicate holds on the restatement's record: a case that has left the branch it exists for fails here."""
import os
import re

import numpy as np
import pytest

import pgo_cases as pc
import pgo_host
import pgo_restate as pr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def host():
    return pgo_host.build()


@pytest.mark.parametrize("name", pc.NAMES)
def test_the_header_equals_the_restatement_and_the_case_is_on_its_branch(host, name):
    g, want = pc.case(name), pc.expected(name)
    got = pgo_host.host_run(host, g, **g["params"])
    print(f"{name}: N {g['poses'].shape[0]} E {len(g['src'])} trials {want['iterations']} accepted {want['accepted']} PCG "
          f"{want['pcg_iterations_total']} stop {want['stop_reason']} valid {int(want['valid'])} pruned {want['n_pruned']}")
    assert pr.differences(got, want) == [], (name, pr.differences(got, want))
    assert np.array_equal(pr.bits(got["pcg_rr"]), pr.bits(want["pcg_rr"])), name
    assert pc.WANTS[name](want, g), name


def test_the_case_list_is_the_one_the_suite_claims():
    """Every branch family is present, the mirrored constants are the headers', and the two cut-short cases end where the
    longer runs they are cut from have their rejections."""
    for n in ("rejects", "ends_on_a_reject", "stop_lambda", "stop_step_at_optimum", "stop_relative", "max_iterations_0",
              "max_iterations_1", "max_iterations_ceiling", "non_finite_start", "non_finite_trial", "pcg_cap_1",
              "pcg_converges", "zero_gradient", "precond_refuses", "free_hub", "fixed_hub", "isolated_free_node",
              "fixed_fixed_edge", "several_fixed", "shuffled_edges", "parallel_edges_many", "mu_nonpositive", "all_uncertain",
              "outlier_loops", "outlier_loops_ends_on_a_reject", "only_uncertain_edges_on_a_node", "info_scales",
              "zero_information", "half_turn"):
        assert n in pc.NAMES, n
    for n in (170, 171, 256, 257, 1024, 1025, 2049):
        assert f"nodes_{n}" in pc.NAMES
    for e in (64, 65, 256, 257, 512, 513):
        assert f"edges_{e}" in pc.NAMES
    assert len(set(pc.NAMES)) == len(pc.NAMES) == 42
    hdr = open(os.path.join(ROOT, "include", "quatro_hip.h")).read()
    math = open(os.path.join(ROOT, "include", "qtr_pgo_math.h")).read()
    assert int(re.search(r"#define QTR_PGO_MAX_ITERATIONS (\d+)", hdr).group(1)) == pc.MAX_ITERATIONS
    assert "#define QTR_PGO_THREADS 1024" in math and pr.THREADS == 1024
    assert 6 * 170 < pr.THREADS < 6 * 171  # (the dot product's stride falls between the two node counts)
    assert "#define QTR_PGO_LAMBDA_MAX 1e32" in math and pr.LAMBDA_MAX == 1e32
    # the cut-short runs are prefixes of the long ones: the same trace rows up to the cut, and the long run goes on
    for short, long_, params in (("ends_on_a_reject", "rejects", {}),
                                 ("outlier_loops_ends_on_a_reject", None, dict(max_iterations=60))):
        s = pc.expected(short)
        full = pc.expected(long_) if long_ else pc.restate(dict(pc.case(short), params=dict(pc.case(short)["params"], **params)))
        k = s["iterations"]
        assert np.array_equal(pr.bits(s["trace"]), pr.bits(full["trace"][:1 + k])) and full["iterations"] > k
        assert s["accepted"] == int(full["trace"][1:1 + k, 3].sum()) and full["trace"][k, 3] == 0.0
    # the shuffled ring is a ring with loops: same multiset of undirected edges as the unshuffled graph
    g = pc.case("shuffled_edges")
    plain = pr.ring(20, 6, 16, noise=pc.NOISE)
    und = lambda s, d: sorted((min(a, b), max(a, b)) for a, b in zip(s.tolist(), d.tolist()))
    assert und(g["src"], g["dst"]) == und(plain["src"], plain["dst"])
    assert not np.array_equal(pr.bits(pc.expected("shuffled_edges")["poses"]),
                              pr.bits(pgo_host.restate_run(plain, max_iterations=6)["poses"]))  # (sums are in edge order)
