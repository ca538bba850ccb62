"""mmseq_order_tree without a device: the index rule on its numpy restatement
(tests/order_tree_ref.py), the Python surface's argument checks, and the chunk planner
(csrc/order_tree_plan.h) as a stand-alone host program under the address and undefined-behaviour
sanitizers (tests/order_tree_plan_main.cpp).
"""
import itertools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import beam_batch_ref as R
import order_score_ref as S
import order_tree_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# N: (flat N! (N-1), tree sum_t N!/(N-t)!) node-steps per story
STEP_TABLE = {7: (30240, 3620), 8: (282240, 28961), 9: (2903040, 260650)}


# ------------------------------------------------------------------------------ the index rule
@pytest.mark.parametrize("N", range(1, 9))
def test_unranked_table_is_itertools_order(N):
    want = np.array(list(itertools.permutations(range(N))), np.int64).reshape(-1, N)
    assert np.array_equal(T.unrank_table(N), want)
    ks = range(len(want)) if N <= 6 else range(0, len(want), 97)
    for k in ks:
        assert T.unrank(N, k) == want[k].tolist()
    assert T.unrank(N, len(want) - 1) == list(range(N))[::-1]


def test_node_counts():
    for N, (flat, tree) in STEP_TABLE.items():
        assert T.flat_steps(N) == flat and T.node_steps(N) == tree
        assert T.level_width(N, N - 1) == math.factorial(N)
    assert T.node_steps(1) == 0 and T.node_steps(2) == 1
    assert [round(f / t, 1) for f, t in STEP_TABLE.values()] == [8.4, 9.7, 11.1]


@pytest.mark.parametrize("rule", ["descending", "all_steps"])
def test_wrong_rank_rules_are_rejected(rule):
    for N in (3, 4, 5):
        want = np.array(list(itertools.permutations(range(N))), np.int64)
        assert not np.array_equal(T.unrank_table(N, rule), want), (rule, N)


# ------------------------------------------------------------------- the surface's argument checks
def _enc(N, B=1, H=16):
    return S.enc(R.random_case(B, N, H, R.SEED))


def test_surface_argument_checks():
    from multimodal_sequencing_amd import berson
    assert berson.TREE_MAX_N == 9 and berson.EXACT_MAX_N == 7
    model = S.StandIn(R.random_case(1, 3, 16, R.SEED)["p"])
    with pytest.raises(ValueError, match="method must be 'flat' or 'tree'"):
        berson.exact_order_batch(None, model, _enc(3), method="prefix")
    with pytest.raises(ValueError, match="exceeds 9"):
        berson.exact_order_batch(None, model, _enc(10), method="tree")
    with pytest.raises(ValueError, match="exceeds 9"):
        berson.enumerate_orders_batch(None, model, _enc(10))
    with pytest.raises(ValueError, match="exceeds 9"):
        berson.order_posterior_batch(None, model, _enc(10), source="tree")
    # the defaults are what they were
    with pytest.raises(ValueError, match="exceeds 7"):
        berson.exact_order_batch(None, model, _enc(8))
    with pytest.raises(ValueError, match="exceeds 7"):
        berson.exact_order_batch(None, model, _enc(8), method="flat")
    with pytest.raises(ValueError, match="exceeds 7"):
        berson.order_posterior_batch(None, model, _enc(8), source="exact")
    with pytest.raises(ValueError, match="source must be"):
        berson.order_posterior_batch(None, model, _enc(3), source="greedy")


def test_enumeration_argument_checks():
    import argparse
    from multimodal_sequencing_amd import berson
    with pytest.raises(ValueError, match="enumeration must be 'flat' or 'tree'"):
        berson.berson_pointer_network_batch(None, None, None, {}, decode="exact",
                                            enumeration="prefix")
    with pytest.raises(ValueError, match="enumeration must be 'flat' or 'tree'"):
        berson.berson_pointer_network_batch(argparse.Namespace(order_enumeration="trie"), None,
                                            None, {}, decode="mbr_tau")
    with pytest.raises(ValueError, match="'beam', 'exact', 'mbr_acc' or 'mbr_tau'"):
        berson.berson_pointer_network_batch(None, None, None, {}, decode="greedy",
                                            enumeration="tree")


# ----------------------------------------------------------------- the planner under sanitizers
def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


@pytest.fixture(scope="module")
def plan_main(tmp_path_factory):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("order_tree_plan") / "order_tree_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "multimodal_sequencing_amd", "csrc"),
                    os.path.join(ROOT, "tests", "order_tree_plan_main.cpp"), "-o", exe],
                   check=True)
    return exe


def _rows_values(B, N):
    widest = B * math.factorial(N) // 2 if N > 1 else B
    # the minimum, two primes (chunks that align with no level width), one row short of the
    # widest level, and a value larger than the widest level
    vals = {B * N, max(B * N, 4099), max(B * N, 127), max(B * N, widest - 1), widest + 1000}
    return sorted(vals)


@pytest.mark.parametrize("B", [1, 3, 32])
def test_planner_covers_every_node_once(plan_main, B):
    args, want = [], []
    for N in range(1, 10):
        for rows in _rows_values(B, N):
            for H in (16, 1022):
                args += [str(N), str(B), str(H), str(rows)]
                want.append((N, B, H, rows))
    res = subprocess.run([plan_main] + args, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = [ln.split() for ln in res.stdout.splitlines()]
    assert len(lines) == len(want)
    for ln, (N, B_, H, rows) in zip(lines, want):
        assert ln[0] == "ok" and [int(v) for v in ln[1:5]] == [N, B_, H, rows]
        chunks, steps, nbytes = int(ln[5]), int(ln[6]), int(ln[7])
        assert steps == T.node_steps(N) and nbytes % 16 == 0
        widest = B * math.factorial(N) // 2
        if rows > widest and widest * 4 * H < 2 ** 31 - 1:  # unchunked: one chunk per level
            assert chunks == max(N - 1, 0)
        else:
            assert chunks >= max(N - 1, 0)
