"""Scoring candidate orders on the host (berson.score_orders_host, check_orders,
exact_from_scores), no GPU: the torch teacher-forced scorer runs on a CPU stand-in for the model
(tests/order_score_ref.StandIn, the oracle's primitives behind `step`) and is compared with
beam_batch_ref.order_score, the reference's formulation step by step. Bound: R.bound.
"""
import pytest
import torch

import beam_batch_ref as R
import order_score_ref as S
from multimodal_sequencing_amd import berson


def test_host_scorer_matches_reference_all_orders_n3():
    B, N, H = 2, 3, 128
    case, perms, want = S.ref_nll(B, N, H)
    assert len(perms) == 6
    nll, steps = berson.score_orders_host(None, S.StandIn(case["p"]), S.enc(case), perms,
                                          return_steps=True)
    assert nll.shape == (B, 6) and steps.shape == (B, 6, N - 1)
    for b in range(B):
        for k in range(6):
            got, ref = float(nll[b, k]), float(want[b, k])
            print(f"story {b} {perms[k]}: {got:.6f} reference {ref:.6f} diff {abs(got - ref):.2e}")
            assert abs(got - ref) < R.bound(ref), (b, perms[k], got, ref)
    assert torch.allclose(steps.sum(-1), nll, rtol=1e-6, atol=0)
    # per-story lists [B][K][N]: story 1 gets the list reversed
    per = torch.tensor([perms, perms[::-1]])
    nll2 = berson.score_orders_host(None, S.StandIn(case["p"]), S.enc(case), per)
    assert torch.equal(nll2[0], nll[0]) and torch.equal(nll2[1], nll[1].flip(0))
    # chunked along K: same numbers
    nll3 = berson.score_orders_host(None, S.StandIn(case["p"]), S.enc(case), perms, chunk=4)
    assert torch.allclose(nll3, nll, rtol=1e-6, atol=0)


def test_host_scorer_single_sentence_and_single_step():
    c1 = R.random_case(2, 1, 128, R.SEED)
    nll, steps = berson.score_orders_host(None, S.StandIn(c1["p"]), S.enc(c1), [[0]], True)
    assert nll.tolist() == [[0.0], [0.0]] and steps.shape == (2, 1, 0)
    case, perms, want = S.ref_nll(2, 2, 128)
    nll = berson.score_orders_host(None, S.StandIn(case["p"]), S.enc(case), perms)
    for b in range(2):
        for k in range(2):
            assert abs(float(nll[b, k]) - float(want[b, k])) < R.bound(float(want[b, k]))


@pytest.mark.parametrize("orders, word", [
    ([[0, 1, 2], [0, 0, 2]], "candidate 1"),               # a repeat
    ([[0, 1, 3]], "candidate 0"),                          # out of range
    ([[0, 1, 2], [2, 1, 0], [-1, 1, 2]], "candidate 2"),   # negative
    ([[0, 1]], "[K][3]"),                                  # wrong width
    ([[0, 1, 2], [0, 1]], "N = 3"),                        # ragged
    ([[[0, 1, 2]], [[0, 1, 2]], [[0, 1, 2]]], "B = 2"),    # wrong story count
    ([[[0, 1, 2]], [[1, 1, 2]]], "candidate 0 of story 1"),
    ([0, 1, 2], "[K][3]"),                                 # no candidate axis
])
def test_host_validation_names_the_candidate(orders, word):
    with pytest.raises(ValueError) as e:
        berson.check_orders(orders, 2, 3)
    assert word in str(e.value), str(e.value)


def test_host_validation_accepts_lists_and_tensors():
    o = berson.check_orders([[2, 0, 1], [0, 1, 2]], 2, 3)
    assert o.dtype == torch.int64 and o.tolist() == [[2, 0, 1], [0, 1, 2]]
    o = berson.check_orders(torch.tensor([[[2, 0, 1]], [[0, 1, 2]]], dtype=torch.int32), 2, 3)
    assert o.dtype == torch.int64 and tuple(o.shape) == (2, 1, 3)
    with pytest.raises(ValueError):
        berson.check_orders(torch.tensor([[0.0, 1.0, 2.0]]), 2, 3)


def test_exact_tie_rule_lowest_candidate_index():
    inf = float("inf")
    nll = torch.tensor([[3.0, 1.0, 2.0, 1.0, 5.0],    # tie between 1 and 3 -> 1, margin 0
                        [0.5, 0.5, 0.5, 0.5, 0.5],    # all equal -> 0
                        [9.0, 8.0, 7.0, 6.0, 5.5],    # strictly descending -> 4, margin 0.5
                        [2.0, inf, 2.0, inf, 1.0],    # inf (invalid) candidates never win
                        [-0.0, 0.0, 1.0, 1.0, 1.0]])  # -0 == +0: a tie, index 0
    idx, best, margin = berson.exact_from_scores(nll)
    assert idx.tolist() == [1, 0, 4, 4, 0]
    assert best.tolist() == [1.0, 0.5, 5.5, 1.0, 0.0]
    assert margin.tolist() == [0.0, 0.0, 0.5, 1.0, 0.0]
    idx, best, margin = berson.exact_from_scores(torch.tensor([[4.0]]))
    assert idx.tolist() == [0] and best.tolist() == [4.0] and margin.tolist() == [inf]


def test_exact_refuses_large_n():
    c = R.random_case(1, 8, 16, R.SEED)
    with pytest.raises(ValueError):
        berson.exact_order_batch(None, S.StandIn(c["p"]), S.enc(c))
