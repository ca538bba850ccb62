"""Decoding from the pairwise head, host side: the float64 restatement of the subset DP
(tests/pairwise_order_ref.py) against brute force over all N! orders, the tie rule on exactly
summable weights, the legacy topological decode, and the Python surface's argument checks. The
device kernels are compared with the same restatement in tests/test_pairwise_order_gpu.py.
"""
import numpy as np
import pytest
import torch

import beam_batch_ref as R
import order_score_ref as S
import pairwise_order_ref as PW

SEED = 100


def _bits64(x):
    return np.asarray(x, np.float64).view(np.int64)


@pytest.mark.parametrize("N", [1, 2, 3, 5, 7, 9])
def test_restatement_matches_brute_force(N):
    w = PW.random_weights(N, SEED + N)
    got = PW.pairwise_order_ref(w, rounded=False)
    want = PW.brute_force(w)
    assert got["order"].tolist() == want["order"].tolist()
    assert abs(got["pnll"] - want["pnll"]) <= 1e-12
    if N == 1:
        assert got["margin"] == np.inf and want["margin"] == np.inf
    else:
        assert abs(got["margin"] - want["margin"]) <= 1e-12
    for k in ("logz", "entropy"):
        assert abs(got[k] - want[k]) <= 1e-9, (k, got[k], want[k])
    for k in ("position", "before"):
        assert np.abs(got[k] - want[k]).max() <= 1e-9, k
    pos, bef = got["position"], got["before"]
    assert np.abs(pos.sum(0) - 1).max() <= 1e-9 and np.abs(pos.sum(1) - 1).max() <= 1e-9
    off = ~np.eye(N, dtype=bool)
    assert np.abs((bef + bef.T)[off] - 1).max(initial=0.0) <= 1e-9
    assert not bef[~off].any()
    # the scorer's restatement is the brute force's G
    perms = PW.all_perms(N)
    assert np.array_equal(PW.pairwise_score_ref(w, perms), (-want["G"]).astype(np.float32))


@pytest.mark.parametrize("N", [2, 3, 5, 7])
def test_ties_on_dyadic_weights_are_bit_equal_to_brute_force(N):
    tied = 0
    for seed in range(SEED, SEED + 6):
        w = PW.dyadic_weights(N, seed)
        got = PW.pairwise_order_ref(w, rounded=False)
        want = PW.brute_force(w)
        assert got["order"].tolist() == want["order"].tolist(), seed
        assert np.array_equal(_bits64(got["pnll"]), _bits64(want["pnll"])), seed
        assert np.array_equal(_bits64(got["margin"]), _bits64(want["margin"])), seed
        tied += want["margin"] == 0.0
    assert tied or N == 2  # the cases do hold ties: the lowest-index rule is exercised


@pytest.mark.parametrize("N", [1, 2, 5, 8])
def test_all_zero_weights_give_the_identity(N):
    got = PW.pairwise_order_ref(np.zeros((N, N), np.float32))
    assert got["order"].tolist() == list(range(N))
    assert got["pnll"] == 0.0
    if N == 1:
        assert got["margin"] == np.inf and got["logz"] == 0.0
        assert got["position"].tolist() == [[1.0]] and got["before"].tolist() == [[0.0]]
    else:
        assert got["margin"] == 0.0
        assert abs(float(got["logz"]) - float(np.log(float(np.prod(np.arange(1, N + 1)))))) < 1e-5
        assert np.abs(got["position"] - 1.0 / N).max() < 1e-6


def test_invalid_story_in_the_restatement():
    for bad in (np.nan, -np.inf, np.inf):
        w = PW.random_weights(4, SEED)
        w[2, 1] = bad
        got = PW.pairwise_order_ref(w)
        assert got["order"].tolist() == [-1] * 4 and got["pnll"] == np.inf and got["margin"] == 0
        assert got["logz"] == -np.inf and got["entropy"] == 0
        assert not got["position"].any() and not got["before"].any()
        assert np.isposinf(PW.pairwise_score_ref(w, PW.all_perms(4))).all()
    w = PW.random_weights(4, SEED)
    w[3, 3] = np.nan  # the diagonal is never read
    assert PW.pairwise_order_ref(w)["order"].min() >= 0


def test_scorer_restatement_rejects_non_permutations():
    w = PW.random_weights(5, SEED)
    o = np.array([[0, 1, 2, 3, 4], [0, 1, 1, 3, 4], [-1, 1, 2, 3, 4], [0, 1, 2, 3, 5],
                  [1 << 40, 1, 2, 3, 4], [4, 3, 2, 1, 0]], np.int64)
    got = PW.pairwise_score_ref(w, o)
    assert np.isfinite(got).tolist() == [True, False, False, False, False, True]


# ------------------------------------------------------------------------ the legacy decode
def test_topological_order_on_transitive_tournaments():
    """A hidden order with every pair decided its way: each pair term of G is individually maximal
    under that order, so the optimum is forced and the depth-first sort must find it."""
    from multimodal_sequencing_amd import berson
    N = 6
    rng = np.random.RandomState(SEED)
    for _ in range(50):
        hidden = rng.permutation(N)
        rank = np.argsort(hidden)
        mag = rng.uniform(0.1, 2.0, (N, N))
        mag = np.triu(mag, 1) + np.triu(mag, 1).T
        w = np.where(rank[:, None] < rank[None, :], -0.05 * mag, -mag).astype(np.float32)
        np.fill_diagonal(w, 0.0)
        want = PW.pairwise_order_ref(w)["order"].tolist()
        assert want == hidden.tolist()
        assert berson.topological_order_host(w.tolist()) == want
        assert berson.topological_order_host(torch.from_numpy(w)) == want


def test_topological_order_edge_rule_on_equal_weights():
    from multimodal_sequencing_amd import berson
    assert berson.topological_order_host(np.zeros((4, 4)).tolist()) == [0, 1, 2, 3]
    assert berson.topological_order_host([[0.0]]) == [0]
    # a 3-cycle 0 -> 1 -> 2 -> 0: depth-first from 0 finishes 2, 1, 0
    w = [[0, 1, 0], [0, 0, 1], [1, 0, 0]]
    assert berson.topological_order_host(w) == [0, 1, 2]


# ------------------------------------------------------------------------ the Python surface
def test_pairwise_weights():
    from multimodal_sequencing_amd import berson
    assert berson.PAIRWISE_MAX_N == 12
    B, N = 3, 5
    cs = torch.from_numpy(np.random.RandomState(SEED).standard_normal((B, N, N, 2))
                          .astype(np.float32))
    w = berson.pairwise_weights(cs)
    assert w.dtype == torch.float32 and tuple(w.shape) == (B, N, N) and w.is_contiguous()
    for b in range(B):
        want = PW.weights_from_logits(cs[b].numpy())
        assert np.abs(w[b].numpy() - want).max() <= 1e-6
        assert not np.diag(w[b].numpy()).any()
    with pytest.raises(ValueError, match="cs_mat must be"):
        berson.pairwise_weights(cs[..., 0])
    # the pair-list form agrees with the matrix form
    N = 4
    rows = np.random.RandomState(SEED + 1).standard_normal((N * (N - 1), 2))
    mat = np.zeros((N, N, 2))
    for j, (a, c) in enumerate(PW.pair_list(N)):
        mat[a, c] = rows[j]
    assert np.array_equal(PW.weights_from_pairs(rows, N), PW.weights_from_logits(mat))
    from multimodal_sequencing_amd.process_inputs import pairs_generator
    assert [list(p) for p in PW.pair_list(N)] == pairs_generator(N)[0]


def test_surface_argument_checks():
    from multimodal_sequencing_amd import berson
    model = S.StandIn(R.random_case(1, 3, 16, R.SEED)["p"])
    model.pairwise_loss_lam = 0.6
    with pytest.raises(ValueError, match="exceeds 12"):
        berson.pairwise_order_batch(None, model, S.enc(R.random_case(1, 13, 16, R.SEED)))
    with pytest.raises(ValueError, match="method must be 'flat' or 'tree'"):
        berson.joint_order_batch(None, model, S.enc(R.random_case(1, 3, 16, R.SEED)),
                                 method="prefix")
    with pytest.raises(ValueError, match="exceeds 7"):
        berson.joint_order_batch(None, model, S.enc(R.random_case(1, 8, 16, R.SEED)))
    with pytest.raises(ValueError, match="exceeds 9"):
        berson.joint_order_batch(None, model, S.enc(R.random_case(1, 10, 16, R.SEED)),
                                 method="tree")
    with pytest.raises(ValueError, match="no permutation"):
        berson.pairwise_score_orders(None, model, S.enc(R.random_case(1, 3, 16, R.SEED)),
                                     [[0, 1, 1]])


def test_decode_names():
    from multimodal_sequencing_amd import berson
    for name in ("pairwise", "joint"):  # past the name check: the next check speaks
        with pytest.raises(ValueError, match="enumeration must be 'flat' or 'tree'"):
            berson.berson_pointer_network_batch(None, None, None, {}, decode=name,
                                                enumeration="prefix")
    with pytest.raises(ValueError) as e:
        berson.berson_pointer_network_batch(None, None, None, {}, decode="greedy")
    msg = str(e.value)
    assert "'beam', 'exact', 'mbr_acc' or 'mbr_tau'" in msg
    assert "'pairwise'" in msg and "'joint'" in msg


def test_abi_signatures():
    from multimodal_sequencing_amd import _native
    assert len(_native._SIGS["mmseq_pairwise_order_workspace"][1]) == 2
    assert len(_native._SIGS["mmseq_pairwise_order"][1]) == 13
    assert len(_native._SIGS["mmseq_pairwise_score"][1]) == 8
    assert [n for n, _, _ in _native.PAIRWISE_OUTPUTS] == [
        "order", "pnll", "margin", "logz", "position", "before", "entropy"]
    lib = _native.lib()  # loads without a GPU; the workspace query runs on the host
    assert lib.mmseq_pairwise_order_workspace(4, 13) == 0
    assert lib.mmseq_pairwise_order_workspace(4, 0) == 0
    assert lib.mmseq_pairwise_order_workspace(-1, 5) == 0
    for B, N in ((0, 5), (1, 1), (32, 5), (2, 11), (0, 12), (3, 12)):
        n = lib.mmseq_pairwise_order_workspace(B, N)
        assert n > 0 and n % 16 == 0, (B, N, n)
