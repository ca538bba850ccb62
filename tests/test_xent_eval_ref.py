"""Pins the yardstick of the evaluation kernel's tests (tests/xent_eval_ref.py) on the CPU, before
any GPU run: the restatement agrees with the O(V^2) definition, the header's invariants hold on
tie-heavy rows, and the comparison the GPU test uses (check_exact) rejects a flipped tie rule and
an off-by-one rank."""
import numpy as np
import pytest

from xent_eval_ref import brute_force, check_exact, xent_eval_ref

IGNORE = -100


def _ties(M, V, seed, levels=(-1.5, -0.0, 0.0, 0.75, 2.0)):
    rng = np.random.RandomState(seed)
    return rng.choice(np.asarray(levels, np.float64), size=(M, V))


def _labels(M, V, seed):
    rng = np.random.RandomState(seed + 1)
    lab = rng.randint(0, V, M).astype(np.int64)
    lab[0] = 0
    if M > 1:
        lab[1] = V - 1
    if M > 2:
        lab[2] = IGNORE
    if M > 3:
        lab[3] = V  # not ignore_index: NaN loss, rank -1
    return lab


@pytest.mark.parametrize("V,k", [(1, 1), (2, 5), (7, 0), (9, 8), (40, 5)])
def test_restatement_is_the_definition(V, k):
    for seed, make in ((0, _ties), (1, lambda M, V, s: np.random.RandomState(s).randn(M, V))):
        x = make(6, V, seed)
        lab = _labels(6, V, seed)
        want = xent_eval_ref(x, V, lab, IGNORE, k)
        rank, idx, val = brute_force(x, V, lab, IGNORE, k)
        assert np.array_equal(want["rank"], rank)
        assert np.array_equal(want["topk_idx"], idx)
        assert np.array_equal(want["topk_logit"], val)
        check_exact(want, want, lab, IGNORE, V, k)


def test_padding_columns_are_not_data():
    x = _ties(4, 16, 3)
    lab = _labels(4, 11, 3)
    a = xent_eval_ref(x, 11, lab, IGNORE, 5)
    x[:, 11:] = np.inf
    b = xent_eval_ref(x, 11, lab, IGNORE, 5)
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), key


def test_loss_and_lse_values():
    x = np.log(np.asarray([[0.5, 0.25, 0.125, 0.125]]))
    out = xent_eval_ref(x, 4, [1], IGNORE, 2)
    assert abs(out["lse"][0]) < 1e-12 and abs(out["loss_row"][0] - np.log(4.0)) < 1e-12
    assert out["rank"][0] == 1 and out["topk_idx"][0].tolist() == [0, 1]
    out = xent_eval_ref(x, 4, [IGNORE], IGNORE, 2)
    assert out["loss_row"][0] == 0 and out["rank"][0] == -1 and out["topk_idx"][0].tolist() == [0, 1]
    assert np.isnan(xent_eval_ref(x, 4, [-5], IGNORE, 2)["loss_row"][0])


def _flipped(x, V, labels, k):
    """The wrong tie rule: (value descending, column DESCENDING)."""
    out = xent_eval_ref(x[:, :V][:, ::-1], V, [V - 1 - l if 0 <= l < V else l for l in labels],
                        IGNORE, k)
    out["topk_idx"] = np.where(out["topk_idx"] >= 0, V - 1 - out["topk_idx"], -1).astype(np.int32)
    return out


def test_comparison_rejects_a_flipped_tie_rule_and_an_off_by_one_rank():
    V, k = 64, 5
    x, lab = _ties(8, V, 7), _labels(8, V, 7)
    want = xent_eval_ref(x, V, lab, IGNORE, k)
    check_exact(want, want, lab, IGNORE, V, k)
    with pytest.raises(AssertionError):
        check_exact(_flipped(x, V, lab, k), want, lab, IGNORE, V, k)
    off = dict(want)
    off["rank"] = np.where(want["rank"] >= 0, want["rank"] + 1, -1).astype(np.int32)
    with pytest.raises(AssertionError):
        check_exact(off, want, lab, IGNORE, V, k)
    # without ties both orders agree, so the rejection above is the tie rule's
    y = np.random.RandomState(9).permutation(8 * V).reshape(8, V).astype(np.float64)
    check_exact(_flipped(y, V, lab, k), xent_eval_ref(y, V, lab, IGNORE, k), lab, IGNORE, V, k)
