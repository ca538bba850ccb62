"""Restatement of mmseq_xent_eval (include/mmseq.h) in numpy, in float64 on the exact bf16 / fp32
values of the logits: the yardstick of tests/test_xent_eval_gpu.py and test_pretrain_eval_gpu.py,
pinned on the CPU by tests/test_xent_eval_ref.py.

Candidate order: (value descending, column ascending), values compared as numbers (-0.0 == +0.0).
  rank[r]  = #{c : x[c] > x[lab]} + #{c < lab : x[c] == x[lab]}; -1 without a usable label
  topk     = the first k columns of that order; (-1, -inf) past V
"""
import numpy as np


def xent_eval_ref(x, V, labels, ignore_index, k):
    """x: [M][>= V] array of the logits' exact values; labels: int [M]. Returns a dict of
    lse f64 [M], loss_row f64 [M] (0 ignored, NaN for another label outside [0, V)), rank int32
    [M], topk_idx int32 [M][k], topk_logit f32 [M][k]."""
    x = np.asarray(x, np.float64)[:, :V]
    labels = np.asarray(labels, np.int64)
    M = x.shape[0]
    mx = x.max(1, keepdims=True)
    lse = (mx + np.log(np.exp(x - mx).sum(1, keepdims=True)))[:, 0]
    loss = np.zeros(M)
    rank = np.full(M, -1, np.int32)
    idx = np.full((M, k), -1, np.int32)
    val = np.full((M, k), -np.inf, np.float32)
    for r in range(M):
        order = np.argsort(-x[r], kind="stable")  # value descending, then column ascending
        n = min(k, V)
        idx[r, :n] = order[:n]
        val[r, :n] = x[r, order[:n]]
        lab = int(labels[r])
        if lab == ignore_index:
            continue
        if not 0 <= lab < V:
            loss[r] = np.nan
            continue
        loss[r] = lse[r] - x[r, lab]
        rank[r] = int((x[r] > x[r, lab]).sum() + (x[r, :lab] == x[r, lab]).sum())
    return {"lse": lse, "loss_row": loss, "rank": rank, "topk_idx": idx, "topk_logit": val}


def brute_force(x, V, labels, ignore_index, k):
    """The definition itself, O(V^2) per row: column c's position is the number of columns that
    come before it. Returns (rank, topk_idx, topk_logit)."""
    x = np.asarray(x, np.float64)[:, :V]
    M = x.shape[0]
    rank = np.full(M, -1, np.int32)
    idx = np.full((M, k), -1, np.int32)
    val = np.full((M, k), -np.inf, np.float32)
    for r in range(M):
        pos = np.zeros(V, np.int64)
        for c in range(V):
            pos[c] = sum(1 for d in range(V)
                         if x[r, d] > x[r, c] or (x[r, d] == x[r, c] and d < c))
        for c in range(V):
            if pos[c] < k:
                idx[r, pos[c]], val[r, pos[c]] = c, x[r, c]
        lab = int(labels[r])
        if lab != ignore_index and 0 <= lab < V:
            rank[r] = pos[lab]
    return rank, idx, val


def check_exact(got, want, labels, ignore_index, V, k):
    """The comparison every test of the kernel uses: rank, topk_idx and topk_logit equal the
    restatement's exactly (integers and exact values, no tolerance), and the two invariants of the
    header hold on `got` alone."""
    rank = np.asarray(got["rank"])
    idx, val = np.asarray(got["topk_idx"]), np.asarray(got["topk_logit"])
    labels = np.asarray(labels, np.int64)
    assert rank.dtype == np.int32 and np.array_equal(rank, want["rank"]), \
        f"rank {rank.tolist()[:8]} != {want['rank'].tolist()[:8]}"
    assert idx.shape == (len(labels), k) and np.array_equal(idx, want["topk_idx"]), "topk_idx"
    assert np.array_equal(val, want["topk_logit"]), "topk_logit"
    usable = (labels != ignore_index) & (labels >= 0) & (labels < V)
    assert np.array_equal(rank >= 0, usable)
    if k:
        assert np.array_equal(rank == 0, usable & (idx[:, 0] == labels))
        among = (idx == labels[:, None]).any(1) & usable
        assert np.array_equal((rank >= 0) & (rank < k), among)
