"""Batched evaluation loop and the host double of the batched device beam search, on the CPU.

Loop: berson_evaluate with per_gpu_eval_batch_size = 4 over 10 stories, with a stand-in for the
batched pointer network, must leave the same truth / predicted lists, result files and line order
as the batch-size-1 loop with the matching one-story stand-in: single- and multi-reference golds,
with and without max_eval_steps = 7 (which counts stories and cuts the second batch short).

Double: tests/beam_batch_ref.beam_batch_host restates the kernel's formulation (fixed slots,
pw_k projected once, keys as sums of projected rows, rank selection); on the seeds of the GPU
kernel test it must give oracle.berson_oracle.beam_order's order for every story, and its best
score must equal the teacher-forced score of that order in the reference's formulation.
"""
import argparse

import pytest
import torch

import beam_batch_ref as R
from oracle import berson_oracle as O

from multimodal_sequencing_amd import evaluate as E

N = 5


def _dataset(multiref):
    g = torch.Generator().manual_seed(3)
    items = []
    for b in range(10):
        ids = torch.randint(2, 50, (12,), generator=g)
        lab = torch.randperm(N, generator=g)
        if multiref:
            lab = torch.stack([lab, torch.randperm(N, generator=g)])
        items.append((ids, torch.ones(12, dtype=torch.int64), torch.zeros(1), lab,
                      f"story{b}###{b}", torch.zeros(1)))
    return items


def _order_of(ids):
    """A stand-in prediction that depends on the story alone."""
    return [int(x) for x in torch.argsort(ids[:N], stable=True)]


class _Model:
    def eval(self):
        pass


def _run(tmp_path, monkeypatch, bs, multiref, limit):
    out = tmp_path / f"bs{bs}"
    out.mkdir()
    args = argparse.Namespace(task_names=["sind"], output_dir=str(out), local_rank=-1,
                              per_gpu_eval_batch_size=bs, n_gpu=1, max_eval_steps=limit,
                              multimodal=False, include_num_img_regional_features=False,
                              eval_save_all_results=True, max_story_length=N,
                              multiref_metrics="max", beam_size=16)
    seen, sizes = {}, []
    real = E.cal_result

    def spy(truth, predicted, best_acc, f, args):
        seen["truth"], seen["predicted"] = list(truth), list(predicted)
        return real(truth, predicted, best_acc, f, args=args)

    def one(args, model, tok, inputs):
        assert inputs["input_ids"].shape[0] == 1 and inputs["labels"].shape == (1, N)
        return _order_of(inputs["input_ids"][0])

    def many(args, model, tok, inputs):
        assert inputs["labels"].shape == (inputs["input_ids"].shape[0], N)
        sizes.append(inputs["input_ids"].shape[0])
        return [_order_of(row) for row in inputs["input_ids"]]

    monkeypatch.setattr(E, "cal_result", spy)
    ds = _dataset(multiref)
    res = E.berson_evaluate(args, _Model(), lambda *a, **k: ds, None, pointer_network=one,
                            pointer_network_batch=many)
    files = {n: (out / n).read_text() for n in
             ("output_order.txt", "all_predictions.csv", "eval_results_split_test.txt",
              "all_eval_results.txt")}
    return res, seen, files, sizes


@pytest.mark.parametrize("limit", [0, 7])
@pytest.mark.parametrize("multiref", [False, True])
def test_batched_loop_equals_one_story_loop(tmp_path, monkeypatch, multiref, limit):
    r1, s1, f1, z1 = _run(tmp_path, monkeypatch, 1, multiref, limit)
    r4, s4, f4, z4 = _run(tmp_path, monkeypatch, 4, multiref, limit)
    assert z1 == [] and z4 == ([4, 3] if limit else [4, 4, 2])
    assert len(s1["truth"]) == (limit or 10)
    assert s4["truth"] == s1["truth"] and s4["predicted"] == s1["predicted"]
    assert r4 == r1
    assert f4 == f1
    lines = f4["output_order.txt"].splitlines()
    ds = _dataset(multiref)
    assert [ln.split("|||")[0] for ln in lines] == \
        [" ".join(map(str, _order_of(it[0]))) for it in ds[:len(lines)]]
    assert [ln.split(",")[0] for ln in f4["all_predictions.csv"].splitlines()[1:]] == \
        [f"story{b}" for b in range(len(lines))]


def test_batched_loop_one_sentence_stories(tmp_path, monkeypatch):
    """One-sentence stories are "predicted" as their gold order without a decode. (cal_result's
    tau metric divides by zero on a set of one-sentence stories alone, at any batch size, so the
    loop is checked up to its call.)"""
    ds = [(torch.zeros(4, dtype=torch.int64), torch.ones(4, dtype=torch.int64), torch.zeros(1),
           torch.zeros(1, dtype=torch.int64), f"s{b}###0", torch.zeros(1)) for b in range(3)]
    args = argparse.Namespace(task_names=["sind"], output_dir=str(tmp_path), local_rank=-1,
                              per_gpu_eval_batch_size=2, n_gpu=1, max_eval_steps=0,
                              multimodal=False, eval_save_all_results=False, max_story_length=1,
                              multiref_metrics="max")

    def never(*a, **k):
        raise AssertionError("no decode expected")

    seen = {}

    def stub(truth, predicted, best_acc, f, args):
        seen["truth"], seen["predicted"] = truth, predicted
        f.close()
        return 1.0, 1.0, 1.0

    monkeypatch.setattr(E, "cal_result", stub)
    E.berson_evaluate(args, _Model(), lambda *a, **k: ds, None, pointer_network=never,
                      pointer_network_batch=never)
    assert (tmp_path / "output_order.txt").read_text().splitlines() == ["0|||0"] * 3
    assert seen["truth"] == [[0]] * 3 and seen["predicted"] == [[0]] * 3


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "B%d_N%d_W%d_H%d" % c)
def test_host_double_matches_oracle(case):
    B, N_, W, H = case
    c = R.random_case(B, N_, H, R.SEED)
    orders, bests, finals, _ = R.beam_batch_host(c, W)
    for b in range(B):
        want = O.beam_order(c["p"], R.oracle_enc(c, b), W)
        assert orders[b] == want, (case, b)
        ref = R.order_score(c, b, want)
        assert abs(bests[b] - ref) < R.bound(ref), (case, b, bests[b], ref)
        assert finals[b] == sorted(finals[b])


def test_host_double_tie_rule():
    """tanh_linear.weight = 0: every score ties and the lowest flat index decides."""
    c = R.random_case(3, 5, 128, R.SEED, tie=True)
    orders, _, _, _ = R.beam_batch_host(c, 16)
    assert orders == [O.beam_order(c["p"], R.oracle_enc(c, b), 16) for b in range(3)]
    assert orders == [[0, 1, 2, 3, 4]] * 3
