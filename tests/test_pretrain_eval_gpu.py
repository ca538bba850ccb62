"""Pretraining evaluation (pretraining.LXRTPretraining.evaluate_batch, fill_mask and
pretrain_evaluate, the restatement of trainers/run_pretraining.py:377-511) on the tiny reference
fixtures pretrain_mm_tiny_{isp,pisp,mrm} and pretrain_tiny.

  evaluate_batch   loss / losses / answer bit-equal to model(batch) under no_grad in eval mode (so
                   fp32 inherits the fixtures' 1e-4 parity with the reference); the masked-LM
                   statistics equal tests/xent_eval_ref.py applied to the logit buffer the kernel
                   was given; the objective accuracy is the arg-max of the head's recorded scores
  pretrain_evaluate  replayed step by step with the same seed, streams and draws
"""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from counter_init import counter_state_dict
from test_pretrain_mm import KINDS, build_mm, load_mm
from xent_eval_ref import check_exact, xent_eval_ref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multimodal_sequencing_amd import _native as N
    from multimodal_sequencing_amd import pretraining as P

DEV = "cuda"
PAD, CLS, IGNORE = 1, 0, -100
TASK = "wikihow"
_DRAW_KEYS = {"isp": ["swap"], "pisp": ["swap", "count", "patch_src"], "mrm": ["mask_idx", "shuffle"]}


class _Tokenizer:
    """What mask_tokens_sentence and fill_mask read of a tokenizer."""
    pad_token, mask_token = "<pad>", "<mask>"

    def __init__(self, vocab):
        self.ids = {"<pad>": PAD, "<mask>": vocab - 1}
        self.vocab = vocab

    def convert_tokens_to_ids(self, token):
        return self.ids[token]

    def convert_ids_to_tokens(self, ids):
        return [f"w{int(i)}" for i in ids]

    def __len__(self):
        return self.vocab


def _weights(meta):
    params = counter_state_dict({k: tuple(v) for k, v in meta["shapes"].items()})
    params["cls.predictions.decoder.weight"] = params["bert.embeddings.word_embeddings.weight"]
    return {k: torch.from_numpy(v) for k, v in params.items()}


_MODELS = {}


def _model(kind, dtype):
    """The fixture's model with its counter-initialised weights, in eval mode (built once)."""
    if (kind, dtype) not in _MODELS:
        meta, _ = load_mm(kind)
        m = build_mm(meta, DEV, dtype)
        m.load_state_dict(_weights(meta))
        _MODELS[kind, dtype] = m
    m = _MODELS[kind, dtype]
    m.eval()
    return m


def _batch(kind, d, device=None):
    b = {k: torch.from_numpy(d[k]) for k in ("input_ids", "attention_mask", "token_type_ids",
                                             "masked_lm_labels")}
    if device is not None:
        b = {k: v.to(device) for k, v in b.items()}
    b["images"] = torch.from_numpy(d["images"])
    b["draws"] = {k: d[k] for k in ["objective", "sub_idx"] + _DRAW_KEYS[kind]}
    return b


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and \
        torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


# ---- evaluate_batch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_evaluate_batch_has_the_forwards_bits(kind, dtype):
    meta, d = load_mm(kind)
    m = _model(kind, dtype)
    for device in (None, DEV):
        with torch.no_grad():
            loss, losses, answer = m(_batch(kind, d, device))
        eloss, elosses, eanswer, stats = m.evaluate_batch(_batch(kind, d, device))
        assert _bits_equal(loss, eloss) and _bits_equal(losses, elosses)
        assert _bits_equal(answer, eanswer)
        assert not eloss.requires_grad and stats["objective"] == KINDS[kind]
        assert _bits_equal(stats["mlm"]["mean_loss"], elosses[0, 1])
        if dtype == torch.float32:
            assert abs(eloss.item() - float(d["loss"])) < 1e-4


def test_evaluate_batch_needs_eval_mode():
    _, d = load_mm("isp")
    m = _model("isp", torch.float32)
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.evaluate_batch(_batch("isp", d, DEV))
    m.eval()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_mlm_statistics_are_the_restatements(kind, dtype, monkeypatch):
    meta, d = load_mm(kind)
    m = _model(kind, dtype)
    seen = []
    real = N.xent_eval

    def spy(logits, V, labels, *rest):
        seen.append((logits.clone(), V, labels.clone()))
        real(logits, V, labels, *rest)

    monkeypatch.setattr(N, "xent_eval", spy)
    k = 5
    totals = torch.zeros(4, dtype=torch.float64, device=DEV)
    _, losses, _, stats = m.evaluate_batch(_batch(kind, d, DEV), topk=k, totals=totals)
    mlm = stats["mlm"]
    (logits, V, labels), = seen
    assert V == meta["config"]["joint"]["vocab"] and logits.shape[1] == (V + 63) // 64 * 64
    # rows / labels: torch.nonzero order over the sub-sampled labels
    sub_lab = P.subsample_text(d["input_ids"], d["attention_mask"], None, d["masked_lm_labels"],
                               d["sub_idx"], meta["config"]["N"], CLS, PAD, IGNORE)[3]
    flat = sub_lab.reshape(-1)
    rows = torch.nonzero(flat != IGNORE).view(-1)
    assert rows.numel() > 0 and stats["seq_len"] == sub_lab.shape[1]
    assert torch.equal(mlm["rows"].cpu().long(), rows) and torch.equal(mlm["labels"].cpu(), flat[rows])
    assert torch.equal(labels.cpu(), flat[rows])
    want = xent_eval_ref(logits.float().double().cpu().numpy(), V, flat[rows].numpy(), IGNORE, k)
    got = {n: mlm[n].cpu().numpy() for n in ("rank", "topk_idx", "topk_logit")}
    check_exact(got, want, flat[rows].numpy(), IGNORE, V, k)
    np.testing.assert_allclose(mlm["lse"].cpu().numpy(), want["lse"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(mlm["loss_row"].cpu().numpy(), want["loss_row"], rtol=1e-4, atol=1e-4)
    assert abs(float(mlm["mean_loss"]) - want["loss_row"].mean()) < 1e-4
    t = totals.tolist()
    assert t[1] == rows.numel() and t[2] == int((want["rank"] == 0).sum())
    assert t[3] == int((want["rank"] < k).sum())
    assert abs(t[0] - math.fsum(mlm["loss_row"].cpu().tolist())) <= 1e-12 * abs(t[0])


@pytest.mark.parametrize("kind", list(KINDS))
def test_objective_accuracy_is_the_argmax_of_the_recorded_scores(kind):
    _, d = load_mm(kind)
    m = _model(kind, torch.float32)
    _, _, _, stats = m.evaluate_batch(_batch(kind, d, DEV))
    scores, labels = m.last_objective_logits.cpu(), m.last_objective_labels.cpu()
    assert int(stats["objective_correct"]) == int((scores.argmax(-1) == labels).sum())
    assert int(stats["objective_count"]) == labels.numel()
    assert stats["objective_correct"].is_cuda and stats["objective_count"].is_cuda
    assert torch.equal(stats["objective_logits"].cpu(), scores)
    assert torch.equal(stats["objective_labels"].cpu(), labels)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_fill_mask(dtype):
    meta, d = load_mm("pisp")
    m = _model("pisp", dtype)
    k = 5
    tok = _Tokenizer(meta["config"]["joint"]["vocab"])
    out = P.fill_mask(m, _batch("pisp", d, DEV), k=k, tokenizer=tok)
    n = out["gold"].numel()
    probs = out["probs"]
    assert probs.shape == (n, k) and n > 0
    assert bool((probs.double().sum(1) <= 1.0).all())
    assert bool((probs[:, :-1] >= probs[:, 1:]).all())
    first = out["rank"] == 0
    assert torch.equal(probs[first, 0], torch.exp(-out["loss_row"][first]))
    assert torch.equal(out["ids"][first, 0], out["gold"][first])
    # (story, position) address the sub-sampled text
    sub_lab = P.subsample_text(d["input_ids"], d["attention_mask"], None, d["masked_lm_labels"],
                               d["sub_idx"], meta["config"]["N"], CLS, PAD, IGNORE)[3]
    assert torch.equal(sub_lab[out["story"].cpu(), out["position"].cpu()], out["gold"].cpu())
    assert out["tokens"][0] == [f"w{i}" for i in out["ids"][0].tolist()]
    assert len(out["gold_tokens"]) == n


def test_mlm_eval_without_labels_covers_every_row():
    """labels=None: fill-mask over whole sequences; rank -1 and loss 0 throughout, and the k best
    words of a row are those the labelled evaluation of the same row reports."""
    from multimodal_sequencing_amd import kernels as K
    meta, _ = load_mm("isp")
    m = _model("isp", torch.bfloat16)
    H, V = meta["config"]["joint"]["hidden"], meta["config"]["joint"]["vocab"]
    gen = torch.Generator().manual_seed(1)
    lang = torch.randn(2, 6, H, generator=gen).to(DEV, torch.bfloat16)
    free = K.mlm_eval(lang, None, IGNORE, m.store, m.bert.store, 3)
    assert free["rows"].tolist() == list(range(12)) and free["topk_idx"].shape == (12, 3)
    assert bool((free["rank"] == -1).all()) and not bool(free["loss_row"].any())
    labels = torch.randint(0, V, (2, 6), generator=gen)
    told = K.mlm_eval(lang, labels, IGNORE, m.store, m.bert.store, 3)
    assert torch.equal(told["topk_idx"], free["topk_idx"])
    assert _bits_equal(told["topk_logit"], free["topk_logit"]) and _bits_equal(told["lse"], free["lse"])
    assert bool((told["rank"] >= 0).all())


# ---- pretrain_evaluate ----------------------------------------------------------------------------
def _dataset(d, n=5):
    """n map-style items (input_ids, attention_mask, token_type_ids, labels, images) cycling over
    the fixture's stories, the images of every repeat rolled so that no two items are equal."""
    B = d["input_ids"].shape[0]
    items = []
    for i in range(n):
        b = i % B
        items.append((torch.from_numpy(d["input_ids"][b]), torch.from_numpy(d["attention_mask"][b]),
                      torch.from_numpy(d["token_type_ids"][b]), torch.zeros(1, dtype=torch.int64),
                      torch.from_numpy(np.roll(d["images"][b], i // B, axis=0))))
    return items


def _args(tmp_path, **kw):
    a = dict(task_names=[TASK], output_dir=str(tmp_path), per_gpu_eval_batch_size=2, n_gpu=1,
             max_eval_steps=0, local_rank=-1, mlm_probability=0.3, cls_id=CLS,
             mlm_ignore_index=IGNORE)
    a.update(kw)
    return SimpleNamespace(**a)


_ALL = {}


def _all_objectives_model():
    """All three objectives in one model (seeded initial weights), so the draws pick among them."""
    if not _ALL:
        meta, d = load_mm("isp")
        _ALL["m"] = build_mm(meta, DEV, torch.float32, objectives=list(P.MM_OBJECTIVES))
        _ALL["meta"], _ALL["d"] = meta, d
    _ALL["m"].eval()
    return _ALL["m"], _ALL["meta"], _ALL["d"]


def _replay(m, items, tok, args, seed, topk, limit=0):
    """pretrain_evaluate's definition, step by step through evaluate_batch."""
    rng = np.random.RandomState(seed)
    losses, nll, tokens, first, ink = [], [], 0, 0, 0
    per = {}
    bs = args.per_gpu_eval_batch_size
    for step, at in enumerate(range(0, len(items), bs)):
        chunk = items[at:at + bs]
        ids = torch.stack([c[0] for c in chunk]).to(DEV)
        images = torch.stack([c[-1] for c in chunk])
        ids, labels = P.mask_tokens_sentence(ids, tok, args, seed=seed, stream_id=2 + step)
        g = images.shape[-1] // m.bert.vision["patch"]
        batch = {"input_ids": ids, "masked_lm_labels": labels, "images": images,
                 "attention_mask": torch.stack([c[1] for c in chunk]).to(DEV),
                 "draws": m.draw_mm(len(chunk), images.shape[1], 1 + 2 * g * g, rng=rng)}
        loss, _, _, stats = m.evaluate_batch(batch, topk=topk)
        losses.append(float(loss.double()))
        rank = stats["mlm"]["rank"].cpu()
        nll += stats["mlm"]["loss_row"].cpu().tolist()
        tokens += rank.numel()
        first += int((rank == 0).sum())
        ink += int(((rank >= 0) & (rank < topk)).sum())
        p = per.setdefault(stats["objective"], [0, 0, 0.0, 0])
        p[0] += int(stats["objective_correct"])
        p[1] += int(stats["objective_count"])
        p[2] += float(stats["objective_loss"].double())
        p[3] += 1
        if limit and step + 1 >= limit:
            break
    return losses, nll, tokens, first, ink, per


def test_pretrain_evaluate_is_its_replay(tmp_path):
    m, meta, d = _all_objectives_model()
    tok = _Tokenizer(meta["config"]["joint"]["vocab"])
    items = _dataset(d)
    args = _args(tmp_path)
    seed, topk = 3, 5
    state, calls = m.rng.get_state(), P._MASK_CALLS[0]
    res = P.pretrain_evaluate(args, m, lambda a, tasks, t, evaluate: items, tok, seed=seed, topk=topk)
    assert args.eval_batch_size == 2
    losses, nll, tokens, first, ink, per = _replay(m, items, tok, args, seed, topk)
    assert len(losses) == 3  # 5 items in batches of 2: the last batch holds one story
    assert abs(res[f"{TASK}_loss"] - sum(losses) / 3) <= 1e-12 * abs(sum(losses) / 3)
    assert res[f"{TASK}_mlm_tokens"] == tokens and tokens > 0
    want = math.exp(math.fsum(nll) / tokens)
    assert res[f"{TASK}_perplexity"] > 0
    assert abs(res[f"{TASK}_perplexity"] - want) <= 1e-6 * want
    assert abs(res[f"{TASK}_mlm_loss"] - math.fsum(nll) / tokens) <= 1e-9
    assert res[f"{TASK}_mlm_acc"] == first / tokens
    assert res[f"{TASK}_mlm_acc_top{topk}"] == ink / tokens
    for name in P.MM_OBJECTIVES:
        if name in per:
            c, n, ls, nb = per[name]
            assert res[f"{TASK}_{name}_batches"] == nb
            assert res[f"{TASK}_{name}_acc"] == c / n
            assert abs(res[f"{TASK}_{name}_loss"] - ls / nb) <= 1e-12 * abs(ls / nb)
        else:
            assert f"{TASK}_{name}_batches" not in res
    assert sum(p[3] for p in per.values()) == 3
    # the model's own stream and the process-wide mask counter are untouched
    after = m.rng.get_state()
    assert after[0] == state[0] and np.array_equal(after[1], state[1]) and after[2:] == state[2:]
    assert P._MASK_CALLS[0] == calls
    # the file: sorted "key = value" lines
    lines = open(os.path.join(str(tmp_path), "eval_results.txt")).read().splitlines()
    assert lines == ["%s = %s" % (key, str(res[key])) for key in sorted(res)]


def test_pretrain_evaluate_is_a_function_of_the_seed_and_stops_at_max_eval_steps(tmp_path):
    m, meta, d = _all_objectives_model()
    tok = _Tokenizer(meta["config"]["joint"]["vocab"])
    items = _dataset(d)
    load = lambda a, tasks, t, evaluate: items  # noqa: E731
    a = P.pretrain_evaluate(_args(tmp_path), m, load, tok, prefix="a", seed=3)
    b = P.pretrain_evaluate(_args(tmp_path), m, load, tok, prefix="b", seed=3)
    c = P.pretrain_evaluate(_args(tmp_path), m, load, tok, prefix="c", seed=4)
    assert a == b
    assert os.path.exists(os.path.join(str(tmp_path), "a", "eval_results.txt"))
    # another seed masks other tokens
    masks = []
    for seed in (3, 4):
        ids = torch.stack([it[0] for it in items[:2]]).to(DEV)
        masks.append(P.mask_tokens_sentence(ids, tok, _args(tmp_path), seed=seed, stream_id=2)[1])
    assert not torch.equal(masks[0], masks[1])
    assert (a[f"{TASK}_mlm_tokens"], a[f"{TASK}_loss"]) != (c[f"{TASK}_mlm_tokens"], c[f"{TASK}_loss"])
    # two steps only
    args = _args(tmp_path, max_eval_steps=2)
    two = P.pretrain_evaluate(args, m, load, tok, prefix="two", seed=3)
    losses, nll, tokens, _, _, per = _replay(m, items, tok, args, 3, 5, limit=2)
    assert len(losses) == 2 and two[f"{TASK}_mlm_tokens"] == tokens
    assert abs(two[f"{TASK}_loss"] - sum(losses) / 2) <= 1e-12 * abs(sum(losses) / 2)
    assert sum(two[f"{TASK}_{n}_batches"] for n in per) == 2


def test_pretrain_evaluate_image_only_stage(tmp_path):
    from test_pretrain import _build, _load
    meta, d = _load()
    m = _build(meta, DEV, torch.float32)
    B = d["input_ids"].shape[0]
    items = [(torch.from_numpy(d["input_ids"][i % B]), torch.zeros(1), torch.zeros(1), torch.zeros(1),
              torch.from_numpy(d["images"][i % B])) for i in range(3)]
    args = _args(tmp_path)
    state = m.rng.get_state()
    res = P.pretrain_evaluate(args, m, lambda a, tasks, t, evaluate: items, None, seed=5)
    assert np.array_equal(m.rng.get_state()[1], state[1])
    rng = np.random.RandomState(5)
    losses, correct, count = [], 0, 0
    for at in (0, 2):
        images = torch.stack([it[-1] for it in items[at:at + 2]])
        g = images.shape[-1] // m.bert.vision["patch"]
        draws = m.draw(images.shape[0], images.shape[1], 1 + 2 * g * g, rng=rng)
        with torch.no_grad():
            want = m({"images": images, "draws": draws})
        loss, lss, answer, stats = m.evaluate_batch({"images": images, "draws": draws})
        assert _bits_equal(loss, want[0]) and _bits_equal(lss, want[1]) and _bits_equal(answer, want[2])
        assert "mlm" not in stats and stats["objective"] == P.MRM
        losses.append(float(loss.double()))
        correct += int(stats["objective_correct"])
        count += int(stats["objective_count"])
    assert count == 3 * 10
    assert abs(res[f"{TASK}_loss"] - sum(losses) / 2) <= 1e-12 * abs(sum(losses) / 2)
    assert res[f"{TASK}_perplexity"] == 0.0
    assert res[f"{TASK}_{P.MRM}_acc"] == correct / count and res[f"{TASK}_{P.MRM}_batches"] == 2
    assert f"{TASK}_mlm_tokens" not in res
