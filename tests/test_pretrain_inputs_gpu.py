"""Pretraining inputs on the device (csrc/inputs.hip): mmseq_mlm_mask against its numpy
restatement bit for bit, mmseq_subsample_text against the reference's recorded sub-sampling and
against the host function on ragged batches, mmseq_rows_compact against torch.nonzero's order, the
model with a device batch against the same batch on the host (bitwise), and dynamic masking end to
end. Kernel buffers sit in guard bands (tests/guard_util.py): nothing outside the declared extents
may change.
"""
import glob
import itertools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from golden_util import GOLDEN
from guard_util import Guarded
from mlm_mask_ref import mlm_mask_ref
from multimodal_sequencing_amd import _native as N
from multimodal_sequencing_amd import kernels as K
from multimodal_sequencing_amd import pretraining as P
from test_pretrain_mm import KINDS, build_mm, load_mm

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD, CLS, SEP, IGNORE = 1, 0, 2, -100


def _guarded(data, dtype=torch.int64):
    """A [rows][cols] tensor (1-D data: [n][1]) inside guard bands holding `data`, the rest a fixed
    bit pattern."""
    data = torch.as_tensor(data)
    data = data.view(-1, 1) if data.dim() == 1 else data
    g = Guarded(data.shape[0], data.shape[1], dtype=dtype, device=DEV).fill_pattern()
    g.set(data.to(DEV, dtype))
    return g.snapshot()


def _blank(rows, cols, dtype=torch.int64):
    return Guarded(rows, cols, dtype=dtype, device=DEV).fill_pattern().snapshot()


# ---- 1. masking: kernel == restatement -----------------------------------------------------------
def _mask_ids(B, L, vocab, seed):
    rs = np.random.RandomState(seed)
    ids = rs.randint(2, vocab, size=(B, L)).astype(np.int64)
    if L >= 300:  # five cls tokens per row, ragged trailing padding
        ids[:, ::60] = CLS
        for b in range(B):
            ids[b, L - 37 * (b + 1):] = PAD
    elif L > 1:
        ids[:, 0] = CLS
        ids[B - 1, L - L // 3:] = PAD
    return ids


@pytest.mark.parametrize("B,L", [(1, 1), (3, 61), (2, 300), (5, 64), (4, 65)])
def test_mlm_mask_equals_restatement(B, L):
    for vocab, p, (seed, stream) in itertools.product((50265, 7), (0.0, 0.1, 0.8, 1.0),
                                                      ((3, 0), (2 ** 40 + 17, 2))):
        ids = _mask_ids(B, L, vocab, 100 + L)
        mask_id = vocab - 1
        want = mlm_mask_ref(ids, PAD, CLS, mask_id, vocab, IGNORE, p, seed, stream)
        g_ids, g_lab = _guarded(ids), _blank(B, L)
        N.mlm_mask(g_ids.v2, g_lab.v2, PAD, CLS, mask_id, vocab, IGNORE, p, seed, stream)
        tag = f"B {B} L {L} vocab {vocab} p {p} key {(seed, stream)}"
        assert np.array_equal(g_ids.v2.cpu().numpy(), want[0]), tag
        assert np.array_equal(g_lab.v2.cpu().numpy(), want[1]), tag
        g_ids.check_untouched("mlm_mask ids " + tag)
        g_lab.check_untouched("mlm_mask labels " + tag)
        special = torch.from_numpy((ids == PAD) | (ids == CLS))
        assert torch.equal(g_ids.v2.cpu()[special], torch.from_numpy(ids)[special])


def test_mlm_mask_repeats_with_its_seed_and_differs_with_another():
    ids = torch.from_numpy(_mask_ids(5, 64, 50265, 1)).to(DEV)
    runs = []
    for seed in (11, 11, 12):
        x = ids.clone()
        runs.append((x, K.mlm_mask(x, PAD, CLS, 50264, 50265, IGNORE, 0.5, seed)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert not torch.equal(runs[0][1], runs[2][1])
    assert not torch.equal(runs[0][0], ids)


def test_mlm_mask_bad_arguments_write_nothing():
    ids = _mask_ids(3, 61, 50265, 2)
    g_ids, g_lab = _guarded(ids), _blank(3, 61)
    before = (g_ids.buf.clone(), g_lab.buf.clone())
    with pytest.raises(N.NativeError, match="vocab"):
        N.mlm_mask(g_ids.v2, g_lab.v2, PAD, CLS, 0, CLS + 1, IGNORE, 0.15, 0)  # vocab <= cls + 1
    with pytest.raises(N.NativeError, match="vocab"):
        N.mlm_mask(g_ids.v2, g_lab.v2, PAD, 7, 0, 7, IGNORE, 0.15, 0)
    with pytest.raises(N.NativeError):
        N.mlm_mask(torch.from_numpy(ids), g_lab.v2, PAD, CLS, 5, 50265, IGNORE, 0.15, 0)  # CPU ids
    with pytest.raises(ValueError):
        N.mlm_mask(g_ids.v2.to(torch.int32), g_lab.v2, PAD, CLS, 5, 50265, IGNORE, 0.15, 0)
    with pytest.raises(ValueError):
        N.mlm_mask(g_ids.v2, g_lab.v2[:, :60], PAD, CLS, 5, 50265, IGNORE, 0.15, 0)
    torch.cuda.synchronize()
    assert torch.equal(g_ids.buf, before[0]) and torch.equal(g_lab.buf, before[1])


# ---- 2. / 3. sub-sampling ------------------------------------------------------------------------
def _subsample_raw(ids, mask, tt, lab, sub_idx, n_steps):
    """The raw binding on guarded buffers -> (outputs on the host, bad-story count)."""
    B, L = ids.shape
    n_sub = np.asarray(sub_idx).shape[1]
    pad = L // n_steps * n_sub
    ins = [None if t is None else _guarded(t) for t in (ids, mask, tt, lab)]
    sub = _guarded(np.asarray(sub_idx, np.int64))
    outs = [None if t is None else _blank(B, pad) for t in (ids, mask, tt, lab)]
    status = _guarded(np.zeros(2, np.int32), torch.int32)
    v = lambda g: None if g is None else g.v2  # noqa: E731
    N.subsample_text(v(ins[0]), v(ins[1]), v(ins[2]), v(ins[3]), sub.v2, n_steps, CLS, PAD, IGNORE,
                     v(outs[0]), v(outs[1]), v(outs[2]), v(outs[3]), status.v2.view(-1))
    for g in ins + [sub]:
        if g is not None:  # inputs: not a single element changes
            assert torch.equal(g.ibuf, g._snap), "subsample_text wrote to an input"
    for g in outs:
        if g is not None:
            g.check_untouched("subsample_text output")
    st = status.v2.view(-1).tolist()
    assert st[1] == 0  # only status[0] is the kernel's
    status.check_untouched("subsample_text status")
    return [None if g is None else g.v2.cpu() for g in outs], st[0]


def _sub_fixtures():
    names = []
    for f in sorted(glob.glob(os.path.join(GOLDEN, "pretrain_mm_*.json"))):
        name = os.path.basename(f)[:-5]
        with np.load(os.path.join(GOLDEN, name + ".npz")) as d:
            if "sub::input_ids" in d.files:
                names.append(name)
    return names


@pytest.mark.parametrize("name", _sub_fixtures())
def test_subsample_reproduces_the_reference(name):
    meta = json.load(open(os.path.join(GOLDEN, name + ".json")))
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    if "input_ids" not in d:  # the real-size fixture regenerates its inputs from the seed
        from make_golden_pretrain_mm import mm_inputs
        ids, mask, labels, _ = mm_inputs(meta["config"], meta["seed"] + 1)
        d.update(input_ids=ids, attention_mask=mask, masked_lm_labels=labels)
    keys = ["input_ids", "attention_mask", "token_type_ids", "masked_lm_labels"]
    ins = [torch.from_numpy(d[k]) if k in d else None for k in keys]
    outs, bad = _subsample_raw(*ins, d["sub_idx"], meta["config"]["N"])
    assert bad == 0
    checked = 0
    for k, o in zip(keys, outs):
        if "sub::" + k in d:
            assert np.array_equal(o.numpy(), d["sub::" + k]), k
            checked += 1
    assert checked >= 3


N_STEPS, N_SUB = 5, 2
PAIRS = list(itertools.combinations(range(N_STEPS), 2))


def _story(rs, L, lens):
    """A story row: step k = cls, lens[k] - 2 tokens, sep; the last step as long as lens[4] says,
    then padding. Returns None when it does not fit."""
    if sum(lens) > L:
        return None
    row = np.full(L, PAD, np.int64)
    at = 0
    for n in lens:
        row[at:at + n] = [CLS] + list(rs.randint(3, 50, size=n - 2)) + [SEP]
        at += n
    return row


def _cases(L):
    """(row, pair) cases: forced cls positions 63, 64, 65, 127, 128 where L allows, then random
    ones until every ascending pair has occurred; every case is valid for the host function."""
    rs = np.random.RandomState(1000 + L)
    per = L // N_STEPS
    out, seen, cls_at = [], set(), set()
    if L >= 300:
        for lens, pair in (([63, 20, 30, 30, 40], (0, 1)), ([64, 9, 30, 30, 40], (0, 1)),
                           ([65, 55, 30, 30, 40], (0, 1)), ([63, 64, 10, 30, 40], (1, 2)),
                           ([64, 64, 2, 30, 40], (1, 2)), ([63, 2, 50, 2, 50], (2, 4))):
            out.append((_story(rs, L, lens), pair))
    while len(seen) < len(PAIRS) or len(out) % 7:
        lens = [int(rs.randint(2, per + 1)) for _ in range(N_STEPS)]
        pair = PAIRS[rs.randint(len(PAIRS))]
        out.append((_story(rs, L, lens), pair))
        seen.add(pair)
    for row, pair in out:
        cls_at.update(np.nonzero(row == CLS)[0].tolist())
    assert seen == set(PAIRS)
    if L >= 300:
        assert {63, 64, 65, 127, 128} <= cls_at
    return out


def _tensors(rows, seed):
    rs = np.random.RandomState(seed)
    ids = torch.from_numpy(np.stack(rows))
    mask = (ids != PAD).long()
    tt = torch.from_numpy(rs.randint(0, 2, size=tuple(ids.shape)).astype(np.int64))
    lab = torch.from_numpy(np.where(rs.rand(*ids.shape) < 0.3, rs.randint(3, 50, size=tuple(ids.shape)),
                                    IGNORE).astype(np.int64))
    return ids, mask, tt, lab


@pytest.mark.parametrize("L", [30, 300, 320])
def test_subsample_equals_host_function_on_ragged_batches(L):
    cases = _cases(L)
    batches = [cases[k:k + 7] for k in range(0, len(cases), 7)] + [[c] for c in cases[:7]]
    assert {len(b) for b in batches} == {1, 7}
    for n, batch in enumerate(batches):
        ids, mask, tt, lab = _tensors([r for r, _ in batch], n)
        sub = np.asarray([p for _, p in batch], np.int64)
        for use_tt, use_lab in itertools.product((True, False), repeat=2):
            a = (ids, mask, tt if use_tt else None, lab if use_lab else None)
            want = P.subsample_text(*a, sub, N_STEPS, CLS, PAD, IGNORE)
            got, bad = _subsample_raw(*a, sub, N_STEPS)
            assert bad == 0
            for w, g in zip(want, got):
                assert (w is None) == (g is None)
                if w is not None:
                    assert torch.equal(w, g), (L, n, use_tt, use_lab)
        # the Python surface: host tensors are copied over, device tensors are used where they are
        want = P.subsample_text(ids, mask, tt, lab, sub, N_STEPS, CLS, PAD, IGNORE)
        for move in (lambda t: t, lambda t: t.to(DEV)):
            got = P.subsample_text_device(move(ids), move(mask), move(tt), move(lab), sub, N_STEPS,
                                          CLS, PAD, IGNORE)
            assert all(g.is_cuda and torch.equal(w, g.cpu()) for w, g in zip(want, got))


def test_subsample_error_stories_are_counted_and_padded():
    L = 300
    per = L // N_STEPS
    rs = np.random.RandomState(5)
    good = _story(rs, L, [30, 40, 50, 60, 20])
    four = _story(rs, L, [30, 40, 50, 60])              # four cls tokens only
    long_ = _story(rs, L, [per + 3, per, 10, 10, 20])   # steps 0 + 1: 123 > 120 tokens
    rows = [good, four, long_, four, good, good, good]
    subs = [(0, 3), (1, 4), (0, 1), (2, 3), (3, 4), (1, 2), (0, 4)]
    raises = [False, True, True, True, False, False, False]
    ids, mask, tt, lab = _tensors(rows, 9)
    for b, bad in enumerate(raises):  # the host function, story by story
        a = [t[b:b + 1] for t in (ids, mask, tt, lab)]
        if bad:
            with pytest.raises((ValueError, IndexError)):
                P.subsample_text(*a, [subs[b]], N_STEPS, CLS, PAD, IGNORE)
    got, n_bad = _subsample_raw(ids, mask, tt, lab, np.asarray(subs), N_STEPS)
    assert n_bad == sum(raises) == 3
    for b, bad in enumerate(raises):
        if bad:
            assert (got[0][b] == PAD).all() and (got[1][b] == 0).all() and (got[2][b] == 0).all()
            assert (got[3][b] == IGNORE).all()
        else:
            want = P.subsample_text(*[t[b:b + 1] for t in (ids, mask, tt, lab)], [subs[b]], N_STEPS,
                                    CLS, PAD, IGNORE)
            for w, g in zip(want, got):
                assert torch.equal(w[0], g[b]), b
    with pytest.raises(ValueError, match="3 stories"):
        P.subsample_text_device(ids.to(DEV), mask.to(DEV), tt.to(DEV), lab.to(DEV), np.asarray(subs),
                                N_STEPS, CLS, PAD, IGNORE)
    with pytest.raises(ValueError, match="1 story"):
        P.subsample_text_device(ids[1:2], mask[1:2], None, None, [subs[1]], N_STEPS, CLS, PAD, IGNORE)
    with pytest.raises(N.NativeError):  # n_steps beyond one wave's 64
        P.subsample_text_device(ids, mask, None, None, np.asarray(subs), 65, CLS, PAD, IGNORE)


# ---- 4. compaction -------------------------------------------------------------------------------
def _compact_labels(R, density, seed):
    rs = np.random.RandomState(seed)
    lab = rs.randint(0, 50265, size=R).astype(np.int64)
    if density == "last":
        keep = np.zeros(R, bool)
        keep[-1] = True
    else:
        keep = rs.rand(R) < density
    return torch.from_numpy(np.where(keep, lab, IGNORE))


@pytest.mark.parametrize("R", [1, 64, 65, 1023, 1024, 1025, 4097, 70001])
def test_rows_compact_is_nonzero_order(R):
    for density in (0.0, 0.15, 1.0, "last"):
        labels = _compact_labels(R, density, R)
        want_src = torch.nonzero(labels != IGNORE).view(-1)
        n = want_src.numel()
        g_lab = _guarded(labels)
        runs = []
        for _ in range(2):
            src, out, count = _blank(R, 1, torch.int32), _blank(R, 1), _blank(1, 1, torch.int32)
            N.rows_compact(g_lab.v2.view(-1), IGNORE, src.v2.view(-1), out.v2.view(-1),
                           count.v2.view(-1))
            assert count.v2.item() == n, (R, density)
            assert torch.equal(src.v2.view(-1)[:n].cpu(), want_src.to(torch.int32)), (R, density)
            assert torch.equal(out.v2.view(-1)[:n].cpu(), labels[want_src]), (R, density)
            beyond = (torch.arange(R) >= n).view(R, 1).to(DEV)
            src.check_untouched(f"rows_compact src R {R} density {density}", also=beyond)
            out.check_untouched(f"rows_compact labels R {R} density {density}", also=beyond)
            count.check_untouched("rows_compact count")
            runs.append((src.ibuf.clone(), out.ibuf.clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        assert torch.equal(g_lab.ibuf, g_lab._snap)
        s, l = K.labelled_rows(labels.to(DEV), IGNORE, DEV)  # the Python surface, device labels
        hs, hl = K.labelled_rows(labels, IGNORE, DEV)          # and host labels: the present code
        assert torch.equal(s, hs) and torch.equal(l, hl) and s.dtype == torch.int32


# ---- 5. the model: device batch == host batch ------------------------------------------------------
def _weights(meta):
    from counter_init import counter_state_dict
    params = counter_state_dict({k: tuple(v) for k, v in meta["shapes"].items()})
    params["cls.predictions.decoder.weight"] = params["bert.embeddings.word_embeddings.weight"]
    return {k: torch.from_numpy(v) for k, v in params.items()}


def _batch(kind, d, device=None, labels=True):
    keys = {"isp": ["swap"], "pisp": ["swap", "count", "patch_src"], "mrm": ["mask_idx", "shuffle"]}
    b = {k: torch.from_numpy(d[k]) for k in ("input_ids", "attention_mask", "token_type_ids",
                                             "masked_lm_labels")}
    if device is not None:
        b = {k: v.to(device) for k, v in b.items()}
    if not labels:
        del b["masked_lm_labels"]
    b["images"] = torch.from_numpy(d["images"])
    b["draws"] = {k: d[k] for k in ["objective", "sub_idx"] + keys[kind]}
    return b


def _model(meta, dtype, train=False):
    m = build_mm(meta, DEV, dtype)
    m.load_state_dict(_weights(meta))
    m.train(train)
    m.zero_grad()
    return m


@pytest.mark.parametrize("kind", list(KINDS))
def test_model_device_batch_equals_host_batch_fp32(kind, monkeypatch):
    meta, d = load_mm(kind)
    runs = []
    for device in (None, DEV):
        m = _model(meta, torch.float32)
        if device is not None:  # the device path has its own compaction and ONE read-back
            def no(*a, **k):
                raise AssertionError("the device path went through labelled_rows")
            monkeypatch.setattr(K, "labelled_rows", no)
        loss, losses, answer = m(_batch(kind, d, device))
        loss.backward()
        torch.cuda.synchronize()
        runs.append((loss.detach(), losses, answer, [s.grad.clone() for s in m.stores()]))
    (la, sa, aa, ga), (lb, sb, ab, gb) = runs
    print(kind, "host batch", la.item(), "device batch", lb.item(), "reference", float(d["loss"]))
    assert torch.equal(la, lb) and torch.equal(sa, sb) and torch.equal(aa, ab)
    for x, y in zip(ga, gb):
        assert torch.equal(x, y)
    assert abs(lb.item() - float(d["loss"])) < 1e-4


@pytest.mark.parametrize("kind", list(KINDS))
def test_model_device_batch_equals_host_batch_bf16_train_step(kind):
    from multimodal_sequencing_amd.trainer import FusedAdamW, train_step
    meta, d = load_mm(kind)
    ends = []
    for device in (None, DEV):
        m = _model(meta, torch.bfloat16, train=True)
        loss = train_step(m, FusedAdamW(m.stores(), lr=1e-3, warmup=0, total_steps=10),
                          [_batch(kind, d, device)])
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss))
        ends.append((loss.clone(), [s.master.clone() for s in m.stores()]))
    assert torch.equal(ends[0][0], ends[1][0])
    for x, y in zip(ends[0][1], ends[1][1]):
        assert torch.equal(x, y)


def test_model_device_batch_needs_every_tensor_on_the_device():
    meta, d = load_mm("isp")
    m = _model(meta, torch.float32)
    b = _batch("isp", d, DEV)
    b["masked_lm_labels"] = b["masked_lm_labels"].cpu()
    with pytest.raises(ValueError, match="masked_lm_labels"):
        m(b)
    with pytest.raises(ValueError, match="mask_tokens_sentence"):
        m(_batch("isp", d, DEV, labels=False))


# ---- 6. dynamic masking, end to end ----------------------------------------------------------------
class _Tokenizer:
    """What mask_tokens_sentence reads of a tokenizer."""
    pad_token, mask_token = "<pad>", "<mask>"

    def __init__(self, vocab):
        self.ids = {"<pad>": PAD, "<mask>": vocab - 1}
        self.vocab = vocab

    def convert_tokens_to_ids(self, token):
        return self.ids[token]

    def __len__(self):
        return self.vocab


def test_dynamic_masking_end_to_end(monkeypatch):
    meta, d = load_mm("pisp")
    vocab = meta["config"]["joint"]["vocab"]
    tok = _Tokenizer(vocab)
    args = SimpleNamespace(mlm_probability=0.3, cls_id=CLS, mlm_ignore_index=IGNORE)
    seen = []
    fwd = N.xent_fwd

    def spy(logits, V, lab, ignore, lse, loss_row, stats):
        seen.append(logits.shape[0])
        fwd(logits, V, lab, ignore, lse, loss_row, stats)

    monkeypatch.setattr(N, "xent_fwd", spy)
    losses = []
    for seed in (21, 21, 22):
        ids = torch.from_numpy(d["input_ids"]).to(DEV)
        out, labels = P.mask_tokens_sentence(ids, tok, args, seed=seed)
        assert out.data_ptr() == ids.data_ptr() and labels.is_cuda  # in place, on the device
        want = mlm_mask_ref(d["input_ids"], PAD, CLS, vocab - 1, vocab, IGNORE, 0.3, seed, 0)
        assert np.array_equal(out.cpu().numpy(), want[0])
        assert np.array_equal(labels.cpu().numpy(), want[1])
        b = _batch("pisp", d, DEV, labels=False)
        b.update(input_ids=out, masked_lm_labels=labels)
        m = _model(meta, torch.float32)
        loss, _, _ = m(b)
        assert bool(torch.isfinite(loss))
        sub_lab = P.subsample_text(out.cpu(), b["attention_mask"].cpu(), None, labels.cpu(),
                                   d["sub_idx"], meta["config"]["N"], CLS, PAD, IGNORE)[3]
        rows = int((sub_lab != IGNORE).sum())
        assert rows > 0 and seen[-1] == rows
        losses.append(loss.detach().clone())
    assert torch.equal(losses[0], losses[1])
    assert not torch.equal(losses[0], losses[2])
    # host ids are copied to the device; seed=None never repeats a key
    host = torch.from_numpy(d["input_ids"])
    a = P.mask_tokens_sentence(host.clone(), tok, args)
    b = P.mask_tokens_sentence(host.clone(), tok, args)
    assert a[0].is_cuda and a[1].is_cuda
    assert not torch.equal(a[1], b[1])
