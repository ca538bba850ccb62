"""Text+image pretraining (MLM + ISP / PISP / MRM; pretraining.LXRTPretraining with
multimodal_img_part = False) against the reference-generated fixtures pretrain_mm_tiny_{isp,pisp,
mrm} (tests/golden/make_golden_pretrain_mm.py: the reference run in-process, eval mode, every
np.random draw recorded). CPU part: names, shapes and order of the parameters, the draws, and the
host restatement of the text sub-sampling. The GPU parity is tests/test_pretrain_mm_gpu.py.
"""
import json
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN
from multimodal_sequencing_amd import model_zoo
from multimodal_sequencing_amd.lxrt import LXRTConfig
from multimodal_sequencing_amd.pretraining import (ISP, MM_OBJECTIVES, MRM, PISP, LXRTPretraining,
                                                   subsample_text)

KINDS = {"isp": ISP, "pisp": PISP, "mrm": MRM}


def load_mm(kind):
    name = f"pretrain_mm_tiny_{kind}"
    meta = json.load(open(os.path.join(GOLDEN, name + ".json")))
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    k = 0
    while os.path.exists(os.path.join(GOLDEN, f"{name}_g{k}.npz")):  # the gradients, in parts
        d.update(np.load(os.path.join(GOLDEN, f"{name}_g{k}.npz")))
        k += 1
    return meta, d


def build_mm(meta, device, dtype, objectives=None):
    if objectives is None:
        objectives = [meta["objective"]]
    return model_zoo.build_pretrain_mm_from_golden(meta["config"], objectives, device=device,
                                                   dtype=dtype)


class Replay:
    """np.random's choice / rand / randint / shuffle replaying a recorded stream, call by call."""

    def __init__(self, stream):
        self.it = iter(stream)

    def _next(self, kind):
        k, v = next(self.it)
        assert k == kind, (k, kind)
        return v

    def choice(self, a, size=None, replace=True, p=None):
        v = np.asarray(self._next("choice"))
        n = len(a) if hasattr(a, "__len__") else int(a)
        assert v.size == (1 if size is None else size) and not replace
        if v.size and v.dtype.kind in "iu":  # drawn from the population it was recorded for
            pop = list(a) if hasattr(a, "__len__") else list(range(n))
            assert all(int(x) in pop for x in v.reshape(-1)), (v, pop[:3], pop[-3:])
        return v

    def rand(self):
        return float(self._next("rand"))

    def randint(self, low, high=None):
        v = int(self._next("randint"))
        assert low <= v < high
        return v

    def shuffle(self, x):
        x[:] = self._next("shuffle")

    def done(self):
        return next(self.it, None) is None


@pytest.mark.parametrize("kind", list(KINDS))
def test_state_dict_and_parameter_order_are_the_references(kind):
    meta, _ = load_mm(kind)
    m = build_mm(meta, "cpu", torch.float32)
    ours = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    ref = {k: tuple(v) for k, v in meta["shapes"].items()}
    assert set(ours) == set(ref), (sorted(set(ours) - set(ref)), sorted(set(ref) - set(ours)))
    for k in ref:
        assert ours[k] == ref[k], k
    assert [n for n, _ in m.named_parameters()] == meta["parameter_order"]
    sd = m.state_dict()
    assert sd["cls.predictions.decoder.weight"].data_ptr() == \
        sd["bert.embeddings.word_embeddings.weight"].data_ptr()  # tied (:1164-1167)


def test_all_three_objectives_register_in_constructor_order():
    meta, _ = load_mm("mrm")
    m = build_mm(meta, "cpu", torch.float32, objectives=list(MM_OBJECTIVES))
    heads = [n for n, _ in m.named_parameters() if not n.startswith("bert.")]
    first = [n.split(".")[0] for n in heads]
    order = [x for i, x in enumerate(first) if x not in first[:i]]
    assert order == ["image_swapping_mlp", "patch_based_image_swapping_mlp",
                     "patch_based_mrm_classification_head", "cls", "obj_predict_head", "answer_head"]
    # two of three: the subset keeps that order
    m2 = build_mm(meta, "cpu", torch.float32, objectives=[MRM, ISP])
    first = [n.split(".")[0] for n, _ in m2.named_parameters() if not n.startswith("bert.")]
    assert [x for i, x in enumerate(first) if x not in first[:i]][:3] == \
        ["image_swapping_mlp", "patch_based_mrm_classification_head", "cls"]


@pytest.mark.parametrize("kind", list(KINDS))
def test_draw_replays_the_recorded_stream(kind):
    """draw_mm consumes the reference's recorded np.random stream call by call (kinds, populations
    and ranges checked by Replay) and returns the recorded structured draws."""
    meta, d = load_mm(kind)
    m = build_mm(meta, "cpu", torch.float32)
    c = meta["config"]
    g2 = (c["vit"]["res"] // c["vit"]["patch"]) ** 2
    Tv = 1 + 2 * g2
    rp = Replay(meta["stream"])
    dr = m.draw_mm(c["B"], c["N"], Tv, rng=rp)
    assert rp.done()
    assert dr["objective"] == meta["objective"] == str(d["objective"])
    keys = {"isp": ["sub_idx", "swap"], "pisp": ["sub_idx", "swap", "count", "patch_src"],
            "mrm": ["sub_idx", "mask_idx", "shuffle"]}[kind]
    for k in keys:
        assert np.array_equal(dr[k], d[k]), k
    if kind != "mrm":  # the stories the generator promised
        assert meta["swapped_stories"] and meta["unswapped_stories"]
        assert np.nonzero(d["swap"])[0].tolist() == meta["swapped_stories"]
    if kind == "pisp":
        assert meta["zero_count_stories"] == np.nonzero(d["count"] == 0)[0].tolist() != []


@pytest.mark.parametrize("obj", MM_OBJECTIVES)
def test_draw_shapes_and_ranges(obj):
    meta, _ = load_mm("mrm")
    m = build_mm(meta, "cpu", torch.float32, objectives=[obj])
    B, N, g2 = 64, 5, 16
    Tv = 1 + 2 * g2
    dr = m.draw_mm(B, N, Tv)
    assert dr["objective"] == obj
    assert dr["sub_idx"].shape == (B, 2) and (np.diff(dr["sub_idx"], axis=1) > 0).all()
    assert dr["sub_idx"].min() >= 0 and dr["sub_idx"].max() < N
    if obj == ISP:
        assert dr["swap"].shape == (B,) and 0 < dr["swap"].sum() < B
    elif obj == PISP:
        assert ((dr["count"] >= 0) & (dr["count"] < g2)).all()
        src = dr["patch_src"]
        assert src.shape == (B, Tv)
        ident = np.arange(Tv)
        class_token_moved = False
        for b in range(B):
            assert sorted(src[b]) == list(ident)  # a permutation
            moved = np.nonzero(src[b] != ident)[0]
            assert len(moved) == (2 * dr["count"][b] if dr["swap"][b] else 0)
            lo = moved[moved < 1 + g2]
            # rows of [0, 1 + g^2) trade places with rows of [1 + g^2, Tv) only
            assert (src[b][lo] >= 1 + g2).all() and (src[b][moved[moved >= 1 + g2]] < 1 + g2).all()
            class_token_moved |= bool(src[b][0] != 0)
        assert class_token_moved  # the class token belongs to the first range (64 stories)
    else:
        mi = dr["mask_idx"]
        assert mi.shape == (B, 10)
        assert ((mi[:, :5] >= 1) & (mi[:, :5] < 1 + g2)).all()
        assert ((mi[:, 5:] >= 1 + g2) & (mi[:, 5:] < Tv)).all()
        assert (np.diff(mi[:, :5], axis=1) > 0).all() and (np.diff(mi[:, 5:], axis=1) > 0).all()
        for row in dr["shuffle"]:
            assert sorted(row) == list(range(10))


def test_pisp_zero_count_still_labels_a_swap():
    """A story whose count is 0 swaps nothing and is still labelled 0 when rand() > 0.5."""
    meta, _ = load_mm("pisp")
    m = build_mm(meta, "cpu", torch.float32)
    stream = [["choice", [PISP]], ["choice", [1, 3]], ["randint", 7], ["randint", 0],
              ["choice", []], ["choice", []], ["choice", []], ["choice", []], ["rand", 0.9],
              ["choice", [1, 0]]]
    rp = Replay(stream)
    dr = m.draw_mm(1, 5, 33, rng=rp)
    assert rp.done() and dr["swap"].tolist() == [1] and dr["count"].tolist() == [0]
    assert np.array_equal(dr["patch_src"][0], np.arange(33))


@pytest.mark.parametrize("kind", list(KINDS))
def test_text_subsampling_matches_reference(kind):
    meta, d = load_mm(kind)
    c = meta["config"]
    ids, mask, tt, lab = subsample_text(torch.from_numpy(d["input_ids"]),
                                        torch.from_numpy(d["attention_mask"]),
                                        torch.from_numpy(d["token_type_ids"]),
                                        torch.from_numpy(d["masked_lm_labels"]), d["sub_idx"],
                                        c["N"], 0, 1, meta["mlm_ignore_index"])
    assert d["token_type_ids"].max() == 1  # both types present, so the types' cut is pinned too
    assert np.array_equal(tt.numpy(), d["sub::token_type_ids"])
    assert ids.shape == (c["B"], c["per_seq"] * 2)
    assert np.array_equal(ids.numpy(), d["sub::input_ids"])
    assert np.array_equal(mask.numpy(), d["sub::attention_mask"])
    assert np.array_equal(lab.numpy(), d["sub::masked_lm_labels"])
    assert ((lab != meta["mlm_ignore_index"]).sum(1) >= 1).all()  # a labelled token per story


def test_text_subsampling_ragged_steps_and_padding():
    """Steps of unequal length: a step runs to the next cls token, the last one L // N tokens."""
    ids = torch.tensor([[0, 5, 2, 0, 6, 7, 8, 2, 0, 9, 2, 1]])  # steps of 3, 5, 4 (L // N = 4)
    lab = torch.arange(100, 112)[None]
    out = subsample_text(ids, (ids != 1).long(), torch.zeros_like(ids), lab, [[0, 2]], 3, 0, 1, -100)
    assert out[0].tolist() == [[0, 5, 2, 0, 9, 2, 1, 1]]
    assert out[1].tolist() == [[1, 1, 1, 1, 1, 1, 0, 0]]
    assert out[2].tolist() == [[0] * 8]
    assert out[3].tolist() == [[100, 101, 102, 108, 109, 110, 111, -100]]
    with pytest.raises(ValueError):  # steps 1 + 2 hold 9 tokens > 8
        subsample_text(ids, (ids != 1).long(), None, lab, [[1, 2]], 3, 0, 1, -100)


@pytest.mark.parametrize("objectives", [["multimodal_swapping", ISP], ["margin_loss"],
                                        ["multimodal_margin_loss"], ["time_contrastive"],
                                        ["image_sequence_predictions"],
                                        ["whole_image_sequence_swapping", MRM], []])
def test_unsupported_objectives_raise(objectives):
    meta, _ = load_mm("isp")
    with pytest.raises(NotImplementedError) as e:
        build_mm(meta, "cpu", torch.float32, objectives=objectives)
    for o in objectives:
        if o not in MM_OBJECTIVES:
            assert o in str(e.value)


def test_rn50_and_text_only_pretraining_raise():
    cfg = LXRTConfig(vocab_size=300, hidden_size=128, num_hidden_layers=1, num_attention_heads=2,
                     intermediate_size=512, max_position_embeddings=64, type_vocab_size=2)
    kw = dict(multimodal_img_part=False, cls_id=0, sep_id=2, pad_id=1, max_story_length=5,
              multimodal_pretrain_objectives=[ISP], pretraining=True, device="cpu",
              compute_dtype=torch.float32)
    with pytest.raises(NotImplementedError, match="RN50"):
        LXRTPretraining(cfg, clip_model_name="RN50", **kw)
    with pytest.raises(NotImplementedError, match="text"):
        LXRTPretraining(cfg, multimodal_text_part=True, clip_model_name="ViT-B/16", **kw)
