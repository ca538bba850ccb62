"""Pair expansion in image-only mode (process_inputs_for_berson.py:198-204): the host
prepare_berson_inputs(img_part=True) equals the reference's pair tensors bit for bit on the three
imgonly fixtures; the default path still equals `tiny`'s; a batch without text."""
import numpy as np
import pytest
import torch

from golden_util import load_fixture
from imgonly_util import IMGONLY_FIXTURES, load_imgonly
from multimodal_sequencing_amd.process_inputs import (pairs_generator, prepare_berson_inputs,
                                                      prepare_berson_inputs_host)


def _check(pair, d):
    keys = [k for k in d if k.startswith("pair::")]
    assert len(keys) == 10
    for k in keys:
        got = pair[k[6:]]
        assert got.dtype == torch.int64
        assert np.array_equal(got.numpy(), d[k]), k


@pytest.mark.parametrize("name", IMGONLY_FIXTURES)
def test_img_part_pairs_equal_reference(name):
    meta, d, _ = load_imgonly(name, params=False)
    N = meta["config"]["N"]
    _check(prepare_berson_inputs(d["input_ids"], d["labels"], N, img_part=True), d)
    _check(prepare_berson_inputs_host(d["input_ids"], d["labels"], N, img_part=True), d)
    assert (d["pair::sep_positions"] == np.array([0, 1])).all()


def test_default_path_unchanged():
    meta, d, _ = load_fixture("tiny")
    N = meta["config"]["N"]
    _check(prepare_berson_inputs(d["input_ids"], d["labels"], N), d)
    _check(prepare_berson_inputs(d["input_ids"], d["labels"], N, img_part=False), d)


def test_img_part_changes_sep_positions_only():
    meta, d, _ = load_imgonly("imgonly_tiny", params=False)
    N = meta["config"]["N"]
    a = prepare_berson_inputs(d["input_ids"], d["labels"], N)
    b = prepare_berson_inputs(d["input_ids"], d["labels"], N, img_part=True)
    for k in a:
        assert torch.equal(a[k], b[k]) == (k != "sep_positions"), k


def test_batch_without_text():
    meta, d, _ = load_imgonly("imgonly_tiny", params=False)
    N = meta["config"]["N"]
    full = prepare_berson_inputs(d["input_ids"], d["labels"], N, img_part=True)
    bare = prepare_berson_inputs(None, torch.tensor(d["labels"]), N, img_part=True)
    for k in ("pairs_list", "passage_length", "pairs_num", "sep_positions", "ground_truth",
              "mask_cls", "pairwise_labels"):
        assert torch.equal(full[k], bare[k]), k
    B, npair = d["labels"].shape[0], pairs_generator(N)[1]
    for k in ("input_ids", "attention_mask", "token_type_ids"):
        assert tuple(bare[k].shape) == (B, npair, 2) and bare[k].dtype == torch.int64
    with pytest.raises(ValueError):
        prepare_berson_inputs(None, d["labels"], N)
    with pytest.raises(ValueError):
        prepare_berson_inputs(None, torch.tensor(d["labels"][:, :-1]), N, img_part=True)
