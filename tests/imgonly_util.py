"""Shared helpers of the image-only (multimodal_img_part) tests: load the imgonly_* fixtures
(tests/golden/make_golden_imgonly.py), their inputs and their counter-based weights."""
import json
import os

import torch

from counter_init import counter_state_dict
from golden_util import GOLDEN
from make_golden_imgonly import load_parts

IMGONLY_FIXTURES = ["imgonly_tiny", "imgonly_tiny_g3", "imgonly_real_config3"]
_CACHE = {}


def load_imgonly(name, params=True):
    """-> (meta, arrays, counter weights or None). The arrays include input_ids / labels / images:
    stored for the tiny fixtures, regenerated from the recorded seed for the real-shape one."""
    if name not in _CACHE:
        with open(os.path.join(GOLDEN, name + ".json")) as f:
            meta = json.load(f)
        d = load_parts(name)
        if not meta["inputs_stored"]:
            from make_golden_real import real_inputs
            d["input_ids"], d["labels"], d["images"] = real_inputs(meta["input_seed"],
                                                                   meta["config"])
        for v in d.values():
            v.setflags(write=False)
        _CACHE[name] = (meta, d)
    meta, d = _CACHE[name]
    p = None
    if params:
        p = {k: torch.from_numpy(v) for k, v in
             counter_state_dict({k: tuple(s) for k, s in meta["shapes"].items()}).items()}
    return meta, d, p


_MODELS = {}


def build_model(name, dtype, cached=False):
    """BertForOrdering of an imgonly fixture with its counter weights, in eval mode, on the GPU.
    cached=True: one model per (name, dtype) shared by the tests that neither train it nor touch
    its weights (gradients zeroed on every hand-out)."""
    from multimodal_sequencing_amd import model_zoo
    if cached and (name, dtype) in _MODELS:
        m = _MODELS[(name, dtype)]
        m.eval()
        m.zero_grad()
        return m
    meta, _d, params = load_imgonly(name)
    m = model_zoo.build_from_golden(meta["config"], device="cuda", dtype=dtype)
    m.load_state_dict(params)
    m.eval()
    m.zero_grad()
    if cached:
        _MODELS[(name, dtype)] = m
    return m


def story_inputs(d, b=None, device=None):
    """The model's input dict for the whole fixture batch, or for story b alone."""
    sl = slice(None) if b is None else slice(b, b + 1)
    images = torch.tensor(d["images"][sl])  # copies: the cached fixture arrays stay read-only
    return {"input_ids": torch.tensor(d["input_ids"][sl]), "labels": torch.tensor(d["labels"][sl]),
            "images": images.to(device) if device else images}
