"""Image-only ordering: the misuses that used to run silently (or could) raise, and a batch without
text orders exactly as one with it."""
import pytest
import torch

from golden_util import load_fixture
from imgonly_util import build_model, load_imgonly, story_inputs

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multimodal_sequencing_amd import berson, model_zoo
    from multimodal_sequencing_amd.lxrt import CLIP_VISION, LXRTConfig, LXRTModel


def test_flag_and_inner_model_must_agree():
    meta, d, _ = load_imgonly("imgonly_tiny", params=False)
    inputs = story_inputs(d, device="cuda")
    # an image-only inner model under a text+image head: what ran silently before
    m = build_model("imgonly_tiny", torch.float32)
    m.args.multimodal_img_part = False
    with pytest.raises(ValueError, match="multimodal_img_part"):
        m(inputs)
    with pytest.raises(ValueError, match="multimodal_img_part"):
        berson.berson_pointer_network_batch(m.args, m, None, inputs)
    # and the other way round
    tmeta, td, _ = load_fixture("tiny")
    m2 = model_zoo.build_from_golden(tmeta["config"], device="cuda", dtype=torch.float32)
    m2.args.multimodal_img_part = True
    with pytest.raises(ValueError, match="multimodal_img_part"):
        m2({"input_ids": torch.from_numpy(td["input_ids"]), "labels": torch.from_numpy(td["labels"]),
            "images": torch.from_numpy(td["images"]).cuda()})


def test_images_are_required():
    meta, d, _ = load_imgonly("imgonly_tiny", params=False)
    m = build_model("imgonly_tiny", torch.float32, cached=True)
    inputs = story_inputs(d, device="cuda")
    del inputs["images"]
    with pytest.raises(ValueError, match="images"):
        m(inputs)
    b = berson._batch_inputs(m, story_inputs(d, device="cuda"))
    b["images"] = None
    with pytest.raises(ValueError, match="images"):
        m.encode(**b)


def test_rn50_image_only_is_refused():
    cfg = LXRTConfig(vocab_size=300, hidden_size=128, num_hidden_layers=1, num_attention_heads=2,
                     intermediate_size=256)
    with pytest.raises(NotImplementedError, match="one sequence per image"):
        LXRTModel(cfg, multimodal_img_part=True, clip_model_name="RN50",
                  vision=dict(CLIP_VISION["RN50"]), device="cuda", compute_dtype=torch.float32)
    with pytest.raises(ValueError, match="exclusive"):
        LXRTModel(cfg, multimodal_img_part=True, multimodal_text_part=True, device="cuda")


def test_batch_without_text_orders_the_same():
    meta, d, _ = load_imgonly("imgonly_tiny", params=False)
    m = build_model("imgonly_tiny", torch.float32, cached=True)
    full = story_inputs(d, device="cuda")
    want = berson.berson_pointer_network_batch(m.args, m, None, full)
    s_want = m.last_beam_scores.clone()
    bare = {"images": full["images"]}  # no input_ids, no labels: N and B come from the images
    got = berson.berson_pointer_network_batch(m.args, m, None, bare)
    assert got == want
    assert torch.equal(m.last_beam_scores, s_want)
    assert berson.berson_pointer_network(m.args, m, None, {"images": full["images"][:1]}) == want[0]
    loss_full = m(full)[0]
    loss_bare = m({"images": full["images"], "labels": full["labels"]})[0]
    assert loss_bare.item() == loss_full.item()
    m.zero_grad()
