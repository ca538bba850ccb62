"""Image-only ordering: the beam order of every fixture story is the reference's. fp32: identical
(the fixtures' input seeds were picked so that the reference beam's best hypothesis leads the
second by more than 1e-3, fp32 noise being ~1e-5). bf16: identical, or a printed near-tie whose
fp32 score gap is below NEAR_TIE (the rule of test_parity_gpu.py)."""
import pytest
import torch

from imgonly_util import IMGONLY_FIXTURES, build_model, load_imgonly, story_inputs

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multimodal_sequencing_amd.berson import (berson_pointer_network,
                                                  berson_pointer_network_batch)

NEAR_TIE = 5e-3


@pytest.mark.parametrize("name", IMGONLY_FIXTURES)
def test_fp32_beam_order_matches_reference(name):
    meta, d, _ = load_imgonly(name, params=False)
    assert min(meta["margins"]) > 1e-3
    m = build_model(name, torch.float32, cached=True)
    want = [[int(x) for x in o] for o in d["order"]]
    for b in range(len(want)):
        order = berson_pointer_network(m.args, m, None, story_inputs(d, b, device="cuda"))
        assert order == want[b], (b, order, want[b])
    assert berson_pointer_network_batch(m.args, m, None, story_inputs(d, device="cuda")) == want


def _order_nll(m, inp, order):
    with torch.no_grad():
        m({**inp, "labels": torch.tensor([order])})
    return float(m.last_loss_terms[0]) * (len(order) - 1)


@pytest.mark.parametrize("name", IMGONLY_FIXTURES)
def test_bf16_beam_order_matches_reference(name):
    meta, d, _ = load_imgonly(name, params=False)
    m = build_model(name, torch.bfloat16, cached=True)
    for b in range(d["order"].shape[0]):
        inp = story_inputs(d, b, device="cuda")
        order = berson_pointer_network(m.args, m, None, inp)
        ref = [int(x) for x in d["order"][b]]
        if order == ref:
            continue
        m32 = build_model(name, torch.float32, cached=True)
        gap = _order_nll(m32, inp, order) - _order_nll(m32, inp, ref)
        print(f"NEAR-TIE {name} story {b}: bf16 order {order} vs reference {ref}, fp32 score gap "
              f"{gap:.3e} (reference beam margin {meta['margins'][b]:.3e})")
        assert abs(gap) < NEAR_TIE, (name, b, order, ref, gap)
