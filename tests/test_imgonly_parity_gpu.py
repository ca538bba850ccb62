"""Image-only ordering (multimodal_img_part) in fp32 against the reference's own outputs
(tests/golden/imgonly_*, tolerances of test_parity_gpu.py): loss, total gradient norm, every
stored gradient, the parameters the reference never reaches, and the intermediates."""
import numpy as np
import pytest
import torch

from imgonly_util import IMGONLY_FIXTURES, build_model, load_imgonly, story_inputs

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multimodal_sequencing_amd import berson


@pytest.mark.parametrize("name", IMGONLY_FIXTURES)
def test_fp32_loss_grads_match_reference(name):
    meta, d, _ = load_imgonly(name, params=False)
    m = build_model(name, torch.float32, cached=True)
    loss = m(story_inputs(d, device="cuda"))[0]
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: (None if p.grad is None else p.grad.detach().cpu())
             for k, p in m.named_parameters()}
    m.zero_grad()
    ref, gn_ref = float(d["loss"]), float(d["grad_norm"])
    gn = sum(float((g.double() ** 2).sum()) for g in grads.values() if g is not None) ** 0.5
    print(f"{name}: loss {loss.item():.7f} ref {ref:.7f}; grad norm {gn:.6f} ref {gn_ref:.6f}")
    assert abs(loss.item() - ref) < 1e-4, (loss.item(), ref)
    assert abs(gn - gn_ref) < 1e-3 * gn_ref, (gn, gn_ref)
    checked = 0
    for k in d:
        if k.startswith("g::"):
            np.testing.assert_allclose(grads[k[3:]].numpy(), d[k], rtol=2e-3, atol=1e-5, err_msg=k)
            checked += 1
    assert checked > 10
    assert len(meta["nograd"]) == 24
    for k in meta["nograd"]:  # never reached by the reference: None there, None or zeros here
        assert k in grads, k
        assert grads[k] is None or not bool(grads[k].any()), k
    reached = set(grads) - set(meta["nograd"])
    assert all(grads[k] is not None and bool(grads[k].any()) for k in reached)


@pytest.mark.parametrize("name", IMGONLY_FIXTURES)
def test_fp32_intermediates_match_reference(name):
    meta, d, _ = load_imgonly(name, params=False)
    m = build_model(name, torch.float32, cached=True)
    b = berson._batch_inputs(m, story_inputs(d, device="cuda"))
    sep_before = b["sep_positions"].clone()
    with torch.no_grad():
        visn, Tv = m.bert.encode_visual(b["images"], b["pairs_list"])
        enc = m.encode(**b)
    assert Tv == meta["Tv"] and tuple(visn.shape[:2]) == (d["i::visn_fc"].shape[0], Tv)
    assert torch.equal(b["sep_positions"], sep_before)  # not shifted in place
    assert (sep_before.cpu().numpy() == np.array([0, 1])).all()
    visn = visn.cpu().numpy()
    if "i::rows" in d:
        visn = visn[:, d["i::rows"]]
    np.testing.assert_allclose(visn, d["i::visn_fc"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(enc[0].cpu().numpy(), d["i::final_seq"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(enc[6].cpu().numpy(), d["i::cls_score"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(enc[3].cpu().numpy(), d["i::original_key"], rtol=1e-4, atol=1e-4)


def test_inner_forward_returns_visual_rows_and_pooler():
    """LXRTModel.forward in this mode: ((visn_feats, None), pooler.dense(visn_feats[:, 0]))."""
    meta, d, params = load_imgonly("imgonly_tiny")
    m = build_model("imgonly_tiny", torch.float32, cached=True)
    b = berson._batch_inputs(m, story_inputs(d, device="cuda"))
    P = b["input_ids"].shape[0] * b["input_ids"].shape[1]
    with torch.no_grad():
        (visn, none), pooled = m.bert(b["input_ids"].reshape(P, -1), visual_feats=b["images"],
                                      pairs_list=b["pairs_list"])
    assert none is None
    np.testing.assert_allclose(visn.cpu().numpy(), d["i::visn_fc"], rtol=1e-4, atol=1e-4)
    w, bias = params["bert.pooler.dense.weight"].double(), params["bert.pooler.dense.bias"].double()
    want = torch.tensor(d["i::visn_fc"][:, 0]).double() @ w.t() + bias
    np.testing.assert_allclose(pooled.cpu().numpy(), want.numpy(), rtol=1e-4, atol=1e-4)
