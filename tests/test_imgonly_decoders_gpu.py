"""One image-only encode feeds every decoder (imgonly_tiny, fp32): everything downstream of the
10-tuple `encode` returns runs unchanged on an image-only model."""
import pytest
import torch

from imgonly_util import build_model, load_imgonly, story_inputs

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multimodal_sequencing_amd import berson

DECODES = ["beam", "exact", "mbr_tau", "pairwise", "joint"]


def _setup():
    meta, d, _ = load_imgonly("imgonly_tiny", params=False)
    return meta, d, build_model("imgonly_tiny", torch.float32, cached=True), \
        story_inputs(d, device="cuda")


def test_every_decode_returns_permutations():
    meta, d, m, inputs = _setup()
    B, N = d["labels"].shape
    got, scores = {}, {}
    for decode in DECODES:
        orders = berson.berson_pointer_network_batch(m.args, m, None, inputs, decode=decode)
        assert len(orders) == B, decode
        for o in orders:
            assert sorted(o) == list(range(N)), (decode, o)
        got[decode], scores[decode] = orders, m.last_beam_scores.clone()
    assert got["beam"] == [[int(x) for x in o] for o in d["order"]]
    # the beam order rescored by mmseq_order_score: the two kernels agree within 1e-4 ...
    cand = torch.tensor(got["beam"])[:, None, :]
    rescored = berson.berson_score_orders(m.args, m, None, inputs, cand)[:, 0]
    print("beam", scores["beam"].tolist(), "rescored", rescored.tolist(), "exact",
          scores["exact"].tolist())
    assert float((rescored - scores["beam"]).abs().max()) < 1e-4
    # ... and the optimum over all N! orders is no worse than the beam's order: exactly so under
    # the scorer both go through, and against the beam kernel's own score up to that agreement
    assert bool((scores["exact"] <= rescored).all())
    assert bool((scores["exact"] <= scores["beam"] + 1e-4).all())
    post = berson.berson_order_posterior(m.args, m, None, inputs)
    assert float(post["logz"].abs().max()) < 1e-4
    assert post["map_order"].tolist() == got["exact"]


def test_sequence_loss_without_its_term_is_the_training_loss():
    meta, d, m, inputs = _setup()

    def grads():
        torch.cuda.synchronize()
        return [s.grad.clone() for s in m.stores()]

    m.zero_grad()
    want = m(inputs)[0]
    want.backward()
    g_want = grads()
    m.zero_grad()
    loss, terms = berson.sequence_loss(m.args, m, inputs, seq_lam=0.0, samples=4)
    loss.backward()
    g_got = grads()
    m.zero_grad()
    print(f"model(inputs) {want.item():.6f} sequence_loss {loss.item():.6f}")
    assert abs(loss.item() - want.item()) < 1e-4
    assert abs(want.item() - float(d["loss"])) < 1e-4
    for i, (x, y) in enumerate(zip(g_got, g_want)):
        assert float(y.abs().max()) > 0, i
        torch.testing.assert_close(x, y, rtol=2e-3, atol=1e-5)
