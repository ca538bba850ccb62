"""Image-only ordering in train mode on imgonly_tiny (dropout at visn_fc, the span pool and the
inter-paragraph encoder): with the forward index pinned the loss is a deterministic function of the
weights and the backward is its gradient (central finite difference along the gradient, 2 %, as
test_parity_gpu.test_train_mode_dropout_gradient_is_consistent); two backward passes agree bit
for bit."""
import pytest
import torch

from imgonly_util import build_model, load_imgonly, story_inputs

pytestmark = pytest.mark.gpu


def test_train_mode_dropout_gradient_is_consistent():
    meta, d, _ = load_imgonly("imgonly_tiny", params=False)
    m = build_model("imgonly_tiny", torch.float32)
    m.train()
    inputs = story_inputs(d, device="cuda")

    def loss_at(fwd_index):
        m.bert._n_fwd = fwd_index
        return m(inputs)[0]

    def grads():
        torch.cuda.synchronize()
        return [s.grad.clone() for s in m.stores()]

    m.zero_grad()
    l0 = loss_at(0)
    l0.backward()
    g0 = grads()
    assert abs(l0.item() - float(d["loss"])) > 1e-4  # dropout is active
    m.zero_grad()
    l0b = loss_at(0)
    l0b.backward()
    g0b = grads()
    assert l0b.item() == l0.item()  # the mask is a pure function of (seed, site, element)
    for a, b in zip(g0, g0b):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))  # backward: bit for bit
    assert loss_at(5).item() != l0.item()  # another forward index draws another mask
    named = dict(m.named_parameters())
    gdir = {k: p.grad.detach().clone() for k, p in named.items()}
    gn = sum(float((g.double() ** 2).sum()) for g in gdir.values()) ** 0.5
    eps = 1e-3
    base = {k: p.detach().clone() for k, p in named.items()}
    vals = []
    for sgn in (1, -1):
        with torch.no_grad():
            for k, p in named.items():
                p.copy_(base[k] + sgn * eps * gdir[k] / gn)
        for s in m.stores():
            s.shadow_stale = True
        vals.append(loss_at(0).item())
    fd = (vals[0] - vals[1]) / (2 * eps)
    print(f"train-mode loss {l0.item():.6f} (eval {float(d['loss']):.6f}); |grad| {gn:.6f}, "
          f"finite difference {fd:.6f}")
    assert abs(fd - gn) < 2e-2 * gn, (fd, gn)
