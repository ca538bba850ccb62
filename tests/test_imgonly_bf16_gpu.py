"""Image-only ordering in bf16 (the benchmarked dtype) on imgonly_tiny: loss within 2e-2 relative
of the reference's, per-tensor gradient cosine > 0.98 (test_parity_gpu.py's bf16 bounds). The
visual rows reach the span pool and sentence_tran in bf16; no fp32 copy of them is made."""
import pytest
import torch

from imgonly_util import build_model, load_imgonly, story_inputs

pytestmark = pytest.mark.gpu


def test_bf16_close_to_reference():
    meta, d, _ = load_imgonly("imgonly_tiny", params=False)
    m = build_model("imgonly_tiny", torch.bfloat16, cached=True)
    loss = m(story_inputs(d, device="cuda"))[0]
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
    m.zero_grad()
    ref = float(d["loss"])
    print(f"bf16 loss {loss.item():.6f} ref {ref:.6f}")
    assert abs(loss.item() - ref) < 2e-2 * abs(ref), (loss.item(), ref)
    worst = (1.0, None)
    checked = 0
    for k in d:
        if k.startswith("g::"):
            a = torch.tensor(d[k]).double().flatten()
            b = grads[k[3:]].double().flatten()
            if a.norm() < 1e-6:
                continue
            cos = float(a @ b / (a.norm() * b.norm() + 1e-30))
            worst = min(worst, (cos, k))
            checked += 1
    print(f"worst gradient cosine {worst[0]:.5f} at {worst[1]} over {checked} tensors")
    assert checked > 60
    assert worst[0] > 0.98, worst
    for k in meta["nograd"]:
        assert not bool(grads[k].any()), k


def test_bf16_rows_stay_bf16():
    """The head reads the [P][Tv][H] rows in the compute dtype: the span pool's saved input and the
    gradient it returns are bf16 tensors (a full fp32 copy would be 773 MB at config 3)."""
    from multimodal_sequencing_amd import berson, kernels as K
    meta, d, _ = load_imgonly("imgonly_tiny", params=False)
    m = build_model("imgonly_tiny", torch.bfloat16, cached=True)
    seen = []
    real = K.SpanPoolFn.forward

    def spy(ctx, top, score, sep, drop=None):
        seen.append((top.dtype, tuple(top.shape)))
        return real(ctx, top, score, sep, drop)

    K.SpanPoolFn.forward = staticmethod(spy)
    try:
        with torch.no_grad():
            m.encode(**berson._batch_inputs(m, story_inputs(d, device="cuda")))
    finally:
        K.SpanPoolFn.forward = staticmethod(real)
    P = d["i::visn_fc"].shape[0]
    assert seen == [(torch.bfloat16, (P, meta["Tv"], meta["config"]["joint"]["hidden"]))]
