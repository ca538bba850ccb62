"""The 256 x 256 TN weight-gradient kernel through mmseq_gemm_wgrad: dW += dY^T X and
db += colsum(dY) on bf16 inputs, at the smallest shapes where its tile grid, its K split and the
distribution of the bias column sums over the column tiles can go wrong.

Shapes (out x in): 256 x 256 (one tile: every K-tile's column sums belong to the one block of a
split), 264 x 520 (ragged tiles, three column tiles), 768 x 256 and 256 x 768 (K-tile -> column
tile distribution with one and three column tiles), 2304 x 768 (the QKV tile grid, 27 tiles).
K: 128 and 256 (one and two 128-row steps, unsplit: the kernel accumulates into dW itself), 1026 and
4100 (no multiple of 128; 4100 is split four ways), 12416 (eleven splits of 18 K-tiles, the last
of 14, so every split gives every one of three column tiles at least four K-tiles).

Each case runs with the bias gradient, without it, and with no workspace (then the K range is not
split and the first column tile's blocks add the column sums to db directly). The smallest shapes
that split (256 x 256 and 264 x 520 at K = 4100, 264 x 520 at K = 12416) also run with a
workspace of exactly two splits and their bias partial rows, 2 (tn256 M + M N) floats: the planner
then stops in the middle of its fit loop (two splits instead of four or twelve). Reference: float64
dY^T X and column sums of the same bf16 inputs; bound 1e-4 sqrt(K) (1 + max |ref|), as
test_gemm_wgrad_fused_bias. Two consecutive calls must agree bit for bit.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multimodal_sequencing_amd import _native as nat

DEV = "cuda"
KS = (128, 256, 1026, 4100, 12416)
CASES = [(M, N, K) for (M, N) in ((256, 256), (264, 520), (768, 256), (256, 768)) for K in KS]
CASES.append((2304, 768, 4100))


TWO_SPLITS = "two splits"
TWO_SPLIT_CASES = ((256, 256, 4100), (264, 520, 4100), (264, 520, 12416))


def _wgrad(dY, X, gW, gb, workspace):
    """mmseq_gemm_wgrad with the binding's workspace, with none at all, or (TWO_SPLITS) with the
    binding's buffer and workspace_bytes for two splits with their bias partial rows."""
    ws = nat.gemm_workspace(dY.device) if workspace else None
    M, N = gW.shape
    ws_bytes = ws.numel() * 4 if workspace else 0
    if workspace == TWO_SPLITS:
        ws_bytes = 2 * ((N + 255) // 256 * M + M * N) * 4
        assert ws_bytes <= ws.numel() * 4
    nat._check(nat.lib().mmseq_gemm_wgrad(M, N, dY.shape[0], nat._p(dY), M, nat._p(X), N,
                                          nat._p(gW), N, nat._p(gb), nat.dt(dY), nat.GEMM_AUTO,
                                          nat._p(ws), ws_bytes,
                                          nat._stream()), "mmseq_gemm_wgrad")


@pytest.mark.parametrize("M,N,K", CASES)
def test_wgrad_tn(M, N, K):
    g = torch.Generator(device=DEV).manual_seed(M * 3 + N * 5 + K)
    dY = torch.randn(K, M, generator=g, device=DEV).bfloat16()
    X = torch.randn(K, N, generator=g, device=DEV).bfloat16()
    W0 = torch.randn(M, N, generator=g, device=DEV)
    b0 = torch.randn(M, generator=g, device=DEV)
    refW = W0.double() + dY.double().t() @ X.double()
    refb = b0.double() + dY.double().sum(0)
    boundW = 1e-4 * math.sqrt(K) * (1 + refW.abs().max().item())
    boundb = 1e-4 * math.sqrt(K) * (1 + refb.abs().max().item())
    legs = [(True, True), (False, True), (True, False)]
    if (M, N, K) in TWO_SPLIT_CASES:
        legs.append((True, TWO_SPLITS))
    for bias, workspace in legs:
        outs = []
        for _ in range(2):
            gW, gb = W0.clone(), (b0.clone() if bias else None)
            _wgrad(dY, X, gW, gb, workspace)
            outs.append((gW, gb))
        torch.cuda.synchronize()
        tag = f"bias={bias} workspace={workspace}"
        assert torch.equal(outs[0][0], outs[1][0]), tag
        errW = (outs[0][0].double() - refW).abs().max().item()
        print(f"{tag}: errW {errW:.3e} (bound {boundW:.3e})")
        assert errW <= boundW, (tag, errW)
        if bias:
            assert torch.equal(outs[0][1], outs[1][1]), tag
            errb = (outs[0][1].double() - refb).abs().max().item()
            print(f"{tag}: errb {errb:.3e} (bound {boundb:.3e})")
            assert errb <= boundb, (tag, errb)
