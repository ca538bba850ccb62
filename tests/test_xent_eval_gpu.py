"""mmseq_xent_eval (csrc/loss.hip, the forward's kernel instantiated with K >= 0) against the numpy
restatement tests/xent_eval_ref.py and against mmseq_xent_fwd on the same buffer.

  lse, loss_row            torch.equal (as bits) to mmseq_xent_fwd's
  rank, topk_idx, _logit   exactly the restatement's: integers and exact values, no tolerance

A sweep of the 256 threads covers one 16-byte chunk each: 2048 bf16 or 1024 fp32 columns. The
shapes are the smallest that reach each mechanism: fewer columns than a chunk (2, 7), a whole chunk
and one more (8, 9), a ragged single sweep (1005), exactly one bf16 sweep and one column more
(2048, 2049), a third, ragged sweep (4100), and once the real vocabulary (50265).
"""
import math

import numpy as np
import pytest
import torch

from guard_util import Guarded
from xent_eval_ref import check_exact, xent_eval_ref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import native_raw as raw
    from multimodal_sequencing_amd import _native as N

DEV = "cuda"
IGNORE = -100
DTS = [torch.float32, torch.bfloat16]
CODE = {torch.float32: 0, torch.bfloat16: 1}
KS = (0, 1, 5, 8)


def _ld(V, extra=0):
    return (V + 63) // 64 * 64 + extra


def _buffer(data, ld, pad=0.0):
    """[M][ld] device buffer of data's dtype: data in the first V columns, `pad` in the others."""
    M, V = data.shape
    buf = torch.full((M, ld), pad, dtype=data.dtype)
    buf[:, :V] = data
    return buf.to(DEV)


def _exact(data):
    return data.float().double().numpy()


def _labels(M, V, gen):
    lab = torch.randint(0, V, (M,), generator=gen)
    lab[0] = 0
    if M > 1:
        lab[1] = V - 1
    if M > 2:
        lab[2] = IGNORE
    return lab


def _eval(buf, V, labels, k, totals=None, stats=None):
    M = buf.shape[0]
    out = {"lse": torch.empty(M, device=DEV), "loss_row": torch.empty(M, device=DEV),
           "rank": torch.empty(M, dtype=torch.int32, device=DEV),
           "topk_idx": torch.empty(M, k, dtype=torch.int32, device=DEV),
           "topk_logit": torch.empty(M, k, device=DEV)}
    N.xent_eval(buf, V, labels, IGNORE, k, out["lse"], out["loss_row"], out["rank"],
                out["topk_idx"] if k else None, out["topk_logit"] if k else None, totals, stats)
    return out


def _fwd(buf, V, labels):
    M = buf.shape[0]
    lse, row, stats = (torch.empty(n, device=DEV) for n in (M, M, 2))
    N.xent_fwd(buf, V, labels, IGNORE, lse, row, stats)
    return lse, row, stats


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(data, labels, ks=KS, ld=None):
    """One buffer, every k: bit equality with the forward and exactness against the restatement.
    Returns the outputs of the last k."""
    M, V = data.shape
    buf = _buffer(data, _ld(V) if ld is None else ld)
    lab = labels.to(DEV)
    lse, row, stats = _fwd(buf, V, lab)
    x = _exact(data)
    out = None
    for k in ks:
        st = torch.empty(2, device=DEV)
        out = _eval(buf, V, lab, k, stats=st)
        assert torch.equal(_bits(out["lse"]), _bits(lse)), f"lse bits differ from xent_fwd, k={k}"
        assert torch.equal(_bits(out["loss_row"]), _bits(row)), f"loss_row bits differ, k={k}"
        assert torch.equal(_bits(st), _bits(stats)), f"mean / count bits differ, k={k}"
        want = xent_eval_ref(x, V, labels.numpy(), IGNORE, k)
        got = {n: out[n].cpu().numpy() for n in ("rank", "topk_idx", "topk_logit")}
        check_exact(got, want, labels.numpy(), IGNORE, V, k)
        np.testing.assert_allclose(out["lse"].cpu().numpy(), want["lse"], rtol=1e-5, atol=1e-5)
    return out


# -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("V", [2, 7, 8, 9, 1005, 2048, 2049, 4100])
def test_shapes(V, dt):
    for M in (1, 3, 37):
        gen = torch.Generator().manual_seed(1000 * V + M)
        data = (torch.randn(M, V, generator=gen) * 3).to(dt)
        _check(data, _labels(M, V, gen))


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
def test_real_vocabulary_and_a_wider_ld(dt):
    gen = torch.Generator().manual_seed(5)
    data = (torch.randn(3, 50265, generator=gen) * 3).to(dt)
    _check(data, _labels(3, 50265, gen), ks=(5,))
    data = (torch.randn(3, 1005, generator=gen) * 3).to(dt)
    _check(data, _labels(3, 1005, gen), ks=(5,), ld=_ld(1005, 192))


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("V", [9, 2049, 4100])
def test_ties(V, dt):
    """Five distinct values, all exact in bf16: hundreds of columns tie with the maximum and with
    the gold value. Labels at column 0, at V - 1 and inside the runs; the last row holds only
    -0.0 and +0.0."""
    gen = torch.Generator().manual_seed(V)
    levels = torch.tensor([-1.5, -0.25, 0.5, 0.75, 2.0])
    M = 7
    data = levels[torch.randint(0, 5, (M, V), generator=gen)]
    data[M - 1] = torch.where(torch.rand(V, generator=gen) < 0.5, torch.tensor(-0.0),
                              torch.tensor(0.0))
    data[M - 2, V // 3:2 * V // 3] = 2.0  # one long run of the maximum
    labels = torch.tensor([0, V - 1, V // 2, V // 3, 2 * V // 3 - 1, V // 2, V // 2])
    out = _check(data.to(dt), labels)
    # the zeros of either sign tie: the first 8 columns win, whatever their sign
    assert out["topk_idx"][M - 1].tolist() == list(range(8))
    assert int(out["rank"][M - 1]) == V // 2


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
def test_placement_of_the_winners(dt):
    """Where the k largest sit: inside one thread's chunk, spread over the waves, all in the last,
    partial chunk, all in the second sweep."""
    cn = 8 if dt == torch.bfloat16 else 4
    sweep = 256 * cn
    V = 2 * sweep + cn - 1  # a third sweep of one partial chunk (thread 0)
    gen = torch.Generator().manual_seed(11)
    base = torch.rand(4, V, generator=gen)  # in [0, 1): every winner below beats it
    big = 8.0 + torch.arange(8, dtype=torch.float32)
    places = [
        [37 * cn + e % cn + (e // cn) * sweep for e in range(8)],      # one thread's chunks
        [cn * (64 * (e % 4) + 5 * (e // 4)) + 1 for e in range(8)],   # two per wave
        [2 * sweep + e for e in range(cn - 1)],                       # the last, partial chunk
        [sweep + cn * 29 * e + 3 for e in range(8)],                  # the second sweep
    ]
    for r, cols in enumerate(places):
        base[r, cols] = big[torch.randperm(len(cols), generator=gen)]
    labels = torch.tensor([p[0] for p in places])
    for k in (1, cn - 1, 5, 8):
        out = _check(base.to(dt), labels, ks=(k,))
        for r, cols in enumerate(places):
            n = min(k, len(cols))
            assert set(out["topk_idx"][r, :n].tolist()) <= set(cols)


def test_k_larger_than_v():
    data = torch.tensor([[0.5, 0.5], [-1.0, 3.0]], dtype=torch.bfloat16)
    out = _check(data, torch.tensor([1, 0]), ks=(5,))
    assert out["topk_idx"].tolist() == [[0, 1, -1, -1, -1], [1, 0, -1, -1, -1]]
    assert bool(torch.isneginf(out["topk_logit"][:, 2:]).all())
    assert out["rank"].tolist() == [1, 1]


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
def test_rows_without_a_usable_label(dt):
    V = 1005
    gen = torch.Generator().manual_seed(3)
    data = (torch.randn(4, V, generator=gen) * 2).to(dt)
    labels = torch.tensor([IGNORE, -5, V, 17])
    out = _check(data, labels, ks=(0, 5))
    assert out["rank"].tolist()[:3] == [-1, -1, -1] and int(out["rank"][3]) >= 0
    loss = out["loss_row"].cpu()
    assert float(loss[0]) == 0.0 and bool(torch.isnan(loss[1:3]).all()) and float(loss[3]) > 0
    assert bool((out["topk_idx"] >= 0).all()), "top-k is written for every row"


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
def test_padding_columns_change_no_bit(dt):
    V, ld = 1005, _ld(1005, 64)
    gen = torch.Generator().manual_seed(4)
    data = (torch.randn(3, V, generator=gen) * 2).to(dt)
    labels = _labels(3, V, gen).to(DEV)
    outs = []
    for pad in (0.0, float("nan"), float("inf"), 3e38):
        totals = torch.zeros(4, dtype=torch.float64, device=DEV)
        o = _eval(_buffer(data, ld, pad), V, labels, 8, totals)
        outs.append([_bits(o[n]) for n in sorted(o)] + [totals.view(torch.int64)])
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("M,V,k", [(5, 100, 5), (3, 2049, 8), (1, 7, 1)])
def test_guard_bands(M, V, k, dt):
    gen = torch.Generator().manual_seed(M + V)
    data = (torch.randn(M, V, generator=gen) * 2).to(dt)
    labels = _labels(M, V, gen).to(DEV)
    ld = _ld(V)
    logits = Guarded(M, V, ld, dt, DEV).set(data.to(DEV))
    logits.fill_outside(float("nan"))
    g = {"lse": Guarded(1, M, device=DEV), "loss_row": Guarded(1, M, device=DEV),
         "rank": Guarded(1, M, dtype=torch.int32, device=DEV),
         "topk_idx": Guarded(M, k, dtype=torch.int32, device=DEV),
         "topk_logit": Guarded(M, k, device=DEV),
         "totals": Guarded(1, 4, dtype=torch.float64, device=DEV)}
    for b in g.values():
        b.fill_pattern()
    g["totals"].view.zero_()
    for b in g.values():
        b.snapshot()
    raw.call("mmseq_xent_eval", M, V, raw.p(logits.t), ld, raw.p(labels), IGNORE, k,
             raw.p(g["lse"].t), raw.p(g["loss_row"].t), raw.p(g["rank"].t), raw.p(g["topk_idx"].t),
             raw.p(g["topk_logit"].t), raw.p(g["totals"].t), CODE[dt])
    torch.cuda.synchronize()
    for name, b in g.items():
        b.check_untouched(name)
    want = xent_eval_ref(_exact(data), V, labels.cpu().numpy(), IGNORE, k)
    got = {"rank": g["rank"].view.reshape(M).cpu().numpy(),
           "topk_idx": g["topk_idx"].v2.cpu().numpy(), "topk_logit": g["topk_logit"].v2.cpu().numpy()}
    check_exact(got, want, labels.cpu().numpy(), IGNORE, V, k)
    assert g["totals"].view.reshape(4)[1].item() == float((labels != IGNORE).sum())


def test_totals_accumulate_exactly_and_repeat():
    k = 5
    runs = []
    for _ in range(2):
        totals = torch.zeros(4, dtype=torch.float64, device=DEV)
        losses, ranks = [], []
        g2 = torch.Generator().manual_seed(8)
        for M, V in ((37, 1005), (300, 64)):  # 300 rows: more than one row per thread
            data = (torch.randn(M, V, generator=g2) * 2).to(torch.bfloat16)
            labels = _labels(M, V, g2)
            labels[M // 2] = IGNORE
            o = _eval(_buffer(data, _ld(V)), V, labels.to(DEV), k, totals)
            keep = (labels != IGNORE)
            losses += o["loss_row"].cpu()[keep].tolist()
            ranks += o["rank"].cpu()[keep].tolist()
        runs.append(totals.cpu())
        t = totals.tolist()
        assert t[1] == len(losses) and t[2] == sum(r == 0 for r in ranks)
        assert t[3] == sum(0 <= r < k for r in ranks)
        want = math.fsum(losses)  # the fp32 loss_row values, summed exactly
        assert abs(t[0] - want) <= 1e-12 * abs(want)
    assert torch.equal(runs[0].view(torch.int64), runs[1].view(torch.int64))


def test_optional_outputs():
    gen = torch.Generator().manual_seed(2)
    data = (torch.randn(3, 9, generator=gen)).to(torch.bfloat16)
    labels = _labels(3, 9, gen).to(DEV)
    buf = _buffer(data, 64)
    a = _eval(buf, 9, labels, 0)  # k == 0: NULL top-k pointers, totals NULL
    b = _eval(buf, 9, labels, 5, torch.zeros(4, dtype=torch.float64, device=DEV))
    for n in ("lse", "loss_row", "rank"):
        assert torch.equal(_bits(a[n]), _bits(b[n]))


def test_rejections_launch_nothing():
    """k outside [0, 8], an unaligned base and an ld that is no multiple of 16 bytes: the status
    code says so and no output changes (nothing here runs a kernel on such an argument)."""
    M, V, ld = 3, 100, 128
    flat = torch.zeros(M * ld + 8, dtype=torch.bfloat16, device=DEV)
    labels = torch.zeros(M, dtype=torch.int64, device=DEV)
    outs = [torch.full((M,), 7.0, device=DEV), torch.full((M,), 7.0, device=DEV),
            torch.full((M,), 7, dtype=torch.int32, device=DEV),
            torch.full((M, 8), 7, dtype=torch.int32, device=DEV), torch.full((M, 8), 7.0, device=DEV),
            torch.full((4,), 7.0, dtype=torch.float64, device=DEV)]

    def status(ptr, ld_, k):
        return raw.status("mmseq_xent_eval", M, V, ptr, ld_, raw.p(labels), IGNORE, k,
                          *[raw.p(o) for o in outs], 1)

    assert status(raw.p(flat), ld, 9) == raw.EINVAL
    assert status(raw.p(flat), ld, -1) == raw.EINVAL
    assert status(raw.p(flat) + 2, ld, 5) == N.EUNSUPPORTED
    assert status(raw.p(flat), 100 + 2, 5) == N.EUNSUPPORTED  # 204 bytes: no multiple of 16
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == 7).all())
    assert status(raw.p(flat), ld, 8) == 0
    torch.cuda.synchronize()
    assert not bool((outs[2] == 7).any())
    with pytest.raises(ValueError):
        _eval(flat[:M * ld].view(M, ld), V, labels, 9)
