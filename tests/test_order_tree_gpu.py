"""All N! pointer scores from the prefix tree on the device (csrc/beam.hip mmseq_order_tree,
berson.enumerate_orders_batch / exact_order_batch(method="tree") / order_posterior_batch(
source="tree") / berson_pointer_network_batch(enumeration="tree")).

Inputs: beam_batch_ref.random_case at SEED = 100. References: the float64 walker of exactly this
tree (order_posterior_ref.step_rows64 / nll64, whole tree up to N = 7) and the flat device scorer
(mmseq_order_score). Bound throughout: R.bound = 4e-4 * max(1, |x|).

Figures of one run on an MI355X: largest difference from float64 3.5e-6 (0.001 of the bound, at
(1,7,16)); tree and flat scorer bit-identical on all four shapes and on decisive_tiny, as were the
three chunk schedules among themselves (printed, not asserted: it holds only where the GEMM's rows
do not depend on its row count); N = 9: logsumexp(-nll) = -2.7e-8 against an allowance of 6.8e-3,
the arg-min was the beam's order. The whole file took 5 s.
"""
import math
import random

import numpy as np
import pytest
import torch

import beam_batch_ref as R
import order_posterior_ref as P
from guard_util import Guarded
from test_order_posterior import case_rows
from test_order_posterior_gpu import _Stub, _same, _stub_enc
from test_order_score_gpu import _bits, _e2e, _fix_bound, _inputs, _score

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multimodal_sequencing_amd import _native as NV
    from multimodal_sequencing_amd import berson

OK, EINVAL, EUNSUPPORTED = 0, -1, -2


def _unchunked(B, N):
    return max(B * N, B * math.factorial(N) // 2)


def _tree(case, rows=None, orders=True, fill=None):
    """One mmseq_order_tree -> (nll [B][N!], orders [N!][N] or None) on the CPU. `fill`: what the
    workspace holds on entry."""
    B, N, H = case["B"], case["N"], case["H"]
    K = math.factorial(N)
    rows = _unchunked(B, N) if rows is None else rows
    dev, wts = _inputs(case)
    nll = torch.full((B, K), float("nan"), device="cuda")
    o = torch.full((K, N), -7, dtype=torch.int64, device="cuda") if orders else None
    nbytes = NV.order_tree_workspace(B, N, H, rows)
    assert nbytes > 0 and nbytes % 16 == 0
    ws = torch.zeros(nbytes // 4, dtype=torch.float32, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    assert NV.order_tree(*dev, wts, rows, nll, o, ws) == OK
    torch.cuda.synchronize()
    return nll.cpu(), (o.cpu() if orders else None)


_REF64 = {}


def _ref64(B, N, H):
    """(case, float64 NLLs [B][N!]) of the whole tree, once per shape; H = 16 shares the CPU
    tests' cache."""
    if (B, N, H) not in _REF64:
        if H == 16:
            case, _rows, _perms, nll = case_rows(B, N)
        else:
            case = R.random_case(B, N, H, R.SEED)
            c64 = P.case64(case)
            perms = P.all_perms(N)
            nll = np.stack([P.nll64(P.step_rows64(c64, b), perms) for b in range(B)])
        _REF64[(B, N, H)] = (case, nll)
    return _REF64[(B, N, H)]


def _within(got, want, what):
    """Every entry of got within R.bound of want (numpy [B][K]); -> largest error / bound."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    ratio = np.abs(got - want) / (R.BOUND * np.maximum(1.0, np.abs(want)))
    worst = float(ratio.max(initial=0.0))
    print(f"{what}: largest |difference| {float(np.abs(got - want).max(initial=0.0)):.3e}, "
          f"largest difference / bound {worst:.3f}")
    assert worst < 1.0, (what, np.unravel_index(int(ratio.argmax()), ratio.shape), worst)
    return worst


# ------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("shape", [(1, 1, 16), (2, 2, 128), (2, 3, 128), (3, 5, 128), (1, 7, 16)],
                         ids=lambda c: "B%d_N%d_H%d" % c)
def test_every_order_against_float64(shape):
    B, N, H = shape
    case, want = _ref64(B, N, H)
    nll, orders = _tree(case)
    assert np.array_equal(orders.numpy(), P.all_perms(N))
    if N == 1:
        assert nll.tolist() == [[0.0]] * B
        return
    _within(nll.numpy(), want, f"tree vs float64 {shape}")


# ---------------------------------------------------------------------- against the flat scorer
@pytest.mark.parametrize("shape", [(3, 5, 128), (2, 6, 130), (1, 4, 1024), (2, 8, 16)],
                         ids=lambda c: "B%d_N%d_H%d" % c)
def test_every_order_against_the_flat_scorer(shape):
    B, N, H = shape
    case = R.random_case(B, N, H, R.SEED)
    nll, orders = _tree(case)
    perms = P.all_perms(N)
    assert np.array_equal(orders.numpy(), perms)
    flat = _score(case, perms, steps=False)[0]
    _within(nll.numpy(), flat.numpy(), f"tree vs mmseq_order_score {shape}")
    print(f"{shape}: bit-identical to the flat scorer: {bool(torch.equal(_bits(nll), _bits(flat)))}")


# ----------------------------------------------------------------------------------------- N = 9
def test_n9_all_362880_orders():
    B, N, H = 1, 9, 16
    case = R.random_case(B, N, H, R.SEED)
    rows = 8192  # the four widest levels go in chunks
    nll, orders = _tree(case, rows=rows)
    assert tuple(nll.shape) == (1, 362880) and bool(torch.isfinite(nll).all())
    o = orders.numpy()
    assert o[0].tolist() == list(range(9)) and o[-1].tolist() == list(range(9))[::-1]
    assert (np.sort(o, -1) == np.arange(9)).all() and (np.diff(_rank_keys(o)) > 0).all()
    # the pointer decoder is a distribution over the orders: logsumexp(-nll) = 0 within the
    # allowance of tests/test_order_posterior_gpu.py for logz, 2 sum_k p_k expm1(bound(nll_k)),
    # p taken from the scores themselves (no float64 walk of this tree exists at N = 9)
    v = nll[0].numpy().astype(np.float64)
    m = v.min()
    logz = float(np.log(np.exp(m - v).sum()) - m)
    p = np.exp(-v - logz)
    allow = 2.0 * float((p * np.expm1(R.BOUND * np.maximum(1.0, np.abs(v)))).sum())
    print(f"N = 9: logsumexp(-nll) = {logz:.3e}, allowance {allow:.3e}")
    assert abs(logz) <= allow
    # 64 seeded orders, the beam's own and the arg-min against the flat scorer
    dev, wts = _inputs(case)
    border = torch.empty(B, N, dtype=torch.int64, device="cuda")
    bscore = torch.empty(B, dtype=torch.float32, device="cuda")
    ws = torch.zeros(NV.beam_workspace(B, N, H, 16) // 4, device="cuda")
    assert NV.beam_search(*dev, wts, 16, border, bscore, ws) == OK
    rng = random.Random(R.SEED)
    best = int(nll[0].argmin())
    cand = [rng.sample(range(N), N) for _ in range(64)] + [border[0].tolist(), o[best].tolist()]
    index = {tuple(r): k for k, r in enumerate(o.tolist())}
    flat = _score(case, cand, steps=False)[0][0]
    got = np.array([float(nll[0, index[tuple(c)]]) for c in cand])
    _within(got[None], flat.numpy()[None], "N = 9: 64 orders, the beam's and the arg-min")
    beam = float(bscore[0])
    print(f"N = 9: min nll {float(nll[0, best]):.6f} at {o[best].tolist()}, beam {beam:.6f} at "
          f"{border[0].tolist()}")
    assert float(nll[0, best]) <= beam + R.bound(beam)
    assert abs(float(flat[-1]) - float(nll[0, best])) < R.bound(float(flat[-1]))


def _rank_keys(o):
    """Orders [K][N] as base-N integers: ascending iff the table is lexicographic."""
    N = o.shape[1]
    return (o * (N ** np.arange(N - 1, -1, -1, dtype=np.int64))).sum(-1)


# -------------------------------------------------------------------------------------- chunking
@pytest.mark.parametrize("shape,prime", [((3, 5, 128), 23), ((2, 7, 16), 47)],
                         ids=["B3_N5_H128", "B2_N7_H16"])
def test_chunked_walks_agree(shape, prime):
    """rows at the minimum B * N, at a prime whose share per story (23 // 3 = 7, 47 // 2 = 23) is
    a prime that divides no level width, and unchunked."""
    B, N, H = shape
    case = R.random_case(B, N, H, R.SEED)
    per = prime // B
    assert all(math.factorial(N) // math.factorial(N - t) % per for t in range(1, N))
    runs = []
    for rows in (B * N, prime, _unchunked(B, N)):
        a, oa = _tree(case, rows=rows)
        b, ob = _tree(case, rows=rows, fill=float("nan"))
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(oa, ob), rows
        assert np.array_equal(oa.numpy(), P.all_perms(N))
        runs.append(a.numpy())
    for i, j in ((0, 1), (0, 2), (1, 2)):
        _within(runs[i], runs[j], f"{shape} schedules {i} and {j}")
        print(f"{shape} schedules {i} and {j} bit-identical: {np.array_equal(runs[i], runs[j])}")


# --------------------------------------------------------------------------------------- hygiene
def _raw(case, N_arg, rows, nll, orders, ws, ws_bytes=None):
    B, _N, H = case["B"], case["N"], case["H"]
    dev, wts = _inputs(case)
    ptrs = [t.data_ptr() for t in dev + wts]
    st = NV.lib().mmseq_order_tree(B, N_arg, H, *ptrs, rows,
                                   None if nll is None else nll.data_ptr(),
                                   None if orders is None else orders.data_ptr(), ws.data_ptr(),
                                   ws.numel() * 4 if ws_bytes is None else ws_bytes, NV._stream())
    torch.cuda.synchronize()
    return st, dev, wts


def test_hygiene_guards_workspace_and_status():
    B, N, H = 3, 5, 128
    K = 120
    case = R.random_case(B, N, H, R.SEED)
    dev, wts = _inputs(case)
    rows = 23
    nbytes = NV.order_tree_workspace(B, N, H, rows)
    assert nbytes > 0 and NV.order_tree_workspace(B, N, H, B * N - 1) == 0
    assert NV.order_tree_workspace(B, 0, H, rows) == 0 and NV.order_tree_workspace(B, 10, H, 999) == 0
    # the workspace is a function of (B, N, H, rows)
    assert NV.order_tree_workspace(B, N, H, rows) == nbytes != NV.order_tree_workspace(B, N, H, 24)
    outs = []
    for fill, with_orders in ((0.0, True), (float("nan"), True), (float("nan"), False)):
        gn = Guarded(B, K, dtype=torch.float32, device="cuda").fill_pattern().snapshot()
        go = Guarded(K, N, dtype=torch.int64, device="cuda").fill_pattern().snapshot()
        gw = Guarded(1, nbytes // 4, dtype=torch.float32, device="cuda").fill_pattern()
        gw.view.fill_(fill)
        gw.snapshot()
        assert NV.order_tree(*dev, wts, rows, gn.view[0], go.view[0] if with_orders else None,
                             gw.view[0, 0]) == OK
        torch.cuda.synchronize()
        gn.check_untouched("order_tree nll")
        go.check_untouched("order_tree orders")
        gw.check_untouched("order_tree workspace")
        if not with_orders:  # NULL orders: the table is left alone altogether
            assert torch.equal(go.ibuf, go._snap)
        outs.append((gn.view[0].clone(), go.view[0].clone()))
    assert bool(torch.isfinite(outs[0][0]).all())
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])), "NaN in the workspace reached nll"
    assert torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(_bits(outs[1][0]), _bits(outs[2][0])), "orders = NULL changed nll"
    assert np.array_equal(outs[0][1].cpu().numpy(), P.all_perms(N))

    # status codes, nothing launched: the outputs keep every bit of their pattern
    gn = Guarded(B, K, dtype=torch.float32, device="cuda").fill_pattern().snapshot()
    go = Guarded(K, N, dtype=torch.int64, device="cuda").fill_pattern().snapshot()
    ws = torch.zeros(nbytes // 4, dtype=torch.float32, device="cuda")
    nll, orders = gn.view[0], go.view[0]
    assert _raw(case, 0, rows, nll, orders, ws)[0] == EUNSUPPORTED
    assert _raw(case, 10, 10 * B, nll, orders, ws)[0] == EUNSUPPORTED
    assert _raw(case, N, B * N - 1, nll, orders, ws)[0] == EINVAL
    assert _raw(case, N, rows, nll, orders, ws, ws_bytes=nbytes - 16)[0] == EINVAL
    assert _raw(case, N, rows, None, orders, ws)[0] == EINVAL
    assert torch.equal(gn.ibuf, gn._snap) and torch.equal(go.ibuf, go._snap)
    assert bool((ws == 0).all())


# --------------------------------------------------------------------------------------- surface
def test_surface_on_the_fixture():
    m, d, inputs = _e2e(torch.float32)
    ref_orders = [[int(x) for x in o] for o in d["order"]]
    beam0 = berson.berson_pointer_network_batch(m.args, m, None, inputs)
    beam_s0 = m.last_beam_scores.clone()
    exact0 = berson.berson_pointer_network_batch(m.args, m, None, inputs, decode="exact")
    exact_s0 = m.last_beam_scores.clone()

    with torch.no_grad():
        enc = m.encode(**berson._batch_inputs(m, inputs))
    order, score, margin = berson.exact_order_batch(m.args, m, enc, method="tree")
    assert order.tolist() == ref_orders
    nll, perms = berson.enumerate_orders_batch(m.args, m, enc, return_orders=True)
    assert perms.cpu().numpy().tolist() == d["perms"].astype(np.int64).tolist()
    assert torch.equal(berson.enumerate_orders_batch(m.args, m, enc), nll)  # cached workspace
    worst = 0.0
    for b in range(nll.shape[0]):
        for k in range(nll.shape[1]):
            want = float(d["perm_nll"][b, k])
            worst = max(worst, abs(float(nll[b, k]) - want) / _fix_bound(want))
            assert abs(float(nll[b, k]) - want) < _fix_bound(want), (b, k)
    print(f"decisive_tiny through the tree: largest error / bound {worst:.3f}")
    assert torch.equal(_bits(score), _bits(nll.min(1).values))
    got = berson.berson_pointer_network_batch(m.args, m, None, inputs, decode="exact",
                                              enumeration="tree")
    assert got == ref_orders and torch.equal(_bits(m.last_beam_scores), _bits(score))

    # source="tree" against source="exact" at N = 5
    tree = berson.order_posterior_batch(m.args, m, enc, source="tree")
    flat = berson.order_posterior_batch(m.args, m, enc, source="exact")
    assert torch.equal(tree["orders"], flat["orders"])
    print("decisive_tiny: tree and flat nll bit-identical:",
          bool(torch.equal(_bits(tree["nll"]), _bits(flat["nll"]))),
          f"largest difference {float((tree['nll'] - flat['nll']).abs().max()):.3e}")
    ref = np.asarray(d["perm_nll"], np.float64)
    for b in range(ref.shape[0]):
        srt = np.sort(ref[b])
        tie = srt[1] - srt[0] < 2 * _fix_bound(float(srt[1]))
        for k in P.INT_OUT:
            assert tie or int(tree[k][b]) == int(flat[k][b]), (b, k)
        for k in P.F32_OUT:
            err = float((tree[k][b] - flat[k][b]).abs().max())
            assert err <= 1e-6, (b, k, err)
    via_args = berson.berson_pointer_network_batch(
        _with(m.args, order_enumeration="tree"), m, None, inputs, decode="mbr_acc")
    assert via_args == tree["mbr_acc_order"].tolist()

    # the defaults: bit for bit what they were before the new calls ran on this model
    assert berson.berson_pointer_network_batch(m.args, m, None, inputs) == beam0
    assert torch.equal(_bits(m.last_beam_scores), _bits(beam_s0))
    assert berson.berson_pointer_network_batch(m.args, m, None, inputs, decode="exact") == exact0
    assert torch.equal(_bits(m.last_beam_scores), _bits(exact_s0))


def _with(args, **kw):
    import argparse
    out = argparse.Namespace(**vars(args))
    for k, v in kw.items():
        setattr(out, k, v)
    return out


def test_tree_source_at_n8_is_the_reduction_of_its_own_scores():
    case = R.random_case(1, 8, 16, R.SEED)
    model, enc = _Stub(case), _stub_enc(case)
    post = berson.order_posterior_batch(None, model, enc, source="tree")
    assert tuple(post["nll"].shape) == (1, 40320) and tuple(post["orders"].shape) == (40320, 8)
    perms = post["orders"].cpu().numpy()
    assert np.array_equal(perms, P.all_perms(8))
    want = P.posterior_ref(perms, post["nll"].cpu().numpy(), 0)
    _same({k: post[k].cpu().numpy() for k in P.F32_OUT + P.INT_OUT}, want, "N=8 tree")
    for name in ("map", "mbr_acc", "mbr_tau"):
        assert post[name + "_order"][0].tolist() == perms[int(post[name + "_index"][0])].tolist()
    with pytest.raises(ValueError, match="exceeds 7"):  # the default source is what it was
        berson.order_posterior_batch(None, model, enc)


def test_decodes_enumerate_through_the_tree_at_n9(monkeypatch):
    import argparse
    case = R.random_case(1, 9, 16, R.SEED)
    model, enc = _Stub(case), _stub_enc(case)
    model.encode = lambda **kw: enc
    model.n_steps, model.device_ = 9, torch.device("cuda")
    monkeypatch.setattr(berson, "_batch_inputs", lambda mdl, inputs: {})
    args = argparse.Namespace(mbr_samples=40, mbr_seed=12)
    want = berson.order_posterior_batch(args, model, enc, source="tree")
    assert tuple(want["nll"].shape) == (1, 362880)
    got = berson.berson_pointer_network_batch(args, model, None, {}, decode="exact",
                                              enumeration="tree")
    assert got == want["map_order"].tolist() and sorted(got[0]) == list(range(9))
    assert torch.equal(_bits(model.last_beam_scores), _bits(want["nll"].min(1).values))
    got = berson.berson_pointer_network_batch(args, model, None, {}, decode="mbr_tau",
                                              enumeration="tree")
    assert got == want["mbr_tau_order"].tolist() and sorted(got[0]) == list(range(9))
    # without the argument the same call samples, and "exact" refuses, as before
    smp = berson.order_posterior_batch(args, model, enc, source="sample", samples=40, seed=12)
    assert berson.berson_pointer_network_batch(args, model, None, {}, decode="mbr_tau") == \
        smp["mbr_tau_order"].tolist()
    with pytest.raises(ValueError, match="exceeds 7"):
        berson.berson_pointer_network_batch(args, model, None, {}, decode="exact")
