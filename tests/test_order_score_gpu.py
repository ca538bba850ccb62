"""Scoring candidate orders, n-best and exact decode on the device (csrc/beam.hip
mmseq_order_score / mmseq_beam_search_nbest, berson.score_orders_batch / exact_order_batch /
beam_nbest_batch / berson_score_orders) against the CPU reference and the reference fixtures.

Kernel tests: beam_batch_ref.random_case at SEED = 100; the expected score of a candidate is
beam_batch_ref.order_score (the reference's formulation through the oracle's primitives), the
expected per-step terms come from the host scorer on the CPU stand-in (tests/order_score_ref.py,
which tests/test_order_score.py ties to order_score). Bound: R.bound = 4e-4 * max(1, |score|).
Rank order is compared only across pairs of reference scores farther apart than twice the bound.
"""
import random

import numpy as np
import pytest
import torch

import beam_batch_ref as R
import order_score_ref as S
from guard_util import Guarded
from test_order_gpu import _load, _model, _nll, _picks
from make_golden_real import real_inputs

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multimodal_sequencing_amd import _native as NV
    from multimodal_sequencing_amd import berson

_W_NAMES = ("decoder.weight_ih_l0", "decoder.bias_ih_l0", "decoder.weight_hh_l0",
            "decoder.bias_hh_l0", "query_linear.weight", "query_linear.bias", "pw_k.weight",
            "tanh_linear.weight", "tanh_linear.bias")
_IN_NAMES = ("doc", "okey", "hist", "h0", "c0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _inputs(case):
    return ([case[k].cuda().contiguous() for k in _IN_NAMES],
            [case["p"][n].cuda().contiguous() for n in _W_NAMES])


def _score(case, orders, steps=True, fill=None):
    """One mmseq_order_score -> (nll [B][K], step_nll [B][K][N-1] or None) on the CPU."""
    B, N, H = case["B"], case["N"], case["H"]
    o = torch.as_tensor(orders, dtype=torch.int64).cuda().contiguous()
    K = o.shape[-2]
    dev, wts = _inputs(case)
    nll = torch.full((B, K), float("nan"), device="cuda")
    st = torch.full((B, K, N - 1), float("nan"), device="cuda") if steps else None
    nbytes = NV.order_score_workspace(B, N, H, K)
    assert nbytes > 0 and nbytes % 16 == 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    assert NV.order_score(*dev, wts, o, nll, st, ws) == 0
    torch.cuda.synchronize()
    return nll.cpu(), (st.cpu() if steps else None)


def _random_perms(N, K, seed):
    rng = random.Random(seed)
    return [rng.sample(range(N), N) for _ in range(K)]


def _candidates(N, K):
    if K == "all":
        return None  # all N! in itertools order
    if K == "rep257":
        perms = S.all_perms(N)
        rng = random.Random(R.SEED)
        return [perms[rng.randrange(len(perms))] for _ in range(257)]
    return _random_perms(N, K, R.SEED)


# (B, N, H, K): what each case can break
KERNEL_CASES = [(3, 5, 128, "all"),     # base
                (2, 3, 128, "all"),
                (3, 4, 128, "all"),
                (2, 2, 128, "all"),     # a single step
                (1, 1, 128, "all"),     # nll 0
                (2, 9, 128, 64),        # pointed mask past 8 bits, N no multiple of the 4 waves
                (1, 16, 128, 3),        # the maximum N
                (1, 5, 1024, "all"),    # the models' widths
                (1, 5, 768, "all"),
                (2, 4, 136, "all"),     # H no multiple of 64
                (33, 4, 128, 1),
                (2, 5, 128, "rep257")]  # K aligned to nothing


@pytest.mark.parametrize("shape", KERNEL_CASES, ids=lambda c: "B%d_N%d_H%d_K%s" % c)
def test_kernel_matches_cpu_reference(shape):
    B, N, H, K = shape
    case, cand, want = S.ref_nll(B, N, H, _candidates(N, K))
    nll, steps = _score(case, cand)
    assert nll.shape == want.shape and steps.shape == (B, len(cand), N - 1)
    if N == 1:
        assert nll.tolist() == [[0.0]] * B
        return
    worst = 0.0
    for b in range(B):
        for k in range(len(cand)):
            got, ref = float(nll[b, k]), float(want[b, k])
            worst = max(worst, abs(got - ref) / R.bound(ref))
            assert abs(got - ref) < R.bound(ref), (b, cand[k], got, ref)
    print(f"{shape}: largest |nll - reference| / bound = {worst:.3f}")
    # step_nll: sums to nll, and each step within the bound of the reference's step
    ssum = torch.zeros_like(nll)
    for t in range(N - 1):  # in step order, as the header states
        ssum = ssum + steps[:, :, t]
    assert bool(((ssum - nll).abs() <= 1e-6 * nll.abs()).all()), float((ssum - nll).abs().max())
    ref_steps = S.ref_steps(case, cand)
    for b in range(B):
        for k in range(len(cand)):
            for t in range(N - 1):
                got, ref = float(steps[b, k, t]), float(ref_steps[b, k, t])
                assert abs(got - ref) < R.bound(ref), (b, cand[k], t, got, ref)


def _adjacent(ref_row):
    """Reference order of the candidates and, per adjacent pair, whether it is decided (farther
    apart than twice the bound)."""
    srt = sorted(range(len(ref_row)), key=lambda i: (ref_row[i], i))
    decided = [ref_row[srt[i + 1]] - ref_row[srt[i]] >
               2 * R.bound(max(abs(ref_row[srt[i]]), abs(ref_row[srt[i + 1]])))
               for i in range(len(srt) - 1)]
    return srt, decided


@pytest.mark.parametrize("shape", [(2, 3, 128), (3, 4, 128), (3, 5, 128), (1, 5, 1024)],
                         ids=lambda c: "B%d_N%d_H%d" % c)
def test_rank_order(shape):
    B, N, H = shape
    case, cand, want = S.ref_nll(B, N, H)
    nll, _ = _score(case, cand, steps=False)
    skipped = pairs = 0
    for b in range(B):
        ref_row, got_row = want[b].tolist(), nll[b].tolist()
        srt, decided = _adjacent(ref_row)
        pairs += len(decided)
        skipped += len(decided) - sum(decided)
        if N <= 4:  # no near-ties at this seed: the whole ranking is decided
            assert all(decided), (b, decided)
            assert sorted(range(len(got_row)), key=lambda i: (got_row[i], i)) == srt, b
        for i, dec in enumerate(decided):
            if dec:
                assert got_row[srt[i]] < got_row[srt[i + 1]], (b, cand[srt[i]], cand[srt[i + 1]])
        assert min(range(len(got_row)), key=lambda i: (got_row[i], i)) == srt[0], b
        assert decided[0], (b, "the best margin must be decided")
    print(f"{shape}: {skipped} of {pairs} adjacent pairs closer than twice the bound")
    assert skipped <= 0.10 * pairs, (skipped, pairs)


def test_per_story_candidate_lists_equal_shared_form():
    B, N, H = 3, 5, 128
    case, cand, _ = S.ref_nll(B, N, H)
    shared, sh_steps = _score(case, cand)
    rng = random.Random(7)
    shuf = [rng.sample(range(120), 120) for _ in range(B)]
    assert len({tuple(s) for s in shuf}) == B
    per = [[cand[i] for i in shuf[b]] for b in range(B)]
    nll, steps = _score(case, per)
    for b in range(B):
        back = torch.empty(120, dtype=torch.int64)
        back[torch.tensor(shuf[b])] = torch.arange(120)
        assert torch.equal(_bits(nll[b][back]), _bits(shared[b])), b
        assert torch.equal(_bits(steps[b][back]), _bits(sh_steps[b])), b


def _guarded_call(case, orders, poison):
    """mmseq_order_score with every buffer inside guard bands; the inputs' surroundings hold 0 or
    NaN (int64 orders: 0 or 2^40), the workspace 0 or NaN throughout."""
    B, N, H = case["B"], case["N"], case["H"]
    K = len(orders)
    gin = []
    for name in _IN_NAMES:
        t = case[name]
        gin.append(Guarded(t.numel() // t.shape[-1], t.shape[-1], device="cuda").set(t.cuda()))
    gw = []
    for name in _W_NAMES:
        t = case["p"][name]
        cols = t.shape[-1] if t.dim() > 1 else t.numel()
        gw.append(Guarded(t.numel() // cols, cols, device="cuda").set(t.cuda()))
    for g in gin + gw:
        g.fill_outside(float("nan") if poison else 0.0)
    go = Guarded(K, N, dtype=torch.int64, device="cuda")
    go.buf[~go.inside] = (1 << 40) if poison else 0
    go.set(torch.tensor(orders, dtype=torch.int64).cuda())
    gn = Guarded(B, K, device="cuda").fill_pattern()
    gs = Guarded(B * K, N - 1, device="cuda").fill_pattern()
    nbytes = NV.order_score_workspace(B, N, H, K)
    gws = Guarded(1, nbytes // 4, device="cuda").fill_pattern()
    gws.view.fill_(float("nan") if poison else 0.0)
    for g in (go, gn, gs, gws):
        g.snapshot()
    dev = [g.view.reshape(case[n].shape) for g, n in zip(gin, _IN_NAMES)]
    wts = [g.view.reshape(case["p"][n].shape) for g, n in zip(gw, _W_NAMES)]
    st = NV.order_score(*dev, wts, go.v2, gn.v2, gs.view.reshape(B, K, N - 1), gws.v2.reshape(-1))
    assert st == 0
    torch.cuda.synchronize()
    gn.check_untouched("nll")
    gs.check_untouched("step_nll")
    gws.check_untouched("workspace")
    go.check_untouched("orders", also=torch.ones(1, K, N, dtype=torch.bool, device="cuda"))
    return gn.v2.cpu().clone(), gs.view.reshape(B, K, N - 1).cpu().clone()


def test_invalid_candidates_are_inf_and_touch_nothing_else():
    B, N, H = 2, 5, 128
    case = R.random_case(B, N, H, R.SEED)
    good = _random_perms(N, 8, 3)
    bad = [list(g) for g in good]
    bad[1][0] = -1
    bad[3][2] = N
    bad[4][1] = 1 << 40
    bad[6][3] = bad[6][0]                # a repeat within the first N - 1 entries
    bad[7][4] = bad[7][0]                # a repeat in the LAST entry only: never read, still valid
    invalid = [1, 3, 4, 6]
    clean = [list(g) for g in good]      # the valid ones, the invalid slots holding a valid copy
    for k in invalid:
        clean[k] = list(good[0])
    want, want_steps = _guarded_call(case, clean, poison=False)
    for poison in (False, True):
        nll, steps = _guarded_call(case, bad, poison)
        for k in range(8):
            if k in invalid:
                assert bool(torch.isposinf(nll[:, k]).all()), (k, nll[:, k])
                assert bool(torch.isposinf(steps[:, k]).all()), (k, steps[:, k])
            else:
                assert torch.equal(_bits(nll[:, k]), _bits(want[:, k])), (poison, k)
                assert torch.equal(_bits(steps[:, k]), _bits(want_steps[:, k])), (poison, k)
                assert bool(torch.isfinite(nll[:, k]).all())
    # the copies of candidate 0 planted in the clean call are duplicates: identical bits
    for k in invalid:
        assert torch.equal(_bits(want[:, k]), _bits(want[:, 0]))


def test_duplicates_and_determinism():
    B, N, H = 3, 5, 128
    case = R.random_case(B, N, H, R.SEED)
    cand = _random_perms(N, 37, 5)
    cand[29] = list(cand[2])
    a, sa = _score(case, cand, fill=0)
    assert torch.equal(_bits(a[:, 29]), _bits(a[:, 2])) and torch.equal(_bits(sa[:, 29]), _bits(sa[:, 2]))
    b, sb = _score(case, cand, fill=0xFF)  # every workspace float a NaN
    c, sc = _score(case, cand, fill=0)
    for x, sx in ((b, sb), (c, sc)):
        assert torch.equal(_bits(x), _bits(a)) and torch.equal(_bits(sx), _bits(sa))
    assert bool(torch.isfinite(a).all())


def test_abi_rejects_unsupported_and_bad_buffers():
    B, N, H, K = 2, 5, 128, 4
    case = R.random_case(B, N, H, R.SEED)
    dev, wts = _inputs(case)
    o = torch.tensor(_random_perms(N, K, 1), dtype=torch.int64).cuda()
    nll = torch.full((B, K), -7.0, device="cuda")
    st = torch.full((B, K, 16), -7.0, device="cuda")
    nbytes = NV.order_score_workspace(B, N, H, K)
    assert nbytes > 0
    assert NV.order_score_workspace(B, 17, H, K) == 0 and NV.order_score_workspace(B, N, H, 0) == 0
    assert NV.order_score_workspace(B, N, H, 1 << 22) == 0 and NV.order_score_workspace(B, 0, H, K) == 0
    ws = torch.zeros(nbytes + 16, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0
    L = NV.lib()
    ins = [t.data_ptr() for t in dev + wts]
    stream = torch.cuda.current_stream().cuda_stream

    def call(n=N, k=K, nll_p=nll.data_ptr(), ws_p=ws.data_ptr(), wbytes=nbytes, orders_p=o.data_ptr()):
        return L.mmseq_order_score(B, n, H, k, *ins, orders_p, 0, nll_p, st.data_ptr(), ws_p, wbytes,
                                   stream)

    for kw, want in (({"n": 17}, -2), ({"k": 0}, -2), ({"k": 1 << 22}, -2), ({"n": 0}, -2),
                     ({"nll_p": None}, -1), ({"orders_p": None}, -1), ({"ws_p": None}, -1),
                     ({"wbytes": nbytes - 16}, -1), ({"ws_p": ws.data_ptr() + 4}, -1)):
        assert call(**kw) == want, kw
        assert L.mmseq_last_error().decode().startswith("order_score"), L.mmseq_last_error()
        torch.cuda.synchronize()
        assert bool((nll == -7.0).all()) and bool((st == -7.0).all()) and not bool(ws.any()), kw
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(nll).all()) and bool((nll > 0).all())
    # what the call wrote is the [B][K][N-1] block at the front of st
    assert bool((st.reshape(-1)[B * K * (N - 1):] == -7.0).all())


# ------------------------------------------------------------------------------------- n-best
def _nbest(case, W):
    B, N, H = case["B"], case["N"], case["H"]
    dev, wts = _inputs(case)
    orders = torch.full((B, W, N), -7, dtype=torch.int64, device="cuda")
    scores = torch.full((B, W), -7.0, device="cuda")
    count = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    ws = torch.zeros(NV.beam_workspace(B, N, H, W), dtype=torch.uint8, device="cuda")
    assert NV.beam_search_nbest(*dev, wts, W, orders, scores, count, ws) == 0
    torch.cuda.synchronize()
    return orders.cpu(), scores.cpu(), count.cpu()


def _beam(case, W):
    B, N, H = case["B"], case["N"], case["H"]
    dev, wts = _inputs(case)
    order = torch.full((B, N), -1, dtype=torch.int64, device="cuda")
    score = torch.full((B,), float("nan"), device="cuda")
    ws = torch.zeros(NV.beam_workspace(B, N, H, W), dtype=torch.uint8, device="cuda")
    assert NV.beam_search(*dev, wts, W, order, score, ws) == 0
    torch.cuda.synchronize()
    return order.cpu(), score.cpu()


@pytest.mark.parametrize("shape", [(2, 3, 16, 128), (3, 4, 32, 128)], ids=lambda c: "B%d_N%d_W%d_H%d" % c)
def test_nbest_full_enumeration(shape):
    """The beam is exhaustive: every permutation, in the reference's rank order. For N = 3 the
    last step also selects the three pointed (~1e9) entries; they are not reported."""
    B, N, W, H = shape
    case, perms, want = S.ref_nll(B, N, H)
    orders, scores, count = _nbest(case, W)
    nfact = len(perms)
    assert count.tolist() == [nfact] * B
    for b in range(B):
        srt, decided = _adjacent(want[b].tolist())
        assert all(decided), b
        assert orders[b, :nfact].tolist() == [perms[i] for i in srt], b
        for r, i in enumerate(srt):
            ref = float(want[b, i])
            assert abs(float(scores[b, r]) - ref) < R.bound(ref), (b, r)
        assert bool((orders[b, nfact:] == -7).all()) and bool((scores[b, nfact:] == -7.0).all())


def test_nbest_n5_w16():
    B, N, W, H = 3, 5, 16, 128
    case, perms, want = S.ref_nll(B, N, H)
    index = {tuple(p): i for i, p in enumerate(perms)}
    orders, scores, count = _nbest(case, W)
    o1, s1 = _beam(case, W)
    for b in range(B):
        n = int(count[b])
        assert 1 <= n <= W
        assert orders[b, 0].tolist() == o1[b].tolist()
        assert torch.equal(_bits(scores[b, :1]), _bits(s1[b:b + 1]))
        got = [tuple(o) for o in orders[b, :n].tolist()]
        assert len(set(got)) == n and all(sorted(o) == list(range(N)) for o in got), (b, got)
        sc = scores[b, :n].tolist()
        assert sc == sorted(sc), (b, sc)
        for r in range(n):
            ref = float(want[b, index[got[r]]])
            assert abs(sc[r] - ref) < R.bound(ref), (b, r, sc[r], ref)
        assert bool((orders[b, n:] == -7).all()) and bool((scores[b, n:] == -7.0).all())


def test_nbest_edges():
    c = R.random_case(3, 1, 128, R.SEED)           # N = 1
    orders, scores, count = _nbest(c, 16)
    assert count.tolist() == [1] * 3 and orders[:, 0, 0].tolist() == [0] * 3
    assert scores[:, 0].tolist() == [0.0] * 3 and bool((scores[:, 1:] == -7.0).all())
    case, perms, want = S.ref_nll(2, 2, 128)       # N = 2: one step, both orders
    orders, scores, count = _nbest(case, 16)
    o1, s1 = _beam(case, 16)
    assert count.tolist() == [2, 2]
    for b in range(2):
        srt = sorted(range(2), key=lambda i: float(want[b, i]))
        assert orders[b, :2].tolist() == [perms[i] for i in srt]
        assert orders[b, 0].tolist() == o1[b].tolist()
        assert torch.equal(_bits(scores[b, :1]), _bits(s1[b:b + 1]))
        for r, i in enumerate(srt):
            assert abs(float(scores[b, r]) - float(want[b, i])) < R.bound(float(want[b, i]))
        assert bool((orders[b, 2:] == -7).all())
    c = R.random_case(2, 5, 128, R.SEED)           # W = 1: greedy, one hypothesis
    orders, scores, count = _nbest(c, 1)
    o1, s1 = _beam(c, 1)
    assert count.tolist() == [1, 1] and orders[:, 0].tolist() == o1.tolist()
    assert torch.equal(_bits(scores[:, 0]), _bits(s1))


def test_beam_search_unchanged_around_the_new_entries():
    B, N, W, H = 3, 5, 16, 128
    case, perms, _ = S.ref_nll(B, N, H)
    o0, s0 = _beam(case, W)
    _nbest(case, W)
    _score(case, perms)
    o1, s1 = _beam(case, W)
    assert torch.equal(o0, o1) and torch.equal(_bits(s0), _bits(s1))
    host_orders, host_scores, _, _ = R.beam_batch_host(case, W)
    assert o0.tolist() == host_orders
    for b in range(B):
        assert abs(float(s0[b]) - host_scores[b]) < R.bound(host_scores[b])


# ------------------------------------------------------- end to end on the reference's fixture
_E2E = {}


def _e2e(dtype):
    if dtype not in _E2E:
        meta, d = _load("decisive_tiny")
        m = _model("decisive_tiny", meta, dtype)
        ids, labels, images = real_inputs(meta["input_seed"], meta["config"])
        inputs = {"input_ids": torch.from_numpy(ids), "labels": torch.from_numpy(labels),
                  "images": torch.from_numpy(images).cuda()}
        _E2E[dtype] = (m, d, inputs)
    return _E2E[dtype]


def _fix_bound(want):
    return 4e-4 * max(1.0, abs(want))


def test_end_to_end_all_orders_fp32():
    m, d, inputs = _e2e(torch.float32)
    B = d["perm_nll"].shape[0]
    assert B == 4 and d["perms"].shape == (120, 5)
    calls = []
    enc0 = m.encode
    m.encode = lambda *a, **k: (calls.append(1), enc0(*a, **k))[1]
    try:
        nll = berson.berson_score_orders(m.args, m, None, inputs, d["perms"])
    finally:
        del m.encode
    assert len(calls) == 1 and nll.is_cuda and tuple(nll.shape) == (B, 120)
    nll = nll.cpu()
    worst = 0.0
    for b in range(B):
        for k in range(120):
            want = float(d["perm_nll"][b, k])
            worst = max(worst, abs(float(nll[b, k]) - want) / _fix_bound(want))
            assert abs(float(nll[b, k]) - want) < _fix_bound(want), (b, k, float(nll[b, k]), want)
    print(f"decisive_tiny: 480 NLLs, largest error / bound {worst:.3f}")


def test_end_to_end_exact_decode_fp32():
    m, d, inputs = _e2e(torch.float32)
    ref_orders = [[int(x) for x in o] for o in d["order"]]
    with torch.no_grad():
        enc = m.encode(**berson._batch_inputs(m, inputs))
        order, score, margin = berson.exact_order_batch(m.args, m, enc)
        assert order.tolist() == ref_orders
        for b in range(len(ref_orders)):
            srt = np.sort(d["perm_nll"][b])
            want = float(srt[1] - srt[0])
            assert abs(float(margin[b]) - want) < 2 * _fix_bound(float(srt[1])), (b, float(margin[b]), want)
            assert abs(float(score[b]) - float(srt[0])) < _fix_bound(float(srt[0]))
        # the beam's own score of its order against the scorer's: same kernels, other GEMM rows
        beam_order, beam_score = berson.beam_decode_batch(m.args, m, enc)
        nll = berson.score_orders_batch(m.args, m, enc, beam_order[:, None, :])[:, 0]
        diff = (beam_score - nll).abs().cpu()
        print(f"beam score vs scorer on the beam's order: largest difference {float(diff.max()):.3e}")
        for b in range(len(ref_orders)):
            assert float(diff[b]) < R.bound(float(nll[b])), (b, float(diff[b]))
    got = berson.berson_pointer_network_batch(m.args, m, None, inputs, decode="exact")
    assert got == ref_orders
    assert torch.equal(_bits(m.last_beam_scores), _bits(score))
    assert berson.berson_pointer_network_batch(m.args, m, None, inputs) == ref_orders
    with pytest.raises(ValueError):
        berson.berson_pointer_network_batch(m.args, m, None, inputs, decode="greedy")


def test_end_to_end_nbest_fp32():
    m, d, inputs = _e2e(torch.float32)
    with torch.no_grad():
        enc = m.encode(**berson._batch_inputs(m, inputs))
        orders, scores, count = berson.beam_nbest_batch(m.args, m, enc)
        beam_order, beam_score = berson.beam_decode_batch(m.args, m, enc)
    assert torch.equal(orders[:, 0], beam_order) and torch.equal(_bits(scores[:, 0]), _bits(beam_score))
    index = {tuple(int(x) for x in p): i for i, p in enumerate(d["perms"])}
    for b in range(orders.shape[0]):
        n = int(count[b])
        assert 1 <= n <= orders.shape[1]
        for r in range(n):
            want = float(d["perm_nll"][b, index[tuple(orders[b, r].tolist())]])
            assert abs(float(scores[b, r]) - want) < _fix_bound(want), (b, r)
        assert bool((orders[b, n:] == -1).all()) and bool(torch.isposinf(scores[b, n:]).all())


def test_end_to_end_three_scorers_bf16():
    m, d, inputs = _e2e(torch.bfloat16)
    with torch.no_grad():
        enc = m.encode(**berson._batch_inputs(m, inputs))
    for b in range(4):
        picks = _picks(d["perm_nll"][b])
        cand = [[int(x) for x in d["perms"][j]] for j in picks]
        with torch.no_grad():
            dev = berson.score_orders_batch(m.args, m, enc, cand)[b].cpu()
            host = berson.score_orders_host(m.args, m, enc, cand)[b].cpu()
        one = {k: v[b:b + 1] for k, v in inputs.items()}
        for i, o in enumerate(cand):
            full = _nll(m, one, o)
            print(f"story {b} {o}: device {float(dev[i]):.6f} host {float(host[i]):.6f} forward {full:.6f}")
            assert abs(float(dev[i]) - float(host[i])) < R.bound(float(host[i])), (b, o)
            assert abs(float(dev[i]) - full) < R.bound(full), (b, o)
            assert abs(float(host[i]) - full) < R.bound(full), (b, o)
