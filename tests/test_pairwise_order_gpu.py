"""Decoding from the pairwise head on the device (csrc/pairwise.hip mmseq_pairwise_order /
mmseq_pairwise_score, berson.pairwise_weights / pairwise_order_batch / pairwise_score_orders /
joint_order_batch / berson_pointer_network_batch(decode="pairwise" | "joint")) against the float64
restatement (tests/pairwise_order_ref.py) on the SAME f32 weights.

Tolerances. The max path (order, pnll, margin, the scorer's pnll) is f64 additions of f32 values
in a stated order and comparisons: equal to the restatement bit for bit. The distribution adds
f64 exp / log, where the device's and numpy's may differ in the last f64 place (~1e-16 relative,
~1e-12 after 2^N terms): position and before (<= 1) within 1e-6 absolute, the bound of
tests/test_order_posterior_gpu.py for the same quantities; logz and entropy can then differ in the
final rounding to f32 alone: two f32 spacings of the expected value, floor 2.4e-7 (two spacings
at 1.0, for values near 0).
"""
import numpy as np
import pytest
import torch

import beam_batch_ref as R
import pairwise_order_ref as PW
from guard_util import Guarded
from test_order_score_gpu import _bits, _e2e

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multimodal_sequencing_amd import _native as NV
    from multimodal_sequencing_amd import berson

SEED = 100
SENTINEL = 7


# ------------------------------------------------------------------------------ helpers
_REF = {}


def _ref(kind, N, seed):
    """(w f32 [N][N], the restatement's outputs for it), computed once per (kind, N, seed)."""
    key = (kind, N, seed)
    if key not in _REF:
        w = PW.random_weights(N, seed) if kind == "random" else PW.dyadic_weights(N, seed)
        w.setflags(write=False)
        _REF[key] = (w, PW.pairwise_order_ref(w))
    return _REF[key]


def _stack(refs):
    return np.stack([w for w, _ in refs]), {k: np.stack([r[k] for _, r in refs])
                                            for k in refs[0][1]}


def _order(w, what="pairwise_order"):
    """One mmseq_pairwise_order into guarded outputs and a guarded, NaN-filled workspace -> dict of
    CPU numpy arrays."""
    wt = torch.as_tensor(np.asarray(w, np.float32)).cuda().contiguous()
    B, N = wt.shape[0], wt.shape[1]
    guards, out = {}, {}
    for name, dtype, nn in NV.PAIRWISE_OUTPUTS:
        g = Guarded(B, N ** nn, dtype=dtype, device="cuda").fill_pattern().snapshot()
        guards[name] = g
        out[name] = g.view[0].view((B,) + (N,) * nn)
    nbytes = NV.pairwise_order_workspace(B, N)
    assert nbytes > 0 and nbytes % 16 == 0
    gw = Guarded(1, nbytes // 4, dtype=torch.float32, device="cuda")
    gw.buf.fill_(float("nan"))
    gw.snapshot()
    assert NV.pairwise_order(wt, out, gw.view[0, 0]) == 0
    torch.cuda.synchronize()
    for name, g in guards.items():
        g.check_untouched(f"{what} {name}")
    gw.check_untouched(f"{what} workspace")
    return {k: t.cpu().numpy().copy() for k, t in out.items()}


def _spacing_tol(want):
    return np.maximum(2 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64), 2.4e-7)


def _f32bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(got, want, what):
    assert got["order"].tolist() == want["order"].tolist(), (what, got["order"], want["order"])
    for k in ("pnll", "margin"):
        assert np.array_equal(_f32bits(got[k]), _f32bits(want[k])), (what, k, got[k], want[k])
    for k in ("position", "before"):
        err = np.abs(got[k].astype(np.float64) - want[k].astype(np.float64)).max(initial=0.0)
        assert err <= 1e-6, (what, k, err)
    for k in ("logz", "entropy"):
        a, b = got[k].astype(np.float64), want[k].astype(np.float64)
        inf = np.isinf(b)
        assert np.array_equal(np.isinf(a), inf) and np.array_equal(a[inf], b[inf]), (what, k)
        assert (np.abs(a[~inf] - b[~inf]) <= _spacing_tol(b[~inf])).all(), (what, k, a, b)


def _same_bits(a, b, what):
    for k in a:
        x = a[k] if k == "order" else _f32bits(a[k])
        y = b[k] if k == "order" else _f32bits(b[k])
        assert np.array_equal(x, y), (what, k)


# ------------------------------------------------------------------------------ pairwise_order
ORDER_SHAPES = [(1, 1), (1, 2), (3, 3), (2, 5), (1, 7), (2, 9), (1, 12)]


@pytest.mark.parametrize("shape", ORDER_SHAPES, ids=lambda c: "B%d_N%d" % c)
def test_order_matches_restatement(shape):
    B, N = shape
    w, want = _stack([_ref("random", N, SEED + 17 * b + N) for b in range(B)])
    got = _order(w)
    _same(got, want, shape)
    assert np.abs(got["position"].sum(1) - 1).max() < 1e-5
    assert np.abs(got["position"].sum(2) - 1).max() < 1e-5
    again = _order(w)
    _same_bits(got, again, "two calls")
    if B > 1:  # story 0 alone: the same bits as in company
        alone = _order(w[:1])
        _same_bits(alone, {k: v[:1] for k, v in got.items()}, "story 0 alone")


@pytest.mark.parametrize("shape", [(3, 3), (3, 5), (2, 7), (1, 9), (1, 12)],
                         ids=lambda c: "B%d_N%d" % c)
def test_order_dyadic_ties(shape):
    """Weights that are multiples of 0.25: every f64 sum is exact and equal scores abound, so the
    lowest-index rule and the h2 = h1 rule decide; order, pnll and margin bit-equal (the max path),
    the distribution within its bounds."""
    B, N = shape
    w, want = _stack([_ref("dyadic", N, SEED + b) for b in range(B)])
    _same(_order(w), want, shape)


@pytest.mark.parametrize("N", [1, 4, 12])
def test_order_all_zero_weights(N):
    got = _order(np.zeros((2, N, N), np.float32))
    for b in range(2):
        assert got["order"][b].tolist() == list(range(N))
        assert got["pnll"][b] == 0.0
        assert got["margin"][b] == (np.inf if N == 1 else 0.0)
    if N == 1:
        assert got["logz"].tolist() == [0.0, 0.0] and got["position"].ravel().tolist() == [1.0, 1.0]


def test_order_invalid_stories():
    N = 5
    w, want = _stack([_ref("random", N, SEED + s) for s in (1, 2, 3, 4)])
    w = w.copy()
    w[0, 3, 1] = np.nan
    w[2, 0, 4] = -np.inf
    w[3, 2, 2] = np.nan  # the diagonal is never read: story 3 stays valid
    got = _order(w)
    for b in (0, 2):
        assert got["order"][b].tolist() == [-1] * N
        assert got["pnll"][b] == np.inf and got["margin"][b] == 0.0
        assert got["logz"][b] == -np.inf and got["entropy"][b] == 0.0
        assert not got["position"][b].any() and not got["before"][b].any()
    for b in (1, 3):  # the neighbours: what they give alone, and what the restatement gives
        alone = _order(w[b:b + 1])
        _same_bits(alone, {k: v[b:b + 1] for k, v in got.items()}, f"story {b} beside invalid ones")
        _same(alone, {k: v[b:b + 1] for k, v in want.items()}, f"story {b}")


def test_order_abi_limits():
    def call(B, N, ws_bytes, N_buf=None):
        Nb = N if N_buf is None else N_buf
        w = torch.zeros(B, Nb, Nb, device="cuda")
        out = {name: torch.full((B,) + (Nb,) * nn, SENTINEL, dtype=dtype, device="cuda")
               for name, dtype, nn in NV.PAIRWISE_OUTPUTS}
        ws = torch.full((max(ws_bytes, 16) // 4,), float(SENTINEL), device="cuda")
        try:
            st = NV.lib().mmseq_pairwise_order(
                B, N, w.data_ptr(), *(out[name].data_ptr() for name, _, _ in NV.PAIRWISE_OUTPUTS),
                ws.data_ptr(), ws_bytes, None)
        finally:
            torch.cuda.synchronize()
        assert all(bool((t == SENTINEL).all()) for t in out.values())
        assert bool((ws == SENTINEL).all())
        return st
    assert NV.pairwise_order_workspace(1, 13) == 0 and NV.pairwise_order_workspace(1, 0) == 0
    assert call(1, 13, 1 << 20) == NV.EUNSUPPORTED
    assert call(1, 0, 1 << 20, N_buf=4) == NV.EUNSUPPORTED
    need = NV.pairwise_order_workspace(2, 12)
    assert call(2, 12, need - 16) == -1  # MMSEQ_EINVAL
    assert call(2, 5, 8) == -1
    # the wrapper: the status for an unsupported shape, an exception for a bad workspace
    w = torch.zeros(1, 13, 13, device="cuda")
    out = {name: torch.full((1,) + (13,) * nn, SENTINEL, dtype=dtype, device="cuda")
           for name, dtype, nn in NV.PAIRWISE_OUTPUTS}
    assert NV.pairwise_order(w, out, torch.zeros(4, device="cuda")) == NV.EUNSUPPORTED
    w = torch.zeros(2, 12, 12, device="cuda")
    out = {name: torch.full((2,) + (12,) * nn, SENTINEL, dtype=dtype, device="cuda")
           for name, dtype, nn in NV.PAIRWISE_OUTPUTS}
    with pytest.raises(NV.NativeError):
        NV.pairwise_order(w, out, torch.zeros(4, device="cuda"))
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in out.values())


# ------------------------------------------------------------------------------ pairwise_score
def _score(w, orders, what="pairwise_score"):
    """One mmseq_pairwise_score into a guarded output -> pnll f32 [B][K] numpy."""
    wt = torch.as_tensor(np.asarray(w, np.float32)).cuda().contiguous()
    o = torch.as_tensor(np.asarray(orders), dtype=torch.int64).cuda().contiguous()
    B, K = wt.shape[0], o.shape[-2]
    g = Guarded(B, K, dtype=torch.float32, device="cuda").fill_pattern().snapshot()
    assert NV.pairwise_score(wt, o, g.view[0]) == 0
    torch.cuda.synchronize()
    g.check_untouched(what)
    return g.view[0].cpu().numpy().copy()


@pytest.mark.parametrize("N", [2, 5, 9])
@pytest.mark.parametrize("K", [1, 257, "all"])
def test_score_matches_restatement(N, K):
    """Story 0 random, story 1 dyadic; a list shared by both and a list per story."""
    refs = [_ref("random", N, SEED + N), _ref("dyadic", N, SEED + N)]
    w, want_order = _stack(refs)
    perms = PW.all_perms(N)
    rng = np.random.RandomState(SEED + N)
    if K == "all":
        shared = perms
        per_story = np.stack([perms, perms[::-1]])
    else:
        shared = perms[rng.randint(0, len(perms), K)]
        per_story = np.stack([perms[rng.randint(0, len(perms), K)] for _ in range(2)])
    got = _score(w, shared)
    for b in range(2):
        assert np.array_equal(_f32bits(got[b]), _f32bits(PW.pairwise_score_ref(w[b], shared))), b
    got2 = _score(w, per_story)
    for b in range(2):
        assert np.array_equal(_f32bits(got2[b]),
                              _f32bits(PW.pairwise_score_ref(w[b], per_story[b]))), b
    if K != "all":
        return
    # the arg-min over all N! (lowest index = lexicographically smallest) is the DP's optimum
    idx, best, _margin = berson.exact_from_scores(torch.from_numpy(got).cuda())
    idx, best = idx.cpu().numpy(), best.cpu().numpy()
    for b in range(2):
        assert perms[idx[b]].tolist() == want_order["order"][b].tolist(), b
    want = want_order["pnll"]
    assert abs(float(best[0]) - float(want[0])) <= 2 * float(np.spacing(np.abs(want[0])))
    assert _f32bits(best[1:2]).tolist() == _f32bits(want[1:2]).tolist()


def test_score_invalid_candidates_and_weights():
    N = 5
    w = np.stack([_ref("random", N, SEED + s)[0] for s in (1, 2, 3)]).copy()
    w[1, 4, 0] = np.inf
    w[2, 1, 1] = np.nan  # the diagonal is never read
    perms = PW.all_perms(N)
    orders = perms[np.random.RandomState(SEED).randint(0, len(perms), 300)].copy()  # > one tile
    orders[0, 2], orders[7, 0], orders[9, 4], orders[11] = N, -1, 1 << 40, [0, 1, 1, 3, 4]
    orders[299, 4] = -(1 << 40)
    got = _score(w, orders)
    for b in range(3):
        assert np.array_equal(_f32bits(got[b]), _f32bits(PW.pairwise_score_ref(w[b], orders))), b
    bad = [0, 7, 9, 11, 299]
    assert np.isposinf(got[:, bad]).all() and np.isposinf(got[1]).all()
    ok = np.setdiff1d(np.arange(300), bad)
    assert np.isfinite(got[0, ok]).all() and np.isfinite(got[2, ok]).all()


def test_score_abi_limits():
    def call(N, K):
        w = torch.zeros(1, N, N, device="cuda")
        o = torch.zeros(max(K, 1), N, dtype=torch.int64, device="cuda")
        pnll = torch.full((1, max(K, 1)), float(SENTINEL), device="cuda")
        st = NV.lib().mmseq_pairwise_score(1, N, K, w.data_ptr(), o.data_ptr(), 0,
                                           pnll.data_ptr(), None)
        torch.cuda.synchronize()
        assert bool((pnll == SENTINEL).all())
        return st
    assert call(17, 3) == NV.EUNSUPPORTED
    assert call(5, 0) == NV.EUNSUPPORTED
    w = torch.zeros(2, 4, 4, device="cuda")
    o = torch.zeros(2, 3, 4, dtype=torch.int64, device="cuda")
    pnll = torch.full((2, 3), float(SENTINEL), device="cuda")
    st = NV.lib().mmseq_pairwise_score(2, 4, 3, w.data_ptr(), o.data_ptr(), 5, pnll.data_ptr(),
                                       None)  # a story stride below K * N
    torch.cuda.synchronize()
    assert st == -1 and bool((pnll == SENTINEL).all())
    # N = 16, the limit: the identity and its reverse
    w16 = np.random.RandomState(SEED).standard_normal((1, 16, 16)).astype(np.float32)
    o16 = np.stack([np.arange(16), np.arange(16)[::-1]])
    assert np.array_equal(_f32bits(_score(w16, o16)[0]),
                          _f32bits(PW.pairwise_score_ref(w16[0], o16)))


# ------------------------------------------------------- end to end on the reference's fixture
_ENC = {}


def _enc():
    if not _ENC:
        m, d, inputs = _e2e(torch.float32)
        m.eval()
        with torch.no_grad():
            _ENC["enc"] = m.encode(**berson._batch_inputs(m, inputs))
    return _ENC["enc"]


def test_end_to_end_weights_fp32():
    m, d, inputs = _e2e(torch.float32)
    enc = _enc()
    B, N = enc[0].shape[0], enc[0].shape[1]
    w = berson.pairwise_weights(enc[7]).cpu().numpy()
    rows = enc[6].view(B, N * (N - 1), 2).cpu().numpy()
    for b in range(B):
        want = PW.weights_from_pairs(rows[b], N)
        assert np.abs(w[b] - want).max() <= 1e-6, b
        assert not np.diag(w[b]).any()


def test_end_to_end_loss_identity_fp32():
    """model(labels = L) reports mean_b J_b(L[b]): the pointer part within the project's score
    bound (R.bound(nll) / (N - 1) per story; the forward's GEMMs run at other row counts than the
    scorer's), the pairwise part, f32 log_softmax sums of 20 terms on either side, within 1e-6."""
    m, d, inputs = _e2e(torch.float32)
    enc = _enc()
    B, N = enc[0].shape[0], enc[0].shape[1]
    lam = float(m.pairwise_loss_lam)
    assert lam == 0.6
    for seed in (SEED, SEED + 1, SEED + 2):
        rng = np.random.RandomState(seed)
        L = torch.from_numpy(np.stack([rng.permutation(N) for _ in range(B)]).astype(np.int64))
        with torch.no_grad():
            loss = float(m({**inputs, "labels": L})[0])
            l_pair = float(m.last_loss_terms[1])
            nll = berson.score_orders_batch(m.args, m, enc, L[:, None, :].cuda())[:, 0]
            pnll = berson.pairwise_score_orders(m.args, m, enc, L[:, None, :].cuda())[:, 0]
        nll, pnll = nll.cpu().numpy().astype(np.float64), pnll.cpu().numpy().astype(np.float64)
        J = nll / (N - 1) + lam * pnll / (N * (N - 1))
        bound = float(np.mean([R.bound(v) for v in nll])) / (N - 1) + 1e-6
        print(f"labels seed {seed}: loss {loss:.7f} mean J {J.mean():.7f} "
              f"difference {abs(loss - J.mean()):.3e} bound {bound:.3e}")
        assert abs(loss - J.mean()) <= bound, (seed, loss, J.mean())
        v = float((pnll / (N * (N - 1))).mean())
        print(f"labels seed {seed}: pairwise loss {l_pair:.7f} from pnll {v:.7f}")
        assert abs(l_pair - v) <= 1e-5 * max(1.0, abs(v)), (seed, l_pair, v)
        # the host list form is validated and gives the same bits
        host = berson.pairwise_score_orders(m.args, m, enc, L[:, None, :].tolist())[:, 0]
        assert np.array_equal(host.cpu().numpy().astype(np.float64), pnll)


def test_end_to_end_decodes_fp32():
    m, d, inputs = _e2e(torch.float32)
    enc = _enc()
    B, N = enc[0].shape[0], enc[0].shape[1]
    lam = float(m.pairwise_loss_lam)
    # (e) before: what beam and exact return now
    before = {}
    for name in ("beam", "exact"):
        orders = berson.berson_pointer_network_batch(m.args, m, None, inputs, decode=name)
        before[name] = (orders, _bits(m.last_beam_scores).clone())
    # (c) decode="pairwise" is pairwise_order_batch
    post = berson.pairwise_order_batch(m.args, m, enc)
    got = berson.berson_pointer_network_batch(m.args, m, None, inputs, decode="pairwise")
    assert got == post["order"].tolist()
    assert torch.equal(_bits(m.last_beam_scores), _bits(post["pnll"]))
    ref = PW.pairwise_order_batch_ref(post["w"].cpu().numpy())
    _same({k: v.cpu().numpy() for k, v in post.items() if k != "w"}, ref, "decisive_tiny")
    for b in range(B):
        print(f"story {b}: pairwise {got[b]} pnll {float(post['pnll'][b]):.5f} margin "
              f"{float(post['margin'][b]):.5f} entropy {float(post['entropy'][b]):.4f} "
              f"topological {berson.topological_order_host(post['w'][b].cpu())}")
    # (d) decode="joint": the host arg-min of J over the 120 orders
    perms = torch.from_numpy(PW.all_perms(N)).cuda()
    with torch.no_grad():
        nll = berson.score_orders_batch(m.args, m, enc, perms).cpu().numpy().astype(np.float64)
        pnll = berson.pairwise_score_orders(m.args, m, enc, perms).cpu().numpy().astype(np.float64)
    J = nll / (N - 1) + lam * pnll / (N * (N - 1))
    index = {tuple(p): i for i, p in enumerate(PW.all_perms(N).tolist())}
    for kw in ({}, {"enumeration": "tree"}):
        got = berson.berson_pointer_network_batch(m.args, m, None, inputs, decode="joint", **kw)
        scores = m.last_beam_scores.cpu().numpy()
        for b in range(B):
            srt = np.argsort(J[b], kind="stable")
            margin = J[b, srt[1]] - J[b, srt[0]]
            bound = R.bound(float(nll[b, srt[0]])) / (N - 1) + 1e-6
            k = index[tuple(got[b])]
            print(f"story {b} {kw or 'flat'}: joint {got[b]} J {scores[b]:.6f} host min "
                  f"{J[b, srt[0]]:.6f} margin {margin:.3e} bound {bound:.3e}")
            if margin > 2 * bound:
                assert k == int(srt[0]), (b, kw, got[b])
            else:
                assert J[b, k] - J[b, srt[0]] <= bound, (b, kw, got[b])
            assert abs(float(scores[b]) - J[b, k]) <= R.bound(float(nll[b, k])) / (N - 1) + 1e-6, \
                (b, kw)
    order, Jdev, _margin = berson.joint_order_batch(m.args, m, enc, lam=0.0)
    exact, s_exact, _ = berson.exact_order_batch(m.args, m, enc)
    assert torch.equal(order, exact)  # lam = 0: the pointer decoder's optimum alone
    assert torch.allclose(Jdev * (N - 1), s_exact, rtol=1e-6, atol=0)
    # (e) after: the same orders and the same score bits
    for name in ("beam", "exact"):
        orders = berson.berson_pointer_network_batch(m.args, m, None, inputs, decode=name)
        assert orders == before[name][0], name
        assert torch.equal(_bits(m.last_beam_scores), before[name][1]), name
