"""Gradients of candidate-order scores on the device (csrc/order_grad.hip mmseq_order_score_bwd,
kernels.OrderScoreFn, berson.score_orders_grad / score_orders_autograd / order_loss /
sequence_loss).

Kernel tests: beam_batch_ref.random_case at SEED = 100. The expected gradients are autograd
through tests/order_grad_ref.scores in float64 (the reference's dense formulation); the same
restatement in float32 on the CPU measures what fp32 rounding alone costs, and the kernel may be
four times worse (it sums the projected key blocks in another order; the attention accuracy test
uses the same factor). Model tests: the `tiny` / `tiny_n4` fixtures in fp32 and eval mode.
"""
import random

import pytest
import torch

import beam_batch_ref as R
import order_grad_ref as G
from golden_util import load_fixture
from guard_util import Guarded

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multimodal_sequencing_amd import _native as NV
    from multimodal_sequencing_amd import berson, model_zoo
    from multimodal_sequencing_amd.trainer import FusedAdamW, train_step

FACTOR = 4.0      # kernel error / fp32 restatement error, relative L2
ELEM_RTOL = 2e-3  # the project's gradient rtol, against the tensor's largest |reference|
ZERO_FLOOR = 1e-6  # tensors whose gradient is analytically zero
_IN_SHAPES = {"doc": lambda B, N, H: (B, N, H), "okey": lambda B, N, H: (B, N, H),
              "hist": lambda B, N, H: (B, N, N, H + 2), "h0": lambda B, N, H: (B, H),
              "c0": lambda B, N, H: (B, H)}

# (B, N, H, K): what each case can break
SHAPES = [(3, 5, 128, 7),     # base case
          (2, 2, 128, 2),     # a single step
          (1, 1, 128, 1),     # N = 1: zero input gradients, weights untouched
          (2, 9, 128, 5),     # pointed mask past 8 bits
          (1, 16, 128, 2),    # the maximum N
          (2, 4, 136, 3),     # H no multiple of 64
          (1, 5, 768, 4),     # the models' width
          (33, 4, 128, 1),    # an odd story count above 32
          (2, 5, 128, 257)]   # 257 repeated orders


def _bits(t):
    return t.contiguous().view(torch.int32)


def _orders(B, N, K, seed):
    """[B][K][N]: seeded permutations per story; K = 257 draws them (with repeats) from 24."""
    rng = random.Random(seed)
    pool = [rng.sample(range(N), N) for _ in range(24)]
    rows = [[pool[rng.randrange(24)] if K == 257 else rng.sample(range(N), N) for _ in range(K)]
            for _ in range(B)]
    return torch.tensor(rows, dtype=torch.int64)


def _dnll(B, K, seed):
    g = torch.Generator().manual_seed(seed)
    d = torch.rand(B, K, generator=g) * 2 - 1
    d[torch.rand(B, K, generator=g) < 0.2] = 0.0  # some exact zeros
    if B * K > 3:
        d.view(-1)[1] = 0.0
    return d


_REF = {}


def _reference(shape):
    """(case, orders, dnll, float64 gradients, float32 CPU gradients), once per shape."""
    if shape not in _REF:
        B, N, H, K = shape
        case = R.random_case(B, N, H, R.SEED)
        orders, dnll = _orders(B, N, K, R.SEED), _dnll(B, K, R.SEED)
        _n64, g64 = G.grads(case, orders, dnll, torch.float64)
        _n32, g32 = G.grads(case, orders, dnll, torch.float32)
        _REF[shape] = (case, orders, dnll, g64, g32)
    return _REF[shape]


def _device_grads(case, orders, dnll, fill=None, base=0.0, guarded=False):
    """One mmseq_order_score_bwd -> ({name: gradient on the CPU}, the Guarded outputs or None).
    The accumulated weight gradients start at `base`."""
    B, N, H = case["B"], case["N"], case["H"]
    K = orders.shape[-2]
    ins = [case[k].cuda().contiguous() for k in G.INPUTS]
    wts = [case["p"][n].cuda().contiguous() for n in G.WEIGHTS]
    wts_t = [case["p"][n].t().contiguous().cuda() for n in berson.K.ORDER_WEIGHTS_T]
    guards = None
    if guarded:
        guards = [Guarded(1, int(torch.tensor(_IN_SHAPES[n](B, N, H)).prod()), device="cuda")
                  for n in G.INPUTS]
        guards += [Guarded(1, w.numel(), device="cuda") for w in wts]
        for g in guards[:5]:
            g.fill_pattern().snapshot()
        for g in guards[5:]:
            g.fill_pattern()
            g.view.fill_(base)
            g.snapshot()
        dins = [g.view.view(_IN_SHAPES[n](B, N, H)) for g, n in zip(guards[:5], G.INPUTS)]
        dws = [g.view.view(w.shape) for g, w in zip(guards[5:], wts)]
    else:
        dins = [torch.full(_IN_SHAPES[n](B, N, H), float("nan"), device="cuda") for n in G.INPUTS]
        dws = [torch.full_like(w, base) for w in wts]
    nbytes = NV.order_score_bwd_workspace(B, N, H, K)
    assert nbytes > 0 and nbytes % 16 == 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    st = NV.order_score_bwd(*ins, wts, wts_t, orders.cuda().contiguous(), dnll.cuda().contiguous(),
                            dins, dws, ws)
    assert st == 0
    torch.cuda.synchronize()
    out = {n: t.cpu().clone() for n, t in zip(G.NAMES, dins + dws)}
    return out, guards


def _errors(got, ref64):
    """(L2 error, largest element error, largest |reference|); the L2 error is relative unless
    the reference is zero."""
    d = got.double() - ref64
    scale = float(ref64.abs().max())
    l2 = float(d.norm())
    if scale > 0:
        l2 /= float(ref64.norm())
    return l2, float(d.abs().max()), scale


@pytest.mark.parametrize("shape", SHAPES, ids=lambda c: "B%d_N%d_H%d_K%d" % c)
def test_kernel_matches_float64(shape):
    B, N, H, K = shape
    case, orders, dnll, g64, g32 = _reference(shape)
    got, _ = _device_grads(case, orders, dnll)
    for name in G.NAMES:
        ref = g64[name]
        # analytically zero: everything at N = 1, doc and W_ih at N = 2 (x = 0), and always
        # tanh_linear.bias (a shift of every live logit); float64 leaves rounding noise there
        zero = float(ref.abs().max()) < 1e-12
        if zero:
            ref = torch.zeros_like(ref)
        e_dev, m_dev, scale = _errors(got[name], ref)
        e_32, _m32, _ = _errors(g32[name], ref)
        ratio = e_dev / e_32 if e_32 > 0 else float("inf") if e_dev > 0 else 0.0
        print(f"{shape} {name}: L2 error {e_dev:.3e} fp32 restatement {e_32:.3e} ratio "
              f"{ratio:.2f}; element error {m_dev:.3e} of max|ref| {scale:.3e}")
        assert bool(torch.isfinite(got[name]).all()), name
        if zero:
            assert e_dev <= max(FACTOR * e_32, ZERO_FLOOR), (name, e_dev, e_32)
            assert m_dev <= ZERO_FLOOR, (name, m_dev)
        else:
            assert e_dev <= FACTOR * e_32, (name, e_dev, e_32)
            assert m_dev <= ELEM_RTOL * scale, (name, m_dev, scale)
    if N == 1:  # written zeros, weights untouched
        base, _ = _device_grads(case, orders, dnll, base=0.75)
        for name in G.INPUTS:
            assert float(got[name].abs().max()) == 0.0, name
        for name in G.WEIGHTS:
            assert bool((base[name] == 0.75).all()), name
    if N == 2:
        base, _ = _device_grads(case, orders, dnll, base=0.75)
        assert float(got["doc"].abs().max()) == 0.0
        assert bool((base["decoder.weight_ih_l0"] == 0.75).all())
        assert not bool((base["decoder.bias_ih_l0"] == 0.75).all())


def test_weight_gradients_accumulate():
    case, orders, dnll, _g64, _g32 = _reference(SHAPES[0])
    zero, _ = _device_grads(case, orders, dnll)
    base, _ = _device_grads(case, orders, dnll, base=0.5)
    for name in G.INPUTS:
        assert torch.equal(_bits(zero[name]), _bits(base[name])), name
    for name in G.WEIGHTS:
        d = (base[name] - 0.5 - zero[name]).abs().max()
        assert float(d) <= 1e-6 * max(1.0, float(zero[name].abs().max())), (name, float(d))


def test_reproducible_and_workspace_contents_irrelevant():
    case, orders, dnll, _g64, _g32 = _reference(SHAPES[0])
    a, _ = _device_grads(case, orders, dnll, fill=0)
    b, _ = _device_grads(case, orders, dnll, fill=0)
    c, _ = _device_grads(case, orders, dnll, fill=0xFF)  # every workspace float a NaN
    for name in G.NAMES:
        assert torch.equal(_bits(a[name]), _bits(b[name])), name
        assert torch.equal(_bits(a[name]), _bits(c[name])), name
        assert bool(torch.isfinite(a[name]).all()), name


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[5], SHAPES[2]], ids=lambda c: "B%d_N%d_H%d_K%d" % c)
def test_nothing_written_outside_the_outputs(shape):
    case, orders, dnll, _g64, _g32 = _reference(shape)
    plain, _ = _device_grads(case, orders, dnll, base=0.25)
    got, guards = _device_grads(case, orders, dnll, base=0.25, guarded=True)
    for name, g in zip(G.NAMES, guards):
        g.check_untouched(name)
        assert torch.equal(_bits(got[name]), _bits(plain[name])), name


@pytest.mark.parametrize("bad", [[0, 0, 1, 2, 3], [0, 1, -1, 2, 3], [0, 1, 2, 5, 3]],
                         ids=["repeat", "negative", "N"])
def test_invalid_candidate_contributes_exactly_zero(bad):
    case, orders, dnll, _g64, _g32 = _reference(SHAPES[0])
    o_bad, d_bad = orders.clone(), dnll.clone()
    o_bad[1, 3] = torch.tensor(bad)
    d_bad[1, 3] = float("nan")
    d_zero = dnll.clone()
    d_zero[1, 3] = 0.0
    got, _ = _device_grads(case, o_bad, d_bad)
    want, _ = _device_grads(case, orders, d_zero)
    for name in G.NAMES:
        assert bool(torch.isfinite(got[name]).all()), name
        assert bool((got[name] == want[name]).all()), name


def test_abi_status_codes():
    B, N, H, K = 2, 5, 128, 4
    case = R.random_case(B, N, H, R.SEED)
    assert NV.order_score_bwd_workspace(B, 17, H, K) == 0
    assert NV.order_score_bwd_workspace(B, N, H, 0) == 0
    assert NV.order_score_bwd_workspace(B, N, H, 1 << 22) == 0
    nbytes = NV.order_score_bwd_workspace(B, N, H, K)
    ins = [case[k].cuda().contiguous() for k in G.INPUTS]
    wts = [case["p"][n].cuda().contiguous() for n in G.WEIGHTS]
    wts_t = [case["p"][n].t().contiguous().cuda() for n in berson.K.ORDER_WEIGHTS_T]
    o = _orders(B, N, K, 1).cuda()
    dnll = torch.ones(B, K, device="cuda")
    dins = [torch.full(_IN_SHAPES[n](B, N, H), -7.0, device="cuda") for n in G.INPUTS]
    dws = [torch.full_like(w, -7.0) for w in wts]
    ws = torch.zeros(nbytes + 16, dtype=torch.uint8, device="cuda")
    L = NV.lib()
    stream = torch.cuda.current_stream().cuda_stream
    ptr = [t.data_ptr() for t in ins + wts + wts_t]
    outs = [t.data_ptr() for t in dins + dws]

    def call(n=N, k=K, stride=K * N, first=ptr[0], out0=outs[0], ws_p=ws.data_ptr(), wbytes=nbytes):
        return L.mmseq_order_score_bwd(B, n, H, k, first, *ptr[1:], o.data_ptr(), stride,
                                       dnll.data_ptr(), out0, *outs[1:], ws_p, wbytes, stream)

    for kw, want in (({"n": 17}, -2), ({"k": 0}, -2), ({"k": 1 << 22}, -2), ({"n": 0}, -2),
                     ({"first": None}, -1), ({"out0": None}, -1), ({"stride": K * N - 1}, -1),
                     ({"ws_p": None}, -1), ({"wbytes": nbytes - 16}, -1),
                     ({"ws_p": ws.data_ptr() + 4}, -1)):
        assert call(**kw) == want, kw
        assert L.mmseq_last_error().decode().startswith("order_score_bwd"), L.mmseq_last_error()
        torch.cuda.synchronize()
        assert all(bool((t == -7.0).all()) for t in dins + dws) and not bool(ws.any()), kw
    assert call() == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in dins + dws)


# ------------------------------------------------------------ finite differences of the forward
_FD_NAMES = ("okey",) + G.WEIGHTS


def _risk(nll, orders, gold):
    return berson.order_loss(nll, orders, gold, "risk", alpha=0.25)


def _fd_ratio(loss_at, x, g, eps):
    """(L(x) - L(x - eps g)) / (eps |g|^2) and the loss difference."""
    base = loss_at(x)
    moved = loss_at({n: (v - eps * g[n] if n in g else v) for n, v in x.items()})
    norm2 = sum(float((g[n].double() ** 2).sum()) for n in g)
    return (base - moved) / (eps * norm2), base - moved


def test_gradient_predicts_the_forwards_finite_difference():
    """With g the device gradient of a risk loss with respect to the head weights and okey,
    (L(x) - L(x - eps g)) / (eps |g|^2) through mmseq_order_score lies within 1 +- 0.05; eps is
    the largest of a geometric grid at which the float64 restatement's own ratio (with its own
    gradient) is within 1 +- 0.02 and its loss moves by at least 1e-2."""
    B, N, H, K = SHAPES[0]
    case = R.random_case(B, N, H, R.SEED)
    orders = _orders(B, N, K, R.SEED)
    gold = orders[:, 0].clone()

    # the restatement: its loss, its gradient, eps
    x64 = G.leaves(case, torch.float64)
    loss64 = _risk(G.scores(x64, orders), orders, gold)
    loss64.backward()
    g64 = {n: x64[n].grad for n in _FD_NAMES}
    x64 = {n: v.detach() for n, v in x64.items()}

    def loss_cpu(x):
        with torch.no_grad():
            return float(_risk(G.scores(x, orders), orders, gold))

    eps = None
    for k in range(12):
        e = 4.0 * 0.5 ** k
        ratio, dl = _fd_ratio(loss_cpu, x64, g64, e)
        print(f"float64 restatement: eps {e:.4g} ratio {ratio:.4f} loss difference {dl:.4f}")
        if abs(ratio - 1) <= 0.02 and dl >= 1e-2:
            eps = e
            break
    assert eps is not None, "no eps with a ratio within 2 % and a loss difference of 1e-2"

    # the device: dL/dnll by autograd on the scores of mmseq_order_score, then the new entry
    def loss_dev(x, want_nll=False):
        c = dict(case, p={n: x[n] for n in G.WEIGHTS}, **{n: x[n] for n in G.INPUTS})
        ins = [c[k].float().cuda().contiguous() for k in G.INPUTS]
        wts = [c["p"][n].float().cuda().contiguous() for n in G.WEIGHTS]
        nll = torch.empty(B, K, device="cuda")
        ws = torch.zeros(NV.order_score_workspace(B, N, H, K), dtype=torch.uint8, device="cuda")
        assert NV.order_score(*ins, wts, orders.cuda(), nll, None, ws) == 0
        nll = nll.cpu()
        return nll if want_nll else float(_risk(nll, orders, gold))

    x32 = {n: v.float() for n, v in x64.items()}
    nll = loss_dev(x32, want_nll=True).requires_grad_(True)
    (dnll,) = torch.autograd.grad(_risk(nll, orders, gold), nll)
    c32 = dict(case, p={n: x32[n] for n in G.WEIGHTS})
    grads, _ = _device_grads(c32, orders, dnll)
    g = {n: grads[n] for n in _FD_NAMES}
    ratio, dl = _fd_ratio(loss_dev, x32, g, eps)
    print(f"device: eps {eps:.4g} ratio {ratio:.4f} loss difference {dl:.4f}")
    assert abs(ratio - 1) <= 0.05, (ratio, dl, eps)


# ------------------------------------------------------------------------------- the trained path
_MODELS = {}


def _fixture(name, dtype=torch.float32):
    if (name, dtype) not in _MODELS:
        meta, d, params = load_fixture(name)
        m = model_zoo.build_from_golden(meta["config"], device="cuda", dtype=dtype)
        m.load_state_dict(params)
        m.eval()
        inputs = {"input_ids": torch.from_numpy(d["input_ids"]),
                  "labels": torch.from_numpy(d["labels"]),
                  "images": torch.from_numpy(d["images"]).cuda()}
        _MODELS[(name, dtype)] = (m, inputs)
    return _MODELS[(name, dtype)]


def _store_grads(m):
    torch.cuda.synchronize()
    return [s.grad.clone() for s in m.stores()]


def _assert_grads_close(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert float(y.abs().max()) > 0, (what, i)
        torch.testing.assert_close(x, y, rtol=2e-3, atol=1e-5, msg=lambda s: f"{what} store {i}: {s}")


@pytest.mark.parametrize("name", ["tiny", "tiny_n4"])
def test_sequence_loss_without_its_term_is_the_training_loss(name):
    m, inputs = _fixture(name)
    m.zero_grad()
    want = m(inputs)[0]
    want.backward()
    g_want = _store_grads(m)
    m.zero_grad()
    loss, terms = berson.sequence_loss(m.args, m, inputs, seq_lam=0.0, samples=4)
    loss.backward()
    g_got = _store_grads(m)
    m.zero_grad()
    print(f"{name}: model(inputs) {float(want):.6f} sequence_loss {float(loss):.6f} terms "
          f"{ {k: float(v) for k, v in terms.items()} }")
    assert abs(float(loss) - float(want)) < 1e-4
    assert abs(float(terms["ptr"]) - float(m.last_loss_terms[0])) < 1e-4
    assert abs(float(terms["pair"]) - float(m.last_loss_terms[1])) < 1e-4
    _assert_grads_close(g_got, g_want, name)


@pytest.mark.parametrize("name", ["tiny", "tiny_n4"])
def test_device_and_autograd_gradients_agree_under_risk(name):
    m, inputs = _fixture(name)
    b = berson._batch_inputs(m, inputs)
    gold = b["ground_truth"]
    perms = G.all_perms(gold.shape[1]).cuda()
    out = []
    for fn in (berson.score_orders_grad, berson.score_orders_autograd):
        m.zero_grad()
        nll = fn(m.args, m, m.encode(**b), perms)
        loss = berson.order_loss(nll, perms, gold, "risk")
        loss.backward()
        out.append((nll.detach(), float(loss), _store_grads(m)))
    m.zero_grad()
    (n0, l0, g0), (n1, l1, g1) = out
    with torch.no_grad():
        same = berson.score_orders_batch(m.args, m, m.encode(**b), perms)
    assert torch.equal(_bits(n0), _bits(same))  # the forward is mmseq_order_score
    assert float((n0 - n1).abs().max()) < R.BOUND * max(1.0, float(n1.abs().max()))
    assert abs(l0 - l1) < 1e-4
    _assert_grads_close(g0, g1, name)


def test_risk_over_all_orders_is_the_posteriors_expected_tau():
    m, inputs = _fixture("tiny")
    b = berson._batch_inputs(m, inputs)
    gold = b["ground_truth"]
    B, N = gold.shape
    with torch.no_grad():
        enc = m.encode(**b)
        post = berson.order_posterior_batch(m.args, m, enc, source="exact")
        got = float(berson.order_loss(post["nll"], post["orders"], gold, "risk", metric="tau"))
    before = post["before"].double().cpu()
    want = 0.0
    for s in range(B):
        o = gold[s].tolist()
        tau = sum(before[s, o[i], o[j]] - before[s, o[j], o[i]]
                  for i in range(N) for j in range(i + 1, N)) / (N * (N - 1) / 2)
        want += (1.0 - float(tau)) / B
    print(f"risk over {post['nll'].shape[1]} orders {got:.7f}, 1 - gain_tau(gold) {want:.7f}")
    assert abs(got - want) < 1e-5


def test_chunked_gradients_equal_unchunked(monkeypatch):
    m, inputs = _fixture("tiny_n4")
    b = berson._batch_inputs(m, inputs)
    with torch.no_grad():
        enc0 = m.encode(**b)
    B, N, H = enc0[0].shape
    perms = G.all_perms(N).cuda()
    assert perms.shape[0] == 24
    g = torch.Generator().manual_seed(3)
    w = (torch.rand(B, 24, generator=g) * 2 - 1).cuda()

    def run():
        leaves = [t.detach().clone().requires_grad_(True)
                  for t in (enc0[0], enc0[3], enc0[5], enc0[7], enc0[2][0], enc0[2][1])]
        enc = (leaves[0], None, (leaves[4], leaves[5]), leaves[1], None, leaves[2], None, leaves[3],
               None, None)
        m.zero_grad()
        nll = berson.score_orders_grad(m.args, m, enc, perms)
        (nll * w).sum().backward()
        torch.cuda.synchronize()
        return nll.detach().clone(), [t.grad.clone() for t in leaves] + [m.store.grad.clone()]

    n_one, g_one = run()
    cap = NV.order_score_bwd_workspace(B, N, H, 8)
    assert berson.K.order_grad_chunk(B, N, H, 24, berson.SCORE_WS_CAP)[0] == 24
    monkeypatch.setattr(berson, "SCORE_WS_CAP", cap)
    kc = berson.K.order_grad_chunk(B, N, H, 24, cap)[0]
    assert (24 + kc - 1) // kc >= 3, kc
    n_chunk, g_chunk = run()
    m.zero_grad()
    assert float((n_one - n_chunk).norm() / n_one.norm()) <= 1e-6
    for i, (a, c) in enumerate(zip(g_one, g_chunk)):
        rel = float((a - c).norm() / a.norm())
        print(f"tensor {i}: chunked vs unchunked relative L2 {rel:.2e}")
        assert rel <= 1e-6, (i, rel)


def test_one_bf16_training_step():
    m, inputs = _fixture("tiny", torch.bfloat16)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    m.train()
    try:
        m.zero_grad()
        seen = {}

        def model(inp):  # the model-like callable trainer.train_step takes
            loss, terms = berson.sequence_loss(m.args, m, inp, candidates="sample", samples=8)
            seen.update(terms)
            return (loss,)

        model.zero_grad = m.zero_grad
        opt = FusedAdamW(m.stores(), lr=1e-4, warmup=0, total_steps=10)
        # the gradients, before the update consumes them
        loss = model(inputs)[0]
        loss.backward()
        torch.cuda.synchronize()
        print({k: float(v) for k, v in seen.items()}, float(loss))
        assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(v)) for v in seen.values())
        for s in m.stores():
            assert bool(torch.isfinite(s.grad).all()) and float(s.grad.abs().max()) > 0
        m.zero_grad()
        loss = train_step(model, opt, [inputs])
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss))
        for s in m.stores():
            assert bool(torch.isfinite(s.master).all())
    finally:
        m.eval()
        m.load_state_dict(state)
        m.zero_grad()
