"""Gradients of candidate-order scores, no GPU: the float64 restatement the GPU tests differentiate
(tests/order_grad_ref.scores) against the reference's step-by-step score, as a distribution over
permutations and against central differences; berson.order_loss against its numpy restatement.
"""
from types import SimpleNamespace

import pytest
import torch

import beam_batch_ref as R
import order_grad_ref as G
import order_score_ref as S
from multimodal_sequencing_amd import berson, evaluate


def _seeded_orders(B, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.stack([torch.randperm(N, generator=g) for _ in range(K)])
                        for _ in range(B)])


@pytest.mark.parametrize("B, N, H, K", [(3, 5, 128, 8), (2, 4, 136, 24)])
def test_restatement_matches_reference_scores(B, N, H, K):
    """K = 24 at N = 4 is every order; at N = 5 eight seeded ones shared by the stories."""
    cand = G.all_perms(N) if K == 24 else _seeded_orders(1, N, K, 7)[0]
    case, _cand, want = S.ref_nll(B, N, H, cand.tolist())
    orders = cand[None].expand(B, -1, -1)
    for dtype in (torch.float64, torch.float32):
        with torch.no_grad():
            nll = G.scores(G.leaves(case, dtype, False), orders)
        worst = 0.0
        for b in range(B):
            for k in range(K):
                got, ref = float(nll[b, k]), float(want[b, k])
                worst = max(worst, abs(got - ref) / R.bound(ref))
                assert abs(got - ref) < R.bound(ref), (dtype, b, cand[k].tolist(), got, ref)
        print(f"{dtype}: worst |diff| / bound = {worst:.3f}")


def test_restatement_is_a_distribution_over_permutations():
    case = R.random_case(2, 4, 128, R.SEED)
    with torch.no_grad():
        nll = G.scores(G.leaves(case, torch.float64, False), G.all_perms(4)[None].expand(2, -1, -1))
    total = torch.exp(-nll).sum(-1)
    print("sum over 24 orders of exp(-nll):", total.tolist())
    assert nll.shape == (2, 24) and float((total - 1).abs().max()) < 1e-9


def test_autograd_matches_central_differences():
    """Eight seeded elements of each of the 14 tensors, h = 1e-6 in float64: within 1e-6 of the
    tensor's largest gradient entry, and never asked to be closer than the rounding of the
    difference quotient itself, 16 eps |L| / 2h (about 2e-9 |L|): the gradient of tanh_linear.bias
    is analytically zero (a shift of every live logit), so its largest entry is rounding noise."""
    B, N, H, K = 2, 4, 16, 3
    case = R.random_case(B, N, H, R.SEED)
    orders = _seeded_orders(B, N, K, 3)
    g = torch.Generator().manual_seed(11)
    dnll = torch.rand(B, K, generator=g, dtype=torch.float64) * 2 - 1
    _nll, grad = G.grads(case, orders, dnll, torch.float64)
    x = G.leaves(case, torch.float64, False)
    h = 1e-6

    def loss():
        with torch.no_grad():
            return float((G.scores(x, orders) * dnll).sum())

    floor = 16 * 2.0 ** -52 * abs(loss()) / (2 * h)
    for name in G.NAMES:
        flat, gflat = x[name].view(-1), grad[name].reshape(-1)
        scale = float(gflat.abs().max())
        worst = 0.0
        for i in torch.randperm(flat.numel(), generator=g)[:8].tolist():
            keep = float(flat[i])
            flat[i] = keep + h
            up = loss()
            flat[i] = keep - h
            down = loss()
            flat[i] = keep
            fd = (up - down) / (2 * h)
            worst = max(worst, abs(fd - float(gflat[i])))
        tol = max(1e-6 * scale, floor)
        print(f"{name}: max|grad| {scale:.2e} worst |fd - grad| {worst:.2e} bound {tol:.2e}")
        assert worst < tol, (name, worst, tol)


# ---- order_loss -------------------------------------------------------------------------------------
def _loss_case(B, N, K, seed, dup_gold=True):
    g = torch.Generator().manual_seed(seed)
    orders = _seeded_orders(B, N, K, seed)
    gold = torch.stack([torch.randperm(N, generator=g) for _ in range(B)])
    if dup_gold:
        orders[:, 0] = gold
    nll = torch.rand(B, K, generator=g) * 6
    return nll, orders, gold


@pytest.mark.parametrize("metric", ["tau", "acc"])
def test_gains_are_cal_result_per_story(metric):
    N = 5
    perms = G.all_perms(N)
    gold = torch.tensor([[2, 0, 4, 1, 3]])
    got = berson.order_gains(perms, gold, metric)[0]
    args = SimpleNamespace(ref_json_file=None)
    for k in range(0, 120, 7):
        acc, _pmr, tau = evaluate.cal_result([gold[0].tolist()], [perms[k].tolist()], [], None, args)
        want = tau if metric == "tau" else acc
        assert abs(float(got[k]) - want) < 1e-6, (perms[k].tolist(), float(got[k]), want)
        assert abs(G.gain(perms[k].tolist(), gold[0].tolist(), metric) - want) < 1e-12
    one = berson.order_gains(torch.zeros(3, 1, dtype=torch.int64), torch.zeros(1, 1, dtype=torch.int64),
                             metric)
    assert one.tolist() == [[1.0, 1.0, 1.0]]


@pytest.mark.parametrize("kind", ["risk", "set_nll", "margin"])
@pytest.mark.parametrize("K", [1, 6])
def test_order_loss_matches_numpy(kind, K):
    nll, orders, gold = _loss_case(3, 5, K, 5)
    for kw in ({}, {"metric": "acc", "alpha": 0.5, "margin": 2.5}):
        got = float(berson.order_loss(nll, orders, gold, kind, **kw))
        want = G.order_loss(nll.numpy(), orders.numpy(), gold.numpy(), kind, **kw)
        print(kind, K, kw, got, want)
        assert abs(got - want) < 1e-5 * max(1.0, abs(want)), (kind, K, kw, got, want)
    # one list [K][N] shared by the stories
    shared = orders[0].clone()
    got = float(berson.order_loss(nll, shared, gold[:1].expand(3, -1), kind))
    want = G.order_loss(nll.numpy(), shared[None].expand(3, -1, -1).numpy(),
                        gold[:1].expand(3, -1).numpy(), kind)
    assert abs(got - want) < 1e-5 * max(1.0, abs(want))


def test_order_loss_ignores_infinite_candidates():
    nll, orders, gold = _loss_case(2, 4, 6, 9)
    nll[:, 2] = float("inf")
    nll[1, 4] = float("inf")
    nll.requires_grad_(True)
    for kind in ("risk", "set_nll", "margin"):
        loss = berson.order_loss(nll, orders, gold, kind)
        want = G.order_loss(nll.detach().numpy(), orders.numpy(), gold.numpy(), kind)
        assert abs(float(loss.detach()) - want) < 1e-5 * max(1.0, abs(want)), (kind, want)
        (grad,) = torch.autograd.grad(loss, nll)
        assert torch.isfinite(grad).all() and float(grad[:, 2].abs().max()) == 0.0
    # risk without the +inf columns is the same number
    a = berson.order_loss(nll[:1], orders[:1], gold[:1], "risk")
    b = berson.order_loss(nll[:1, [0, 1, 3, 4, 5]], orders[:1, [0, 1, 3, 4, 5]], gold[:1], "risk")
    assert abs(float(a) - float(b)) < 1e-6


def test_set_nll_over_all_orders_is_zero():
    case = R.random_case(2, 4, 128, R.SEED)
    perms = G.all_perms(4)
    with torch.no_grad():
        nll = G.scores(G.leaves(case, torch.float64, False), perms[None].expand(2, -1, -1))
    gold = torch.tensor([[0, 1, 2, 3], [3, 1, 0, 2]])
    refs = torch.ones(2, 24, dtype=torch.bool)
    assert abs(float(berson.order_loss(nll, perms, gold, "set_nll", refs=refs))) < 1e-9
    # the default refs: the gold order alone, i.e. its pointer loss
    k = [perms.tolist().index(g) for g in gold.tolist()]
    want = float((nll[0, k[0]] + nll[1, k[1]]) / 2 / 3)
    assert abs(float(berson.order_loss(nll, perms, gold, "set_nll")) - want) < 1e-12


def test_margin_active_and_inactive():
    gold = torch.tensor([[0, 1, 2]])
    orders = torch.tensor([[[0, 1, 2], [1, 0, 2], [2, 1, 0]]])
    active = torch.tensor([[2.0, 2.5, 4.0]], requires_grad=True)   # 1 + 2 - 2.5 = 0.5 > 0
    loss = berson.order_loss(active, orders, gold, "margin")
    assert abs(float(loss) - 0.5 / 2) < 1e-7
    (g,) = torch.autograd.grad(loss, active)
    assert torch.allclose(g, torch.tensor([[0.5, -0.5, 0.0]]))
    inactive = torch.tensor([[1.0, 2.5, 4.0]], requires_grad=True)  # 1 + 1 - 2.5 < 0
    loss = berson.order_loss(inactive, orders, gold, "margin")
    (g,) = torch.autograd.grad(loss, inactive)
    assert float(loss) == 0.0 and float(g.abs().max()) == 0.0
    assert abs(float(berson.order_loss(inactive, orders, gold, "margin", margin=3.0)) - 0.75) < 1e-7


def test_order_loss_rejects_unknown_names():
    nll, orders, gold = _loss_case(1, 3, 2, 1)
    with pytest.raises(ValueError):
        berson.order_loss(nll, orders, gold, "hinge")
    with pytest.raises(ValueError):
        berson.order_loss(nll, orders, gold, "risk", metric="pmr")


def test_candidate_set_takes_repeats_out():
    o = torch.tensor([[[0, 1, 2], [1, 0, 2], [0, 1, 2], [1, 0, 2], [2, 1, 0]]])
    got = berson._candidate_set(o)
    assert got.tolist() == [[[0, 1, 2], [1, 0, 2], [-1, -1, -1], [-1, -1, -1], [2, 1, 0]]]
