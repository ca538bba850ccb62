"""Differentiable restatement of mmseq_order_score's slot forward for the gradient tests, and the
sequence-level losses restated in numpy.

`scores` is the forward of include/mmseq.h (mmseq_order_score_bwd) in torch at any dtype, in the
REFERENCE's dense formulation: one pw_k dot product per key over cat[l1, l2, forw, back], as
order_score_ref.StandIn.step, so it does not share the kernel's projected-block sums. Autograd
through it in float64 is the expected gradient; the same in float32 is the yardstick for the
kernel's rounding error.
"""
import itertools

import numpy as np
import torch

WEIGHTS = ("decoder.weight_ih_l0", "decoder.bias_ih_l0", "decoder.weight_hh_l0",
           "decoder.bias_hh_l0", "query_linear.weight", "query_linear.bias", "pw_k.weight",
           "tanh_linear.weight", "tanh_linear.bias")
INPUTS = ("doc", "okey", "hist", "h0", "c0")
NAMES = INPUTS + WEIGHTS  # the 14 gradient tensors


def leaves(case, dtype, requires_grad=True):
    """The 14 differentiable tensors of a beam_batch_ref.random_case as fresh leaves."""
    x = {n: case[n].detach().to(dtype).clone() for n in INPUTS}
    x.update({n: case["p"][n].detach().to(dtype).clone() for n in WEIGHTS})
    for v in x.values():
        v.requires_grad_(requires_grad)
    return x


def scores(x, orders):
    """x: the 14 tensors by name; orders int64 [B][K][N] (permutations) -> nll [B][K]."""
    doc, okey, hist = x["doc"], x["okey"], x["hist"]
    B, N, H = doc.shape
    K = orders.shape[1]
    R = B * K
    y = orders.reshape(R, N)
    bidx = torch.arange(B).repeat_interleave(K)
    ridx = torch.arange(R)
    h, c = x["h0"][bidx], x["c0"][bidx]
    hist_r, okey_r = hist[bidx], okey[bidx]
    nll = doc.new_zeros(R)
    eye = torch.eye(N, dtype=torch.bool)
    for t in range(N - 1):
        xin = doc[bidx, y[:, t - 1]] if t > 0 else doc.new_zeros(R, H)
        gates = xin @ x["decoder.weight_ih_l0"].t() + x["decoder.bias_ih_l0"] + \
            h @ x["decoder.weight_hh_l0"].t() + x["decoder.bias_hh_l0"]
        i, f, g, o = gates.chunk(4, -1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        q = h @ x["query_linear.weight"].t() + x["query_linear.bias"]
        pointed = torch.zeros(R, N, dtype=torch.bool)
        if t > 0:
            pointed[ridx[:, None], y[:, :t]] = True
        alive = ~pointed
        mask = alive[:, :, None] & alive[:, None, :] & ~eye[None]
        live = hist_r * mask[..., None].to(hist_r.dtype)
        forw, back = live.mean(2), live.mean(1)
        zeros = hist_r.new_zeros(R, N, H + 2)
        l1 = hist_r[ridx, y[:, t - 1]] if t > 0 else zeros
        l2 = hist_r[ridx, y[:, t - 2]] if t > 1 else zeros
        keys = torch.cat([l1, l2, forw, back], -1) @ x["pw_k.weight"].t()
        a = torch.tanh(q[:, None] + keys + okey_r)
        e = a @ x["tanh_linear.weight"].reshape(-1) + x["tanh_linear.bias"].reshape(())
        e = e.masked_fill(pointed, -1e9)
        nll = nll - torch.log_softmax(e, -1)[ridx, y[:, t]]
    return nll.view(B, K)


def grads(case, orders, dnll, dtype):
    """Autograd gradients of sum(dnll * nll) at `dtype` -> (nll [B][K], {name: gradient})."""
    x = leaves(case, dtype)
    nll = scores(x, orders)
    if nll.requires_grad and orders.shape[-1] > 1:
        (nll * dnll.to(dtype)).sum().backward()
    return nll.detach(), {n: (torch.zeros_like(v) if v.grad is None else v.grad) for n, v in x.items()}


def all_perms(N):
    return torch.tensor(list(itertools.permutations(range(N))), dtype=torch.int64)


# ---- the losses, restated in numpy -----------------------------------------------------------------
def gain(order, gold, metric):
    """evaluate.cal_result's per-story accuracy / Kendall's tau of one order."""
    order, gold = list(order), list(gold)
    n = len(gold)
    if metric == "acc":
        return sum(a == b for a, b in zip(order, gold)) / n
    if n == 1:
        return 1.0
    g = set(itertools.combinations(gold, 2))
    p = set(itertools.combinations(order, 2))
    return 1 - 2 * (len(p) - len(p & g)) / (n * (n - 1) / 2)


def order_loss(nll, orders, gold, kind, metric="tau", alpha=1.0, margin=1.0, refs=None):
    """float64 numpy: nll [B][K], orders [B][K][N], gold [B][N] -> the mean loss over stories."""
    nll = np.asarray(nll, dtype=np.float64)
    orders, gold = np.asarray(orders), np.asarray(gold)
    B, K = nll.shape
    N = gold.shape[1]
    steps = max(N - 1, 1)
    out = []
    for b in range(B):
        if refs is None:
            ref = np.array([list(orders[b, k]) == list(gold[b]) for k in range(K)])
        else:
            ref = np.asarray(refs[b], dtype=bool)
        if kind == "risk":
            z = -alpha * nll[b]
            w = np.exp(z - z[np.isfinite(z)].max())
            w = w / w.sum()
            out.append(sum(w[k] * (1 - gain(orders[b, k], gold[b], metric)) for k in range(K)
                           if w[k] > 0))
        elif kind == "set_nll":
            z = -nll[b][ref]
            out.append(-(z.max() + np.log(np.exp(z - z.max()).sum())) / steps)
        else:
            right = nll[b][ref].min()
            wrong = nll[b][~ref].min() if (~ref).any() else np.inf
            out.append(max(0.0, margin + right - wrong) / steps)
    return float(np.mean(out))
