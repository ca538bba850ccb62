"""Host double of the batched device beam search (csrc/beam.hip, include/mmseq.h
mmseq_beam_search) and the seeded inputs its tests share.

`beam_batch_host` restates the KERNEL's formulation in torch on the CPU: fixed beam slots, the
four blocks of pw_k projected once per story, keys as sums of projected rows, the k smallest of
the flat scores by (score, flat index). `order_score` is the teacher-forced score of one order in
the REFERENCE's formulation (oracle.berson_oracle primitives, dense pw_k input), so the two
do not share the reordered sums. oracle.berson_oracle.beam_order is the expected order.
"""
import numpy as np
import torch

from oracle import berson_oracle as O

BOUND = 4e-4  # tests/test_order_gpu.py:100, the bound on pointer NLLs
SEED = 100
# (B, N, W, H): what each case can break
CASES = [(3, 5, 16, 128),   # base case
         (2, 3, 16, 128),   # k exceeds the unpointed count: pointed entries are selected
         (2, 9, 16, 128),   # flat size 144: more than two waves of entries in the selection
         (2, 5, 1, 128),    # greedy
         (2, 5, 3, 128),    # 15 flat entries, a beam that is no power of two
         (2, 2, 16, 128),   # a single step
         (33, 4, 16, 128),  # an odd story count above 32 (and pointed entries kept in the beam)
         (1, 5, 16, 1024)]  # the large models' width


def bound(score):
    return BOUND * max(1.0, abs(score))


def random_case(B, N, H, seed, tie=False):
    """Seeded decoder inputs and weights, scaled so that the pointer logits spread over a few
    nats (margins between hypotheses far above the fp32 noise)."""
    g = torch.Generator().manual_seed(seed)

    def rn(*shape, std=1.0):
        return torch.randn(*shape, generator=g) * std

    def un(*shape, b=1.0):
        return (torch.rand(*shape, generator=g) * 2 - 1) * b

    k = 1.0 / H ** 0.5
    p = {"decoder.weight_ih_l0": un(4 * H, H, b=k), "decoder.bias_ih_l0": un(4 * H, b=k),
         "decoder.weight_hh_l0": un(4 * H, H, b=k), "decoder.bias_hh_l0": un(4 * H, b=k),
         "query_linear.weight": rn(H, H, std=k), "query_linear.bias": rn(H, std=0.1),
         "pw_k.weight": rn(H, 4 * (H + 2), std=0.5 * k),
         "tanh_linear.weight": rn(1, H, std=3.0 * k), "tanh_linear.bias": rn(1, std=0.1)}
    if tie:
        p["tanh_linear.weight"] = torch.zeros(1, H)
    cls_mat = rn(B, N, N, H)
    cs_mat = rn(B, N, N, 2)
    return {"B": B, "N": N, "H": H, "p": p, "doc": rn(B, N, H), "okey": rn(B, N, H),
            "cls_mat": cls_mat, "cs_mat": cs_mat,
            "hist": torch.cat([cls_mat, torch.softmax(cs_mat, -1)], -1).contiguous(),
            "h0": rn(B, H, std=0.5), "c0": rn(B, H, std=0.5)}


def oracle_enc(case, b):
    """The slice of story b in the layout oracle.berson_oracle.beam_order reads."""
    s = slice(b, b + 1)
    return {"clean": case["doc"][s], "okey": case["okey"][s], "cls_mat": case["cls_mat"][s],
            "cs_mat": case["cs_mat"][s], "hcn": (case["h0"][s], case["c0"][s])}


def order_score(case, b, order):
    """Beam score of `order` for story b: sum over t < N - 1 of -log_softmax(e_t)[order[t]], in
    the reference's formulation (modeling_bert.py:1368-1402; oracle beam_order step by step)."""
    p, N, H = case["p"], case["N"], case["H"]
    doc, okeys, hist = case["doc"][b], case["okey"][b:b + 1], case["hist"][b:b + 1]
    h, c = case["h0"][b:b + 1], case["c0"][b:b + 1]
    rela = hist.clone()
    rela_mask = (1 - torch.eye(N, dtype=torch.long))[None].clone()
    pointed = torch.zeros(1, N, dtype=torch.long)
    x = torch.zeros(1, H)
    total = 0.0
    for t in range(N - 1):
        l1 = torch.zeros(1, N)
        l2 = torch.zeros(1, N)
        if t > 0:
            last = order[t - 1]
            x = doc[last][None]
            pointed[0, last] = 1
            rela_mask[0, :, last] = 0
            rela_mask[0, last] = 0
            l1[0, last] = 1
            if t > 1:
                l2[0, order[t - 2]] = 1
        h, c = O.lstm_cell(p, x, h, c)
        q = O.linear(h, p, "query_linear")[:, None]
        left1 = (hist * l1[:, :, None, None]).sum(1)
        left2 = (hist * l2[:, :, None, None]).sum(1)
        rela = rela * (rela_mask[..., None] != 0)
        keys = O.linear(torch.cat([left1, left2, rela.mean(2), rela.mean(1)], -1), p, "pw_k",
                        bias=False)
        e = O.linear(torch.tanh(q + keys + okeys), p, "tanh_linear").squeeze(-1)
        e = e.masked_fill(pointed == 1, -1e9)
        total = float(torch.tensor(total, dtype=torch.float32) - torch.log_softmax(e, -1)[0, order[t]])
    return total


def beam_batch_host(case, W):
    """-> (orders [B][N], best scores [B], final-step hypothesis scores per story ascending,
    per story the smallest gap over the steps between the last entry selected and the first one
    left out: the margin by which the beam's membership is decided; inf where all are taken)."""
    p, B, N, H = case["p"], case["B"], case["N"], case["H"]
    if N == 1:
        return [[0]] * B, [0.0] * B, [[0.0]] * B, [float("inf")] * B
    Wpw = p["pw_k.weight"].view(H, 4, H + 2)
    orders, bests, finals, cuts = [], [], [], []
    for b in range(B):
        hist, doc, okey = case["hist"][b], case["doc"][b], case["okey"][b]
        proj = [hist @ Wpw[:, g].t() for g in range(4)]  # [N][N][H] each
        gx = doc @ p["decoder.weight_ih_l0"].t() + p["decoder.bias_ih_l0"]
        seqs = [[]]
        score = torch.zeros(1)
        h, c = case["h0"][b:b + 1].clone(), case["c0"][b:b + 1].clone()
        cut = float("inf")
        for t in range(N - 1):
            nb = len(seqs)
            xg = torch.stack([gx[s[-1]] for s in seqs]) if t > 0 else p["decoder.bias_ih_l0"][None]
            gates = xg + (h @ p["decoder.weight_hh_l0"].t() + p["decoder.bias_hh_l0"])
            i, f, g, o = gates.chunk(4, -1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            q = h @ p["query_linear.weight"].t() + p["query_linear.bias"]
            e = torch.empty(nb, N)
            for w, s in enumerate(seqs):
                live = torch.ones(N, dtype=torch.bool)
                live[s] = False
                for j in range(N):
                    if not live[j]:
                        e[w, j] = -1e9
                        continue
                    key = torch.zeros(H)
                    if t > 0:
                        key = key + proj[0][s[-1], j]
                    if t > 1:
                        key = key + proj[1][s[-2], j]
                    m = live.clone()
                    m[j] = False
                    key = key + proj[2][j][m].sum(0) / N
                    key = key + proj[3][:, j][m].sum(0) / N
                    e[w, j] = (torch.tanh(q[w] + key + okey[j]) * p["tanh_linear.weight"][0]).sum() \
                        + p["tanh_linear.bias"][0]
            mx = e.max(-1, keepdim=True).values
            logp = (e - mx) - torch.log(torch.exp(e - mx).sum(-1, keepdim=True))
            flat = (score[:, None] - logp).reshape(-1).numpy()
            k = min(W, flat.size)
            srt = np.lexsort((np.arange(flat.size), flat))
            sel = srt[:k]
            if k < flat.size:
                cut = min(cut, float(flat[srt[k]] - flat[srt[k - 1]]))
            par = [int(ix) // N for ix in sel]
            seqs = [seqs[int(ix) // N] + [int(ix) % N] for ix in sel]
            score = torch.from_numpy(flat[sel].copy())
            h, c = h[par], c[par]
        best = seqs[0]
        orders.append(best + sorted(set(range(N)) - set(best))[:1])
        bests.append(float(score[0]))
        finals.append([float(v) for v in score])
        cuts.append(cut)
    return orders, bests, finals, cuts
