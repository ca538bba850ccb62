"""float64 numpy restatement of the posterior over orders (include/mmseq.h mmseq_order_posterior,
csrc/posterior.hip) and of the ancestral sampler's pick rule and uniforms (mmseq_order_sample,
csrc/beam.hip), plus the float64 step distributions of a beam_batch_ref.random_case that the CPU
tests drive them with. No torch in the reduction or the sampler's arithmetic.

Every sum of the reduction runs over the candidates in ascending index order (np.cumsum is
sequential), as the kernel's: the index outputs are compared for equality, ties included.
"""
import itertools

import numpy as np
import torch

import mlm_mask_ref as M
from oracle import berson_oracle as O

F32_OUT = ("logz", "position", "before", "entropy", "map_prob", "exp_acc", "exp_tau")
INT_OUT = ("map_index", "mbr_acc_index", "mbr_tau_index")


def _seqsum(a):
    """Sum over axis 0 in index order."""
    return np.cumsum(a, axis=0, dtype=np.float64)[-1]


def valid_rows(orders, nll):
    """orders [K][N] int64, nll [K] f32 -> bool [K]: finite score and a permutation of 0 .. N-1."""
    N = orders.shape[-1]
    return np.isfinite(nll) & (np.sort(orders, -1) == np.arange(N)).all(-1)


def gains(orders, position, before):
    """(gain_acc, gain_tau) float64 [K] of permutations `orders` [K][N] from the f32 matrices, in
    the stated order: t ascending; (i, j) lexicographic."""
    K, N = orders.shape
    position = np.asarray(position, np.float32)
    before = np.asarray(before, np.float32)
    acc = np.zeros(K, np.float64)
    for t in range(N):
        acc = acc + position[t, orders[:, t]].astype(np.float64)
    acc = acc / np.float64(N)
    tau = np.zeros(K, np.float64)
    for i in range(N):
        for j in range(i + 1, N):
            tau = tau + (before[orders[:, i], orders[:, j]].astype(np.float64)
                         - before[orders[:, j], orders[:, i]].astype(np.float64))
    tau = tau / np.float64(N * (N - 1) // 2) if N > 1 else np.ones(K, np.float64)
    return acc, tau


def posterior_story(orders, nll, mode):
    """One story: orders int64 [K][N], nll f32 [K], mode 0 (weights) / 1 (uniform) -> dict."""
    orders = np.asarray(orders, np.int64)
    nll = np.asarray(nll, np.float32)
    K, N = orders.shape
    ok = valid_rows(orders, nll)
    if not ok.any():
        z = np.zeros((N, N), np.float32)
        return dict(logz=np.float32(-np.inf), position=z, before=z.copy(), entropy=np.float32(0),
                    map_prob=np.float32(0), exp_acc=np.float32(0), exp_tau=np.float32(0),
                    map_index=-1, mbr_acc_index=-1, mbr_tau_index=-1)
    best = nll[ok].min()
    map_index = int(np.nonzero(ok & (nll == best))[0][0])  # -0.0 == +0.0
    if mode == 1:  # equal weights: all tie
        map_index = int(np.nonzero(ok)[0][0])
    x = np.where(ok, np.float64(best) - np.where(ok, nll, best).astype(np.float64), 0.0)
    if mode == 1:
        x = np.zeros(K, np.float64)
    w = np.where(ok, np.exp(x) if mode == 0 else 1.0, 0.0)
    Z, WX = _seqsum(w), _seqsum(w * x)
    safe = np.where(ok[:, None], orders, np.arange(N)[None])
    inv = np.argsort(safe, -1)  # inv[k][s] = position of step s
    ar = np.arange(N)
    at = safe[:, :, None] == ar[None, None, :]              # [k][t][s]
    prec = inv[:, :, None] < inv[:, None, :]                # [k][a][c]
    P = _seqsum(w[:, None, None] * at)
    Bf = _seqsum(w[:, None, None] * prec)
    position = (P / Z).astype(np.float32)
    before = (Bf / Z).astype(np.float32)
    lz = np.log(Z)
    acc, tau = gains(safe, position, before)
    acc = np.where(ok, acc, -np.inf)
    tau = np.where(ok, tau, -np.inf)
    ia, it = int(np.argmax(acc)), int(np.argmax(tau))  # the first of equals
    return dict(logz=np.float32(lz - np.float64(best) if mode == 0 else lz), position=position,
                before=before, entropy=np.float32(lz - WX / Z), map_prob=np.float32(1.0 / Z),
                exp_acc=np.float32(acc[ia]), exp_tau=np.float32(tau[it]), map_index=map_index,
                mbr_acc_index=ia, mbr_tau_index=it)


def posterior_ref(orders, nll, mode):
    """orders [K][N] or [B][K][N], nll [B][K] -> dict of stacked arrays (f32 / int32)."""
    orders = np.asarray(orders, np.int64)
    nll = np.asarray(nll, np.float32)
    rows = [posterior_story(orders if orders.ndim == 2 else orders[b], nll[b], mode)
            for b in range(nll.shape[0])]
    out = {k: np.stack([np.asarray(r[k], np.float32) for r in rows]) for k in F32_OUT}
    out.update({k: np.array([r[k] for r in rows], np.int32) for k in INT_OUT})
    return out


def marginals64(perms, p):
    """(position, before) float64 [N][N] of permutations `perms` [K][N] under weights p [K]
    (normalised here), straight from the definitions."""
    perms = np.asarray(perms, np.int64)
    p = np.asarray(p, np.float64)
    p = p / p.sum()
    N = perms.shape[1]
    inv = np.argsort(perms, -1)
    position = np.einsum("k,kts->ts", p, (perms[:, :, None] == np.arange(N)).astype(np.float64))
    before = np.einsum("k,kac->ac", p, (inv[:, :, None] < inv[:, None, :]).astype(np.float64))
    return position, before


# ------------------------------------------------------------------------------------- sampler
def uniforms(B, S, N, seed, stream_id=0, story0=0, sample0=0):
    """u f32 [B][S][N-1] of mmseq_order_sample: the two-round counter hash of mmseq_mlm_mask at
    element (story0 + b) 2^32 + (sample0 + s)(N - 1) + t, u = (h >> 8) 2^-24. Story 0 from
    sample 0 is mlm_mask_ref.hashes(S (N - 1), seed, stream_id)[0]."""
    k0, k1 = M.key_of(seed, stream_id)
    s, t = np.meshgrid(np.arange(S, dtype=np.uint64), np.arange(N - 1, dtype=np.uint64),
                       indexing="ij")
    lo = M._u32((np.uint64(sample0) + s) * np.uint64(N - 1) + t)
    out = np.empty((B, S, N - 1), np.float32)
    for b in range(B):
        hi = np.uint64(story0 + b)
        h = M.lowbias32(M._u32(M.lowbias32(lo ^ np.uint64(k0)) + (hi ^ np.uint64(k1))))
        out[b] = ((h >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    return out


def pick_ref(row, u):
    """The pick from one row of -log p (+inf where pointed) and its uniform, in float64 ->
    (j, margin): j the first unpointed step whose running sum of exp(-row) exceeds u * total,
    else the last unpointed one; margin = the smallest |running sum - u * total| / total over the
    cumulative boundaries (how close the draw is to flipping under another rounding)."""
    row = np.asarray(row, np.float64)
    live = np.nonzero(np.isfinite(row))[0]
    cum = np.cumsum(np.exp(-row[live]))
    thr = np.float64(u) * cum[-1]
    over = np.nonzero(cum > thr)[0]
    j = int(live[over[0]]) if over.size else int(live[-1])
    return j, float(np.abs(cum - thr).min() / cum[-1])


# ----------------------------------------------------- float64 step distributions of a case
def case64(case):
    """A beam_batch_ref.random_case with every tensor in float64."""
    out = {k: (v.double() if torch.is_tensor(v) else v) for k, v in case.items()}
    out["p"] = {k: v.double() for k, v in case["p"].items()}
    return out


def step_rows64(case, b):
    """{prefix tuple of length 0 .. N-2: float64 row [N] of -log p, +inf where pointed} for story
    b of a case64: BertForOrdering.step (modeling_bert.py:1368-1402) in the reference's dense
    formulation, as beam_batch_ref.order_score, along every prefix."""
    p, N, H = case["p"], case["N"], case["H"]
    doc, okeys, hist = case["doc"][b], case["okey"][b:b + 1], case["hist"][b:b + 1]
    rows = {}

    def walk(prefix, h, c):
        t = len(prefix)
        if t >= N - 1:
            return
        x = doc[prefix[-1]][None] if t > 0 else torch.zeros(1, H, dtype=torch.float64)
        pointed = torch.zeros(1, N, dtype=torch.bool)
        pointed[0, list(prefix)] = True
        live = (~pointed[0]).double()
        mask = live[:, None] * live[None, :] * (1 - torch.eye(N, dtype=torch.float64))
        rela = hist * mask[None, :, :, None]
        zeros = torch.zeros(1, N, H + 2, dtype=torch.float64)
        left1 = hist[:, prefix[-1]] if t > 0 else zeros
        left2 = hist[:, prefix[-2]] if t > 1 else zeros
        h2, c2 = O.lstm_cell(p, x, h, c)
        q = O.linear(h2, p, "query_linear")[:, None]
        keys = O.linear(torch.cat([left1, left2, rela.mean(2), rela.mean(1)], -1), p, "pw_k",
                        bias=False)
        e = O.linear(torch.tanh(q + keys + okeys), p, "tanh_linear").squeeze(-1)
        e = e.masked_fill(pointed, -1e9)
        row = (-torch.log_softmax(e, -1))[0].numpy().copy()
        row[list(prefix)] = np.inf
        rows[prefix] = row
        for j in range(N):
            if j not in prefix:
                walk(prefix + (j,), h2, c2)

    walk((), case["h0"][b:b + 1], case["c0"][b:b + 1])
    return rows


def all_perms(N):
    return np.array(list(itertools.permutations(range(N))), np.int64).reshape(-1, N)


def nll64(rows, orders):
    """float64 NLLs of `orders` [K][N] from step_rows64's rows, summed in step order."""
    out = np.zeros(len(orders), np.float64)
    for k, o in enumerate(orders):
        o = tuple(int(v) for v in o)
        for t in range(len(o) - 1):
            out[k] += rows[o[:t]][o[t]]
    return out


def sample_ref(rows, u):
    """Ancestral samples of one story: rows from step_rows64, u [S][N-1] -> orders int64 [S][N]."""
    S = u.shape[0]
    N = u.shape[1] + 1
    out = np.zeros((S, N), np.int64)
    for s in range(S):
        prefix = ()
        for t in range(N - 1):
            prefix = prefix + (pick_ref(rows[prefix], u[s, t])[0],)
        out[s] = prefix + tuple(sorted(set(range(N)) - set(prefix)))
    return out
