"""float64 numpy restatement of the pairwise head's decode (include/mmseq.h mmseq_pairwise_order /
mmseq_pairwise_score, csrc/pairwise.hip) and a vectorised brute force over all N! orders to check
it against. No torch.

w [N][N]: w[a][c] = the log-evidence that step a precedes step c; the diagonal is never read.
G(o) = sum_{i<j} w[o_i][o_j], pnll = -G, Q(o) = exp(G(o)) / Z. The restatement walks the 2^N
subsets S of steps already placed in the order the header states: g(S, c) adds w[a][c] over a in S
ascending from 0.0 (so g(S) = g(S without its highest step) + that step's row), every
log-sum-exp runs over c ascending shifted by its largest term, every marginal over S ascending.
np.cumsum is sequential, so the max path (additions and comparisons alone) is the kernel's bit for
bit; the exp / log of the distribution are numpy's.
"""
import itertools

import numpy as np

F32_OUT = ("pnll", "margin", "logz", "position", "before", "entropy")


def _seqsum(a, axis=0):
    """Sum along `axis` in index order."""
    if np.shape(a)[axis] == 0:
        return np.zeros(np.delete(np.shape(a), axis), np.float64)
    return np.take(np.cumsum(a, axis=axis, dtype=np.float64), -1, axis=axis)


def all_perms(N):
    return np.array(list(itertools.permutations(range(N))), np.int64).reshape(-1, N)


def pair_list(N):
    """The pair order of the encoder (process_inputs.pairs_generator): i < j, then reversed."""
    one = list(itertools.combinations(range(N), 2))
    return one + [(c, a) for a, c in one]


def weights_from_logits(cs):
    """cs [N][N][2] logits -> w float64 [N][N] in float64 arithmetic, diagonal 0."""
    cs = np.asarray(cs, np.float64)
    m = cs.max(-1, keepdims=True)
    ls = cs - (m + np.log(np.exp(cs - m).sum(-1, keepdims=True)))
    w = ls[..., 1] + ls[..., 0].T
    np.fill_diagonal(w, 0.0)
    return w


def weights_from_pairs(cls_score, N):
    """cls_score [N(N-1)][2], row j the logits of pair pair_list(N)[j] -> w float64 [N][N]."""
    cs = np.zeros((N, N, 2), np.float64)
    for j, (a, c) in enumerate(pair_list(N)):
        cs[a, c] = np.asarray(cls_score[j], np.float64)
    return weights_from_logits(cs)


def random_weights(N, seed):
    """w f32 [N][N] from seeded N(0, 1) f32 logits, log_softmax in f32."""
    cs = np.random.RandomState(seed).standard_normal((N, N, 2)).astype(np.float32)
    m = cs.max(-1, keepdims=True)
    ls = (cs - (m + np.log(np.exp(cs - m).sum(-1, keepdims=True, dtype=np.float32)))).astype(
        np.float32)
    w = (ls[..., 1] + ls[..., 0].T).astype(np.float32)
    np.fill_diagonal(w, 0.0)
    return w


def dyadic_weights(N, seed):
    """w f32 [N][N], multiples of 0.25 in [-1, 0]: every f64 sum of them is exact, ties abound."""
    w = (np.random.RandomState(seed).randint(-4, 1, (N, N)) * 0.25).astype(np.float32)
    np.fill_diagonal(w, 0.0)
    return w


def _finite_off_diagonal(w):
    N = w.shape[0]
    return bool(np.isfinite(w[~np.eye(N, dtype=bool)]).all())


def _invalid(N):
    z = np.zeros((N, N), np.float32)
    return dict(order=np.full(N, -1, np.int64), pnll=np.float32(np.inf), margin=np.float32(0),
                logz=np.float32(-np.inf), position=z, before=z.copy(), entropy=np.float32(0))


def _lse(x):
    """log sum exp(x) over a 1-D x in index order, shifted by the largest entry."""
    m = x.max()
    return m + np.log(_seqsum(np.exp(x - m)))


def pairwise_order_ref(w, rounded=True):
    """One story: w [N][N] (f32 values) -> dict order int64 [N], pnll, margin, logz, entropy,
    position, before [N][N]; rounded once to f32 (rounded=False: the float64 values)."""
    w32 = np.asarray(w, np.float32)
    N = w32.shape[0]
    if not _finite_off_diagonal(w32):
        return _invalid(N)
    wd = w32.astype(np.float64)
    np.fill_diagonal(wd, 0.0)
    states, full = 1 << N, (1 << N) - 1
    g = np.zeros((states, N), np.float64)  # g[S][c]
    for S in range(1, states):
        hb = S.bit_length() - 1
        rest = S ^ (1 << hb)
        g[S] = g[rest] + wd[hb]  # g[0] = 0.0: the sum starts from 0.0
    bits = 1 << np.arange(N)
    free = [np.flatnonzero((S & bits) == 0) for S in range(states)]
    # the optimum
    h1 = np.full(states, -np.inf)
    h2 = np.full(states, -np.inf)
    h1[full] = 0.0
    for S in range(full - 1, -1, -1):
        c = free[S]
        T = S | bits[c]
        vals = np.sort(np.concatenate([g[S, c] + h1[T], g[S, c] + h2[T]]))
        h1[S], h2[S] = vals[-1], vals[-2]
    order, S = [], 0
    for _ in range(N):
        c = free[S]
        hit = c[g[S, c] + h1[S | bits[c]] == h1[S]]
        order.append(int(hit[0]))
        S |= 1 << order[-1]
    # the distribution
    la = np.zeros(states)
    lb = np.zeros(states)
    for T in range(1, states):
        c = np.flatnonzero(T & bits)
        la[T] = _lse(la[T ^ bits[c]] + g[T ^ bits[c], c])
    for S in range(full - 1, -1, -1):
        c = free[S]
        lb[S] = _lse(g[S, c] + lb[S | bits[c]])
    lz = la[full]
    Sall = np.arange(states)
    out_of = (Sall[:, None] & bits[None]) == 0  # [S][c]: c not in S
    p = np.where(out_of, np.exp(((la[:, None] + g) + lb[Sall[:, None] | bits[None]]) - lz), 0.0)
    pop = np.array([bin(S).count("1") for S in range(states)])
    position = np.stack([_seqsum(np.where((pop == t)[:, None], p, 0.0)) for t in range(N)])
    before = np.stack([_seqsum(np.where(~out_of[:, a:a + 1], p, 0.0)) for a in range(N)])
    np.fill_diagonal(before, 0.0)
    off = ~np.eye(N, dtype=bool)
    entropy = lz - _seqsum((before * wd)[off])  # row-major: (a, c) lexicographic
    res = dict(order=np.array(order, np.int64), pnll=-h1[0], margin=h1[0] - h2[0], logz=lz,
               position=position, before=before, entropy=entropy)
    if rounded:
        res = {k: (v if k == "order" else np.float32(v)) for k, v in res.items()}
    return res


def pairwise_order_batch_ref(w):
    """w [B][N][N] -> the dict of stacked per-story results."""
    per = [pairwise_order_ref(x) for x in w]
    return {k: np.stack([r[k] for r in per]) for k in per[0]}


def pairwise_score_ref(w, orders):
    """w [N][N] f32, orders [K][N] int64 -> pnll f32 [K]: -sum_{i<j} w[o_i][o_j], (i, j)
    lexicographic, in float64; +inf for a candidate that is no permutation or a non-finite w."""
    w32 = np.asarray(w, np.float32)
    o = np.asarray(orders, np.int64)
    K, N = o.shape
    ok = (np.sort(o, -1) == np.arange(N)).all(-1)
    if not _finite_off_diagonal(w32):
        ok[:] = False
    wd = w32.astype(np.float64)
    safe = np.where(ok[:, None], o, np.arange(N)[None])
    G = np.zeros(K, np.float64)
    for i in range(N):
        for j in range(i + 1, N):
            G = G + wd[safe[:, i], safe[:, j]]
    return np.where(ok, (-G).astype(np.float32), np.float32(np.inf)).astype(np.float32)


def brute_force(w):
    """All N! orders in float64 -> the same dict, unrounded, plus the runner-up's score."""
    wd = np.asarray(w, np.float32).astype(np.float64)
    N = wd.shape[0]
    perms = all_perms(N)
    G = np.zeros(len(perms), np.float64)
    for i in range(N):
        for j in range(i + 1, N):
            G = G + wd[perms[:, i], perms[:, j]]
    best = G.max()
    k = int(np.flatnonzero(G == best)[0])  # itertools order is lexicographic: the lowest index
    second = np.sort(G)[-2] if len(G) > 1 else -np.inf
    lz = best + np.log(np.exp(G - best).sum())
    p = np.exp(G - lz)
    position = np.stack([np.bincount(perms[:, t], weights=p, minlength=N) for t in range(N)])
    before = np.zeros(N * N)
    for i in range(N):
        for j in range(i + 1, N):
            before += np.bincount(perms[:, i] * N + perms[:, j], weights=p, minlength=N * N)
    return dict(order=perms[k], pnll=-best, margin=best - second, logz=lz, position=position,
                before=before.reshape(N, N), entropy=-(p * (G - lz)).sum(), G=G)
