"""References and case builders for the embedding kernels (csrc/embed.hip); no GPU involved.

  embed_ln_ref     word + position + token-type embedding, LayerNorm, and its backward: the three
                   table gradients with padding_idx = 0, dgamma, dbeta
  vit_im2col_ref   the per-pair image gather + patchify, through unfold
  vit_embed_ref    class token + patch rows + the img_len = 2 position rows cat([pos, pos[:gg]]),
                   ln_pre, and its backward

Each is a closed formula in the dtype asked for (float64 for the tests, float32 for the fp32-miss
figures); autograd is used for the LayerNorm backward only. `act` is the storage type of the
activations: with bfloat16 the reference starts from the bf16-rounded inputs, and the ViT one
normalises the bf16-rounded x, which is what the kernel stores and its backward re-reads.

  ids_from_counts  a row-order id vector whose sorted run layout is exactly `counts`
  chunk_cases      which cases of the chunked table gradient a run layout reaches, restated from
                   the comment above seg_rows_kernel
"""
import torch

F64 = torch.float64


def gen(*seed):
    seed = [s for x in seed for s in (x if isinstance(x, tuple) else (x,))]
    return torch.Generator().manual_seed(sum(int(s) * 1009 ** i for i, s in enumerate(seed)) + 4321)


# -------------------------------------------------------------------------------------------------
# LayerNorm
# -------------------------------------------------------------------------------------------------
def layer_norm(x, gamma, beta, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    rs = (var + eps).rsqrt()
    return (x - mu) * rs * gamma + beta, mu.squeeze(-1), rs.squeeze(-1)


def layer_norm_bwd(x, gamma, beta, eps, dy):
    x_, g_, b_ = (t.detach().clone().requires_grad_(True) for t in (x, gamma, beta))
    y, _, _ = layer_norm(x_, g_, b_, eps)
    return torch.autograd.grad(y, (x_, g_, b_), dy)


def _act(t, act, dtype):
    return t.to(act).to(dtype)


# -------------------------------------------------------------------------------------------------
# text embedding
# -------------------------------------------------------------------------------------------------
def embed_inputs(P, Lt, H, V, NT, seed, ids=None, tt="random", dj_scale=1.0):
    """ids [P][Lt] in [0, V) and tt [P][Lt] in [0, NT) (random unless given; tt = None: no token
    types), the three tables (pos with two rows past Lt, which nothing may touch), gamma, beta and
    the gradient of the text rows."""
    g = gen(seed, P, Lt, H)
    if ids is None:
        ids = torch.randint(0, V, (P, Lt), generator=g)
    if isinstance(tt, str):
        tt = torch.randint(0, NT, (P, Lt), generator=g)
    return dict(ids=ids.reshape(P, Lt), tt=None if tt is None else tt.reshape(P, Lt),
                word=torch.randn(V, H, generator=g), pos=torch.randn(Lt + 2, H, generator=g),
                typ=torch.randn(NT, H, generator=g), gamma=1 + 0.1 * torch.randn(H, generator=g),
                beta=0.1 * torch.randn(H, generator=g), eps=1e-12,
                dj=torch.randn(P, Lt, H, generator=g) * dj_scale)


def embed_ln_ref(d, dtype=F64, act=torch.float32):
    ids, tt = d["ids"], d["tt"]
    P, Lt = ids.shape
    word, pos, typ, gamma, beta = (d[k].to(dtype) for k in ("word", "pos", "typ", "gamma", "beta"))
    H = word.shape[1]
    ty = torch.zeros_like(ids) if tt is None else tt
    e = word[ids] + pos[:Lt][None] + typ[ty]
    y, mu, rs = layer_norm(e, gamma, beta, d["eps"])
    de, dgamma, dbeta = layer_norm_bwd(e, gamma, beta, d["eps"], _act(d["dj"], act, dtype))
    dword = torch.zeros_like(word).index_add_(0, ids.reshape(-1), de.reshape(-1, H))
    dtyp = torch.zeros_like(typ).index_add_(0, ty.reshape(-1), de.reshape(-1, H))
    dpos = torch.zeros_like(pos)
    dpos[:Lt] = de.sum(0)
    dword[0] = 0  # padding_idx = 0 on all three tables
    dtyp[0] = 0
    dpos[0] = 0
    return dict(y=y, mean=mu, rstd=rs, de=de, dword=dword, dtyp=dtyp, dpos=dpos, dgamma=dgamma,
                dbeta=dbeta)


# -------------------------------------------------------------------------------------------------
# ViT patches and embedding
# -------------------------------------------------------------------------------------------------
def vit_im2col_ref(images, pairs, ps):
    """images [B][N][3][R][R], pairs [B][npair][2] -> [B * npair * 2 * gg][3 ps^2]."""
    B, N, _, R, _ = images.shape
    imgs = images[torch.arange(B)[:, None, None], pairs].reshape(-1, 3, R, R)
    gg = (R // ps) ** 2
    return torch.nn.functional.unfold(imgs, ps, stride=ps).transpose(1, 2).reshape(imgs.shape[0] * gg, -1)


def vit_inputs(P, gg, W, seed):
    g = gen(seed, P, gg, W)
    ntok = 1 + 2 * gg
    return dict(gg=gg, po=torch.randn(P, 2 * gg, W, generator=g), cls=torch.randn(W, generator=g),
                pos=torch.randn(gg + 1, W, generator=g), gamma=1 + 0.1 * torch.randn(W, generator=g),
                beta=0.1 * torch.randn(W, generator=g), eps=1e-5,
                dy=torch.randn(P, ntok, W, generator=g))


def vit_embed_ref(d, dtype=F64, act=torch.float32):
    gg = d["gg"]
    po = _act(d["po"], act, dtype)
    P, _, W = po.shape
    cls, pos, gamma, beta = (d[k].to(dtype) for k in ("cls", "pos", "gamma", "beta"))
    x = torch.cat([cls.expand(P, 1, W), po], 1) + torch.cat([pos, pos[:gg]], 0)[None]
    if act != torch.float32:
        x = x.float().to(act).to(dtype)  # the stored x: fp32 sum, rounded once
    y, mu, rs = layer_norm(x, gamma, beta, d["eps"])
    dx, dgamma, dbeta = layer_norm_bwd(x, gamma, beta, d["eps"], _act(d["dy"], act, dtype))
    row = torch.cat([torch.arange(gg + 1), torch.arange(gg)])  # token -> position row
    dpos = torch.zeros_like(pos).index_add_(0, row, dx.sum(0))
    return dict(x=x, y=y, mean=mu, rstd=rs, dx=dx, dpo=dx[:, 1:], dcls=dx[:, 0].sum(0), dpos=dpos,
                dgamma=dgamma, dbeta=dbeta)


# -------------------------------------------------------------------------------------------------
# run layouts of the chunked table gradient
# -------------------------------------------------------------------------------------------------
def ids_from_counts(counts, seed):
    """Id k occurs counts[k] times, the rows shuffled by a seeded permutation: sorted by (id, row)
    the runs are exactly `counts`, while the rows of a run lie scattered."""
    ids = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))
    out = torch.empty_like(ids)
    out[torch.randperm(ids.numel(), generator=gen(seed, 77))] = ids
    return out


def chunk_cases(counts, C=64):
    """The sorted positions are cut into chunks of C. A chunk sums each run of equal ids it holds;
    a piece that began in the chunk (it does not continue the previous chunk's last run) and ends
    in it (the next chunk does not continue it) goes to the table, every other piece to a slot,
    and the chunk where a crossing run began adds the later pieces in chunk order (the join). Id 0
    is the padding run, summed but never stored.

    Returns cases = {(padding, began, ends, "full" | "partial" chunk)}, joins = {pieces added
    after the first}, last_row_join = a crossing run ends on the last row of all."""
    ids = [k for k, c in enumerate(counts) for _ in range(c)]
    n = len(ids)

    def at(i):
        return ids[i] if 0 <= i < n else None

    cases = set()
    for c in range((n + C - 1) // C):
        i0 = c * C
        cnt = min(C, n - i0)
        start = 0
        for j in range(cnt):
            k = ids[i0 + j]
            if j < cnt - 1 and ids[i0 + j + 1] == k:
                continue
            began = start > 0 or at(i0 - 1) != k
            ends = j < cnt - 1 or at(i0 + cnt) != k
            cases.add((k == 0, began, ends, "full" if cnt == C else "partial"))
            start = j + 1
    joins, last_row_join, first = set(), False, 0
    for k, cnt in enumerate(counts):
        if k != 0 and cnt:
            pieces = (first + cnt - 1) // C - first // C
            if pieces:
                joins.add(pieces)
                last_row_join |= first + cnt == n
        first += cnt
    return dict(cases=cases, joins=joins, last_row_join=last_row_join)


# name -> counts from id 0 upward; (P, Lt) with P * Lt = n
LAYOUTS = {
    "a": [0, 64, 64, 64],        # runs that exactly fill chunks
    "b": [0, 63, 1, 64, 1, 63],  # runs ending one before, and on, a boundary
    "c": [0, 1, 192, 1],         # first piece, two whole-chunk middle pieces, tail in a 2-row chunk
    "d": [63, 65],               # padding run, then a run crossing once, ending on the last row
    "e": [130, 5, 200, 1],       # padding run crossing two boundaries; 16-row last chunk
    "f1": [0, 1],                # single chunk
    "f63": [0, 63],              # short chunk
    "f65": [0, 65],              # one-row last chunk
    "g": [0, 64, 129],           # join length 2
}
LAYOUT_SHAPE = {192: (12, 16), 194: (2, 97), 128: (8, 16), 336: (21, 16), 1: (1, 1), 63: (9, 7),
                65: (5, 13), 193: (1, 193)}
EXTRA_ROWS = 3  # table rows past the layout's ids: no row has them


def layout_case(name, role, H, seed=0):
    """The layout's counts as the word ids (role "word") or the token-type ids ("type"); the other
    table draws random ids."""
    counts = LAYOUTS[name]
    n = sum(counts)
    P, Lt = LAYOUT_SHAPE[n]
    run_ids = ids_from_counts(counts, seed).reshape(P, Lt)
    K = len(counts) + EXTRA_ROWS
    if role == "word":
        return embed_inputs(P, Lt, H, K, 3, (seed, 1), ids=run_ids)
    return embed_inputs(P, Lt, H, 50, K, (seed, 2), tt=run_ids)


HIGH_V = 70000


def high_id_case(seed=0):
    """300 rows, H = 4, ids up to V - 1 = 69999: id bits 16 .. 17 of the sort key's upper half. The
    70 rows of id 69999 end the sorted order and cross its last chunk boundary."""
    g = gen(seed, 3)
    ids = torch.randint(0, 10, (300,), generator=g)
    where = torch.randperm(300, generator=g)
    ids[where[:70]] = HIGH_V - 1
    ids[where[70:73]] = 65536
    ids[where[73]] = 65535
    ids[where[74]] = 40000
    return embed_inputs(20, 15, 4, HIGH_V, 2, (seed, 4), ids=ids)


ZIPF = (11, 233, 256)  # n = 2563: ragged in the 4-row, 64-row and 64-position senses at once
ZIPF_V = 3000


def zipf_case(seed=0):
    """Log-uniform ids over [0, 3000): id 0 (padding) and the small ids make runs of several
    chunks, most large ids occur once. dj has sigma 8, so that a row that occurs once still stands
    out of the bf16 tolerance of the tables."""
    P, Lt, H = ZIPF
    g = gen(seed, 5)
    ids = (ZIPF_V ** torch.rand(P, Lt, generator=g, dtype=F64)).long() - 1
    return embed_inputs(P, Lt, H, ZIPF_V, 3, (seed, 6), ids=ids.clamp_(0, ZIPF_V - 1), dj_scale=8.0)


def row_margin(table, ids, rtol, atol):
    """min over the occurring ids != 0 of max |reference row| / (atol + rtol max |reference row|): how
    many tolerances the smallest occurring row stands out of zero."""
    occ = torch.unique(ids)
    m = table[occ[occ != 0]].abs().amax(-1)
    return float((m / (atol + rtol * m)).min()) if m.numel() else float("inf")
