"""Per-row accuracy of the bf16 fast attention kernels: float64 reference, a float64 emulation
that rounds to bf16 where the kernels do, and the metric that compares the two errors.

All tensors are [P][heads][T][64] float64 holding bf16 values widened (the reference sees exactly
what the kernel sees); bias [P][T] additive or None; keep [P][heads][T][T] = the dropout
multiplier (0 or 1/(1-p)) or None.

Rounding sites of the kernels (multimodal_sequencing_amd/csrc/attention.hip), all reproduced by
`emulate`:
  forward (attn_fwd_bf16_kernel `tile`, attn_fwd_tail, attn_fwd32_kernel)
    F1  the unnormalised probabilities exp2(s - m) are packed to bf16 before P V
        (`pf[grp][..] = pack_pair(s...)`)
    F2  the softmax denominator is the sum of those bf16 values (`mma(ones, pf, ...)`: "row sums
        of the bf16 P"), so the LSE the backward reads carries their rounding too
    F3  dropout zeroes dropped entries of the packed bf16 P (`keep_apply2`); 1/(1-p) is applied
        in fp32 with the final 1/l
    F4  the output is stored as bf16 (`Vec4<unsigned short>::st(op, o * inv)`)
  backward (attn_dq_bf16_kernel, attn_dkdv_bf16_kernel)
    B1  delta = rowsum(dO * O) from the STORED bf16 O, fp32 (`dot = fmaf(bf2f(x), bf2f(y), dot)`)
    B2  P is recomputed in fp32 as exp2(s c + bias - L) with the forward's L (F2)
    B3  P times the dropout multiplier is packed to bf16 before P^T dO
        (`pf[grp] = pack_pair(s[grp][0], s[grp][1])` in the dK/dV kernel)
    B4  dS = P (dP mk - delta) is packed to bf16 before dS K and dS^T Q (`dsf = pack_pair(dp...)`
        in both kernels); the softmax scale multiplies the fp32 sums afterwards
    B5  dQ, dK, dV are stored as bf16
Everything else (scores, dP, the sums over keys / queries) is fp32 in the kernels and float64
here: the factor `FACTOR` on the emulation's own error covers fp32 accumulation in tile order,
the exp2 approximations and the spread of a maximum over a few thousand rows.
"""
import torch

FACTOR = 4.0       # kernel row error <= FACTOR x the emulation's row error (both against float64)
FLOOR = 0.01       # of the median row norm of the reference tensor
FP32_ACC = 1e-5    # x sum |terms|: fp32 accumulation, for tensors whose reference is all zero
NAMES = ("out", "dq", "dk", "dv")


def bf(x):
    """Round float64 values to bf16 (through fp32, as the kernels' fp32 values are)."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _scores(q, k, bias, scale):
    s = torch.einsum("phqd,phkd->phqk", q, k) * scale
    if bias is not None:
        s = s + bias.to(s.dtype)[:, None, None, :]
    return s


def reference(q, k, v, bias, scale, keep, dout):
    """softmax(scale q k^T + bias) (* keep) v and its autograd gradient, float64. Also the sums of
    absolute terms of each output element ('*_terms'), the scale of its fp32 accumulation error."""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    s = _scores(q, k, bias, scale)
    lse = torch.logsumexp(s, -1)
    a = torch.softmax(s, -1)
    if keep is not None:
        a = a * keep
    out = a @ v
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), dout)
    r = {"out": out.detach(), "dq": dq, "dk": dk, "dv": dv, "lse": lse.detach()}
    with torch.no_grad():
        ad = a.detach()
        abs_s = ad * (dout.abs() @ v.abs().transpose(-1, -2) * (1 if keep is None else keep)
                      + (dout.abs() * out.abs()).sum(-1, keepdim=True)) * scale
        r["out_terms"] = ad @ v.abs()
        r["dv_terms"] = ad.transpose(-1, -2) @ dout.abs()
        r["dq_terms"] = abs_s @ k.abs()
        r["dk_terms"] = abs_s.transpose(-1, -2) @ q.abs()
    return r


def emulate(q, k, v, bias, scale, keep, dout):
    """The same operation with bf16 rounding at the kernels' sites (module docstring)."""
    s = _scores(q, k, bias, scale)
    m = s.max(-1, keepdim=True).values
    pt = bf(torch.exp(s - m))                                 # F1
    l = pt.sum(-1, keepdim=True)                              # F2
    if keep is not None:
        kept = (keep != 0).to(s.dtype)
        dscale = keep.max()
        out = bf(((pt * kept) @ v) * dscale / l)              # F3, F4
    else:
        out = bf((pt @ v) / l)                                # F4
    lse = (m + torch.log(l)).squeeze(-1)
    delta = (dout * out).sum(-1, keepdim=True)                # B1
    p = torch.exp(s - lse.unsqueeze(-1))                      # B2
    mk = 1.0 if keep is None else keep
    dv = bf(bf(p * mk).transpose(-1, -2) @ dout)              # B3, B5
    dp = dout @ v.transpose(-1, -2)
    ds = bf(p * (dp * mk - delta))                            # B4
    dq = bf((ds @ k) * scale)                                 # B5
    dk = bf((ds.transpose(-1, -2) @ q) * scale)               # B5
    return {"out": out, "dq": dq, "dk": dk, "dv": dv, "lse": lse}


def row_errors(got, ref):
    """Relative L2 error of every (token, head) 64-vector: |got - ref| / (|ref| + floor), floor =
    FLOOR x the median row norm of ref. Rows whose reference is zero (dK / dV of masked keys) are
    thereby held to FLOOR x a typical row, absolutely. Where more than half of the rows are zero
    (dK / dV with all but one key masked) the median is taken over the nonzero rows; None when the
    WHOLE reference is zero."""
    rn = ref.norm(dim=-1)
    floor = FLOOR * rn.flatten().median()
    if float(floor) == 0.0:
        if not bool((rn > 0).any()):
            return None
        floor = FLOOR * rn[rn > 0].median()
    return (got.to(ref.dtype) - ref).norm(dim=-1) / (rn + floor)


def judge(got, ref, emu, names=NAMES):
    """measure(), then AssertionError naming the tensors outside the bound."""
    res, bad = measure(got, ref, emu, names)
    assert not bad, "; ".join(bad)
    return res


def measure(got, ref, emu, names=NAMES):
    """-> ({name: (kernel max row error, emulation max row error)}, [a line per tensor whose
    kernel error exceeds FACTOR x the emulation's]).

    A tensor whose float64 reference is identically zero (dQ and dK when a single key is left
    unmasked: the softmax of one element has no gradient) has no row norm to be relative to, and
    the emulation, float64 where the kernel is fp32, may give no error to scale either. Such a
    tensor is held to the same rule in absolute terms: every row's norm within FACTOR x the
    emulation's largest row norm (nonzero with dropout: delta then comes from a rounded O) plus
    the fp32 accumulation error of the row's own sums, FP32_ACC x |sum |terms|| (the bound `delta`
    is held to). A row whose terms are all zero (a masked key's dK) must be exactly zero. The
    entry reports (largest row norm of got, of the emulation)."""
    res, bad = {}, []
    for n in names:
        ek = row_errors(got[n], ref[n])
        if ek is None:
            gn, en = got[n].double().norm(dim=-1), emu[n].norm(dim=-1).max()
            tn = ref[n + "_terms"].norm(dim=-1)
            allow = torch.where(tn > 0, FACTOR * en + FP32_ACC * tn, torch.zeros_like(tn))
            res[n] = (gn.max().item(), en.item())
            over = (gn - allow).max().item()
            if over > 0:
                bad.append(f"{n}: reference is zero, a row of got exceeds its allowance by {over:.3e}")
            continue
        k, e = ek.max().item(), row_errors(emu[n], ref[n]).max().item()
        res[n] = (k, e)
        if not k <= FACTOR * e:
            bad.append(f"{n}: kernel row error {k:.3e} > {FACTOR:g} x emulation {e:.3e}")
    return res, bad


def split_qkv(qkv, P, T, heads, q_off, k_off, v_off):
    """[P*T][ld] rows -> q, k, v [P][heads][T][64] float64."""
    def sl(off):
        return qkv[:, off:off + heads * 64].reshape(P, T, heads, 64).permute(0, 2, 1, 3).double()
    return sl(q_off), sl(k_off), sl(v_off)


def rows_to_heads(x, P, T, heads):
    """[P*T][>= heads*64] -> [P][heads][T][64] float64."""
    return x[:, :heads * 64].reshape(P, T, heads, 64).permute(0, 2, 1, 3).double()


def key_bias(pattern, P, T, gen):
    """[P][T] additive key bias (0 / -10000) or None. Every pattern leaves at least one key."""
    if pattern == "none":
        return None
    b = torch.zeros(P, T)
    if pattern == "random30":      # key 0 may be masked
        b[torch.rand(P, T, generator=gen) <= 0.3] = -10000.0
        for p in range(P):
            if bool((b[p] != 0).all()):
                b[p, T // 2] = 0.0
    elif pattern == "first_tile":  # the whole first 64-key tile
        assert T > 64
        b[:, :64] = -10000.0
    elif pattern == "last_tile":   # the whole last key tile (one key at T = 64 n + 1)
        assert T > 64
        b[:, (T - 1) // 64 * 64:] = -10000.0
    elif pattern == "one_key":     # all but one key
        b[:] = -10000.0
        for p in range(P):
            b[p, (T // 2 + 5 * p) % T] = 0.0
    else:
        raise ValueError(pattern)
    return b


def make_inputs(P, T, heads, gen, dtype=torch.bfloat16):
    """q, k, v, dout [P][heads][T][64] with the two sequences and the two heads scaled
    differently, so that a bleed between sequences or heads shows in the per-row metric. The
    factors stay <= 1: scores of unit variance or less keep the softmax flat enough that the
    emulation's own dQ error stays near 0.4 % per row. (With q, k scaled by 1.75 the rows with a
    nearly one-hot softmax lose dQ to the cancellation dP - delta, delta coming from the bf16 O
    (site B1), the emulation itself is 5-15 % off on them and FACTOR x that rejects nothing.)"""
    x = torch.randn(4, P, heads, T, 64, generator=gen)
    ps = torch.tensor([1.0, 0.5, 0.8, 0.6])[:P].view(1, P, 1, 1, 1)
    hs = torch.tensor([1.0, 0.7, 0.85, 0.55])[:heads].view(1, 1, heads, 1, 1)
    x = (x * ps * hs).to(dtype)
    return x[0], x[1], x[2], x[3]
