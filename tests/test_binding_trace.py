"""What the ctypes binding (`_native.py`) hands to the C ABI, pinned on the CPU against a recorded
fixture: the declared signature of every entry, and the arguments every public wrapper passes.

The recording fake of test_layer_trace stands in for the library. Every public wrapper of
`_native` that reaches the library is driven once per optional branch with the smallest valid CPU
tensors. A record has test_layer_trace's format with one strengthening: a non-null pointer is
recorded as the NAME this test gave the tensor (`name+bytes` for a pointer into it, `?` for a
buffer the wrapper allocates itself), so two pointer arguments that change places show up. Every
tensor has its own storage. A wrapper that returns an MXFP8 appends a pseudo-record
["MXFP8", q shape, q dtype, scales shape, scales dtype, rows, K, "zeros" | "empty"]: `torch.empty`
is replaced by one that fills uint8 buffers, so that scales the wrapper must zero are told from
scales it may leave as they come.

tests/golden/binding_trace.json holds `signatures` (entry -> [restype, [argtypes]], taken from
the hand-written table the binding had before it read include/mmseq.h) and `calls` (case -> its
records). Equality is exact. Regenerate (only for an intended change of the ABI or of a wrapper)
with

    python tests/test_binding_trace.py --write
"""
import ctypes
import json
import os
import sys

import pytest
import torch

from test_layer_trace import install

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "binding_trace.json")

F32, BF16, I64, I32, U8 = torch.float32, torch.bfloat16, torch.int64, torch.int32, torch.uint8
CTYPE_NAMES = {ctypes.c_int: "c_int", ctypes.c_int64: "c_int64", ctypes.c_float: "c_float",
               ctypes.c_double: "c_double", ctypes.c_uint32: "c_uint32",
               ctypes.c_uint64: "c_uint64", ctypes.c_void_p: "c_void_p",
               ctypes.c_char_p: "c_char_p"}


def _nat():
    from multimodal_sequencing_amd import _native
    return _native


def type_name(t):
    N = _nat()
    return "Rows" if t is N.Rows else "Dropout*" if t is N._dp else CTYPE_NAMES[t]


def signatures():
    return {name: [type_name(res), [type_name(a) for a in args]]
            for name, (res, args) in _nat()._SIGS.items()}


class Names:
    """Named zero tensors, each with its own storage, and the name of a pointer into one."""

    def __init__(self):
        self.tensors = {}

    def __call__(self, name, *shape, dtype=F32):
        assert name not in self.tensors and all(s > 0 for s in shape), name
        t = self.tensors[name] = torch.zeros(*shape, dtype=dtype)
        return t

    def of(self, ptr):
        for name, t in self.tensors.items():
            off = ptr - t.data_ptr()
            if 0 <= off < t.numel() * t.element_size():
                return name if off == 0 else f"{name}+{off}"
        return "?"


class NamedLib:
    """The recording fake, with every non-null pointer of a record replaced by its name."""

    def __init__(self, fake, names):
        self.fake, self.names = fake, names

    def __getattr__(self, name):
        entry = getattr(self.fake, name)
        argtypes = _nat()._SIGS[name][1]

        def named(*args):
            res = entry(*args)
            rec = self.fake.calls[-1]
            for k, (t, a) in enumerate(zip(argtypes, args)):
                if t is ctypes.c_void_p and rec[k + 1]:
                    rec[k + 1] = self.names.of(int(getattr(a, "value", a)))
            return res
        return named


def _mx(calls, m, rows, K):
    assert tuple(m.q.shape) == (rows, (K + 15) // 16 * 16) and m.q.dtype == U8
    assert m.scales.dim() == 1 and m.scales.dtype == U8 and (m.rows, m.K) == (rows, K)
    calls.append(["MXFP8", list(m.q.shape), str(m.q.dtype), list(m.scales.shape),
                  str(m.scales.dtype), m.rows, m.K, "empty" if bool(m.scales.any()) else "zeros"])


# ------------------------------------------------------------------------------------------------
# The cases: name -> f(N, t, calls); N = _native, t = Names, calls = the records so far (MXFP8
# pseudo-records are appended to it).
CASES = {}


def case(f):
    CASES[f.__name__] = f
    return f


def _drop(N):
    return N.drop(0.25, 3, 7)


@case
def gemm(N, t, calls):
    N.gemm(t("A", 4, 8), t("B", 6, 8), t("C", 4, 6), 4, 6, 8)
    N.gemm(t("A2", 2, 8, 4, dtype=BF16), t("B2", 2, 8, 6, dtype=BF16), t("C2", 2, 4, 10), 4, 6, 8,
           trans=1, lda=4, ldb=6, ldc=10, batch=2, sA=32, sB=48, sC=40, bias=t("bias", 6), act=2,
           aux=t("aux", 2, 4, 10), dact=t("dact", 2, 4, 10), resid=t("resid", 2, 4, 12), ldr=12,
           sR=48, alpha=0.5, accumulate=True, drop=_drop(N))
    N.gemm(t("A3", 4, 8), t("B3", 6, 8), t("C3", 4, 6), 4, 6, 8, resid=t("resid3", 4, 6))


@case
def gemm_wgrad(N, t, calls):
    N.gemm_wgrad(t("dy", 5, 6, dtype=BF16), t("x", 5, 8, dtype=BF16), t("gW", 6, 8))
    N.gemm_wgrad(t("dy2", 5, 10), t("x2", 5, 8), t("gW2", 6, 8), gb=t("gb", 6), lddy=10)


@case
def attention(N, t, calls):
    P, T, h = 2, 4, 1
    qkv, out, lse = t("qkv", 8, 192, dtype=BF16), t("out", 8, 64, dtype=BF16), t("lse", 2, 1, 4)
    N.attn_fwd(P, T, h, qkv, 192, 0, 64, 128, None, 0.125, out, 64, lse)
    bits = N.attn_keep_bits(P, T, h, "cpu")
    assert bits.dtype == I64 and tuple(bits.shape) == (4096,)
    t.tensors["bits"] = bits
    N.attn_fwd(P, T, h, qkv, 192, 0, 64, 128, t("kb", 2, 4), 0.125, out, 64, lse, drop=_drop(N),
               keep_bits=bits)
    dout, delta, dqkv = t("dout", 8, 64, dtype=BF16), t("delta", 2, 1, 4), t("dqkv", 8, 192, dtype=BF16)
    N.attn_bwd(P, T, h, qkv, 192, 0, 64, 128, None, 0.125, out, 64, dout, 64, lse, delta, dqkv, 192)
    N.attn_bwd(P, T, h, qkv, 192, 0, 64, 128, t.tensors["kb"], 0.125, out, 64, dout, 64, lse, delta,
               dqkv, 192, drop=_drop(N), keep_bits=bits)


@case
def attention_rows(N, t, calls):
    P, T, Tq, h = 2, 4, 3, 1
    qkv, out, lse = t("qkv", 8, 192, dtype=BF16), t("out", 6, 64, dtype=BF16), t("lse", 2, 1, 4)
    kb, bits = t("kb", 2, 4), t("bits", 16, dtype=I64)
    N.attn_fwd_rows(P, T, Tq, h, qkv, None, 0.125, out, lse)
    N.attn_fwd_rows(P, T, Tq, h, qkv, kb, 0.125, out, lse, drop=_drop(N), keep_bits=bits)
    dout, delta, dqkv = t("dout", 6, 64, dtype=BF16), t("delta", 2, 1, 4), t("dqkv", 8, 192, dtype=BF16)
    N.attn_bwd_rows(P, T, Tq, h, qkv, None, 0.125, out, dout, lse, delta, dqkv)
    N.attn_bwd_rows(P, T, Tq, h, qkv, kb, 0.125, out, dout, lse, delta, dqkv, drop=_drop(N),
                    keep_bits=bits)


@case
def small_attention(N, t, calls):
    B, T, h, d = 2, 3, 2, 4
    q, k, v = t("q", B, T, 8), t("k", B, T, 8), t("v", B, T, 8)
    out, probs = t("out", B, T, 8), t("probs", B, h, T, T)
    N.small_attn_fwd(B, T, h, d, q, k, v, None, 0.5, out, probs)
    N.small_attn_fwd(B, T, h, d, q, k, v, t("kb", B, T), 0.5, out, probs, drop=_drop(N))
    dout, dq, dk, dv = t("dout", B, T, 8), t("dq", B, T, 8), t("dk", B, T, 8), t("dv", B, T, 8)
    N.small_attn_bwd(B, T, h, d, q, k, v, probs, dout, 0.5, dq, dk, dv)
    N.small_attn_bwd(B, T, h, d, q, k, v, probs, dout, 0.5, dq, dk, dv, drop=_drop(N))


@case
def layernorm_fwd(N, t, calls):
    x, y = t("x", 4, 8, dtype=BF16), t("y", 4, 12)
    g, b, mean, rstd = t("gamma", 8), t("beta", 8), t("mean", 4), t("rstd", 4)
    N.layernorm_fwd(4, 8, x, N.rows(8), g, b, 1e-5, y, N.rows(12, 24, 2), mean, rstd)
    N.layernorm_fwd(4, 8, x, N.rows(8), g, b, 1e-5, y, N.rows(12), None, None, drop=_drop(N))
    _mx(calls, N.layernorm_fwd_mxfp8(4, 8, x, g, b, 1e-12), 4, 8)
    _mx(calls, N.layernorm_fwd_mxfp8(4, 8, x, g, b, 1e-12, y=t("y8", 4, 8, dtype=BF16), mean=mean,
                                     rstd=rstd), 4, 8)


def _ln_bwd_args(N, t):
    return (4, 8, t("dy", 4, 8), N.rows(8), t("x", 4, 8), N.rows(9), t("mean", 4), t("rstd", 4),
            t("gamma", 8), t("dx", 4, 8), N.rows(10), t("dres", 4, 8), N.rows(11), t("dgamma", 8),
            t("dbeta", 8))


@case
def layernorm_bwd(N, t, calls):
    a = _ln_bwd_args(N, t)
    dxd, dsum = t("dx_drop", 4, 8), t("dsum", 8)
    N.layernorm_bwd(*a)
    N.layernorm_bwd(*a, drop_dy=_drop(N), dx_drop=dxd, drop_dx=N.drop(0.5, 4, 9))
    N.layernorm_bwd(*a, dx_drop=dxd, drop_dx=_drop(N), dx_drop_rows=N.rows(12, 48, 2))
    N.layernorm_bwd(*a, dx_drop=dxd, drop_dx=_drop(N), dsum=dsum)
    N.layernorm_bwd(*a, drop_dy=_drop(N), dx_drop=dxd, dx_drop_rows=N.rows(12), dsum=dsum)
    N.layernorm_bwd(*a, dsum=dsum, dsum_with_dres=True)
    with pytest.raises(ValueError, match="dsum without dx_drop"):
        N.layernorm_bwd(*a, dsum=dsum)
    no_dres = a[:11] + (None,) + a[12:]
    N.layernorm_bwd(*no_dres, dsum=dsum)


@case
def layernorm_bwd_mxfp8(N, t, calls):
    a = _ln_bwd_args(N, t)
    _mx(calls, N.layernorm_bwd_mxfp8(*a), 4, 8)
    _mx(calls, N.layernorm_bwd_mxfp8(*a, drop_dy=_drop(N), dx_drop=t("dx_drop", 4, 8),
                                     drop_dx=N.drop(0.5, 4, 9)), 4, 8)


@case
def embeddings(N, t, calls):
    P, Lt, H = 2, 3, 8
    ids, tt = t("ids", P, Lt, dtype=I64), t("tt", P, Lt, dtype=I64)
    word, pos, typ, g, b = t("word", 5, H), t("pos", 4, H), t("typ", 2, H), t("gamma", H), t("beta", H)
    joint, mean, rstd = t("joint", P, 5, H, dtype=BF16), t("mean", 6), t("rstd", 6)
    N.embed_ln_fwd(P, Lt, H, ids, tt, word, pos, typ, g, b, 1e-12, joint, 40, mean, rstd)
    N.embed_ln_fwd(P, Lt, H, ids, None, word, pos, typ, g, b, 1e-12, joint, 40, mean, rstd,
                   drop=_drop(N))
    grads = [t(n, *s) for n, s in (("dword", (5, H)), ("dpos", (4, H)), ("dtyp", (2, H)),
                                   ("dgamma", (H,)), ("dbeta", (H,)))]
    dj = t("djoint", P, 5, H, dtype=BF16)
    N.embed_ln_bwd(P, Lt, H, ids, tt, word, pos, typ, g, mean, rstd, dj, 40, *grads)
    N.embed_ln_bwd(P, Lt, H, ids, tt, word, pos, typ, g, mean, rstd, dj, 40, *grads, drop=_drop(N))


@case
def vit_embed(N, t, calls):
    N.vit_im2col(2, 3, 6, 4, 2, t("images", 2, 3, 3, 4, 4), t("pairs", 2, 6, 2, dtype=I64),
                 t("patches", 96, 16, dtype=BF16))
    P, ntok, W = 2, 9, 8
    x, y, mean, rstd = t("x", P, ntok, W), t("y", P, ntok, W), t("mean", 18), t("rstd", 18)
    N.vit_embed_fwd(P, ntok, W, 4, t("patch_out", P, 8, W), t("cls", W), t("pos", 5, W),
                    t("gamma", W), t("beta", W), 1e-5, x, y, mean, rstd)
    N.vit_embed_bwd(P, ntok, W, 4, t("dy", P, ntok, W), x, mean, rstd, t.tensors["gamma"],
                    t("dpatch", P, 8, W), t("dcls", W), t("dpos", 5, W), t("dgamma", W),
                    t("dbeta", W))


@case
def elementwise(N, t, calls):
    N.cast(t("src", 6), t("dst", 6, dtype=BF16))
    N.transpose_cast_batch(t("desc", 2, 5, dtype=I64), 3, t("tsrc", 40), t("tdst", 40, dtype=BF16))
    N.transpose_cast(t("m", 3, 5), t("mt", 5, 3, dtype=BF16))
    N.colsum(t("cx", 4, 8, dtype=BF16), 4, 6, 8, t("cout", 6))
    N.colsum(t.tensors["cx"], 4, 6, 8, t.tensors["cout"], accumulate=False)
    N.act_fwd(t("ax", 7), t("ay", 7), 2)
    N.act_bwd(t("az", 7, dtype=BF16), t("ady", 7, dtype=BF16), t("adz", 7, dtype=BF16), 4)
    N.dropout(t("dx", 9), t("dy", 9), _drop(N))
    N.dropout(t.tensors["dx"], t.tensors["dx"], None)
    N.sumsq(t("sx", 11), t("sout", 1))
    p, g, m, v = t("ap", 10), t("ag", 10), t("am", 10), t("av", 10)
    N.adamw(p, g, m, v, t("mask", 10, dtype=U8), 1e-3, 0.9, 0.999, 1e-6, 0.01, 3, 1.0,
            t("ss", 1), t("shadow", 10, dtype=BF16))
    N.adamw(p, g, m, v, None, 1e-3, 0.9, 0.999, 1e-6, 0.0, 4, 0.0, None, None)


@case
def pointer(N, t, calls):
    B, n, H = 2, 4, 8
    q, key, okey, w, wb = t("q", B, n, H), t("key", B, n, n, H), t("okey", B, n, H), t("w", H), t("wb", 1)
    pointed, tl, tg = t("pointed", B, n, n, dtype=U8), t("tgt_len", B, dtype=I64), t("target", B, n, dtype=I64)
    logp, nll = t("logp", B, n, n), t("nll", B, n)
    N.pointer_fwd(B, n, H, q, key, okey, w, wb, pointed, tl, tg, logp, nll)
    N.pointer_fwd(B, n, H, q, key, okey, w, None, pointed, tl, tg, logp, nll)
    N.pointer_bwd(B, n, H, q, key, okey, w, logp, pointed, tl, tg, t("dnll", B, n), t("dq", B, n, H),
                  t("dkey", B, n, n, H), t("dokey", B, n, H), t("dw", H), t("dwb", 1))


@case
def span_pool(N, t, calls):
    P, Lt, H = 2, 3, 8
    top, score, sep = t("top", P, 5, H, dtype=BF16), t("score", P, Lt), t("sep", P, 2, dtype=I64)
    probs, mix = t("probs", P, 2, Lt), t("mix", P, 2, H)
    N.span_pool_fwd(P, Lt, H, top, 40, score, sep, probs, mix)
    N.span_pool_fwd(P, Lt, H, top, 40, score, sep, probs, mix, drop=_drop(N))
    dmix, dscore, dtop = t("dmix", P, 2, H), t("dscore", P, Lt), t("dtop", P, 5, H, dtype=BF16)
    N.span_pool_bwd(P, Lt, H, top, 40, probs, sep, dmix, dscore, dtop)
    N.span_pool_bwd(P, Lt, H, top, 40, probs, sep, dmix, dscore, dtop, drop=_drop(N))


@case
def pairs(N, t, calls):
    B, L, n, Lp = 2, 12, 3, 7
    ids, starts, lens = t("input_ids", B, L, dtype=I64), t("starts", B, n, dtype=I64), t("lens", B, n, dtype=I64)
    N.pair_scan(ids, t("labels", B, n, dtype=I64), 5, 6, starts, lens, t("plab", B, 6, dtype=I64),
                t("sep_pos", B, 6, 2, dtype=I64), t("status", 2, dtype=I32))
    with pytest.raises(ValueError):
        N.pair_scan(ids, t.tensors["labels"], 5, 6, starts, lens, t.tensors["plab"],
                    t.tensors["sep_pos"], t("status64", 2, dtype=I64))
    N.pair_expand(ids, starts, lens, n, Lp, 1, True, t("out_ids", 12, Lp, dtype=I64),
                  t("out_mask", 12, Lp, dtype=I64), t("out_tt", 12, Lp, dtype=I64))
    with pytest.raises(ValueError):
        N.pair_expand(ids, starts, lens, n, Lp, 1, True, t.tensors["out_ids"],
                      t.tensors["out_mask"], t("out_tt32", 12, Lp, dtype=I32))


@case
def image_resize(N, t, calls):
    N.image_resize_normalize(t("pixels", 60, dtype=U8), t("table", 2, 4, dtype=I64), [3, 2], 3, 4,
                             t("out", 2, 3, 2, 2), (0.5, 0.4, 0.3), (0.2, 0.3, 0.4))


@case
def lstm_cell(N, t, calls):
    B, H = 2, 4
    gx = t("gx", B, 5 * H)
    gh, c, h_out, c_out, act = t("gh", B, 4 * H), t("c", B, H), t("h_out", B, H), t("c_out", B, H), t("act", B, 4 * H)
    N.lstm_cell_fwd(gx, gh, c, h_out, c_out, act)
    N.lstm_cell_fwd(gx[:, :4 * H], gh, c, h_out, c_out, act)
    with pytest.raises(ValueError):
        N.lstm_cell_fwd(gx, gh, c, h_out, c_out, t("act16", B, 4 * H, dtype=BF16))
    dg, dcp = t("dgates", B, 4 * H), t("dc_prev", B, H)
    N.lstm_cell_bwd(act, c, c_out, t("dh", B, H), t("dc_next", B, H), dg, dcp)
    N.lstm_cell_bwd(act, c, c_out, None, None, dg, dcp)


DB, DN, DH = 2, 4, 8  # the decoder cases: B stories of N sentences, hidden H


def _decoder(t):
    B, n, H = DB, DN, DH
    ins = (t("doc", B, n, H), t("okey", B, n, H), t("hist", B, n, n, H + 2), t("h0", B, H), t("c0", B, H))
    shapes = (("w_ih", (4 * H, H)), ("b_ih", (4 * H,)), ("w_hh", (4 * H, H)), ("b_hh", (4 * H,)),
              ("w_q", (H, H)), ("b_q", (H,)), ("w_pw", (H, 4 * (H + 2))), ("w_t", (H,)), ("b_t", (1,)))
    return ins + (tuple(t(n_, *s) for n_, s in shapes),), shapes


@case
def beam(N, t, calls):
    B, n, H, W = DB, DN, DH, 3
    d, _ = _decoder(t)
    ws = t("workspace", 4096, dtype=U8)
    assert N.beam_workspace(B, n, H, W) == 4096
    assert N.beam_search(*d, W, t("order", B, n, dtype=I64), t("score", B), ws) == 0
    with pytest.raises(ValueError):
        N.beam_search(*d, W, t("order32", B, n, dtype=I32), t.tensors["score"], ws)
    assert N.beam_search_nbest(*d, W, t("orders", B, W, n, dtype=I64), t("scores", B, W),
                               t("count", B, dtype=I32), t("workspace32", 1024)) == 0


@case
def order_score(N, t, calls):
    B, n, H, K = DB, DN, DH, 3
    d, _ = _decoder(t)
    ws, nll = t("workspace", 4096, dtype=U8), t("nll", B, K)
    assert N.order_score_workspace(B, n, H, K) == 4096
    assert N.order_score(*d, t("orders_kn", K, n, dtype=I64), nll, None, ws) == 0
    assert N.order_score(*d, t("orders_bkn", B, K, n, dtype=I64), nll, t("step_nll", B, K, n - 1),
                         ws) == 0
    with pytest.raises(ValueError):
        N.order_score(*d, t.tensors["orders_kn"], t("nll_bad", B, K + 1), None, ws)


@case
def order_score_bwd(N, t, calls):
    B, n, H, K = DB, DN, DH, 3
    d, shapes = _decoder(t)
    ws, dnll = t("workspace", 4096, dtype=U8), t("dnll", B, K)
    wt = (t("wt_ih", H, 4 * H), t("wt_hh", H, 4 * H), t("wt_q", H, H), t("wt_pw", 4 * (H + 2), H))
    dins = (t("ddoc", B, n, H), t("dokey", B, n, H), t("dhist", B, n, n, H + 2), t("dh0", B, H),
            t("dc0", B, H))
    dws = tuple(t("d" + n_, *s) for n_, s in shapes)
    assert N.order_score_bwd_workspace(B, n, H, K) == 4096
    assert N.order_score_bwd(*d, wt, t("orders_kn", K, n, dtype=I64), dnll, dins, dws, ws) == 0
    assert N.order_score_bwd(*d, wt, t("orders_bkn", B, K, n, dtype=I64), dnll, dins, dws, ws) == 0


@case
def order_sample(N, t, calls):
    B, n, H, S = DB, DN, DH, 3
    d, _ = _decoder(t)
    ws, orders, nll = t("workspace", 4096, dtype=U8), t("orders", B, S, n, dtype=I64), t("nll", B, S)
    assert N.order_sample_workspace(B, n, H, S) == 4096
    assert N.order_sample(*d, (1 << 64) + 5, (1 << 32) + 6, 7, 8, orders, nll, None, None, ws) == 0
    assert N.order_sample(*d, 5, 6, 0, 0, orders, nll, t("u", B, S, n - 1),
                          t("step_nlp", B, S, n - 1, n), ws) == 0


@case
def order_tree(N, t, calls):
    B, n, H = DB, DN, DH
    d, _ = _decoder(t)
    ws, nll = t("workspace", 4096, dtype=U8), t("nll", B, 24)
    assert N.order_tree_workspace(B, n, H, 64) == 4096
    assert N.order_tree(*d, 64, nll, None, ws) == 0
    assert N.order_tree(*d, 64, nll, t("orders", 24, n, dtype=I64), ws) == 0


@case
def order_posterior(N, t, calls):
    B, K, n = 2, 6, 3
    out = {name: t(name, *((B,) + (n,) * nn), dtype=dtype) for name, dtype, nn in N.POSTERIOR_OUTPUTS}
    nll = t("nll", B, K)
    assert N.order_posterior(t("orders_kn", K, n, dtype=I64), nll, 0, out) == 0
    assert N.order_posterior(t("orders_bkn", B, K, n, dtype=I64), nll, 1, out) == 0
    with pytest.raises(ValueError):
        N.order_posterior(t("orders32", K, n, dtype=I32), nll, 0, out)


@case
def pairwise(N, t, calls):
    B, n, K = 2, 3, 4
    out = {name: t(name, *((B,) + (n,) * nn), dtype=dtype) for name, dtype, nn in N.PAIRWISE_OUTPUTS}
    w = t("w", B, n, n)
    assert N.pairwise_order_workspace(B, n) == 4096
    assert N.pairwise_order(w, out, t("workspace", 4096, dtype=U8)) == 0
    pnll = t("score_pnll", B, K)
    assert N.pairwise_score(w, t("orders_kn", K, n, dtype=I64), pnll) == 0
    assert N.pairwise_score(w, t("orders_bkn", B, K, n, dtype=I64), pnll) == 0
    with pytest.raises(ValueError):
        N.pairwise_score(w, t.tensors["orders_kn"], t("pnll_t", K, B))


@case
def rows_gather(N, t, calls):
    x2, x3, out = t("x2", 6, 8, dtype=BF16), t("x3", 2, 3, 8, dtype=BF16), t("out", 4, 8, dtype=BF16)
    src, keep = t("src", 4, dtype=I32), t("keep", 4, dtype=U8)
    N.rows_gather_fwd(x2, src, None, out)
    N.rows_gather_fwd(x3, src, keep, out)
    N.rows_gather_bwd(out, src, None, x2)
    N.rows_gather_bwd(out, src, keep, x3)
    with pytest.raises(ValueError):
        N.rows_gather_fwd(x2, t("src64", 4, dtype=I64), None, out)


@case
def xent(N, t, calls):
    M, V = 5, 13
    logits, labels = t("logits", M, 16, dtype=BF16), t("labels", M, dtype=I64)
    lse, loss_row, stats = t("lse", M), t("loss_row", M), t("stats", 2)
    N.xent_fwd(logits, V, labels, -100, lse, loss_row, stats)
    with pytest.raises(ValueError):
        N.xent_fwd(logits, V, labels, -100, lse, t("loss_row_short", M - 1), stats)
    N.xent_bwd(logits, V, labels, -100, lse, stats)
    rank = t("rank", M, dtype=I32)
    N.xent_eval(logits, V, labels, -100, 0, lse, loss_row, rank)
    N.xent_eval(logits, V, labels, -100, 2, lse, loss_row, rank, topk_idx=t("topk_idx", M, 2, dtype=I32),
                topk_logit=t("topk_logit", M, 2), totals=t("totals", 4, dtype=torch.float64),
                stats=stats)
    with pytest.raises(ValueError):
        N.xent_eval(logits, V, labels, -100, 2, lse, loss_row, rank)
    with pytest.raises(ValueError):
        N.xent_eval(logits, V, labels, -100, N.XENT_EVAL_MAX_K + 1, lse, loss_row, rank)


@case
def mlm_mask(N, t, calls):
    ids, labels = t("input_ids", 2, 6, dtype=I64), t("labels", 2, 6, dtype=I64)
    N.mlm_mask(ids, labels, 1, 2, 3, 64, -100, 0.15, (1 << 64) + 9)
    N.mlm_mask(ids, labels, 1, 2, 3, 64, -100, 0.15, 9, stream_id=(1 << 32) + 4)
    with pytest.raises(ValueError):
        N.mlm_mask(ids, t("labels32", 2, 6, dtype=I32), 1, 2, 3, 64, -100, 0.15, 9)


@case
def mxfp8_quant(N, t, calls):
    x = t("x", 4, 64, dtype=BF16)
    m = N.quant_mxfp8(x)
    _mx(calls, m, 4, 64)
    t.tensors["m.q"], t.tensors["m.scales"] = m.q, m.scales
    assert N.quant_mxfp8(t("x2", 4, 96)[:, :64], out=m) is m


@case
def mxfp8_attention(N, t, calls):
    P, T, h = 2, 4, 1
    qkv, lse, kb = t("qkv", 8, 192, dtype=BF16), t("lse", 2, 1, 4), t("kb", 2, 4)
    _mx(calls, N.attn_fwd_mxfp8(P, T, h, qkv, 192, 0, 64, 128, kb, 0.125, lse), 8, 64)
    out, dout = t("out", 8, 64, dtype=BF16), t("dout", 8, 64, dtype=BF16)
    delta, dqkv, bits = t("delta", 2, 1, 4), t("dqkv", 8, 192, dtype=BF16), t("bits", 16, dtype=I64)
    _mx(calls, N.attn_bwd_mxfp8(P, T, h, qkv, None, 0.125, out, dout, lse, delta, dqkv), 8, 192)
    _mx(calls, N.attn_bwd_mxfp8(P, T, h, qkv, kb, 0.125, out, dout, lse, delta, dqkv, drop=_drop(N),
                                keep_bits=bits), 8, 192)
    _mx(calls, N.attn_fwd_mxfp8_dual(P, T, h, qkv, 192, 0, 64, 128, None, 0.125, None, 0, lse), 8, 64)
    _mx(calls, N.attn_fwd_mxfp8_dual(P, T, h, qkv, 192, 0, 64, 128, kb, 0.125, out, 64, lse,
                                     drop=_drop(N), keep_bits=bits), 8, 64)


def _operand(N, t, name, rows, K):
    return N.MXFP8(t(name + ".q", rows, K, dtype=U8), t(name + ".scales", 64, dtype=U8), rows, K)


@case
def mxfp8_gemm(N, t, calls):
    a, b = _operand(N, t, "a", 4, 64), _operand(N, t, "b", 24, 64)
    c, bias, resid = t("c", 4, 24, dtype=BF16), t("bias", 24), t("resid", 4, 24, dtype=BF16)
    aux, dact = t("aux", 4, 24, dtype=BF16), t("dact", 4, 24, dtype=BF16)
    assert N.gemm_mxfp8_ex(a, b, c) is None
    assert N.gemm_mxfp8_ex(a, b, c, bias=bias, act=1, aux=aux, resid=resid, drop=_drop(N)) is None
    _mx(calls, N.gemm_mxfp8_ex(a, b, None, bias=bias, act=1, aux=aux, q8=True), 4, 24)
    _mx(calls, N.gemm_mxfp8_ex(a, b, q8=True), 4, 24)
    assert N.gemm_mxfp8_ex(a, b, c, act=2, dact=dact) is None
    _mx(calls, N.gemm_mxfp8_ex(a, b, c, act=2, dact=dact, q8=True), 4, 24)
    with pytest.raises(ValueError):
        N.gemm_mxfp8_ex(a, b, t("c32", 4, 24))
    N.gemm_mxfp8(a, b, c)
    N.gemm_mxfp8(a, b, c, bias=bias, act=1, resid=resid, alpha=0.5)
    x, W = t("x", 4, 64, dtype=BF16), t("W", 24, 64, dtype=BF16)
    _mx(calls, N.gemm_mxfp8_out(x, W), 4, 24)
    _mx(calls, N.gemm_mxfp8_out(x, W, bias=bias, act=1), 4, 24)
    _mx(calls, N.gemm_mxfp8_q8(a, b), 4, 24)
    _mx(calls, N.gemm_mxfp8_q8(a, b, bias=bias, act=2), 4, 24)


@case
def resnet(N, t, calls):
    x = t("x", 2, 4, 4, 3, dtype=BF16)
    N.conv_im2col(x, 3, 2, 1, 32, t("cols", 8, 32, dtype=BF16))
    N.conv_col2im(t("dcols", 8, 32), 2, 4, 4, 3, 3, 2, 1, 32, t("dx", 2, 4, 4, 3))
    bx, g, b = t("bx", 2, 2, 2, 8, dtype=BF16), t("gamma", 8), t("beta", 8)
    mean, rstd, rm, rv, y = t("mean", 8), t("rstd", 8), t("run_mean", 8), t("run_var", 8), t("y", 2, 2, 2, 8, dtype=BF16)
    N.bn_fwd(bx, g, b, None, False, False, 1e-5, 0.1, 8, mean, rstd, rm, rv, y)
    N.bn_fwd(bx, g, b, t("resid", 2, 2, 2, 8, dtype=BF16), True, True, 1e-5, 0.1, 8, mean, rstd, rm, rv, y)
    dy, dg, db, bdx = t("dy", 2, 2, 2, 8, dtype=BF16), t("dgamma", 8), t("dbeta", 8), t("bdx", 2, 2, 2, 8, dtype=BF16)
    N.bn_bwd(dy, y, bx, mean, rstd, g, True, dg, db, bdx)
    N.bn_bwd(dy, y, bx, mean, rstd, g, False, dg, db, bdx, dres=t("dres", 2, 2, 2, 8, dtype=BF16))
    N.avgpool2(x, t("py", 2, 2, 2, 3, dtype=BF16))
    N.avgpool2(t("pdy", 2, 2, 2, 3), t("pdx", 2, 4, 4, 3), backward=True)


@case
def attnpool(N, t, calls):
    P, G, C = 2, 2, 8
    T2 = 2 * G * G + 1
    N.attnpool_gather(t("feats", 3, 4, C, dtype=BF16), t("pairimg", P, 2, dtype=I64), t("pos", 5, C),
                      t("x", P, T2, C, dtype=BF16))
    N.attnpool_gather_bwd(t("dx", 12, T2, C), 3, t("rolepairs", 3, 4, dtype=I64), t("dfeats", 6, 4, C))
    N.attnpool_out(t("a", 6, C, dtype=BF16), G, t("xpos", T2, dtype=I32), t("ypos", T2, dtype=I32),
                   t("ttype", T2, dtype=I32), t("y", 6, T2, C, dtype=BF16))
    N.attnpool_out_bwd(t("dy", P, T2, C), P, T2, C, t("da", P, C), t("token_colsum", T2, C))


# The three wrappers that tested `.is_cuda` themselves, and so refused CPU tensors, until their
# device checks went through _native._dev: recorded after the rest of the fixture.
@case
def xent_bwd_g(N, t, calls):
    M, V = 5, 13
    N.xent_bwd(t("logits", M, 16, dtype=BF16), V, t("labels", M, dtype=I64), -100, t("lse", M),
               t("stats", 2), g=t("g", 1))
    with pytest.raises(ValueError):
        N.xent_bwd(t.tensors["logits"], V, t.tensors["labels"], -100, t.tensors["lse"],
                   t.tensors["stats"], g=t("g2", 2))


@case
def subsample_text(N, t, calls):
    B, L, n_steps, n_sub = 2, 12, 4, 2
    ins = [t(n, B, L, dtype=I64) for n in ("input_ids", "attention_mask", "token_type_ids", "labels")]
    outs = [t(n, B, 6, dtype=I64) for n in ("out_ids", "out_mask", "out_tt", "out_labels")]
    sub, status = t("sub_idx", B, n_sub, dtype=I64), t("status", 1, dtype=I32)
    N.subsample_text(*ins, sub, n_steps, 5, 1, -100, *outs, status)
    N.subsample_text(ins[0], ins[1], None, None, sub, n_steps, 5, 1, -100, outs[0], outs[1], None,
                     None, status)
    with pytest.raises(ValueError):
        N.subsample_text(ins[0], ins[1], ins[2], None, sub, n_steps, 5, 1, -100, outs[0], outs[1],
                         None, None, status)
    with pytest.raises(ValueError):
        N.subsample_text(*ins, sub, n_steps, 5, 1, -100, *outs, t("status64", 1, dtype=I64))


@case
def rows_compact(N, t, calls):
    R = 6
    labels, out_labels = t("labels", R, dtype=I64), t("out_labels", R, dtype=I64)
    src, count = t("src", R, dtype=I32), t("count", 1, dtype=I32)
    N.rows_compact(labels, -100, src, out_labels, count)
    with pytest.raises(ValueError):
        N.rows_compact(labels, -100, t("src64", R, dtype=I64), out_labels, count)


# ------------------------------------------------------------------------------------------------
def run_case(name, setattr_):
    """The records of one case; installs the fake library through setattr_."""
    N = _nat()
    fake, names = install(setattr_), Names()
    lib = NamedLib(fake, names)
    setattr_(N, "lib", lambda: lib)
    real_empty = torch.empty

    def loud_empty(*a, **k):
        x = real_empty(*a, **k)
        return x.fill_(0x5A) if x.dtype == U8 else x
    setattr_(torch, "empty", loud_empty)
    try:
        CASES[name](N, names, fake.calls)
    finally:
        setattr_(torch, "empty", real_empty)
    return fake.calls


def _dump(fix, path):
    with open(path, "w") as f:
        f.write('{"signatures": {\n')
        f.write(",\n".join(f'{json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}'
                           for k, v in fix["signatures"].items()))
        f.write('\n}, "calls": {\n')
        f.write(",\n".join(json.dumps(k) + ": [\n" +
                           ",\n".join(json.dumps(r, separators=(",", ":")) for r in v) + "\n]"
                           for k, v in fix["calls"].items()))
        f.write("\n}}\n")


_GOLD = []


def golden():
    if not _GOLD:
        with open(FIXTURE) as f:
            _GOLD.append(json.load(f))
    return _GOLD[0]


def test_signatures_match_the_recorded_table():
    got, want = signatures(), golden()["signatures"]
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name


@pytest.mark.parametrize("name", list(CASES))
def test_binding_call_trace(name, monkeypatch):
    want = golden()["calls"][name]
    got = json.loads(json.dumps(run_case(name, monkeypatch.setattr)))
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"{name}: record {k} differs:\n got  {a}\n want {b}"
    assert len(got) == len(want), (name, len(got), len(want))


def test_every_status_entry_is_traced():
    gold = golden()
    assert set(gold["calls"]) == set(CASES)
    seen = {r[0] for recs in gold["calls"].values() for r in recs}
    status = {n for n, (res, _) in _nat()._SIGS.items() if res is ctypes.c_int}
    assert len(status) == 72
    assert not status - seen, sorted(status - seen)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    fix = {"signatures": signatures(), "calls": {name: run_case(name, setattr) for name in CASES}}
    if "--write" in sys.argv:
        _dump(fix, FIXTURE)
    n = sum(len(v) for v in fix["calls"].values())
    print(f"{len(fix['signatures'])} signatures, {len(CASES)} cases, {n} records")
