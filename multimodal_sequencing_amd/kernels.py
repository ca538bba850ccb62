"""Autograd Functions over the HIP C ABI.

Layer-level Functions (ViT block, BERT layer, stem, projection, joint input) own their forward
AND backward explicitly: they decide what is saved (flash attention saves LSE, not T x T
probabilities), fuse the residual adds into GEMM epilogues / LayerNorm backward, and write
parameter gradients straight into the flat fp32 grad buffer of the ParamStore with accumulating
wgrad GEMMs (so gradient accumulation over micro-batches is free and the all-reduce can start on
a contiguous slice as soon as a layer's backward finishes). Autograd only sequences the layers:
each Function takes an `anchor` tensor that requires grad so the graph is recorded, and returns
None for it.
"""
import math
import os

import torch

from . import _native as N

GELU, QGELU, TANH, GELU_TANH = (N.ACT[a] for a in ("gelu", "quickgelu", "tanh", "gelu_tanh"))


def _rows(ld):
    return N.rows(ld)


def _colsum(x, out):
    rows = x.numel() // x.shape[-1]
    N.colsum(x, rows, x.shape[-1], x.shape[-1], out, accumulate=True)


def _wgrad(dy, x, gW, gb=None):
    """gW[out][in] += dy^T x  (dy [R][out], x [R][in]) — TN GEMM accumulating in fp32 (split-K
    over R for the bf16 256^2 kernel); with gb the bias gradient gb[out] += sum_r dy[r] is fused
    into the same pass (mmseq_gemm_wgrad)."""
    N.gemm_wgrad(dy, x, gW, gb)


def _linear(x, W, bias=None, act=0, aux=None, resid=None, out=None, out_dtype=None, drop=None):
    """y = dropout(act(x W^T + b)) (+ resid); W [out][in] compute dtype."""
    R = x.numel() // x.shape[-1]
    n_out = W.shape[0]
    if out is None:
        out = torch.empty(R, n_out, device=x.device, dtype=out_dtype or x.dtype)
    N.gemm(x, W, out, R, n_out, x.shape[-1], bias=bias, act=act, aux=aux, resid=resid, drop=drop)
    return out


# ------------------------------------------------------------------------------------------------
# MX-fp8 inference GEMMs (BASELINE config 5): under `fp8_forward()`, the no-grad forward of the
# encoder layers runs QKV, the attention output projection, FC1 and FC2 on the fp8 MFMA (the 256 x
# 256 8-phase schedule with MX-fp8 operands, gemm256.hip F8; weights quantised once per store
# version, activations by mmseq_quant_mxfp8, FC1's output by its own epilogue for FC2). Shapes the
# 8-phase form does not take (K or widths not multiples of 256) keep the round-2 path: FC1 bf16
# with an MX-fp8 epilogue, FC2 fp8, QKV / O bf16. With training=True the TRAINING forward runs the
# same four GEMMs on the fp8 MFMA too (the backward stays bf16): every producer writes the bf16
# tensor the backward reads AND the next GEMM's MX-fp8 operand in one pass (LayerNorm, attention
# mmseq_attn_fwd_mxfp8_dual, FC1 mmseq_gemm_mxfp8_ex with q), dropout masks as in bf16 training.
_FP8 = {"on": False, "train": False, "dgrad": False, "cache": {}, "sites": None}
FP8_SITES = ("qkv", "o", "fc1", "fc2")  # the four GEMMs of every ViT block and joint layer
FP8_VIT_ONLY = tuple(f"vit.{x}" for x in FP8_SITES)


class fp8_forward:
    """Context manager: MX-fp8 encoder GEMMs in torch.no_grad() forwards (and, with
    training=True, in the forward of training steps; with dgrad=True also the backward's four
    data-gradient GEMMs of those layers, dY quantised per call; weight gradients stay bf16).

    sites (eval forward only): a MIXED placement — only the named GEMM sites run on the fp8 MFMA,
    the others in bf16. Names: "qkv", "o", "fc1", "fc2" (both layer kinds) or "vit.<site>" /
    "joint.<site>" (one kind). None (default) = all four, through the fused MX-fp8 producers. A
    layer kind with all four sites on keeps the fused fp8 path and one with none the bf16 path
    (FP8_VIT_ONLY: the ViT on the fp8 MFMA, the joint encoder in bf16, the placement the per-site
    error budget picks); a kind with some sites on runs from unfused blocks (a
    quantisation pass per fp8 GEMM input: the same numbers as the fused producers, which are
    bit-identical to bf16 output + quantiser, tests/test_fp8_gpu.py), i.e. measures placement, not speed."""

    def __init__(self, enabled=True, training=False, dgrad=False, sites=None):
        self.enabled = enabled
        self.training = training
        self.dgrad = dgrad
        if sites is not None:
            sites = frozenset(sites)
            bad = [x for x in sites if x.split(".")[-1] not in FP8_SITES
                   or (x.count(".") == 1 and x.split(".")[0] not in ("vit", "joint")) or x.count(".") > 1]
            if bad or training:
                raise ValueError(f"fp8_forward: sites {bad} (eval only: {FP8_SITES}, vit.* / joint.*)")
        self.sites = sites

    def __enter__(self):
        self.prev = (_FP8["on"], _FP8["train"], _FP8["dgrad"], _FP8["sites"])
        _FP8["on"] = self.enabled
        _FP8["train"] = self.enabled and self.training
        _FP8["dgrad"] = self.enabled and self.training and self.dgrad
        _FP8["sites"] = self.sites if self.enabled else None
        return self

    def __exit__(self, *exc):
        _FP8["on"], _FP8["train"], _FP8["dgrad"], _FP8["sites"] = self.prev
        if not _FP8["on"]:
            _FP8["cache"].clear()


def _fp8_bwd_done(f8):
    """End of a layer backward that ran its dgrads on the fp8 MFMA (the engine chosen in the
    forward): when that backward runs after the fp8_forward() context has exited, the transposed
    weights' fp8 copies it quantised would stay in the cache until another context exits."""
    if f8 and not _FP8["on"]:
        _FP8["cache"].clear()


def _fp8_weight(st, W):
    key = (W.data_ptr(), tuple(W.shape))
    hit = _FP8["cache"].get(key)
    if hit is None or hit[0] is not st or hit[1] != st.version:
        hit = (st, st.version, N.quant_mxfp8(W))
        _FP8["cache"][key] = hit
    return hit[2]


class _Act:
    """An activation (or gradient) on its way to a GEMM: the bf16 / fp32 tensor `t`, its MX-fp8 copy
    `q` (_native.MXFP8), or both. Producers fill in what their engine decides; a consumer GEMM
    takes the form it runs on, so a layer body never asks which one exists."""
    __slots__ = ("t", "q")

    def __init__(self, t=None, q=None):
        self.t, self.q = t, q

    @property
    def rows(self):
        return self.t.shape[0] if self.t is not None else self.q.rows


def _act_in(x):
    """A layer's input x with the MX-fp8 copy the previous layer's last LayerNorm attached
    (_Engine.ln attach=True), if x has not been modified since. The copy is detached from x here:
    x itself is saved for backward, and an attribute would keep the fp8 copy alive with it until
    then; a layer that does not read the copy drops it with the handle."""
    hit = x.__dict__.pop("_mx", None)
    return _Act(x, hit[0] if hit is not None and hit[1] == x._version else None)


class _Engine:
    """How one layer call runs its four GEMMs (FP8_SITES), two LayerNorms and attention, chosen
    once per forward by _engine() and read back from ctx by the backward.

    f8: the GEMM sites on the fp8 MFMA (the others in bf16 / fp32). emit: the sites whose operand
    its PRODUCER also writes in MX-fp8 in the same pass (LayerNorm, attention, FC1's epilogue); at
    an fp8 site outside emit the GEMM quantises its input itself (mmseq_quant_mxfp8: the same
    numbers, the fused producers are bit-identical to bf16 output + quantiser). save: a training
    forward, every producer also writes the bf16 tensor the backward reads (and the GELU
    pre-activation, the attention keep bits). f8dg: the backward's data-gradient GEMMs on the fp8
    MFMA too (weight gradients stay bf16)."""

    def __init__(self, st, f8=(), emit=(), save=False, f8dg=False):
        self.st, self.f8, self.emit = st, frozenset(f8), frozenset(emit)
        self.save, self.f8dg = save, f8dg

    def _q(self, a):
        """a's MX-fp8 copy: the one its producer wrote, else a quantisation pass."""
        return a.q if a.q is not None else N.quant_mxfp8(a.t.view(-1, a.t.shape[-1]))

    # -- forward ----------------------------------------------------------------------------------
    def keep(self, *ts):
        """What the backward reads of handles / tensors the forward is done with: their bf16 tensors
        in a training forward, None otherwise (an eval forward lets go of them here)."""
        out = tuple((t.t if isinstance(t, _Act) else t) if self.save else None for t in ts)
        return out if len(out) > 1 else out[0]

    def linear(self, site, a, W, bias=None, act=0, resid=None, drop=None, to=None, pre=False):
        """dropout(act(a W^T + bias)) (+ resid) at GEMM site `site`, W [out][in] compute dtype (its
        fp8 copy quantised once per store version) -> handle. to: the site that consumes the
        output, if a GEMM. pre=True -> (handle, z), z the pre-activation the backward reads (None
        outside training)."""
        q8 = to in self.emit  # the epilogue writes the consumer's MX-fp8 operand
        z = torch.empty(a.rows, W.shape[0], device=W.device, dtype=W.dtype) if pre and self.save else None
        if site not in self.f8:
            if q8:  # bf16 MFMA, MX-fp8 output only (eval FFN with K % 128: mmseq_gemm_mxfp8_out)
                out = _Act(q=N.gemm_mxfp8_out(a.t, W, bias=bias, act=act))
            else:
                out = _Act(_linear(a.t, W, bias=bias, act=act, aux=z, resid=resid, drop=drop))
        elif q8 and not self.save:  # eval: the output is only the next fp8 GEMM's operand
            out = _Act(q=N.gemm_mxfp8_q8(self._q(a), _fp8_weight(self.st, W), bias=bias, act=act))
        else:
            aq = self._q(a)
            y = torch.empty(aq.rows, W.shape[0], device=W.device, dtype=torch.bfloat16)
            if self.save:
                out = _Act(y, N.gemm_mxfp8_ex(aq, _fp8_weight(self.st, W), y, bias=bias, act=act, aux=z,
                                              resid=resid, drop=drop, q8=q8))
            else:  # eval fp8 sites run without dropout (_engine)
                N.gemm_mxfp8(aq, _fp8_weight(self.st, W), y, bias=bias, act=act, resid=resid)
                out = _Act(y)
        return (out, z) if pre else out

    def ln(self, x, gamma, beta, eps, to, keep=False, attach=False):
        """LayerNorm of x [R][C], the operand of the GEMM at site `to` -> (handle, mean, rstd).
        keep: the caller reads the bf16 output too (a residual). attach (a layer's output, consumed
        by the NEXT layer's first GEMM): the MX-fp8 copy rides on the bf16 tensor, valid while that
        is unmodified (_act_in checks the version). Copies the caller uses directly come in the
        handle only: never attached to a tensor that goes into save_for_backward."""
        R, C = x.shape
        mean = torch.empty(R, device=x.device)
        rstd = torch.empty_like(mean)
        y = torch.empty_like(x) if keep or self.save or to not in self.emit else None
        q = None
        if to in self.emit:
            q = N.layernorm_fwd_mxfp8(R, C, x, gamma, beta, eps, y=y, mean=mean, rstd=rstd)
            if attach:
                y._mx, q = (q, y._version), None
        else:
            N.layernorm_fwd(R, C, x, _rows(C), gamma, beta, eps, y, _rows(C), mean, rstd)
        return (_Act(y, q),) + self.keep(mean, rstd)  # the statistics are the backward's

    def attn(self, P, T, heads, qkv, key_bias, drop=None, Tq=None):
        """Flash attention over packed Q|K|V [P * T][3H] -> (O handle for the `o` GEMM, LSE
        [P][heads][T], the dropout keep mask as bits (1 bit per score, read back by the backward;
        None outside training)). Tq < T: the first Tq query rows of every sequence only, O [P * Tq][H]
        (mmseq_attn_fwd_rows draws the attention-probability mask by the full-size index)."""
        H = qkv.shape[-1] // 3
        scale = 1.0 / math.sqrt(H // heads)
        lse = torch.empty(P, heads, T, device=qkv.device)
        kbits = N.attn_keep_bits(P, T, heads, qkv.device) if drop is not None and self.save else None
        if "o" in self.emit:
            if self.save:
                o = torch.empty(P * T, H, device=qkv.device, dtype=qkv.dtype)
                q = N.attn_fwd_mxfp8_dual(P, T, heads, qkv, 3 * H, 0, H, 2 * H, key_bias, scale, o, H,
                                          lse, drop=drop, keep_bits=kbits)
                return _Act(o, q), lse, kbits
            return _Act(q=N.attn_fwd_mxfp8(P, T, heads, qkv, 3 * H, 0, H, 2 * H, key_bias, scale,
                                           lse)), lse, kbits
        Tq = T if Tq is None else Tq
        o = torch.empty(P * Tq, H, device=qkv.device, dtype=qkv.dtype)
        if Tq < T:
            N.attn_fwd_rows(P, T, Tq, heads, qkv, key_bias, scale, o, lse, drop=drop, keep_bits=kbits)
        else:
            N.attn_fwd(P, T, heads, qkv, 3 * H, 0, H, 2 * H, key_bias, scale, o, H, lse, drop=drop,
                       keep_bits=kbits)
        return _Act(o), lse, kbits

    # -- backward ---------------------------------------------------------------------------------
    def dgrad(self, g, WT, resid=None, act=0, dact=None, q8=False):
        """dx = g W (+ resid) or (g W) * act'(dact), WT the transposed shadow [in][out] -> handle.
        q8: dx feeds the next dgrad directly, so an fp8 dgrad's epilogue writes its MX-fp8 copy too."""
        if not self.f8dg:
            return _Act(_dgrad(g.t, WT, resid=resid, act=act, dact=dact))
        out = torch.empty(g.rows, WT.shape[0], device=g.t.device, dtype=g.t.dtype)
        return _Act(out, N.gemm_mxfp8_ex(self._q(g), _fp8_weight(self.st, WT), out, act=act, dact=dact,
                                         resid=resid, q8=q8))

    def ln_bwd(self, dy, x, mean, rstd, gamma, dx, dres, dgamma, dbeta, dsum, dx_rows=None,
               dx_drop=None, drop_dx=None, dx_drop_rows=None, dsum_with_dres=False):
        """Backward of a LayerNorm whose gradient (dx_drop: dx through the dropout mask drop_dx, else
        dx) is the output gradient of a Linear with bias gradient `dsum` -> (its handle, the bias
        gradient left to that Linear's weight-gradient GEMM). bf16 / fp32: the LN backward sums the
        bias gradient itself (mmseq_layernorm_bwd_ex), so the weight gradient runs without its
        fused bias pass (None). fp8 dgrad: it writes the dgrad's MX-fp8 operand instead, and the
        bias sum stays fused into the weight-gradient GEMM. dsum_with_dres: _native.layernorm_bwd."""
        R, C = x.shape
        g = dx_drop if dx_drop is not None else dx
        if self.f8dg:
            return _Act(g, N.layernorm_bwd_mxfp8(R, C, dy, _rows(C), x, _rows(C), mean, rstd, gamma, dx,
                                                 _rows(C), dres, _rows(C), dgamma, dbeta,
                                                 dx_drop=dx_drop, drop_dx=drop_dx)), dsum
        N.layernorm_bwd(R, C, dy, _rows(C), x, _rows(C), mean, rstd, gamma, dx,
                        dx_rows if dx_rows is not None else _rows(C), dres, _rows(C), dgamma, dbeta,
                        dx_drop=dx_drop, drop_dx=drop_dx,
                        dx_drop_rows=dx_drop_rows, dsum=dsum, dsum_with_dres=dsum_with_dres)
        return _Act(g), None

    def attn_bwd(self, P, T, heads, qkv, key_bias, o, do, lse, drop=None, keep_bits=None, Tq=None):
        """-> handle of dQ|dK|dV [P * T][3H] (fp8 dgrad: also in MX-fp8, the QKV dgrad's operand).
        Tq < T (attn's): dQ = 0 on the rows past Tq; dK / dV over every key row."""
        H = qkv.shape[-1] // 3
        scale = 1.0 / math.sqrt(H // heads)
        dqkv = torch.empty_like(qkv)
        delta = torch.empty(P, heads, T, device=qkv.device)
        if self.f8dg:
            return _Act(dqkv, N.attn_bwd_mxfp8(P, T, heads, qkv, key_bias, scale, o, do, lse, delta, dqkv,
                                               drop=drop, keep_bits=keep_bits))
        if Tq is not None and Tq < T:
            N.attn_bwd_rows(P, T, Tq, heads, qkv, key_bias, scale, o, do, lse, delta, dqkv, drop=drop,
                            keep_bits=keep_bits)
        else:
            N.attn_bwd(P, T, heads, qkv, 3 * H, 0, H, 2 * H, key_bias, scale, o, H, do, H, lse, delta,
                       dqkv, 3 * H, drop=drop, keep_bits=keep_bits)
        return _Act(dqkv)

    def bwd_done(self):
        _fp8_bwd_done(self.f8dg)


def _engine(kind, st, x, Ws, save, drops=(None, None, None), Tq=None):
    """The engine for one forward of a layer of `kind` ("vit" / "joint") with input x [R][K] and
    weights Ws = (qkv, o, fc1, fc2), [out][in]: every eligibility rule lives here.

    - bf16 / fp32 (no site on the fp8 MFMA): fp8_forward() off, an fp32 model, a layer on its text
      rows (Tq: ~1/3 of the rows; the other layers keep the fp8 GEMMs), or shapes fp8 does not take.
    - fp8 training (save, fp8_forward(training=True)): all four GEMMs in the 256 x 256 8-phase
      MX-fp8 form (K and widths multiples of 256), a hidden width the fused MX-fp8 LayerNorm takes
      (<= 1024), >= 256 rows; dropout masks as in bf16 training.
    - mixed placement (eval, fp8_forward(sites=...) with some of the kind's sites on): those sites
      from unfused blocks, no shape guard (a shape the fp8 GEMM cannot take raises). A kind with
      all four sites on is fused, one with none bf16.
    - fused fp8 eval: QKV and O with K a multiple of 256 (attention and hidden dropout off);
      the FFN with K and the intermediate width multiples of 256, else (multiples of 128) FC1 on
      the bf16 MFMA with an MX-fp8 epilogue and FC2 in fp8; the output dropout is off in
      inference. Without fp8 QKV / O the FFN alone still takes whichever of the two forms fits, fed
      by a bf16 LayerNorm."""
    plain = _Engine(st, save=save)
    if not _FP8["on"] or x.dtype != torch.bfloat16 or Tq is not None:
        return plain
    K, I = Ws[2].shape[1], Ws[2].shape[0]
    wide = K % 256 == 0 and K <= 1024 and x.is_contiguous()
    if save:
        if _FP8["train"] and wide and x.shape[0] >= 256 and all(
                W.shape[0] % 256 == 0 and W.shape[1] % 256 == 0 for W in Ws):
            return _Engine(st, FP8_SITES, FP8_SITES, True, _FP8["dgrad"])
        return plain
    sel = _FP8["sites"]
    on = [s for s in FP8_SITES if sel is None or s in sel or f"{kind}.{s}" in sel]
    if 0 < len(on) < len(FP8_SITES):
        return _Engine(st, on) if drops == (None, None, None) else plain
    d_att, d_o, d_out = drops
    f8 = set()
    if on and wide and Ws[0].shape[0] % 256 == 0 and d_att is None and d_o is None:
        assert d_out is None, "eval fp8 path: the output dropout is off in inference"
        f8 = {"qkv", "o"}
    if on and d_out is None and K % 128 == 0 and I % 128 == 0:
        f8.add("fc2")
        if wide and I % 256 == 0 and Ws[3].shape[0] % 256 == 0:
            f8.add("fc1")
    # without fp8 QKV / O the LayerNorm in front of FC1 stays bf16 and FC1 quantises its input
    return _Engine(st, f8, f8 if "qkv" in f8 else f8 - {"fc1"})


def _dgrad(dy, WT, resid=None, act=0, dact=None, out=None):
    """dx = dy W (+ resid), using the transposed shadow WT [in][out]; optionally times act'(dact)."""
    R = dy.numel() // dy.shape[-1]
    n_in = WT.shape[0]
    if out is None:
        out = torch.empty(R, n_in, device=dy.device, dtype=dy.dtype)
    N.gemm(dy, WT, out, R, n_in, dy.shape[-1], resid=resid, act=act, dact=dact)
    return out


class Dropouts:
    """Train-mode dropout descriptors for one forward pass.

    Masks are counter-based (include/mmseq.h `mmseq_dropout`): a site is identified by a 32-bit
    stream id, a forward pass by a 64-bit seed, so the backward regenerates every mask from the
    descriptor saved on the autograd context and nothing T x T or [rows][H] is stored.
    `site(p, *key)` returns None in eval mode or when p == 0 (the kernels then skip the hash).
    """

    def __init__(self, seed, training):
        self.seed = seed
        self.training = training

    def site(self, p, *key):
        if not self.training or p <= 0:
            return None
        h = 0x811C9DC5
        for k in key:  # FNV-1a over the site key -> stream id
            for ch in str(k).encode():
                h = ((h ^ ch) * 0x01000193) & 0xFFFFFFFF
        return N.drop(p, h, self.seed)


EVAL = Dropouts(0, False)


class LayerRefs:
    """Names of one layer's parameters inside a ParamStore (resolved once). `span` is the
    contiguous grad-buffer range the layer's backward completes (reported to the data-parallel
    reducer through ParamStore.grad_ready)."""

    def __init__(self, store, **names):
        self.store = store
        self.__dict__.update(names)
        self.span = store.span(self.names())

    def names(self):
        out = []
        for k, v in self.__dict__.items():
            if k in ("store", "span"):
                continue
            out += v if isinstance(v, list) else [v]
        return out


# the last joint layer on the text rows only (BertLayerFn Tq); off (or MMSEQ_ROWS=0 in the
# environment, for A/B runs): every layer over all T rows
ROWS = {"on": os.environ.get("MMSEQ_ROWS", "1") != "0"}


# ================================================================================================
# BERT layer (post-LN), lxrt/modeling.py:496-507 (BertSelfattLayer + BertIntermediate + BertOutput)
# ================================================================================================
class BertLayerFn(torch.autograd.Function):
    @staticmethod
    def rows_ok(x):
        """The layer can run on the first Tq rows of every sequence only (forward(..., Tq)): bf16 and
        the variant-1 attention kernels (mmseq_attn_fwd_rows). Under fp8_forward() that layer runs
        in bf16 (its text rows are ~1/3 of the rows; the other layers keep the fp8 GEMMs)."""
        return ROWS["on"] and x.dtype == torch.bfloat16 and N._sel["attn"] == 1

    @staticmethod
    def forward(ctx, x, key_bias, anchor, L, P, T, heads, eps, drops=(None, None, None), save=True,
                Tq=None):
        """drops = (attention probs :419, self-output dense :437, output dense :491); save=False
        (the caller runs under no_grad) skips the stores only the backward reads (GELU
        pre-activation). Tq (< T, rows_ok): only the first Tq rows of every sequence leave the
        layer (the last joint layer, whose visual rows _split_with_none discards,
        lxrt/modeling.py:611-618): QKV over all T rows (the keys and values), everything after
        the attention on the P * Tq text rows; returns [P * Tq][H]. Every kept row equals the
        full-size layer's; in train mode the attention-probability mask too (mmseq_attn_fwd_rows
        draws it by the full-size index), while the two hidden-dropout sites after the attention
        (:437, :491) index their masks by the compacted [P * Tq][H] layout: an equally distributed
        draw, regenerated identically by this layer's backward."""
        st = L.store
        H = x.shape[-1]
        d_att, d_o, d_out = drops
        Tq = T if Tq is None else Tq
        Ws = (st.packed(L.qkv_w, "w"), st.w(L.o_w), st.w(L.i_w), st.w(L.out_w))
        eng = _engine("joint", st, x, Ws, save, drops, Tq if Tq < T else None)
        xa = _act_in(x)
        qkv = eng.linear("qkv", xa, Ws[0], st.packed(L.qkv_b, "f32").view(-1)).t
        del xa
        o, lse, kbits = eng.attn(P, T, heads, qkv, key_bias, d_att, Tq)
        xr = x.view(P, T, H)[:, :Tq].reshape(P * Tq, H)  # the residual: x, or (Tq < T) its text rows
        s1 = eng.linear("o", o, Ws[1], st.f32(L.o_b), resid=xr, drop=d_o).t
        del xr
        o = eng.keep(o)
        h1, m1, r1 = eng.ln(s1, st.f32(L.ln1_w), st.f32(L.ln1_b), eps, "fc1", keep=True)
        g, z = eng.linear("fc1", h1, Ws[2], st.f32(L.i_b), act=GELU, to="fc2", pre=True)
        h1 = h1.t
        s2 = eng.linear("fc2", g, Ws[3], st.f32(L.out_b), resid=h1, drop=d_out).t
        gact = eng.keep(g)
        del g
        y, m2, r2 = eng.ln(s2, st.f32(L.ln2_w), st.f32(L.ln2_b), eps, "qkv", keep=True, attach=True)
        if save:
            ctx.save_for_backward(x, key_bias, qkv, o, lse, s1, m1, r1, h1, z, gact, s2, m2, r2)
            ctx.meta = (L, P, T, Tq, heads, drops)
            ctx.kbits = kbits
            ctx.eng = eng
        return y.t

    @staticmethod
    def backward(ctx, dy):
        x, key_bias, qkv, o, lse, s1, m1, r1, h1, z, gact, s2, m2, r2 = ctx.saved_tensors
        L, P, T, Tq, heads, (d_att, d_o, d_out) = ctx.meta  # Tq < T: dy is over the P * Tq text rows
        eng = ctx.eng
        st = L.store
        st.grad_begin()
        H = x.shape[-1]
        dy = dy.contiguous()
        # LN backward also emits the dense-branch gradient through the dropout mask (ds2d) while
        # the residual branch keeps the unmasked one (ds2)
        ds2 = torch.empty_like(dy)
        ds2d = torch.empty_like(dy) if d_out is not None else None
        g2, gb = eng.ln_bwd(dy, s2, m2, r2, st.f32(L.ln2_w), ds2, None, st.g(L.ln2_w), st.g(L.ln2_b),
                            st.g(L.out_b), dx_drop=ds2d, drop_dx=d_out)
        del ds2d
        _wgrad(g2.t, gact, st.g(L.out_w), gb)
        dz = eng.dgrad(g2, st.wt(L.out_w), act=GELU, dact=z, q8=True)
        del g2
        _wgrad(dz.t, h1, st.g(L.i_w), st.g(L.i_b))
        dh1 = eng.dgrad(dz, st.wt(L.i_w), resid=ds2).t
        del dz
        if Tq < T:  # the residual branch's gradient goes straight into its rows of the full-size
            # [P * T] buffer the QKV dgrad adds in fp32 (zero on the visual rows: bit-identical to
            # the full-size layer); the dense branch's (masked) copy stays compact
            ds1 = torch.empty(P * T, H, device=dy.device, dtype=dy.dtype)
            ds1.view(P, T, H)[:, Tq:].zero_()
            g1, gb = eng.ln_bwd(dh1, s1, m1, r1, st.f32(L.ln1_w), ds1, None, st.g(L.ln1_w),
                                st.g(L.ln1_b), st.g(L.o_b), dx_rows=N.rows(H, T * H, Tq),
                                dx_drop=torch.empty_like(dy), drop_dx=d_o, dx_drop_rows=_rows(H))
        else:
            ds1 = torch.empty_like(dy)
            g1, gb = eng.ln_bwd(dh1, s1, m1, r1, st.f32(L.ln1_w), ds1, None, st.g(L.ln1_w),
                                st.g(L.ln1_b), st.g(L.o_b),
                                dx_drop=torch.empty_like(dy) if d_o is not None else None, drop_dx=d_o)
        _wgrad(g1.t, o, st.g(L.o_w), gb)
        do = eng.dgrad(g1, st.wt(L.o_w)).t
        del g1
        dqkv = eng.attn_bwd(P, T, heads, qkv, key_bias, o, do, lse, d_att, ctx.kbits, Tq)
        ctx.kbits = None
        _wgrad(dqkv.t, x, st.packed(L.qkv_w, "g"), st.packed(L.qkv_b, "g").view(-1))
        st.grad_ready(L.span)
        dx = eng.dgrad(dqkv, st.wt(L.qkv_w[0]), resid=ds1).t
        eng.bwd_done()
        return dx, None, None, None, None, None, None, None, None, None, None


# ================================================================================================
# CLIP ViT residual attention block (pre-LN), clip/model.py:204-226
# ================================================================================================
class VitBlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, anchor, L, P, T, heads, eps, save=True):
        """in_proj / out_proj / c_fc / c_proj are the sites qkv / o / fc1 / fc2. The LayerNorm
        outputs are only GEMM operands (pre-LN): in eval they may leave in MX-fp8 alone; a training
        forward keeps the bf16 tensors the weight gradients read."""
        st = L.store
        Ws = (st.w(L.in_w), st.w(L.out_w), st.w(L.fc_w), st.w(L.proj_w))
        eng = _engine("vit", st, h, Ws, save)
        hn, m1, r1 = eng.ln(h, st.f32(L.ln1_w), st.f32(L.ln1_b), eps, "qkv")
        qkv = eng.linear("qkv", hn, Ws[0], st.f32(L.in_b)).t
        hn = eng.keep(hn)
        o, lse, _ = eng.attn(P, T, heads, qkv, None)
        x1 = eng.linear("o", o, Ws[1], st.f32(L.out_b), resid=h).t
        o = eng.keep(o)
        hn2, m2, r2 = eng.ln(x1, st.f32(L.ln2_w), st.f32(L.ln2_b), eps, "fc1")
        g, z = eng.linear("fc1", hn2, Ws[2], st.f32(L.fc_b), act=QGELU, to="fc2", pre=True)
        hn2 = eng.keep(hn2)
        x2 = eng.linear("fc2", g, Ws[3], st.f32(L.proj_b), resid=x1).t
        if save:
            ctx.save_for_backward(h, m1, r1, hn, qkv, o, lse, x1, m2, r2, hn2, z, eng.keep(g))
            ctx.meta = (L, P, T, heads)
            ctx.eng = eng
        return x2

    @staticmethod
    def backward(ctx, dx2):
        h, m1, r1, hn, qkv, o, lse, x1, m2, r2, hn2, z, gact = ctx.saved_tensors
        L, P, T, heads = ctx.meta
        eng = ctx.eng
        st = L.store
        st.grad_begin()
        W = h.shape[-1]
        R = h.shape[0]
        dx2 = dx2.contiguous()
        _wgrad(dx2, gact, st.g(L.proj_w), st.g(L.proj_b))
        dz = eng.dgrad(_Act(dx2), st.wt(L.proj_w), act=QGELU, dact=z, q8=True)
        _wgrad(dz.t, hn2, st.g(L.fc_w), st.g(L.fc_b))
        dhn2 = eng.dgrad(dz, st.wt(L.fc_w)).t
        del dz
        dx1 = torch.empty_like(h)
        # out_proj's output gradient is dx1 = LN gradient + dx2, so its bias gradient is the column
        # sums of dx1 INCLUDING the residual gradient: said with dsum_with_dres
        g1, gb = eng.ln_bwd(dhn2, x1, m2, r2, st.f32(L.ln2_w), dx1, dx2, st.g(L.ln2_w), st.g(L.ln2_b),
                            st.g(L.out_b), dsum_with_dres=True)
        _wgrad(dx1, o, st.g(L.out_w), gb)
        do = eng.dgrad(g1, st.wt(L.out_w)).t
        del g1
        dqkv = eng.attn_bwd(P, T, heads, qkv, None, o, do, lse)
        _wgrad(dqkv.t, hn, st.g(L.in_w), st.g(L.in_b))
        dhn = eng.dgrad(dqkv, st.wt(L.in_w)).t
        dh = torch.empty_like(h)
        N.layernorm_bwd(R, W, dhn, _rows(W), h, _rows(W), m1, r1, st.f32(L.ln1_w), dh, _rows(W),
                        dx1, _rows(W), st.g(L.ln1_w), st.g(L.ln1_b))
        st.grad_ready(L.span)
        eng.bwd_done()
        return dh, None, None, None, None, None, None, None


# ================================================================================================
# ViT stem: pair-image gather + patchify GEMM + class token + positional quirk + ln_pre
# ================================================================================================
class VitStemFn(torch.autograd.Function):
    """conv1 (k = s = patch, no bias) as im2col + GEMM. K = 3 p^2 is padded to the GEMM's
    128-element granularity when it is not a multiple of it (ViT-L/14: 588 -> 640, zero columns in
    the patches and the weight operand), so every patch size takes the MFMA kernels."""

    @staticmethod
    def kpad(K):
        return K if K % 128 == 0 else (K + 127) // 128 * 128

    @staticmethod
    def forward(ctx, images, pairs, anchor, L, patch, eps, cdtype):
        st = L.store
        B, Nst, _, R_, _ = images.shape
        npair = pairs.shape[1]
        P = B * npair
        g = R_ // patch
        gg = g * g
        ntok = 1 + 2 * gg
        Wc = st.w(L.conv_w)  # [W][3][p][p] -> [W][3p^2]
        W = Wc.shape[0]
        K = 3 * patch * patch
        Kp = VitStemFn.kpad(K)
        Wc = Wc.reshape(W, K)
        if Kp != K:
            Wp = torch.zeros(W, Kp, device=images.device, dtype=cdtype)
            Wp[:, :K] = Wc
            Wc = Wp
        patches = torch.empty(P * 2 * gg, Kp, device=images.device, dtype=cdtype)
        N.vit_im2col(B, Nst, npair, R_, patch, images, pairs, patches)
        po = _linear(patches, Wc)
        del patches
        x0 = torch.empty(P * ntok, W, device=images.device, dtype=cdtype)
        h0 = torch.empty_like(x0)
        mean = torch.empty(P * ntok, device=images.device)
        rstd = torch.empty_like(mean)
        N.vit_embed_fwd(P, ntok, W, gg, po, st.f32(L.cls), st.f32(L.pos), st.f32(L.ln_w),
                        st.f32(L.ln_b), eps, x0, h0, mean, rstd)
        ctx.save_for_backward(images, pairs, x0, mean, rstd)
        ctx.meta = (L, patch, cdtype, P, ntok, W, gg)
        return h0

    @staticmethod
    def backward(ctx, dh0):
        images, pairs, x0, mean, rstd = ctx.saved_tensors
        L, patch, cdtype, P, ntok, W, gg = ctx.meta
        st = L.store
        B, Nst, _, R_, _ = images.shape
        dpo = torch.empty(P * (ntok - 1), W, device=x0.device, dtype=cdtype)
        N.vit_embed_bwd(P, ntok, W, gg, dh0.contiguous(), x0, mean, rstd, st.f32(L.ln_w), dpo,
                        st.g(L.cls), st.g(L.pos), st.g(L.ln_w), st.g(L.ln_b))
        K = 3 * patch * patch
        Kp = VitStemFn.kpad(K)
        patches = torch.empty(P * 2 * gg, Kp, device=x0.device, dtype=cdtype)
        N.vit_im2col(B, Nst, pairs.shape[1], R_, patch, images, pairs, patches)  # recompute
        gW = st.g(L.conv_w).view(W, K)  # += dpo^T patches[:, :K]
        N.gemm(dpo, patches, gW, W, K, dpo.shape[0], trans=1, lda=W, ldb=Kp, accumulate=True)
        st.grad_ready(L.span)
        return None, None, None, None, None, None, None


# ================================================================================================
# ViT output projection (x @ proj, no ln_post: clip/model.py:301-304, lxrt:783)
# ================================================================================================
class VitProjFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, anchor, L):
        st = L.store
        out = _linear(h, st.wt(L.proj))  # B(k=w, n=e) = proj[w][e] -> NT operand proj^T [E][W]
        ctx.save_for_backward(h)
        ctx.meta = L
        return out

    @staticmethod
    def backward(ctx, dv):
        (h,) = ctx.saved_tensors
        L = ctx.meta
        st = L.store
        dv = dv.contiguous()
        gp = st.g(L.proj)  # [W][E] += h^T dv
        R = h.shape[0]
        N.gemm(h, dv, gp, gp.shape[0], gp.shape[1], R, trans=1, lda=h.shape[-1], ldb=dv.shape[-1],
               accumulate=True)
        dh = _dgrad(dv, st.w(L.proj))  # dh[r][w] = sum_e dv[r][e] proj[w][e]
        st.grad_ready(L.span)
        return dh, None, None


# ================================================================================================
# Joint input: visn_fc (Linear + LN) and BertEmbeddings (+LN) written in place into the two
# halves of the joint [P][T][H] buffer; additive key mask (lxrt/modeling.py:1537-1545, 1071-1094)
# ================================================================================================
class JointInputFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vout, ids, tt, attn_mask, anchor, L, P, Lt, Tv, eps, cdtype, drops=(None, None)):
        """drops = (BertEmbeddings :369, VisualFeatEncoder :601)."""
        st = L.store
        H = st.f32(L.word).shape[1]
        T = Lt + Tv
        dev = ids.device
        joint = torch.empty(P * T, H, device=dev, dtype=cdtype)
        me = torch.empty(P * Lt, device=dev)
        re = torch.empty_like(me)
        N.embed_ln_fwd(P, Lt, H, ids, tt, st.f32(L.word), st.f32(L.pos), st.f32(L.type),
                       st.f32(L.eln_w), st.f32(L.eln_b), eps, joint, T * H, me, re, drop=drops[0])
        saved = [ids, tt, me, re]
        if vout is not None:
            vpre = _linear(vout, st.w(L.v_w), bias=st.f32(L.v_b))
            mv = torch.empty(P * Tv, device=dev)
            rv = torch.empty_like(mv)
            N.layernorm_fwd(P * Tv, H, vpre, _rows(H), st.f32(L.vln_w), st.f32(L.vln_b), eps,
                            joint[Lt:], N.rows(H, T * H, Tv), mv, rv, drop=drops[1])
            saved += [vout, vpre, mv, rv]
        key_bias = torch.zeros(P, T, device=dev)
        key_bias[:, :Lt] = (1.0 - attn_mask.float()) * -10000.0
        ctx.save_for_backward(*saved)
        ctx.meta = (L, P, Lt, Tv, vout is not None, drops)
        ctx.mark_non_differentiable(key_bias)
        return joint, key_bias

    @staticmethod
    def backward(ctx, djoint, _dkb):
        L, P, Lt, Tv, has_v, drops = ctx.meta
        st = L.store
        sv = ctx.saved_tensors
        ids, tt, me, re = sv[:4]
        H = st.f32(L.word).shape[1]
        T = Lt + Tv
        djoint = djoint.contiguous()
        N.embed_ln_bwd(P, Lt, H, ids, tt, st.f32(L.word), st.f32(L.pos), st.f32(L.type),
                       st.f32(L.eln_w), me, re, djoint, T * H, st.g(L.word), st.g(L.pos),
                       st.g(L.type), st.g(L.eln_w), st.g(L.eln_b), drop=drops[0])
        dvout = None
        if has_v:
            vout, vpre, mv, rv = sv[4:]
            dvpre = torch.empty_like(vpre)
            N.layernorm_bwd(P * Tv, H, djoint[Lt:], N.rows(H, T * H, Tv), vpre, _rows(H), mv, rv,
                            st.f32(L.vln_w), dvpre, _rows(H), None, _rows(H), st.g(L.vln_w),
                            st.g(L.vln_b), drop_dy=drops[1])
            _wgrad(dvpre, vout, st.g(L.v_w), st.g(L.v_b))
        st.grad_ready(L.span)
        if has_v:
            dvout = _dgrad(dvpre, st.wt(L.v_w))
        return dvout, None, None, None, None, None, None, None, None, None, None, None


# ================================================================================================
# Image-only input (multimodal_img_part): JointInputFn's visual half on its own, visn_fc (Linear +
# LN + dropout, lxrt:569-602) over the ViT rows -> [P*Tv][H]; no embedding is computed
# ================================================================================================
class VisnInputFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vout, anchor, L, eps, drop=None):
        st = L.store
        vpre = _linear(vout, st.w(L.v_w), bias=st.f32(L.v_b))
        R, H = vpre.shape
        out = torch.empty_like(vpre)
        mv = torch.empty(R, device=vout.device)
        rv = torch.empty_like(mv)
        N.layernorm_fwd(R, H, vpre, _rows(H), st.f32(L.vln_w), st.f32(L.vln_b), eps, out, _rows(H),
                        mv, rv, drop=drop)
        ctx.save_for_backward(vout, vpre, mv, rv)
        ctx.meta = (L, drop)
        return out

    @staticmethod
    def backward(ctx, dout):
        L, drop = ctx.meta
        st = L.store
        vout, vpre, mv, rv = ctx.saved_tensors
        R, H = vpre.shape
        dvpre = torch.empty_like(vpre)
        N.layernorm_bwd(R, H, dout.contiguous(), _rows(H), vpre, _rows(H), mv, rv, st.f32(L.vln_w),
                        dvpre, _rows(H), None, _rows(H), st.g(L.vln_w), st.g(L.vln_b), drop_dy=drop)
        _wgrad(dvpre, vout, st.g(L.v_w), st.g(L.v_b))
        st.grad_ready(L.span)
        return _dgrad(dvpre, st.wt(L.v_w)), None, None, None, None


# ================================================================================================
# generic pieces used by the (small, fp32) BERSON head
# ================================================================================================
class LinearFn(torch.autograd.Function):
    """y = act(x W^T + b); W, b taken from a ParamStore (grads accumulated into its buffer)."""

    @staticmethod
    def forward(ctx, x, anchor, store, wname, bname, act):
        x = x.contiguous()
        shp = x.shape
        x2 = x.view(-1, shp[-1])
        W = store.w(wname)
        aux = None
        if act:
            aux = torch.empty(x2.shape[0], W.shape[0], device=x.device, dtype=x.dtype)
        y = _linear(x2, W, bias=store.f32(bname) if bname else None, act=act, aux=aux)
        ctx.save_for_backward(x2, aux if act else None)
        ctx.meta = (store, wname, bname, act, shp)
        return y.view(*shp[:-1], W.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, aux = ctx.saved_tensors
        store, wname, bname, act, shp = ctx.meta
        dy = dy.contiguous().view(-1, dy.shape[-1])
        if act:
            dz = torch.empty_like(dy)
            N.act_bwd(aux, dy, dz, act)
            dy = dz
        _wgrad(dy, x2, store.g(wname))
        if bname:
            _colsum(dy, store.g(bname))
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _dgrad(dy, store.wt(wname)).view(shp)
        return dx, None, None, None, None, None


class LinearLowpFn(torch.autograd.Function):
    """y (fp32) = act(x W^T + b) for an fp32-stored head weight applied to a compute-dtype (bf16)
    activation: the GEMMs run on the bf16 MFMA kernels with a per-call bf16 copy of W (and of
    W^T for the dgrad), the fp32 gradient is accumulated into the store. Used in bf16 mode for
    the one large head projection (HierarchicalAttention.sentence_tran over every text token,
    modeling_bert.py:697-699); parity (fp32) mode keeps LinearFn."""

    @staticmethod
    def forward(ctx, x, anchor, store, wname, bname, act):
        x = x.contiguous()
        shp = x.shape
        x2 = x.view(-1, shp[-1])
        W32 = store.f32(wname)
        Wb = torch.empty(W32.shape, device=x.device, dtype=x.dtype)
        N.cast(W32, Wb)
        aux = torch.empty(x2.shape[0], W32.shape[0], device=x.device) if act else None
        y = _linear(x2, Wb, bias=store.f32(bname) if bname else None, act=act, aux=aux,
                    out_dtype=torch.float32)
        ctx.save_for_backward(x2, aux if act else None)
        ctx.meta = (store, wname, bname, act, shp)
        return y.view(*shp[:-1], W32.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, aux = ctx.saved_tensors
        store, wname, bname, act, shp = ctx.meta
        dy = dy.contiguous().view(-1, dy.shape[-1])
        if act:
            dz = torch.empty_like(dy)
            N.act_bwd(aux, dy, dz, act)
            dy = dz
        if bname:
            _colsum(dy, store.g(bname))
        dyb = torch.empty(dy.shape, device=dy.device, dtype=x2.dtype)
        N.cast(dy, dyb)
        _wgrad(dyb, x2, store.g(wname))
        dx = None
        if ctx.needs_input_grad[0]:
            W32 = store.f32(wname)
            WTb = torch.empty(W32.shape[1], W32.shape[0], device=dy.device, dtype=x2.dtype)
            N.transpose_cast(W32, WTb)
            dx = _dgrad(dyb, WTb).view(shp)
        return dx, None, None, None, None, None


class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, anchor, store, prefix, eps):
        x = x.contiguous()
        shp = x.shape
        C = shp[-1]
        R = x.numel() // C
        y = torch.empty_like(x)
        m = torch.empty(R, device=x.device)
        r = torch.empty_like(m)
        N.layernorm_fwd(R, C, x, _rows(C), store.f32(prefix + ".weight"), store.f32(prefix + ".bias"),
                        eps, y, _rows(C), m, r)
        ctx.save_for_backward(x, m, r)
        ctx.meta = (store, prefix)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, m, r = ctx.saved_tensors
        store, prefix = ctx.meta
        C = x.shape[-1]
        R = x.numel() // C
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        N.layernorm_bwd(R, C, dy, _rows(C), x, _rows(C), m, r, store.f32(prefix + ".weight"), dx,
                        _rows(C), None, _rows(C), store.g(prefix + ".weight"),
                        store.g(prefix + ".bias"))
        return dx, None, None, None, None


class SmallAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, key_bias, heads, drop=None):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        B, T, D = q.shape
        d = D // heads
        out = torch.empty_like(q)
        probs = torch.empty(B, heads, T, T, device=q.device)
        N.small_attn_fwd(B, T, heads, d, q, k, v, key_bias, 1.0 / math.sqrt(d), out, probs,
                         drop=drop)
        ctx.save_for_backward(q, k, v, probs)
        ctx.heads = heads
        ctx.drop = drop
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, probs = ctx.saved_tensors
        B, T, D = q.shape
        d = D // ctx.heads
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        N.small_attn_bwd(B, T, ctx.heads, d, q, k, v, probs, dout.contiguous(), 1.0 / math.sqrt(d),
                         dq, dk, dv, drop=ctx.drop)
        return dq, dk, dv, None, None, None


class SpanPoolFn(torch.autograd.Function):
    """HierarchicalAttention span pooling over the text rows of the joint output."""

    @staticmethod
    def forward(ctx, top, score, sep, drop=None):
        P, Lt, H = top.shape
        top = top.contiguous()
        probs = torch.empty(P, 2, Lt, device=top.device)
        mix = torch.empty(P, 2, H, device=top.device)
        N.span_pool_fwd(P, Lt, H, top, Lt * H, score.contiguous(), sep, probs, mix, drop=drop)
        ctx.save_for_backward(top, probs, sep)
        ctx.drop = drop
        return mix

    @staticmethod
    def backward(ctx, dmix):
        top, probs, sep = ctx.saved_tensors
        P, Lt, H = top.shape
        dscore = torch.empty(P, Lt, device=top.device)
        dtop = torch.zeros_like(top)
        N.span_pool_bwd(P, Lt, H, top, Lt * H, probs, sep, dmix.contiguous(), dscore, dtop,
                        drop=ctx.drop)
        return dtop, dscore, None, None


class DropoutFn(torch.autograd.Function):
    """y = dropout(x) with a counter-based mask (the head's nn.Dropout sites); the backward
    applies the same mask to dy."""

    @staticmethod
    def forward(ctx, x, drop):
        x = x.contiguous()
        y = torch.empty_like(x)
        N.dropout(x, y, drop)
        ctx.drop = drop
        return y

    @staticmethod
    def backward(ctx, dy):
        dx = torch.empty_like(dy, memory_format=torch.contiguous_format)
        N.dropout(dy.contiguous(), dx, ctx.drop)
        return dx, None


def dropout(x, drop):
    return x if drop is None else DropoutFn.apply(x, drop)


class LstmCellFn(torch.autograd.Function):
    """One nn.LSTM step from precomputed gate inputs: gx = x W_ih^T + b_ih (a row of the one GEMM
    over all decoder steps) and gh = h W_hh^T + b_hh -> (h', c') (mmseq_lstm_cell_fwd/bwd)."""

    @staticmethod
    def forward(ctx, gx, gh, c):
        B, H = c.shape
        c = c.contiguous()
        gh = gh.contiguous()
        if gx.stride(-1) != 1:
            gx = gx.contiguous()
        h2, c2 = torch.empty_like(c), torch.empty_like(c)
        act = torch.empty(B, 4 * H, device=c.device)
        N.lstm_cell_fwd(gx, gh, c, h2, c2, act)
        ctx.save_for_backward(act, c, c2)
        return h2, c2

    @staticmethod
    def backward(ctx, dh, dc):
        act, c, c2 = ctx.saved_tensors
        dg = torch.empty_like(act)
        dcp = torch.empty_like(c)
        N.lstm_cell_bwd(act, c, c2, None if dh is None else dh.contiguous(),
                        None if dc is None else dc.contiguous(), dg, dcp)
        return dg, dg, dcp


class PointerFn(torch.autograd.Function):
    """e = tanh_linear(tanh(q + key + okey)) -> masked log-softmax -> per-step NLL."""

    @staticmethod
    def forward(ctx, q, key, okey, anchor, store, wname, bname, pointed, tgt_len, target):
        B, Nn, H = q.shape
        q, key, okey = q.contiguous(), key.contiguous(), okey.contiguous()
        logp = torch.empty(B, Nn, Nn, device=q.device)
        nll = torch.empty(B, Nn, device=q.device)
        N.pointer_fwd(B, Nn, H, q, key, okey, store.f32(wname).view(-1), store.f32(bname), pointed,
                      tgt_len, target, logp, nll)
        ctx.save_for_backward(q, key, okey, logp, pointed, tgt_len, target)
        ctx.meta = (store, wname, bname)
        ctx.mark_non_differentiable(logp)
        return nll, logp

    @staticmethod
    def backward(ctx, dnll, _dlogp):
        q, key, okey, logp, pointed, tgt_len, target = ctx.saved_tensors
        store, wname, bname = ctx.meta
        B, Nn, H = q.shape
        dq, dkey = torch.empty_like(q), torch.empty_like(key)
        dokey = torch.zeros_like(okey)
        N.pointer_bwd(B, Nn, H, q, key, okey, store.f32(wname).view(-1), logp, pointed, tgt_len,
                      target, dnll.contiguous(), dq, dkey, dokey, store.g(wname).view(-1),
                      store.g(bname))
        return dq, dkey, dokey, None, None, None, None, None, None, None


ORDER_WEIGHTS = ("decoder.weight_ih_l0", "decoder.bias_ih_l0", "decoder.weight_hh_l0",
                 "decoder.bias_hh_l0", "query_linear.weight", "query_linear.bias", "pw_k.weight",
                 "tanh_linear.weight", "tanh_linear.bias")
ORDER_WEIGHTS_T = ("decoder.weight_ih_l0", "decoder.weight_hh_l0", "query_linear.weight",
                   "pw_k.weight")


def _chunks(n, step):
    """n items in chunks of `step` -> (start, length, whole); whole: the one chunk is all n."""
    for i0 in range(0, n, step):
        k = min(step, n - i0)
        yield i0, k, k == n


def _cached_ws(owner, slot, key, nbytes, device):
    """The f32 workspace `owner` keeps under (slot, key), allocated where there is none and again
    where the one kept is too small or on another device (so a slot with one key grows on
    demand). Used by berson's decoder entries too."""
    cache = owner.__dict__.setdefault(slot, {})
    ws = cache.get(key)
    if ws is None or ws.numel() * 4 < nbytes or ws.device != device:
        ws = cache[key] = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
    return ws


def order_grad_chunk(B, Nn, H, Kn, cap):
    """-> (candidates per call, bytes) of mmseq_order_score_bwd under `cap` bytes."""
    from .berson import _fit_chunk  # berson imports this module
    return _fit_chunk(lambda k: N.order_score_bwd_workspace(B, Nn, H, k), Kn, cap=cap)


class OrderScoreFn(torch.autograd.Function):
    """nll [B][K] = mmseq_order_score of K candidate orders per story (orders int64 [K][N] or
    [B][K][N] on the device), differentiable in doc, okey, hist, h0, c0 and the nine decoder
    weights of `store` (mmseq_order_score_bwd; weight gradients accumulate into store.g(...) like
    PointerFn's). K is split into chunks whose backward workspace stays within `cap` bytes; the
    chunks' input gradients are added in chunk order. An unsupported shape raises
    _native.Unsupported in the forward."""

    @staticmethod
    def forward(ctx, doc, okey, hist, h0, c0, anchor, store, orders, cap):
        B, Nn, H = doc.shape
        Kn = int(orders.shape[-2])
        doc, okey, hist = doc.contiguous(), okey.contiguous(), hist.contiguous()
        h0, c0, orders = h0.contiguous(), c0.contiguous(), orders.contiguous()
        kc, nbytes = order_grad_chunk(B, Nn, H, Kn, cap)
        if nbytes == 0 or N.order_score_workspace(B, Nn, H, kc) == 0:
            raise N.Unsupported(f"OrderScoreFn: B={B} N={Nn} H={H} K={Kn} is outside "
                                "mmseq_order_score's limits")
        # one workspace per store, grown on demand: it serves the forward and the backward
        ws = _cached_ws(store, "_order_grad_ws", None,
                        max(nbytes, N.order_score_workspace(B, Nn, H, kc)), doc.device)
        weights = [store.f32(n) for n in ORDER_WEIGHTS]
        nll = torch.empty(B, Kn, dtype=torch.float32, device=doc.device)
        for k0, k, whole in _chunks(Kn, kc):
            o_c = orders if whole else orders[..., k0:k0 + k, :].contiguous()
            n_c = nll if whole else torch.empty(B, k, dtype=torch.float32, device=doc.device)
            N._check_shape(N.order_score(doc, okey, hist, h0, c0, weights, o_c, n_c, None, ws),
                           "mmseq_order_score")
            if not whole:
                nll[:, k0:k0 + k] = n_c
        ctx.save_for_backward(doc, okey, hist, h0, c0, orders)
        ctx.meta = (store, kc)
        return nll

    @staticmethod
    def backward(ctx, dnll):
        doc, okey, hist, h0, c0, orders = ctx.saved_tensors
        store, kc = ctx.meta
        B, Nn, H = doc.shape
        Kn = int(orders.shape[-2])
        if store.shadow_stale:  # the transposed copies the data-gradient GEMMs read
            store.refresh_shadows()
        weights = [store.f32(n) for n in ORDER_WEIGHTS]
        weights_t = [store.wt(n) for n in ORDER_WEIGHTS_T]
        dweights = [store.g(n) for n in ORDER_WEIGHTS]
        ws = _cached_ws(store, "_order_grad_ws", None, N.order_score_bwd_workspace(B, Nn, H, kc),
                        doc.device)
        dnll = dnll.contiguous().float()
        total = None
        for k0, k, whole in _chunks(Kn, kc):
            o_c = orders if whole else orders[..., k0:k0 + k, :].contiguous()
            g_c = dnll if whole else dnll[:, k0:k0 + k].contiguous()
            dins = [torch.empty_like(t) for t in (doc, okey, hist, h0, c0)]
            N._check_shape(N.order_score_bwd(doc, okey, hist, h0, c0, weights, weights_t, o_c, g_c,
                                             dins, dweights, ws), "mmseq_order_score_bwd")
            if total is None:
                total = dins
            else:
                for a, d in zip(total, dins):
                    a.add_(d)
        return (*total, None, None, None, None)


# ================================================================================================
# text+image pretraining: row selection and the masked-LM loss over the labelled rows
# ================================================================================================
class RowsGatherFn(torch.autograd.Function):
    """out[r] = keep[r] ? x[src[r]] : 0 (mmseq_rows_gather_fwd / _bwd): x [R_in][cols] or
    [P][rpb][cols] with any row / batch strides (a view is read in place), src int32 [R_out] with unique entries in [0, R_in), keep uint8 [R_out] or None. One
    Function for the PISP patch swap (a permutation), the MRM masking (identity src + keep) and the
    compaction of the labelled rows (R_out < R_in)."""

    @staticmethod
    def forward(ctx, x, src, keep=None):
        out = torch.empty(src.numel(), x.shape[-1], device=x.device, dtype=x.dtype)
        N.rows_gather_fwd(x, src, keep, out)
        ctx.save_for_backward(src, keep)
        ctx.x_shape = tuple(x.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        src, keep = ctx.saved_tensors
        dout = dout.contiguous()
        din = torch.empty(ctx.x_shape, device=dout.device, dtype=dout.dtype)
        N.rows_gather_bwd(dout, src, keep, din)
        return din, None, None


def _decoder_wt(store, wname):
    """The tied decoder's dgrad operand: the word table transposed, [H][ld] in the compute dtype with
    ld = vocab rounded up to 64 and zeros in the padding columns (K = ld of the dgrad GEMM, which
    takes the loss kernel's row-padded dlogits as they are). Rebuilt once per store version."""
    W = store.w(wname)
    V, H = W.shape
    ld = (V + 63) // 64 * 64
    hit = getattr(store, "_decoder_wt", None)
    if hit is None or hit[0] != (store.version, wname, W.dtype):
        wt = hit[1] if hit is not None and hit[1].shape == (H, ld) and hit[1].dtype == W.dtype \
            else torch.zeros(H, ld, device=W.device, dtype=W.dtype)
        wt[:, :V].copy_(W.t())
        hit = store._decoder_wt = ((store.version, wname, W.dtype), wt)
    return hit[1]


class VocabXentFn(torch.autograd.Function):
    """mean over the kept rows of CrossEntropy(h W^T + b, labels) for the tied LM decoder
    (lxrt/modeling.py:1164-1173, :2260-2266): the decoder GEMM writes a row-padded logit buffer
    (ld = vocab rounded up to 64), mmseq_xent_fwd reduces it to the loss, mmseq_xent_bwd turns the
    same buffer into dlogits in place, and that buffer is the operand of the NT dgrad GEMM (K = ld)
    and of the TN weight-gradient GEMM, whose result accumulates into the WORD-EMBEDDING gradient
    (the weight is tied) with the bias gradient fused. No [rows][vocab] probabilities are stored
    and no float atomics run: two calls give the same bits. backward() consumes the saved logits,
    so it runs once per forward."""

    @staticmethod
    def forward(ctx, h, anchor, wstore, wname, bstore, bname, labels, ignore_index):
        h = h.contiguous()
        Mc, H = h.shape
        W = wstore.w(wname)
        V = W.shape[0]
        ld = (V + 63) // 64 * 64
        logits = torch.empty(Mc, ld, device=h.device, dtype=h.dtype)
        N.gemm(h, W, logits, Mc, V, H, ldc=ld, bias=bstore.f32(bname))
        lse = torch.empty(Mc, device=h.device)
        loss_row = torch.empty(Mc, device=h.device)
        stats = torch.empty(2, device=h.device)
        labels = labels.contiguous()
        N.xent_fwd(logits, V, labels, ignore_index, lse, loss_row, stats)
        ctx.save_for_backward(h, logits, labels, lse, stats)
        ctx.meta = (wstore, wname, bstore, bname, ignore_index, V)
        ctx.done = False
        ctx.mark_non_differentiable(lse)
        return stats[0].clone(), lse

    @staticmethod
    def backward(ctx, g, _dlse):
        h, dl, labels, lse, stats = ctx.saved_tensors
        wstore, wname, bstore, bname, ignore_index, V = ctx.meta
        if ctx.done:
            raise RuntimeError("VocabXentFn.backward ran twice: it overwrites the saved logits")
        ctx.done = True
        N.xent_bwd(dl, V, labels, ignore_index, lse, stats, g.reshape(1).float().contiguous())
        Mc, ld = dl.shape
        gW, gb = wstore.g(wname), bstore.g(bname)
        # the bf16 TN kernel takes row counts that are multiples of 8: the odd tail of the vocabulary
        # (50265 = 8 * 6283 + 1) is a second, tiny call on the last rows of the table
        V8 = V // 8 * 8 if dl.dtype == torch.bfloat16 and 0 < V // 8 * 8 < V else V
        if Mc:
            N.gemm_wgrad(dl, h, gW[:V8], gb[:V8], lddy=ld)
            if V8 < V:
                N.gemm_wgrad(dl[:, V8:], h, gW[V8:], gb[V8:], lddy=ld)
        dh = None
        if ctx.needs_input_grad[0]:
            dh = torch.empty_like(h)
            N.gemm(dl, _decoder_wt(wstore, wname), dh, Mc, h.shape[1], ld)
        return dh, None, None, None, None, None, None, None


def mlm_mask(input_ids, pad_id, cls_id, mask_id, vocab, ignore_index, p, seed, stream_id=0):
    """Dynamic MLM masking on the device (mmseq_mlm_mask; trainers/train_utils.py:19-66):
    input_ids int64 [B][L] is masked IN PLACE, the labels int64 [B][L] are returned. The same
    (seed, stream_id) gives the same bits."""
    labels = torch.empty_like(input_ids)
    N.mlm_mask(input_ids, labels, int(pad_id), int(cls_id), int(mask_id), int(vocab),
               int(ignore_index), float(p), int(seed), int(stream_id))
    return labels


def compact_rows(labels, ignore_index, count):
    """Device labels -> (src int32 [R], labels int64 [R]) whose first count[0] entries are the
    labelled rows in row order (mmseq_rows_compact); count: int32 [1] on the device, written by the
    kernel and read by the caller, who slices both."""
    flat = labels.reshape(-1).to(torch.int64).contiguous()
    src = torch.empty(flat.numel(), dtype=torch.int32, device=flat.device)
    lab = torch.empty_like(flat)
    N.rows_compact(flat, int(ignore_index), src, lab, count)
    return src, lab


def labelled_rows(labels, ignore_index, device):
    """(src int32 [M] on `device`, labels int64 [M] on `device`) of the rows with a label, in row
    order. The row count is the decoder GEMM's M: host labels give it for free, device labels run
    the compaction kernel and read that one integer back."""
    if labels.is_cuda:
        count = torch.empty(1, dtype=torch.int32, device=labels.device)
        src, lab = compact_rows(labels, ignore_index, count)
        n = int(count.item())
        return src[:n].to(device), lab[:n].to(device)
    flat = labels.reshape(-1)
    src = torch.nonzero(flat != ignore_index).view(-1)
    return src.to(device, torch.int32), flat[src].to(device, torch.int64)


class MlmLossFn:
    """The masked-LM term on the labelled rows only (ignored rows have exactly zero loss and
    gradient): compaction of lang_output's labelled rows (RowsGatherFn), cls.predictions.transform
    (dense + erf-GELU + LayerNorm 1e-12), tied decoder + cls.predictions.bias and the fused loss
    (VocabXentFn). With no labelled row the result is 0 / 0 = NaN, as the reference's.
    `rows`: the (src, labels) pair of labelled_rows when the caller has it already (a device batch
    reads the row count back together with its other status); None computes it from `labels`."""

    @staticmethod
    def apply(lang_output, labels, ignore_index, anchor, head_store, word_store,
              wname="embeddings.word_embeddings.weight", prefix="cls.predictions.", rows=None):
        x = lang_output  # [rows][H] or [P][Lt][H], e.g. the text rows of the joint buffer, in place
        src, lab = labelled_rows(labels, ignore_index, x.device) if rows is None else rows
        hc = RowsGatherFn.apply(x, src, None)
        t = LinearFn.apply(hc, anchor, head_store, prefix + "transform.dense.weight",
                           prefix + "transform.dense.bias", GELU)
        t = LayerNormFn.apply(t, anchor, head_store, prefix + "transform.LayerNorm", 1e-12)
        loss, _ = VocabXentFn.apply(t, anchor, word_store, wname, head_store, prefix + "bias", lab,
                                    ignore_index)
        return loss


# ================================================================================================
# evaluation of the masked-LM head: the loss's one pass, with rank and the k best words
# ================================================================================================
def vocab_eval(h, wstore, wname, bstore, bname, labels, ignore_index, k, totals=None):
    """The evaluation twin of VocabXentFn.forward, under no_grad and with nothing saved: the tied
    decoder GEMM into the row-padded logit buffer exactly as there, then ONE pass of
    mmseq_xent_eval. h [M][H], labels int64 [M] (ignore_index: no label, rank -1, top-k still
    written). Returns a dict of device tensors: lse, loss_row (the forward's bits), rank int32 [M],
    topk_idx int32 [M][k], topk_logit f32 [M][k] in the order (value descending, word id
    ascending), mean_loss (the forward's stats[0] bits). `totals` f64 [4] accumulates (sum of NLL,
    labelled rows, rank 0, rank < k) on the device."""
    with torch.no_grad():
        h = h.detach().contiguous()
        Mc, H = h.shape
        W = wstore.w(wname)
        V = W.shape[0]
        ld = (V + 63) // 64 * 64
        logits = torch.empty(Mc, ld, device=h.device, dtype=h.dtype)
        N.gemm(h, W, logits, Mc, V, H, ldc=ld, bias=bstore.f32(bname))
        dev = h.device
        out = {"lse": torch.empty(Mc, device=dev), "loss_row": torch.empty(Mc, device=dev),
               "rank": torch.empty(Mc, dtype=torch.int32, device=dev),
               "topk_idx": torch.empty(Mc, k, dtype=torch.int32, device=dev),
               "topk_logit": torch.empty(Mc, k, device=dev)}
        stats = torch.empty(2, device=dev)
        N.xent_eval(logits, V, labels.contiguous(), ignore_index, k, out["lse"], out["loss_row"],
                    out["rank"], out["topk_idx"] if k else None, out["topk_logit"] if k else None,
                    totals, stats)
        out["mean_loss"] = stats[0].clone()
    return out


def mlm_eval(lang_output, labels, ignore_index, head_store, word_store, k, rows=None, totals=None,
             wname="embeddings.word_embeddings.weight", prefix="cls.predictions."):
    """The evaluation twin of MlmLossFn.apply: gather the labelled rows, cls.predictions.transform,
    then vocab_eval. Returns vocab_eval's dict plus `rows` (int32: the flat source row of each
    labelled position, in row order) and `labels` (int64, their gold ids). labels=None evaluates
    EVERY row (fill-mask over whole sequences): rank is -1 and the loss 0 throughout."""
    x = lang_output
    with torch.no_grad():
        if labels is None and rows is None:
            n = x.numel() // x.shape[-1]
            src = torch.arange(n, dtype=torch.int32, device=x.device)
            lab = torch.full((n,), int(ignore_index), dtype=torch.int64, device=x.device)
        else:
            src, lab = labelled_rows(labels, ignore_index, x.device) if rows is None else rows
        hc = torch.empty(src.numel(), x.shape[-1], device=x.device, dtype=x.dtype)
        N.rows_gather_fwd(x.detach(), src, None, hc)
        anchor = None
        t = LinearFn.apply(hc, anchor, head_store, prefix + "transform.dense.weight",
                           prefix + "transform.dense.bias", GELU)
        t = LayerNormFn.apply(t, anchor, head_store, prefix + "transform.LayerNorm", 1e-12)
        out = vocab_eval(t, word_store, wname, head_store, prefix + "bias", lab, ignore_index, k,
                         totals)
    out["rows"], out["labels"] = src, lab
    return out
