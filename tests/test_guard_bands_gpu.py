"""Every entry point that takes a leading dimension and has a ragged edge, in buffers with guard
bands and poisoned padding (tests/guard_util.py):

  outputs  live in a buffer filled with a bit pattern; after the call everything outside the
           declared extents (guard rows, gap columns, rows between batches, columns of no head
           slice) must still hold it, bit for bit;
  inputs   the call runs with 0 and with NaN in everything outside the inputs' declared extents;
           all outputs must be finite and torch.equal between the two runs.

Where a layout-independent result is cheap to have (attention, GEMM), the strided result must
also equal, bit for bit, the same entry point's result on the packed production layout.

Shapes are the smallest that reach each kernel; every parametrisation names the dispatch condition
read in the source (csrc/attention.hip, gemm.hip, gemm256.hip, layernorm.hip, loss.hip).
"""
import pytest
import torch

import attn_accuracy as acc
from guard_util import Guarded, poison_check

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import native_raw as raw
    from multimodal_sequencing_amd import _native as nat

DEV = "cuda"
F32, BF16 = 0, 1
TDT = {F32: torch.float32, BF16: torch.bfloat16}


def G(rows, cols, ld=None, dtype=torch.float32, **kw):
    return Guarded(rows, cols, ld, dtype, DEV, **kw)


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen).to(DEV)


# =================================================================================================
# attention
# =================================================================================================
P, HEADS = 2, 2
H = HEADS * 64
# V | Q | K inside a row of 3H + 64 elements, at offsets that are no multiples of H (multiples of 8:
# check_common wants 16-byte aligned slices); the columns 0-7, 136-151, 280-303 and 432-447 belong
# to no head and hold NaN in the poisoned run
LD_QKV, Q_OFF, K_OFF, V_OFF = 3 * H + 64, 152, 304, 8
OFFS = (Q_OFF, K_OFF, V_OFF)
SLICES = [(V_OFF, H), (Q_OFF, H), (K_OFF, H)]
LD_OUT, LD_DOUT, LD_DQKV = H + 8, H + 16, 3 * H + 56  # ld_dout != ld_out, ld_dqkv != ld_qkv
# key tile 64, query block 128 (64 for variant 0 / fp32), the 1-16-row tail block of the forward
# (((T - 1) & 127) < 16: T = 1, 129, 144, 257, 272, 393) and the dK/dV tail fold (1 <= T % 128 <= 16
# with T >= 128: 129, 144, 257, 272, 393), 17 rows just past either (17, 145, 273)
TS = (1, 17, 64, 65, 128, 129, 144, 145, 257, 272, 273, 393)


class AttnCase:
    """Inputs and guarded buffers of one attention problem in the loose layout; Tq < T is the
    _rows form (out / dout hold Tq rows per sequence)."""

    def __init__(self, T, code, Tq=None, bits=False, offs=OFFS, ld_qkv=LD_QKV, ld_dqkv=LD_DQKV,
                 slices=None):
        dt = TDT[code]
        self.T, self.Tq, self.code, self.dt = T, T if Tq is None else Tq, code, dt
        self.offs, self.ld_qkv, self.ld_dqkv = offs, ld_qkv, ld_dqkv
        slices = SLICES if slices is None else slices
        gen = torch.Generator().manual_seed(77 * T + code)
        q, k, v, dout = (t.to(DEV) for t in acc.make_inputs(P, T, HEADS, gen, dt))
        self.rows = {"q": self._flat(q), "k": self._flat(k), "v": self._flat(v)}
        self.qkv = G(P * T, ld_qkv, ld_qkv, dt, col_ranges=slices)
        for n, off in zip("qkv", offs):
            self.qkv.v2[:, off:off + H] = self.rows[n]
        b = acc.key_bias("random30", P, T, gen) if T > 1 else torch.zeros(P, T)
        self.bias = G(P, T, dtype=torch.float32).set(b.to(DEV))
        Tq = self.Tq
        self.dout_rows = self._flat(dout).view(P, T, H)[:, :Tq].reshape(P * Tq, H).contiguous()
        self.dout = G(P * Tq, H, LD_DOUT, dt).set(self.dout_rows)
        self.out = G(P * Tq, H, LD_OUT, dt)
        self.lse = G(P * HEADS, T)
        self.delta = G(P * HEADS, T)
        self.dqkv = G(P * T, ld_dqkv, ld_dqkv, dt, col_ranges=slices)
        # the backward's inputs O and LSE, in input buffers of their own (poisoned outside)
        self.out_in = G(P * Tq, H, LD_OUT, dt)
        self.lse_in = G(P * HEADS, T)
        if Tq < T:  # the forward writes rows < Tq of lse only: the others are padding to the backward
            self.lse_in.inside[:] = False
            self.lse_in._strided(self.lse_in.inside)[:, :, :Tq] = True
        self.bits = None
        if bits:
            words = nat.lib().mmseq_attn_keep_bits_words(P, T, HEADS)
            self.bits = G(P * HEADS * T, words // (P * HEADS * T), dtype=torch.int64)
        self.unwritten = None
        if Tq < T:
            self.unwritten = torch.zeros(1, P * HEADS, T, dtype=torch.bool, device=DEV)
            self.unwritten[:, :, Tq:] = True

    @staticmethod
    def _flat(x):  # [P][heads][T][64] -> [P*T][H]
        return x.permute(0, 2, 1, 3).reshape(-1, H).contiguous()

    def packed_qkv(self):
        return torch.cat([self.rows[n] for n in "qkv"], 1).contiguous()

    def dqkv_slices(self):
        return [self.dqkv.v2[:, off:off + H] for off in self.offs]

    def arm(self, *outs):
        for g in outs:
            if g is not None:
                g.fill_pattern().snapshot()

    def check(self, **outs):
        for name, g in outs.items():
            if g is not None:
                g.check_untouched(name, also=self.unwritten if name in ("lse", "delta") else None)

    def written(self, g):  # the rows of lse / delta the call writes
        return g.v2.view(P, HEADS, self.T)[..., :self.Tq]


def _fwd(c, variant, drop=None):
    def run():
        c.arm(c.out, c.lse, c.bits)
        bits = None if c.bits is None else c.bits.t
        if c.Tq < c.T:
            raw.attn_fwd_rows(P, c.T, c.Tq, HEADS, c.qkv.t, c.ld_qkv, c.offs, c.bias.t, 1 / 8,
                              c.out.t, LD_OUT, c.lse.t, drop, bits)
        else:
            raw.attn_fwd(P, c.T, HEADS, c.qkv.t, c.ld_qkv, c.offs, c.bias.t, 1 / 8, c.out.t,
                         LD_OUT, c.lse.t, c.code, variant, drop, bits)
        c.check(out=c.out, lse=c.lse, keep_bits=c.bits)
        return [c.out.v2, c.written(c.lse)] + ([c.bits.v2] if c.bits is not None else [])
    return poison_check(run, [c.qkv, c.bias], "attn_fwd")


def _bwd(c, variant, out, lse, drop=None, bits=None):
    c.out_in.set(out)
    c.written(c.lse_in).copy_(lse)
    inputs = [c.qkv, c.bias, c.dout, c.out_in, c.lse_in]

    def run():
        c.arm(c.delta, c.dqkv)
        args = (c.qkv.t, c.ld_qkv, c.offs, c.bias.t, 1 / 8, c.out_in.t, LD_OUT, c.dout.t, LD_DOUT,
                c.lse_in.t, c.delta.t, c.dqkv.t, c.ld_dqkv)
        if c.Tq < c.T:
            raw.attn_bwd_rows(P, c.T, c.Tq, HEADS, *args, drop, bits)
        else:
            raw.attn_bwd(P, c.T, HEADS, *args, c.code, variant, drop, bits)
        c.check(delta=c.delta, dqkv=c.dqkv)
        return [c.written(c.delta)] + c.dqkv_slices()
    return poison_check(run, inputs, "attn_bwd")


def _packed_reference(c, variant, drop=None, bits=False):
    """The same entry points on the packed production layout (Q|K|V, ld = 3H, H, H, 3H)."""
    T, Tq, dt = c.T, c.Tq, c.dt
    qkv = c.packed_qkv()
    out = torch.zeros(P * Tq, H, dtype=dt, device=DEV)
    lse = torch.zeros(P, HEADS, T, device=DEV)
    delta = torch.zeros(P, HEADS, T, device=DEV)
    dqkv = torch.zeros(P * T, 3 * H, dtype=dt, device=DEV)
    kb = nat.attn_keep_bits(P, T, HEADS, DEV) if bits else None
    po = (0, H, 2 * H)
    if Tq < T:
        raw.attn_fwd_rows(P, T, Tq, HEADS, qkv, 3 * H, po, c.bias.t, 1 / 8, out, H, lse, drop, kb)
        raw.attn_bwd_rows(P, T, Tq, HEADS, qkv, 3 * H, po, c.bias.t, 1 / 8, out, H, c.dout_rows, H,
                          lse, delta, dqkv, 3 * H, drop, kb)
    else:
        raw.attn_fwd(P, T, HEADS, qkv, 3 * H, po, c.bias.t, 1 / 8, out, H, lse, c.code, variant,
                     drop, kb)
        raw.attn_bwd(P, T, HEADS, qkv, 3 * H, po, c.bias.t, 1 / 8, out, H, c.dout_rows, H, lse,
                     delta, dqkv, 3 * H, c.code, variant, drop, kb)
    return out, lse[..., :Tq], delta[..., :Tq], [dqkv[:, o:o + H] for o in po]


def _attn_roundtrip(c, variant, drop=None):
    fo = _fwd(c, variant, drop)
    out, lse = fo[0], fo[1]
    bo = _bwd(c, variant, out, lse, drop, None if c.bits is None else c.bits.t)
    r_out, r_lse, r_delta, r_dqkv = _packed_reference(c, variant, drop, c.bits is not None)
    assert torch.equal(out, r_out) and torch.equal(lse, r_lse), "forward depends on the layout"
    assert torch.equal(bo[0], r_delta), "delta depends on the layout"
    for n, a, b in zip(("dQ", "dK", "dV"), bo[1:], r_dqkv):
        assert torch.equal(a, b), f"{n} depends on the layout"
    return out, lse, bo


# variant 0 and every fp32 call: attn_fwd_kernel / attn_delta_kernel / attn_dkdv_kernel /
# attn_dq_kernel, 64-row blocks (`dtype == MMSEQ_BF16 && variant` is false); bf16 variant 1:
# attn_fwd_bf16_kernel (+ attn_fwd_tail) and attn_dq_bf16_kernel / attn_dkdv_bf16_kernel<0, FOLD>;
# bf16 variant 2: attn_fwd32_kernel<0, false> forward, the backward of variant 1
@pytest.mark.parametrize("code", [F32, BF16])
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("T", TS)
def test_attn_fwd_bwd(T, variant, code):
    _attn_roundtrip(AttnCase(T, code), variant)


# T = 144 folds its 16-row tail into the last dK/dV block (keep bits only: dmode 1, the counter
# hash, never folds: `tail_fold(ak, dmode == 1 ? 0 : T)`), T = 145 does not; the forward takes
# attn_fwd_bf16_kernel<2 (bits) / 1, false> (wide is false: the dropout index stays below 2^32)
@pytest.mark.parametrize("code", [F32, BF16])
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("bits", [False, True])
@pytest.mark.parametrize("T", [144, 145])
def test_attn_fwd_bwd_dropout(T, bits, variant, code):
    bits = bits and code == BF16 and variant != 0  # keep bits are the bf16 fast kernels' cache
    _attn_roundtrip(AttnCase(T, code, bits=bits), variant, nat.drop(0.1, 5, 2024))


# mmseq_attn_fwd_rows / _bwd_rows: variant 1 with gridDim from Tq (`(Tq + 127) / 128` blocks); the
# header's contract: rows >= Tq of out (there are none: out holds Tq rows), lse and delta
# untouched, dQ exactly 0 there
@pytest.mark.parametrize("T,Tq", [(17, 1), (65, 33), (129, 128), (144, 17), (145, 144), (257, 129),
                                  (272, 16), (273, 129), (393, 17), (393, 385)])
@pytest.mark.parametrize("p_drop,bits", [(0.0, False), (0.1, True)])
def test_attn_rows(T, Tq, p_drop, bits):
    c = AttnCase(T, BF16, Tq=Tq, bits=bits)
    _, _, bo = _attn_roundtrip(c, 1, nat.drop(p_drop, 5, 2024))
    dq = bo[1].view(P, T, H)[:, Tq:]
    assert not bool((dq.view(torch.int16) & 0x7FFF).any()), "dQ of the rows >= Tq is not zero"


# MX-fp8 outputs: attn_fwd_bf16_kernel<DMODE, false, Q8 = true> (mmseq_attn_fwd_mxfp8 is the dual
# entry with out = NULL, no dropout) and the variant-1 backward with a.q8 set (packed Q|K|V
# offsets are part of that entry point; ld_qkv and ld_dqkv stay loose).
# The header leaves the scale bytes of the rows P*T .. next multiple of 64 to the caller: they lie
# inside the declared scale buffer, so the guard check covers only what is beyond it.
@pytest.mark.parametrize("T", TS)
def test_attn_mxfp8(T):
    po, slices = (0, H, 2 * H), [(0, 3 * H)]
    c = AttnCase(T, BF16, offs=po, slices=slices)
    sb1 = nat.lib().mmseq_mxfp8_scale_bytes(P * T, H)
    sb3 = nat.lib().mmseq_mxfp8_scale_bytes(P * T, 3 * H)
    q8, s8 = G(P * T, H, H + 16, torch.uint8), G(1, sb1, dtype=torch.uint8)
    g8, gs8 = G(P * T, 3 * H, 3 * H + 16, torch.uint8), G(1, sb3, dtype=torch.uint8)

    def fwd(dual):
        def run():
            c.arm(c.out, c.lse, q8, s8)
            if dual:
                raw.attn_fwd_mxfp8_dual(P, T, HEADS, c.qkv.t, LD_QKV, po, c.bias.t, 1 / 8, c.out.t,
                                        LD_OUT, c.lse.t, q8.t, H + 16, s8.t)
            else:
                raw.attn_fwd_mxfp8(P, T, HEADS, c.qkv.t, LD_QKV, po, c.bias.t, 1 / 8, c.lse.t, q8.t,
                                   H + 16, s8.t)
            c.check(lse=c.lse, q8=q8, q8_scales=s8, out=c.out)
            return [c.lse.v2, q8.v2, s8.v2] + ([c.out.v2] if dual else [])
        return poison_check(run, [c.qkv, c.bias], "attn_fwd_mxfp8")

    single = fwd(False)
    assert c.out.ibuf.equal(c.out._snap), "mmseq_attn_fwd_mxfp8 has no bf16 output"
    lse, q, s, out = fwd(True)
    assert torch.equal(single[0], lse) and torch.equal(single[1], q) and torch.equal(single[2], s)
    # the bf16 output is bit-identical to variant 1's (the header's claim), whatever the layout
    ref = torch.zeros(P * T, H, dtype=torch.bfloat16, device=DEV)
    rl = torch.zeros(P, HEADS, T, device=DEV)
    raw.attn_fwd(P, T, HEADS, c.packed_qkv(), 3 * H, po, c.bias.t, 1 / 8, ref, H, rl, BF16, 1)
    assert torch.equal(out, ref) and torch.equal(lse.view(P, HEADS, T), rl)

    c.out_in.set(out)
    c.lse_in.set(lse)

    def bwd(with_q8):
        def run():
            c.arm(c.delta, c.dqkv, g8, gs8)
            args = (c.bias.t, 1 / 8, c.out_in.t, LD_OUT, c.dout.t, LD_DOUT, c.lse_in.t, c.delta.t,
                    c.dqkv.t, LD_DQKV)
            if with_q8:
                raw.attn_bwd_mxfp8(P, T, HEADS, c.qkv.t, LD_QKV, *args, g8.t, 3 * H + 16, gs8.t)
            else:
                raw.attn_bwd(P, T, HEADS, c.qkv.t, LD_QKV, po, *args, BF16, 1)
            c.check(delta=c.delta, dqkv=c.dqkv, q8=g8, q8_scales=gs8)
            return [c.delta.v2, c.dqkv.v2[:, :3 * H], g8.v2]
        return poison_check(run, [c.qkv, c.bias, c.dout, c.out_in, c.lse_in], "attn_bwd_mxfp8")

    a, b = bwd(True), bwd(False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "dqkv differs with the MX-fp8 copy"


# ------------------------------------------------------------------------------------------------
# ld_dqkv: what attn_bwd_impl requires is what the stores need, max offset + heads * 64 <= ld_dqkv
# (16-byte rows on the 128-row path), not ld_dqkv >= ld_qkv
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code,variant", [(F32, 0), (BF16, 0), (BF16, 1)])
def test_attn_bwd_ld_dqkv(code, variant):
    T, po = 145, (0, H, 2 * H)
    # a compact dqkv (ld 3H) next to a wider qkv (ld 3H + 64): accepted, and the packed result
    c = AttnCase(T, code, offs=po, ld_dqkv=3 * H, slices=[(0, 3 * H)])
    _attn_roundtrip(c, variant)
    # too narrow for the K slice's last head: MMSEQ_EINVAL and nothing launched
    c.arm(c.delta, c.dqkv)
    for ld in (3 * H - 8, H, 0):
        st = raw.attn_bwd(P, T, HEADS, c.qkv.t, LD_QKV, po, c.bias.t, 1 / 8, c.out_in.t, LD_OUT,
                          c.dout.t, LD_DOUT, c.lse_in.t, c.delta.t, c.dqkv.t, ld, code, variant,
                          check=False)
        assert st == raw.EINVAL, (ld, st)
    # the loose offsets need 304 + 128 columns
    st = raw.attn_bwd(P, T, HEADS, c.qkv.t, LD_QKV, OFFS, c.bias.t, 1 / 8, c.out_in.t, LD_OUT,
                      c.dout.t, LD_DOUT, c.lse_in.t, c.delta.t, c.dqkv.t, K_OFF + H - 8, code,
                      variant, check=False)
    assert st == raw.EINVAL
    torch.cuda.synchronize()
    for g in (c.delta, c.dqkv):
        assert g.ibuf.equal(g._snap), "a rejected call wrote to its outputs"


# =================================================================================================
# GEMM
# =================================================================================================
GELU = 1


def _ws(M, N, K):
    """A guarded workspace of mmseq_gemm_workspace_size bytes (what any split-K plan may use)."""
    n = max(4, (nat.lib().mmseq_gemm_workspace_size(M, N, K) + 15) // 16 * 4)
    return G(1, n)


def _gemm(trans, M, N, K, batch, A, lda, sA, B, ldb, sB, C, ldc, sC, bias, act, aux, dact, resid,
          ldr, sR, accumulate, in_code, out_code, variant, ws):
    p = raw.p
    raw.call("mmseq_gemm", trans, M, N, K, batch, p(A), lda, sA, p(B), ldb, sB, p(C), ldc, sC,
             p(bias), act, p(aux), p(dact), p(resid), ldr, sR, 1.0, int(accumulate), in_code,
             out_code, None, variant, p(ws), ws.numel() * 4)


def _gemm_case(trans, variant, code, M, N, K, mode, batch=1, out_code=None):
    """One mmseq_gemm call in guarded, gapped buffers (lda, ldb > K or M / N with NaN in the gap,
    ldc > N, ldr != ldc, batch strides that leave rows between the batches) and the same call on
    contiguous tensors, which must give the same bits."""
    out_code = code if out_code is None else out_code
    dt, odt = TDT[code], TDT[out_code]
    gen = torch.Generator().manual_seed(M * 131 + N * 17 + K + variant)
    ar, ac = (K, M) if trans else (M, K)  # A is [K][M] in the TN layout
    br, bc = (K, N) if trans else (N, K)
    lda, ldb = ac + 8, bc + 16
    ldc = (N + 7) // 8 * 8 + 8
    ldr = ldc + 8
    sA, sC, sR = (ar + 3) * lda, (M + 5) * ldc, (M + 2) * ldr
    A = G(ar, ac, lda, dt, batch=batch, bstride=sA).set(_randn(gen, batch, ar, ac).to(dt))
    B = G(br, bc, ldb, dt).set((_randn(gen, br, bc) * 0.1).to(dt))
    C = G(M, N, ldc, odt, batch=batch, bstride=sC)
    C0 = _randn(gen, batch, M, N).to(odt)
    bias = G(1, N).set(_randn(gen, N)) if mode == "aux" else None
    resid = G(M, N, ldr, odt, batch=batch, bstride=sR).set(_randn(gen, batch, M, N).to(odt)) \
        if mode == "aux" else None
    aux = G(M, N, ldc, odt) if mode == "aux" and batch == 1 else None
    dact = G(M, N, ldc, odt).set(_randn(gen, M, N).to(odt)) if mode == "dact" else None
    ws = _ws(M, N, K)
    act = GELU if mode in ("aux", "dact") else 0
    t = lambda g: None if g is None else g.t  # noqa: E731

    def run():
        for g in (C, aux, ws):
            if g is not None:
                g.fill_pattern().snapshot()
        if mode == "acc":
            C.set(C0)
        _gemm(trans, M, N, K, batch, A.t, lda, sA if batch > 1 else 0, B.t, ldb, 0, C.t, ldc,
              sC if batch > 1 else 0, t(bias), act, t(aux), t(dact), t(resid), ldr,
              sR if batch > 1 else 0, mode == "acc", code, out_code, variant, ws.t)
        C.check_untouched("C")
        ws.check_untouched("workspace")
        if aux is not None:
            aux.check_untouched("aux_out")
        return [C.view] + ([aux.view] if aux is not None else [])

    got = poison_check(run, [g for g in (A, B, bias, resid, dact) if g is not None], "gemm")
    # contiguous operands, the same call
    cA, cB = A.view.contiguous(), B.view.contiguous()
    cC = C0.clone() if mode == "acc" else torch.zeros(batch, M, N, dtype=odt, device=DEV)
    c = lambda g: None if g is None else g.view.contiguous()  # noqa: E731
    cws = torch.empty(ws.view.numel(), device=DEV)
    caux = None if aux is None else torch.zeros(M, N, dtype=odt, device=DEV)
    _gemm(trans, M, N, K, batch, cA, ac, ar * ac if batch > 1 else 0, cB, bc, 0, cC, N,
          M * N if batch > 1 else 0, c(bias), act, caux, c(dact), c(resid), N,
          M * N if batch > 1 else 0, mode == "acc", code, out_code, variant, cws)
    assert torch.equal(got[0], cC), "C depends on the leading dimensions"
    if aux is not None:
        assert torch.equal(got[1][0], caux), "aux_out depends on the leading dimensions"


def _edge_shapes(tile, step):
    """(M, N) pairs around a tile: 1, tile - 1, tile + 5, 2 tile + 5 rows against N likewise, in
    the steps the kernel's alignment allows (step 8: N % 8 == 0 for the 256-wide NT kernels and
    M % 8 == N % 8 == 0 for the TN fast kernels)."""
    if step == 1:
        v = (1, tile - 1, tile + 5, 2 * tile + 5)
    else:
        v = (step, tile - step, tile + step, 2 * tile + step)
    return [(v[i], v[j]) for i, j in ((0, 3), (1, 2), (2, 1), (3, 0), (3, 3), (1, 1))]


def _nt_cases():
    cases = []
    for variant in range(7):
        # gemm.hip launch_fast: variants 4, 5, 6 (sel.big == 2) send every NT problem with K % 128
        # == 0, batch 1 and, in mmseq_gemm256_nt, bf16 out, N % 8 == 0, ldc % 8 == 0 to the 256 x 256
        # / 256 x 128 / ping-pong kernels; K = 128 is the smallest K they take. Variants 1 (auto:
        # fewer than 256 tiles of 256^2 here), 2 and 3 run the 128 x 128 double-buffer / ring kernels
        # when fast_ok (bf16, 16-byte rows, K % 64 == 0, M * N >= 128 * 128: K = 64), the
        # register-staged 128 x 128 kernel otherwise (M = 1 and the 127-row shapes). Variant 0
        # (disable_fast) is that generic kernel, here with a K that is no multiple of its BK = 64.
        big = variant >= 4
        K = 128 if big else (40 if variant == 0 else 64)
        for M, N in _edge_shapes(256 if big else 128, 8 if big else 1):
            if big:
                M = {8: 1, 248: 255, 264: 261, 520: 517}[M]  # rows need no alignment
            for mode in ("aux", "dact", "acc"):
                cases.append((variant, BF16, M, N, K, mode))
    # fp32 never takes a fast kernel (fast_ok wants bf16): variant only has to be valid. K = 20 is
    # no multiple of the fp32 BK = 32; K = 264 >= 256 with a workspace and < 128 tiles splits K
    # (plan_f32) and finishes in splitk_epi_kernel
    for variant, K in ((0, 20), (1, 264)):
        for M, N in _edge_shapes(128, 1):
            for mode in ("aux", "dact", "acc"):
                cases.append((variant, F32, M, N, K, mode))
    return cases


@pytest.mark.parametrize("variant,code,M,N,K,mode", _nt_cases())
def test_gemm_nt(variant, code, M, N, K, mode):
    _gemm_case(0, variant, code, M, N, K, mode)


def _tn_cases():
    cases = []
    for variant in range(7):
        # TN fast kernels want M % 8 == N % 8 == 0 and M * N >= 128 * 128, any K (72: no multiple of
        # BK). "acc" (fp32 out, no epilogue: `plain`) is the weight gradient: variants 1, 4, 5, 6
        # (sel.big) take gemm256_tn_kernel with the K split planned for the workspace, 2 and 3 the
        # 128 x 128 kernels (plan_tn128 split-K), 0 the generic kernel. "aux" (bf16 out, bias +
        # GELU + aux + residual) is never `plain`: 128 x 128 TN for 1-6.
        for M, N in _edge_shapes(256 if variant >= 4 or variant == 1 else 128, 8):
            cases.append((variant, BF16, M, N, 40 if variant == 0 else 72, "acc", F32))
            cases.append((variant, BF16, M, N, 40 if variant == 0 else 72, "aux", BF16))
    for variant, K in ((0, 20), (1, 264)):  # fp32: the generic kernel / plan_f32 split-K
        for M, N in _edge_shapes(128, 1):
            cases.append((variant, F32, M, N, K, "acc", F32))
            cases.append((variant, F32, M, N, K, "aux", F32))
    return cases


@pytest.mark.parametrize("variant,code,M,N,K,mode,out_code", _tn_cases())
def test_gemm_tn(variant, code, M, N, K, mode, out_code):
    _gemm_case(1, variant, code, M, N, K, mode, out_code=out_code)


# batch = 3 with rows between the batches of A, C and the residual. launch_fast keeps batched
# problems off the 256 x 256 kernel (`batch == 1`), so 1 and 4 run the 128 x 128 double-buffer
# kernel with blockIdx.y = batch, 3 the ring, 0 the generic kernel
@pytest.mark.parametrize("code", [F32, BF16])
@pytest.mark.parametrize("variant", [0, 1, 3, 4])
@pytest.mark.parametrize("mode", ["aux", "acc"])
def test_gemm_nt_batched(variant, code, mode):
    _gemm_case(0, variant, code, 133, 136, 64, mode, batch=3)


# mmseq_gemm_wgrad: bf16 with sel.big (variant 1) and M % 8 == N % 8 == 0 takes wgrad_tn256 (bias
# sums inside the TN kernel, split-K slab + bias partial rows in the workspace, one reduction
# launch); M = 133 fails mmseq_gemm256_tn's M % 8 and variant 2 has no sel.big: both fall back to
# mmseq_gemm TN + colsum_simple_kernel; fp32 always does. K = 2100 is long enough to split.
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("variant,code,M,N,K", [(1, BF16, 264, 136, 2100), (1, BF16, 8, 520, 77),
                                                (1, BF16, 133, 96, 50), (2, BF16, 264, 136, 2100),
                                                (1, F32, 40, 96, 300), (0, F32, 131, 5, 20)])
def test_gemm_wgrad(variant, code, M, N, K, with_bias):
    dt = TDT[code]
    gen = torch.Generator().manual_seed(M + N + K)
    lda, ldb, ldc = M + 8, N + 8, (N + 3) // 4 * 4 + 4
    A = G(K, M, lda, dt).set(_randn(gen, K, M).to(dt))
    B = G(K, N, ldb, dt).set(_randn(gen, K, N).to(dt))
    C, C0 = G(M, N, ldc), _randn(gen, M, N)
    gb, gb0 = (G(1, M), _randn(gen, M)) if with_bias else (None, None)
    ws = _ws(M, N, K)

    def call(a, la, b, lb, c, lc, g, w):
        raw.call("mmseq_gemm_wgrad", M, N, K, raw.p(a), la, raw.p(b), lb, raw.p(c), lc, raw.p(g),
                 code, variant, raw.p(w), w.numel() * 4)

    def run():
        for g in (C, gb, ws):
            if g is not None:
                g.fill_pattern().snapshot()
        C.set(C0)
        if gb is not None:
            gb.set(gb0)
        call(A.t, lda, B.t, ldb, C.t, ldc, None if gb is None else gb.t, ws.t)
        C.check_untouched("C")
        ws.check_untouched("workspace")
        if gb is not None:
            gb.check_untouched("bias_grad")
        return [C.view] + ([gb.view] if gb is not None else [])

    got = poison_check(run, [A, B], "gemm_wgrad")
    cC, cg = C0.clone(), None if gb is None else gb0.clone()
    call(A.view.contiguous(), M, B.view.contiguous(), N, cC, N, cg,
         torch.empty(ws.view.numel(), device=DEV))
    assert torch.equal(got[0][0], cC), "C depends on the leading dimensions"
    if gb is not None:
        assert torch.equal(got[1].flatten(), cg), "bias_grad depends on the leading dimensions"


# =================================================================================================
# two-level mmseq_rows layouts: LayerNorm, row gather
# =================================================================================================
class Rows2:
    """`n` rows of `cols` in a two-level mmseq_rows layout, as the halves of the joint [P][T][H]
    buffer are addressed: rpb rows per batch, ld > cols, bstride > rpb * ld, the last batch ragged
    when rpb does not divide n (its unused rows are padding like the gap columns). rpb = None: one
    level, row r at r * ld ("dense rows")."""

    def __init__(self, n, cols, dtype, rpb, gap=8, pad_rows=2):
        self.n, self.cols = n, cols
        ld = cols + gap
        if rpb is None:
            self.g = G(n, cols, ld, dtype)
            self.layout = nat.rows(ld)
        else:
            nb = -(-n // rpb)
            bs = (rpb + pad_rows) * ld
            self.g = G(rpb, cols, ld, dtype, batch=nb, bstride=bs)
            if nb * rpb > n:
                self.g._strided(self.g.inside)[nb - 1, n - (nb - 1) * rpb:] = False
            self.layout = nat.rows(ld, bs, rpb)
        self.t = self.g.t

    def put(self, data):
        full = torch.zeros(self.g.batch * self.g.rows, self.cols, dtype=self.g.dtype, device=DEV)
        full[:self.n] = data
        self.g.set(full)
        return self

    def get(self):
        return self.g.view.reshape(-1, self.cols)[:self.n]


def _arm(*gs):
    for g in gs:
        if g is not None:
            (g.g if isinstance(g, Rows2) else g).fill_pattern().snapshot()


def _untouched(**gs):
    for name, g in gs.items():
        if g is not None:
            (g.g if isinstance(g, Rows2) else g).check_untouched(name)


def _gs(*xs):
    return [x.g if isinstance(x, Rows2) else x for x in xs if x is not None]


# bf16 with cols % 256 == 0, cols <= 1024 and 16-byte rows (cols = 768): ln_fwd16_kernel<3> and
# ln_bwd16_kernel<3, ...>, for "bwd_ex" the <3, false, true, false, true> form with the column sums
# in the kernel (`cs`: dsum, no input dropout, cols <= 768). cols = 96 and every fp32 call:
# ln_fwd_kernel / ln_bwd_kernel<T, vec = true, 4>, the column sums by mmseq_colsum afterwards.
# rows 1, 7 (three batches of rpb = 3, the last ragged) and 300 (four of 77: more than one block).
@pytest.mark.parametrize("code", [F32, BF16])
@pytest.mark.parametrize("cols", [96, 768])
@pytest.mark.parametrize("rows", [1, 7, 300])
@pytest.mark.parametrize("entry", ["bwd", "bwd_rows", "bwd_ex"])
def test_layernorm(entry, rows, cols, code):
    dt = TDT[code]
    rpb = 77 if rows == 300 else 3
    gen = torch.Generator().manual_seed(rows + cols)
    x = Rows2(rows, cols, dt, rpb).put(_randn(gen, rows, cols).to(dt))
    y = Rows2(rows, cols, dt, rpb, gap=16, pad_rows=1)
    gamma = G(1, cols).set(1 + 0.1 * _randn(gen, cols))
    beta = G(1, cols).set(0.1 * _randn(gen, cols))
    mean, rstd = G(1, rows), G(1, rows)
    eps = 1e-5

    def fwd(xt, xl, yt, yl, mt, rt):
        raw.call("mmseq_layernorm_fwd", rows, cols, raw.p(xt), xl, raw.p(gamma.t), raw.p(beta.t),
                 eps, raw.p(yt), yl, raw.p(mt), raw.p(rt), code, code, None)

    def run_fwd():
        _arm(y, mean, rstd)
        fwd(x.t, x.layout, y.t, y.layout, mean.t, rstd.t)
        _untouched(y=y, mean=mean, rstd=rstd)
        return [y.get(), mean.view, rstd.view]

    yv, mv, rv = poison_check(run_fwd, _gs(x, gamma, beta), "layernorm_fwd")
    cy = torch.zeros(rows, cols, dtype=dt, device=DEV)
    cm, cr = torch.zeros(rows, device=DEV), torch.zeros(rows, device=DEV)
    fwd(x.get().contiguous(), nat.rows(cols), cy, nat.rows(cols), cm, cr)
    assert torch.equal(yv, cy) and torch.equal(mv.flatten(), cm) and torch.equal(rv.flatten(), cr)

    # backward: dy, x, dres each in a layout of its own; dx_drop in dx's layout (bwd), in a
    # two-level layout of its own (bwd_rows) or in dense rows with ld > cols (bwd_ex: dsum needs
    # the summed gradient in dense rows)
    dy = Rows2(rows, cols, dt, rpb, gap=24).put(_randn(gen, rows, cols).to(dt))
    dres = Rows2(rows, cols, dt, rpb, gap=8, pad_rows=1).put(_randn(gen, rows, cols).to(dt))
    mean_in, rstd_in = G(1, rows).set(mv), G(1, rows).set(rv)
    dx = Rows2(rows, cols, dt, rpb, gap=16)
    dxd = {"bwd": Rows2(rows, cols, dt, rpb, gap=16),
           "bwd_rows": Rows2(rows, cols, dt, 5, gap=8, pad_rows=3),
           "bwd_ex": Rows2(rows, cols, dt, None, gap=8)}[entry]
    dg, db = G(1, cols), G(1, cols)
    dsum = G(1, cols) if entry == "bwd_ex" else None
    acc0 = _randn(gen, 3, cols)
    ws = G(1, max(4, nat.lib().mmseq_layernorm_bwd_workspace(rows, cols)))
    drop_dx = nat.drop(0.1, 22, 5)

    def bwd(dyt, dyl, xt, xl, mt, rt, dxt, dxl, drt, drl, dgt, dbt, wst, dxdt, dxdl, dst):
        head = (rows, cols, raw.p(dyt), dyl, raw.p(xt), xl, raw.p(mt), raw.p(rt), raw.p(gamma.t),
                raw.p(dxt), dxl, raw.p(drt), drl, raw.p(dgt), raw.p(dbt), raw.p(wst), code, None,
                raw.p(dxdt))
        if entry == "bwd":
            raw.call("mmseq_layernorm_bwd", *head, raw.d(drop_dx))
        elif entry == "bwd_rows":
            raw.call("mmseq_layernorm_bwd_rows", *head, dxdl, raw.d(drop_dx))
        else:
            raw.call("mmseq_layernorm_bwd_ex", *head, dxdl, raw.d(drop_dx), raw.p(dst))

    def run_bwd():
        _arm(dx, dxd, dg, db, dsum, ws)
        dg.set(acc0[0])  # dgamma, dbeta and dsum accumulate
        db.set(acc0[1])
        if dsum is not None:
            dsum.set(acc0[2])
        bwd(dy.t, dy.layout, x.t, x.layout, mean_in.t, rstd_in.t, dx.t, dx.layout, dres.t,
            dres.layout, dg.t, db.t, ws.t, dxd.t, dxd.layout, None if dsum is None else dsum.t)
        _untouched(dx=dx, dx_drop=dxd, dgamma=dg, dbeta=db, dsum=dsum, workspace=ws)
        return [dx.get(), dxd.get(), dg.view, db.view] + ([dsum.view] if dsum is not None else [])

    got = poison_check(run_bwd, _gs(dy, x, dres, mean_in, rstd_in, gamma), "layernorm_" + entry)
    one = nat.rows(cols)
    cdx, cdxd = (torch.zeros(rows, cols, dtype=dt, device=DEV) for _ in range(2))
    cg, cb, cs = (a.clone() for a in acc0)
    bwd(dy.get().contiguous(), one, x.get().contiguous(), one, cm, cr, cdx, one,
        dres.get().contiguous(), one, cg, cb, torch.empty(ws.view.numel(), device=DEV), cdxd, one,
        cs if dsum is not None else None)
    assert torch.equal(got[0], cdx) and torch.equal(got[1], cdxd), "dx depends on the layout"
    assert torch.equal(got[2].flatten(), cg) and torch.equal(got[3].flatten(), cb)
    if dsum is not None:
        assert torch.equal(got[4].flatten(), cs), "dsum depends on the layout"


# rows_gather_kernel / rows_zero_kernel + rows_scatter_kernel: 16-byte chunks, cols % 8 == 0 (one
# kernel for every shape and dtype; 96 columns are 12 / 24 chunks a row, 768 more than a block's
# 256 threads per two rows). A permutation with a mask, and a compaction of a two-level source.
@pytest.mark.parametrize("code", [F32, BF16])
@pytest.mark.parametrize("R_out,R_in,cols", [(7, 7, 96), (5, 23, 768), (300, 300, 96)])
def test_rows_gather(R_out, R_in, cols, code):
    dt = TDT[code]
    gen = torch.Generator().manual_seed(R_out + cols)
    xin = Rows2(R_in, cols, dt, 5 if R_in < 100 else 77).put(_randn(gen, R_in, cols).to(dt))
    out = Rows2(R_out, cols, dt, None, gap=16)
    src = torch.randperm(R_in, generator=gen)[:R_out].to(DEV, torch.int32)
    keep = (torch.rand(R_out, generator=gen) > 0.3).to(DEV, torch.uint8)

    def run_fwd():
        _arm(out)
        raw.call("mmseq_rows_gather_fwd", R_out, R_in, cols, raw.p(xin.t), xin.layout, raw.p(src),
                 raw.p(keep), raw.p(out.t), out.layout, code)
        _untouched(out=out)
        return [out.get()]

    (o,) = poison_check(run_fwd, _gs(xin), "rows_gather_fwd")
    want = xin.get()[src.long()] * keep[:, None].to(dt)
    assert torch.equal(o, want)

    dout = Rows2(R_out, cols, dt, None, gap=24).put(_randn(gen, R_out, cols).to(dt))
    din = Rows2(R_in, cols, dt, 5 if R_in < 100 else 77, gap=16, pad_rows=1)

    def run_bwd():
        _arm(din)
        raw.call("mmseq_rows_gather_bwd", R_out, R_in, cols, raw.p(dout.t), dout.layout, raw.p(src),
                 raw.p(keep), raw.p(din.t), din.layout, code)
        _untouched(din=din)
        return [din.get()]

    (d,) = poison_check(run_bwd, _gs(dout), "rows_gather_bwd")
    want = torch.zeros(R_in, cols, dtype=dt, device=DEV)
    want[src.long()] = dout.get() * keep[:, None].to(dt)
    assert torch.equal(d, want)


# =================================================================================================
# cross-entropy: logits [M][ld] with V < ld
# =================================================================================================
# xent_fwd_kernel: one workgroup per row over whole 16-byte chunks, the tail chunk masked;
# xent_bwd_kernel: grid.y = ceil(ld / 8192) column segments (BWD_SEG), so ld = 8208 runs a second,
# ragged segment. The header's own promise: columns >= V hold anything on entry (NaN here) and the
# backward overwrites them with exact zeros, so for the backward's output check they are declared
# columns and only the guard rows must stay untouched.
@pytest.mark.parametrize("code", [F32, BF16])
@pytest.mark.parametrize("M,V,ld", [(5, 100, 104), (3, 8195, 8208), (1, 7, 64)])
def test_xent(M, V, ld, code):
    dt = TDT[code]
    gen = torch.Generator().manual_seed(M + V)
    data = _randn(gen, M, V).to(dt)
    labels = torch.randint(0, V, (M,), generator=gen).to(DEV)
    if M > 1:
        labels[1] = -100
    logits = G(M, V, ld, dt).set(data)
    lse, loss_row, stats = G(1, M), G(1, M), G(1, 2)

    def run_fwd():
        _arm(lse, loss_row, stats)
        raw.call("mmseq_xent_fwd", M, V, raw.p(logits.t), ld, raw.p(labels), -100, raw.p(lse.t),
                 raw.p(loss_row.t), raw.p(stats.t), code)
        _untouched(lse=lse, loss_row=loss_row, stats=stats)
        return [lse.view, loss_row.view, stats.view]

    lv, _, sv = poison_check(run_fwd, [logits], "xent_fwd")
    torch.testing.assert_close(lv.flatten().double(), torch.logsumexp(data.double(), -1),
                               rtol=1e-4, atol=1e-4)

    lse_in, stats_in = G(1, M).set(lv), G(1, 2).set(sv)
    io = G(M, ld, ld, dt)  # in / out: all ld columns are the backward's to write
    outs = []
    for fill in (0.0, float("nan")):
        io.fill_pattern()
        io.buf[~io.inside] = fill
        io.v2[:, :V] = data
        io.v2[:, V:] = fill
        lse_in.fill_outside(fill)
        stats_in.fill_outside(fill)
        io.snapshot()
        raw.call("mmseq_xent_bwd", M, V, raw.p(io.t), ld, raw.p(labels), -100, raw.p(lse_in.t),
                 raw.p(stats_in.t), None, code)
        io.check_untouched("dlogits")
        outs.append(io.v2.clone())
    assert bool(torch.isfinite(outs[1].float()).all()) and torch.equal(outs[0], outs[1])
    assert not bool(outs[1][:, V:].float().abs().any()), "columns >= V must be exact zeros"
    if M > 1:
        assert not bool(outs[1][1].float().abs().any()), "an ignored row must be exact zeros"
