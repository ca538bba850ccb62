"""The bf16 fast attention kernels (variant 1 and 2 forward, the 128-row backward, and the _rows /
_mxfp8_dual forwards where they claim bit-identity with variant 1) against a float64 reference,
per (token, head) row: the kernel's relative L2 row error must stay within FACTOR x the error of a
float64 emulation that rounds to bf16 at the kernels' sites (tests/attn_accuracy.py lists them).
The emulation's error is computed here, on the same inputs, never taken from the kernel.

Also: lse against float64 logsumexp (1e-3, as test_attention_rescale_and_zero_bias_tiles), and
delta against the float64 row sum of dO * O, O being the kernel's own stored bf16 output, to fp32
accumulation error (1e-5 x sum |terms|).

Each case prints its kernel / emulation ratios before it asserts (DESIGN.md holds the table).
"""
import functools

import pytest
import torch

import attn_accuracy as acc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import native_raw as raw
    from multimodal_sequencing_amd import _native as nat

DEV = "cuda"
P, HEADS = 2, 2
H = HEADS * 64
BF16 = 1
TS = (17, 65, 129, 145, 265, 273, 393)
PATTERNS = ("none", "random30", "first_tile", "last_tile", "one_key")
# a bias that masks every key is left out: first_tile / last_tile need a second key tile
CASES = [(T, b) for T in TS for b in PATTERNS if T > 64 or b not in ("first_tile", "last_tile")]
PACKED = (3 * H, (0, H, 2 * H), H, H, 3 * H)
# ld_qkv = 3H + 64 with the slices in the order V | Q | K at offsets that are no multiples of H,
# ld_out = H + 8, ld_dout != ld_out, ld_dqkv != ld_qkv (test_guard_bands_gpu's layout)
LOOSE = (3 * H + 64, (152, 304, 8), H + 8, H + 16, 3 * H + 56)


@functools.lru_cache(maxsize=4)
def _problem(T, pattern, p_drop, scale):
    gen = torch.Generator().manual_seed(1000 * T + len(pattern))
    q, k, v, dout = (t.to(DEV) for t in acc.make_inputs(P, T, HEADS, gen))
    bias = acc.key_bias(pattern, P, T, gen)
    bias = None if bias is None else bias.to(DEV)
    keep, drop = None, None
    if p_drop:
        from test_dropout_gpu import _mask
        drop = nat.drop(p_drop, 5, 2024)
        Tp4 = (T + 3) & ~3  # the kernels' dropout row stride (hash quads)
        keep = _mask((P, HEADS, T, Tp4), drop)[..., :T].double()
    args = (q.double(), k.double(), v.double(), bias, scale, keep, dout.double())
    return q, k, v, dout, bias, drop, acc.reference(*args), acc.emulate(*args)


def _rows(x, ld, off=0):
    """[P][heads][T][64] -> [P*T][ld] bf16 rows with the heads at column off."""
    T = x.shape[2]
    buf = torch.zeros(P * T, ld, dtype=torch.bfloat16, device=DEV)
    buf[:, off:off + H] = x.permute(0, 2, 1, 3).reshape(P * T, H)
    return buf


def _report(tag, res):
    print(f"ACC {tag} " + " ".join(
        f"{n}: kernel {k:.3e} emu {e:.3e} ratio {k / e if e else float('nan'):.2f}"
        for n, (k, e) in res.items()))


def _run(T, pattern, variant, p_drop=0.0, bits=False, layout=PACKED, scale=1 / 8, backward=True):
    q, k, v, dout, bias, drop, ref, emu = _problem(T, pattern, p_drop, scale)
    ld_qkv, offs, ld_out, ld_dout, ld_dqkv = layout
    qkv = torch.zeros(P * T, ld_qkv, dtype=torch.bfloat16, device=DEV)
    for x, off in zip((q, k, v), offs):
        qkv[:, off:off + H] = x.permute(0, 2, 1, 3).reshape(P * T, H)
    out = torch.zeros(P * T, ld_out, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(P, HEADS, T, device=DEV)
    kb = nat.attn_keep_bits(P, T, HEADS, DEV) if bits else None
    raw.attn_fwd(P, T, HEADS, qkv, ld_qkv, offs, bias, scale, out, ld_out, lse, BF16, variant,
                 drop, kb)
    tag = f"T={T} bias={pattern} variant={variant} p={p_drop} bits={int(bits)} ld_qkv={ld_qkv} scale={scale:g}"
    got = {"out": acc.rows_to_heads(out, P, T, HEADS)}
    res, bad = acc.measure(got, ref, emu, ("out",))
    lse_err = (lse.double() - ref["lse"]).abs().max().item()
    print(f"ACC {tag} lse max err {lse_err:.3e}")
    if backward:
        do = _rows(dout, ld_dout)
        dqkv = torch.zeros(P * T, ld_dqkv, dtype=torch.bfloat16, device=DEV)
        delta = torch.empty(P, HEADS, T, device=DEV)
        raw.attn_bwd(P, T, HEADS, qkv, ld_qkv, offs, bias, scale, out, ld_out, do, ld_dout, lse,
                     delta, dqkv, ld_dqkv, BF16, variant, drop, kb)
        for n, off in zip(("dq", "dk", "dv"), offs):
            got[n] = acc.rows_to_heads(dqkv[:, off:], P, T, HEADS)
        r2, b2 = acc.measure(got, ref, emu, ("dq", "dk", "dv"))
        res.update(r2)
        bad += b2
        terms = dout.double() * got["out"]  # O as the backward read it: the stored bf16 output
        d_err = (delta.double() - terms.sum(-1)).abs()
        d_allow = acc.FP32_ACC * terms.abs().sum(-1)
        print(f"ACC {tag} delta max err / allowance {(d_err / (d_allow + 1e-300)).max().item():.3f}")
    _report(tag, res)
    assert not bad, "; ".join(bad)
    torch.testing.assert_close(lse.double(), ref["lse"], rtol=1e-3, atol=1e-3)
    if backward:
        assert bool((d_err <= d_allow).all()), "delta is not the fp32 row sum of dO * stored O"
    return qkv, out, lse


@pytest.mark.parametrize("T,pattern", CASES)
def test_variant1_fwd_bwd_rows(T, pattern):
    """attn_fwd_bf16_kernel, with attn_fwd_tail for the last query block when T % 128 is 1 .. 16
    (T = 129, 265, 393; 145 and 273 leave 17 rows, just past it), then attn_dq_bf16_kernel and
    attn_dkdv_bf16_kernel (<0, true>, the tail fold, at the same three T)."""
    qkv, out, lse = _run(T, pattern, 1)
    # bit-identity claims of the header: _rows on its rows < Tq, _mxfp8_dual's bf16 output
    _, _, _, _, bias, _, _, _ = _problem(T, pattern, 0.0, 1 / 8)
    Tq = (T + 1) // 2
    out_r = torch.zeros(P * Tq, H, dtype=torch.bfloat16, device=DEV)
    lse_r = torch.zeros(P, HEADS, T, device=DEV)
    raw.attn_fwd_rows(P, T, Tq, HEADS, qkv, 3 * H, (0, H, 2 * H), bias, 1 / 8, out_r, H, lse_r)
    assert torch.equal(out_r.view(P, Tq, H), out.view(P, T, H)[:, :Tq])
    assert torch.equal(lse_r[..., :Tq], lse[..., :Tq])
    out_d = torch.zeros_like(out)
    lse_d = torch.zeros_like(lse)
    q8 = torch.zeros(P * T, H, dtype=torch.uint8, device=DEV)
    q8s = torch.zeros(nat.lib().mmseq_mxfp8_scale_bytes(P * T, H), dtype=torch.uint8, device=DEV)
    raw.attn_fwd_mxfp8_dual(P, T, HEADS, qkv, 3 * H, (0, H, 2 * H), bias, 1 / 8, out_d, H, lse_d,
                            q8, H, q8s)
    assert torch.equal(out_d, out) and torch.equal(lse_d, lse)


@pytest.mark.parametrize("T,pattern", CASES)
def test_variant2_fwd(T, pattern):
    """attn_fwd32_kernel, the 32x32x16-MFMA forward (the backward of a nonzero variant is variant
    1's, checked above)."""
    _run(T, pattern, 2, backward=False)


@pytest.mark.parametrize("bits", [False, True])
@pytest.mark.parametrize("variant", [1, 2])
def test_dropout(variant, bits):
    """p = 0.1 with the counter-based mask materialised by test_dropout_gpu's helper; keep bits off
    (the backward hashes again, no tail fold) and on (it reads the forward's bits, tail fold)."""
    _run(393, "random30", variant, p_drop=0.1, bits=bits)


@pytest.mark.parametrize("variant", [1, 2])
def test_loose_layout(variant):
    _run(145, "random30", variant, layout=LOOSE)


@pytest.mark.parametrize("variant", [1, 2])
def test_other_scale(variant):
    _run(129, "random30", variant, scale=0.2)
