"""csrc/embed.hip at its chunk, block and width edges, against the float64 references of
tests/embed_ref.py:

  table gradient   run layouts that put every (began, ends) case of seg_rows_kernel into a full and
                   into a partial 64-position chunk, the padding run across chunks, joins of 1, 2
                   and 3 pieces (tests/test_embed_ref.py proves the coverage on the CPU); ids up to
                   69999; a Zipf-like case ragged in every block size at once. Tables ACCUMULATE
                   into noise: untouched rows keep their bits, two calls agree bit for bit, and the
                   workspace (exactly *_workspace() floats between guards) may hold NaN
  embed_ln         ragged 4-row / 64-row blocks, H = 4 .. 1024 with half-empty 64-column trips,
                   Lt = 1, tt / dtype_tab = NULL, P = 0, the rejected calls; the joint buffer with
                   its visual rows and guard bands
  vit_embed        the four half-wave bf16 widths, the generic kernel as their fallback, fp32;
                   gg = 1, where every position index is an edge; dpos row by row
  vit_im2col       the bf16 fast path, bit for bit

Tolerances: those of the same kernel's test in test_kernels_gpu.py (`_close` with its scale
factors; rtol / atol of test_embed_table_grad_fixed_order for the tables), unless the same formula
in fp32 PyTorch on the CPU misses float64 by more at that shape; then 4 x that miss (`FP32_MISS`,
measured with `cpu_fp32_miss()` of this file).
"""
import pytest
import torch

import embed_ref as R
from guard_util import Guarded, poison_check
from test_head_limits_gpu import _ws_runs

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import native_raw as raw
    from multimodal_sequencing_amd import _native as nat

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
CODE = {F32: 0, BF16: 1}
NAME = {F32: "f32", BF16: "bf16"}
TV = 3  # visual rows of a pair in the joint buffer: ld_pair = (Lt + TV) * H

TOL = {F32: 2e-5, BF16: 2e-2}                   # test_kernels_gpu.TOL (rtol = atol)
GRAD = {F32: 2e-5 * 10, BF16: 2e-5 * 300}       # the fp32 gradients: scale 10 / 300
TAB = {F32: (1e-5, 1e-4), BF16: (2e-2, 5e-2)}   # rtol, atol of the tables

# (case..., output) -> max |fp32 PyTorch on the CPU - float64| where that exceeds the existing
# tolerance; the test then allows 4 x this. Everything not listed keeps the existing figures.
FP32_MISS = {
    # two type rows of ~850 terms of sigma ~5 each: elements that cancel to near 0 keep only
    # atol = 1e-4, while the fp32 sum carries the rounding of its ~100-sized partial sums
    ("zipf", "f32", "dtyp"): 4.35e-4,
}


def _norm_close(got, want, tol, key):
    """test_kernels_gpu._close: max |err| <= tol (1 + max |ref|)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, f"{key}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    assert bool(torch.isfinite(got).all()), f"{key}: non-finite output"
    err = float((got - want).abs().max()) if got.numel() else 0.0
    lim = 4 * FP32_MISS[key] if key in FP32_MISS else tol * (1 + float(want.abs().max()) + 1e-6)
    print(f"{key}: max |err| {err:.3g} (limit {lim:.3g})")
    assert err <= lim, f"{key}: max |err| {err:.3g} > {lim:.3g}"


def _elem_close(got, want, rtol, atol, key):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, f"{key}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    assert bool(torch.isfinite(got).all()), f"{key}: non-finite output"
    err = (got - want).abs()
    lim = torch.full_like(want, 4 * FP32_MISS[key]) if key in FP32_MISS else atol + rtol * want.abs()
    over = err - lim
    i = int(over.argmax())
    print(f"{key}: max |err| {float(err.max()):.3g}")
    assert float(over.max()) <= 0, (f"{key}: |err| {float(err.flatten()[i]):.3g} at flat index {i} "
                                    f"(ref {float(want.flatten()[i]):.6g})")


def _bits_equal(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


def _dev(d):
    return {k: v.to(DEV) if torch.is_tensor(v) else v for k, v in d.items()}


# =================================================================================================
# text embedding: calls
# =================================================================================================
GRADS = ("dword", "dpos", "dtyp", "dgamma", "dbeta")


def embed_fills(d, seed):
    g = R.gen(seed, 9)
    src = dict(dword="word", dpos="pos", dtyp="typ", dgamma="gamma", dbeta="beta")
    return {k: torch.randn(d[s].shape, generator=g) for k, s in src.items()}


def embed_fwd_args(v, joint, ld, mean, rstd, act, H=None, P=None):
    P, Lt = v["ids"].shape[0] if P is None else P, v["ids"].shape[1]
    p = raw.p
    return (P, Lt, H or v["word"].shape[1], p(v["ids"]), p(v["tt"]), p(v["word"]), p(v["pos"]),
            p(v["typ"]), p(v["gamma"]), p(v["beta"]), v["eps"], p(joint), ld, p(mean), p(rstd),
            CODE[act], None)


def embed_bwd_args(v, mean, rstd, dj, ld, out, ws, act, H=None, P=None):
    P, Lt = v["ids"].shape[0] if P is None else P, v["ids"].shape[1]
    p = raw.p
    return (P, Lt, H or v["word"].shape[1], p(v["ids"]), p(v["tt"]), p(v["word"]), p(v["pos"]),
            p(v["typ"]), p(v["gamma"]), p(mean), p(rstd), p(dj), ld, p(out["dword"]), p(out["dpos"]),
            p(out.get("dtyp")), p(out["dgamma"]), p(out["dbeta"]), p(ws), CODE[act], None)


def embed_ws(v):
    P, Lt = v["ids"].shape
    return nat.lib().mmseq_embed_ln_bwd_workspace(P, Lt, v["word"].shape[1])


def embed_forward(v, act):
    """Forward into a joint buffer with TV visual rows per pair between guard bands: the visual
    rows and the guards keep their bits. Returns y [P][Lt][H], mean, rstd."""
    P, Lt = v["ids"].shape
    H = v["word"].shape[1]
    joint = Guarded(P, Lt * H, ld=(Lt + TV) * H, dtype=act, device=DEV).fill_pattern().snapshot()
    mean = torch.full((P * Lt,), float("nan"), device=DEV)
    rstd = torch.full((P * Lt,), float("nan"), device=DEV)
    raw.call("mmseq_embed_ln_fwd", *embed_fwd_args(v, joint.t, joint.ld, mean, rstd, act))
    torch.cuda.synchronize()
    joint.check_untouched("embed_ln_fwd joint")
    return joint.v2.reshape(P, Lt, H).clone(), mean, rstd


def embed_backward(v, mean, rstd, djg, fills, ws, act, with_dtyp=True):
    out = {k: f.clone().to(DEV) for k, f in fills.items() if with_dtyp or k != "dtyp"}
    raw.call("mmseq_embed_ln_bwd", *embed_bwd_args(v, mean, rstd, djg.t, djg.ld, out, ws, act))
    torch.cuda.synchronize()
    return out


def check_table(got, fill, ref, ids, act, key):
    """fill + reference; the padding row and the rows of ids no row has keep the fill's bits."""
    _elem_close(got, fill.double() + ref, *TAB[act], key)
    idle = torch.ones(fill.shape[0], dtype=torch.bool)
    idle[torch.unique(ids.cpu())] = False
    idle[0] = True
    assert _bits_equal(got.cpu()[idle], fill[idle]), f"{key}: a row that no id names was written"
    assert bool(((got.cpu() != fill).any(-1) == ~idle).all()), f"{key}: an occurring row kept its fill"


# =================================================================================================
# table gradient layouts
# =================================================================================================
def table_run(d, act, key):
    """Forward, then the backward twice over a guarded workspace of exactly the advertised size,
    zero- and NaN-filled: bit-equal tables; fill + reference."""
    ref = R.embed_ln_ref(d, act=act)
    fills = embed_fills(d, 1)
    v = _dev(d)
    P, Lt = d["ids"].shape
    H = d["word"].shape[1]
    _, mean, rstd = embed_forward(v, act)
    djg = Guarded(P, Lt * H, ld=(Lt + TV) * H, dtype=act, device=DEV).set(v["dj"].to(act))

    def run(ws):
        out = embed_backward(v, mean, rstd, djg, fills, ws, act)
        return [out[k] for k in GRADS]

    outs = dict(zip(GRADS, _ws_runs(embed_ws(v), run)))
    check_table(outs["dword"], fills["dword"], ref["dword"], d["ids"], act, key + ("dword",))
    check_table(outs["dtyp"], fills["dtyp"], ref["dtyp"], d["tt"], act, key + ("dtyp",))
    for k in ("dpos", "dgamma", "dbeta"):
        _norm_close(outs[k], fills[k].double() + ref[k], GRAD[act], key + (k,))
    assert _bits_equal(outs["dpos"][0], fills["dpos"][0])
    return ref


LAYOUT_RUNS = [(n, r, 8) for n in R.LAYOUTS for r in ("word", "type")] + \
              [(n, r, 768) for n in ("c", "e") for r in ("word", "type")]


@pytest.mark.parametrize("name,role,H", LAYOUT_RUNS)
def test_table_grad_layout(name, role, H):
    d = R.layout_case(name, role, H)
    ref = table_run(d, F32, ("layout", name, role, H))
    table, ids = (ref["dword"], d["ids"]) if role == "word" else (ref["dtyp"], d["tt"])
    assert R.row_margin(table, ids, *TAB[F32]) > 100  # a dropped or doubled piece cannot hide


def test_table_grad_ids_past_16_bits():
    d = R.high_id_case()
    assert int(d["ids"].max()) == R.HIGH_V - 1
    ref = table_run(d, F32, ("high_id",))
    assert R.row_margin(ref["dword"], d["ids"], *TAB[F32]) > 100


@pytest.mark.parametrize("act", [F32, BF16])
def test_table_grad_zipf(act):
    """P = 11, Lt = 233, H = 256. bf16: rtol = 2e-2 alone makes 100 tolerances more than any row,
    so the rows are held to stand 100 x out of the absolute part (5e-2)."""
    d = R.zipf_case()
    ref = table_run(d, act, ("zipf", NAME[act]))
    rtol, atol = TAB[act] if act == F32 else (0.0, TAB[act][1])
    assert R.row_margin(ref["dword"], d["ids"], rtol, atol) > 100
    assert R.row_margin(ref["dtyp"], d["tt"], rtol, atol) > 100


# =================================================================================================
# row-block and width edges of embed_ln_fwd / bwd
# =================================================================================================
EDGE_SHAPES = [(1, 1, 4), (3, 7, 100), (5, 13, 1024), (2, 65, 768), (257, 2, 4), (1, 130, 64)]


def edge_case(P, Lt, H, variant="full"):
    return R.embed_inputs(P, Lt, H, 23, 3, 2, tt=None if variant == "no_tt" else "random")


def edge_run(P, Lt, H, act, variant):
    d = edge_case(P, Lt, H, variant)
    key = ("edge", (P, Lt, H), NAME[act])
    ref = R.embed_ln_ref(d, act=act)
    fills = embed_fills(d, 2)
    v = _dev(d)
    y, mean, rstd = embed_forward(v, act)
    _norm_close(y, ref["y"], TOL[act], key + ("y",))
    _norm_close(mean, ref["mean"].reshape(-1), TOL[F32], key + ("mean",))
    _norm_close(rstd, ref["rstd"].reshape(-1), TOL[F32], key + ("rstd",))
    # NaN in the visual rows of djoint (and around it) reaches no output
    djg = Guarded(P, Lt * H, ld=(Lt + TV) * H, dtype=act, device=DEV).set(v["dj"].to(act))
    ws = torch.empty(embed_ws(v), device=DEV)
    with_dtyp = variant == "full"

    def run():
        ws.fill_(float("nan"))
        out = embed_backward(v, mean, rstd, djg, fills, ws, act, with_dtyp)
        return [out[k] for k in GRADS if k in out]

    names = [k for k in GRADS if with_dtyp or k != "dtyp"]
    outs = dict(zip(names, poison_check(run, [djg], "embed_ln_bwd")))
    check_table(outs["dword"], fills["dword"], ref["dword"], d["ids"], act, key + ("dword",))
    if with_dtyp:
        check_table(outs["dtyp"], fills["dtyp"], ref["dtyp"], d["tt"], act, key + ("dtyp",))
    for k in ("dpos", "dgamma", "dbeta"):
        _norm_close(outs[k], fills[k].double() + ref[k], GRAD[act], key + (k,))
    assert _bits_equal(outs["dpos"][0], fills["dpos"][0]), "dpos[0] (padding_idx) was written"
    assert _bits_equal(outs["dpos"][Lt:], fills["dpos"][Lt:]), "dpos rows past Lt were written"


@pytest.mark.parametrize("act", [F32, BF16])
@pytest.mark.parametrize("P,Lt,H", EDGE_SHAPES)
def test_embed_ln_edges(P, Lt, H, act):
    edge_run(P, Lt, H, act, "full")


@pytest.mark.parametrize("act", [F32, BF16])
@pytest.mark.parametrize("P,Lt,H", [(3, 7, 100), (2, 65, 768)])
@pytest.mark.parametrize("variant", ["no_tt", "no_dtype_tab"])
def test_embed_ln_optional_arguments(variant, P, Lt, H, act):
    """tt = NULL with dtype_tab = NULL (every row takes type row 0); tt given, dtype_tab = NULL."""
    edge_run(P, Lt, H, act, variant)


def _sevens(d):
    return {k: torch.full(d[s].shape, 7.0, device=DEV)
            for k, s in dict(dword="word", dpos="pos", dtyp="typ", dgamma="gamma", dbeta="beta").items()}


def test_embed_ln_p0_writes_nothing():
    d = edge_case(3, 7, 100)
    v = _dev(d)
    joint, mean, rstd, ws = (torch.full((64,), 7.0, device=DEV) for _ in range(4))
    out = _sevens(d)
    assert raw.status("mmseq_embed_ln_fwd", *embed_fwd_args(v, joint, 10 * 100, mean, rstd, F32, P=0)) == 0
    assert raw.status("mmseq_embed_ln_bwd",
                      *embed_bwd_args(v, mean, rstd, joint, 10 * 100, out, ws, F32, P=0)) == 0
    torch.cuda.synchronize()
    for t in [joint, mean, rstd, ws] + list(out.values()):
        assert bool((t == 7.0).all()), "a call with P = 0 wrote to a buffer"


@pytest.mark.parametrize("what", ["h1028", "bwd_h6", "dword_offset", "ws_offset"])
def test_embed_ln_rejects(what):
    P, Lt, H = 2, 3, 8
    d = edge_case(P, Lt, 1028)  # every buffer is large enough for the widest call below
    v = _dev(d)
    big = 4 * P * (Lt + TV) * 1028
    joint, ws = torch.full((big,), 7.0, device=DEV), torch.full((big,), 7.0, device=DEV)
    mean, rstd = torch.full((P * Lt,), 7.0, device=DEV), torch.full((P * Lt,), 7.0, device=DEV)
    out = _sevens(d)
    out["dword"] = torch.full((d["word"].numel() + 4,), 7.0, device=DEV)
    arg = dict(out)
    Hc, wsc, st_fwd = H, ws, None
    if what == "h1028":
        Hc = 1028
        st_fwd = raw.status("mmseq_embed_ln_fwd", *embed_fwd_args(v, joint, (Lt + TV) * Hc, mean, rstd, F32, Hc))
    elif what == "bwd_h6":
        Hc = 6
    elif what == "dword_offset":
        arg["dword"] = out["dword"][1:]
    else:
        wsc = ws[1:]
    st = raw.status("mmseq_embed_ln_bwd", *embed_bwd_args(v, mean, rstd, joint, (Lt + TV) * Hc, arg, wsc, F32, Hc))
    torch.cuda.synchronize()
    assert st == raw.EINVAL and st_fwd in (None, raw.EINVAL)
    for t in [joint, ws, mean, rstd] + list(out.values()):
        assert bool((t == 7.0).all()), "a rejected call wrote to a buffer"


def test_embed_ln_bwd_workspace_exact():
    """(2, 65, 768): 130 rows, three 64-row blocks; fp32 and bf16 through table_run's guarded
    workspace of exactly mmseq_embed_ln_bwd_workspace() floats."""
    for act in (F32, BF16):
        table_run(edge_case(2, 65, 768), act, ("edge", (2, 65, 768), NAME[act]))


# =================================================================================================
# ViT embedding
# =================================================================================================
# (activations, W, elements x is moved off its 16-byte alignment)
VIT_WIDTHS = [(BF16, 256, 0), (BF16, 512, 0), (BF16, 768, 0), (BF16, 1024, 0),  # vit_embed_*16<1..4>
              (BF16, 320, 0),                                                    # generic bf16
              (BF16, 512, 4),                                                    # generic, as the fallback
              (F32, 4, 0), (F32, 100, 0), (F32, 1024, 0)]
VIT_SHAPES = [(1, 1), (5, 1), (3, 4), (257, 1)]  # P * ntok = 3, 15, 27, 771
VIT_GRADS = ("dcls", "dpos", "dgamma", "dbeta")


def _shifted(g, k):
    """Move the declared extents of a Guarded k elements into its trailing guard."""
    g.offset += k
    g.view = g._strided(g.buf)
    g.inside.zero_()
    g._strided(g.inside)[:] = True
    return g


def vit_fills(d, seed):
    g = R.gen(seed, 8)
    src = dict(dcls="cls", dpos="pos", dgamma="gamma", dbeta="beta")
    return {k: torch.randn(d[s].shape, generator=g) for k, s in src.items()}


def vit_ws(P, ntok, W):
    return nat.lib().mmseq_vit_embed_bwd_workspace(P, ntok, W)


def vit_forward(v, act, shift):
    P, _, W = v["po"].shape
    gg = v["gg"]
    ntok = 1 + 2 * gg
    p = raw.p
    po = v["po"].to(act).contiguous()
    x = _shifted(Guarded(P * ntok, W, dtype=act, device=DEV), shift).fill_pattern().snapshot()
    y = Guarded(P * ntok, W, dtype=act, device=DEV).fill_pattern().snapshot()
    assert x.t.data_ptr() % 16 == (2 * shift) % 16
    mean = torch.full((P * ntok,), float("nan"), device=DEV)
    rstd = torch.full((P * ntok,), float("nan"), device=DEV)
    raw.call("mmseq_vit_embed_fwd", P, ntok, W, gg, p(po), p(v["cls"]), p(v["pos"]), p(v["gamma"]),
             p(v["beta"]), v["eps"], p(x.t), p(y.t), p(mean), p(rstd), CODE[act])
    torch.cuda.synchronize()
    x.check_untouched("vit_embed_fwd x")
    y.check_untouched("vit_embed_fwd y")
    return x, y, mean, rstd


def vit_backward(v, x, mean, rstd, fills, ws, act):
    P, _, W = v["po"].shape
    gg = v["gg"]
    ntok = 1 + 2 * gg
    p = raw.p
    dy = v["dy"].to(act).contiguous()
    dpo = Guarded(P * 2 * gg, W, dtype=act, device=DEV).fill_pattern().snapshot()
    out = {k: f.clone().to(DEV) for k, f in fills.items()}
    raw.call("mmseq_vit_embed_bwd", P, ntok, W, gg, p(dy), p(x.t), p(mean), p(rstd), p(v["gamma"]),
             p(dpo.t), p(out["dcls"]), p(out["dpos"]), p(out["dgamma"]), p(out["dbeta"]), p(ws),
             CODE[act])
    torch.cuda.synchronize()
    dpo.check_untouched("vit_embed_bwd dpatch_out")
    out["dpo"] = dpo.v2.clone()
    return out


def vit_check(d, ref, fills, x, y, out, act, key):
    P, _, W = d["po"].shape
    gg = d["gg"]
    ntok = 1 + 2 * gg
    _norm_close(x.v2.view(P, ntok, W), ref["x"], TOL[act] * 2, key + ("x",))
    _norm_close(y.v2.view(P, ntok, W), ref["y"], TOL[act] * 2, key + ("y",))
    _norm_close(out["dpo"].view(P, 2 * gg, W), ref["dpo"], TOL[act] * 2, key + ("dpo",))
    for k in VIT_GRADS:
        _norm_close(out[k], fills[k].double() + ref[k], GRAD[act], key + (k,))
    # row by row: position row gg is token gg alone, the rows below it are two tokens each
    dx = ref["dx"]
    for r in range(gg + 1):
        tok = dx[:, r].sum(0) + (dx[:, r + gg + 1].sum(0) if r < gg else 0)
        _norm_close(out["dpos"][r], fills["dpos"][r].double() + tok, GRAD[act], key + ("dpos",))


@pytest.mark.parametrize("P,gg", VIT_SHAPES)
@pytest.mark.parametrize("act,W,shift", VIT_WIDTHS)
def test_vit_embed_edges(act, W, shift, P, gg):
    d = R.vit_inputs(P, gg, W, 1)
    ref = R.vit_embed_ref(d, act=act)
    fills = vit_fills(d, 1)
    v = _dev(d)
    key = ("vit", NAME[act], W, (P, gg))
    ws = torch.full((vit_ws(P, 1 + 2 * gg, W),), float("nan"), device=DEV)
    x, y, mean, rstd = vit_forward(v, act, shift)
    out = vit_backward(v, x, mean, rstd, fills, ws, act)
    vit_check(d, ref, fills, x, y, out, act, key)
    if shift:  # the fallback agrees with the aligned (half-wave) run to the bf16 tolerance
        xa, ya, ma, ra = vit_forward(v, act, 0)
        oa = vit_backward(v, xa, ma, ra, fills, ws, act)
        _norm_close(x.v2, xa.v2, TOL[act] * 2, key + ("x", "aligned"))
        _norm_close(y.v2, ya.v2, TOL[act] * 2, key + ("y", "aligned"))
        _norm_close(out["dpo"], oa["dpo"], TOL[act] * 2, key + ("dpo", "aligned"))
        for k in VIT_GRADS:
            _norm_close(out[k], oa[k], GRAD[act], key + (k, "aligned"))


@pytest.mark.parametrize("W", [512, 320])
def test_vit_embed_bwd_workspace_exact(W):
    """(3, 4) in bf16: W = 512 carves dx0 | LN partials | sp | s0 | column-sum scratch out of the
    workspace, W = 320 (generic) the first two."""
    P, gg, act = 3, 4, BF16
    d = R.vit_inputs(P, gg, W, 1)
    ref = R.vit_embed_ref(d, act=act)
    fills = vit_fills(d, 1)
    v = _dev(d)
    x, y, mean, rstd = vit_forward(v, act, 0)

    def run(ws):
        out = vit_backward(v, x, mean, rstd, fills, ws, act)
        return [out[k].float() for k in VIT_GRADS + ("dpo",)]

    outs = dict(zip(VIT_GRADS + ("dpo",), _ws_runs(vit_ws(P, 1 + 2 * gg, W), run)))
    vit_check(d, ref, fills, x, y, outs, act, ("vit", NAME[act], W, (P, gg)))


# =================================================================================================
# vit_im2col: the bf16 fast path is a copy
# =================================================================================================
@pytest.mark.parametrize("R_,ps", [(32, 16), (64, 32)])
def test_vit_im2col_bf16_fast_exact(R_, ps):
    B, N, npair = 2, 3, 2
    g = R.gen(7, R_)
    images = torch.randn(B, N, 3, R_, R_, generator=g)
    pairs = torch.tensor([[[0, 1], [2, 0]], [[1, 2], [2, 1]]])
    want = R.vit_im2col_ref(images, pairs, ps).bfloat16()
    rows, K = want.shape
    assert K == 3 * ps * ps and rows == B * npair * 2 * (R_ // ps) ** 2
    out = Guarded(rows, K, dtype=BF16, device=DEV).fill_pattern().snapshot()
    img, pr = images.to(DEV), pairs.to(DEV)
    raw.call("mmseq_vit_im2col", B, N, npair, R_, ps, raw.p(img), raw.p(pr), raw.p(out.t), K, CODE[BF16])
    torch.cuda.synchronize()
    out.check_untouched("vit_im2col patches")
    assert torch.equal(out.v2.cpu().view(torch.int16), want.view(torch.int16))


# =================================================================================================
def cpu_fp32_miss():
    """How far the same formulas in fp32 PyTorch on the CPU are from float64, for every case above,
    against the tolerance of each output: prints the entries FP32_MISS needs (python -c 'import
    test_embed_edges_gpu as t; t.cpu_fp32_miss()' from tests/; no GPU involved)."""
    worst = {}

    def report(key, a32, a64, tol=None, rtol=None, atol=None):
        err = (a32.double() - a64).abs()
        if tol is not None:
            over = float(err.max()) - tol * (1 + float(a64.abs().max()))
        else:
            over = float((err - (atol + rtol * a64.abs())).max())
        worst[key] = float(err.max())
        if over > 0:
            print(f"{key}: fp32 miss {float(err.max()):.3g}  <-- exceeds: list it")

    def embed(d, act, key):
        a, b = R.embed_ln_ref(d, torch.float32, act), R.embed_ln_ref(d, R.F64, act)
        report(key + ("y",), a["y"], b["y"], tol=TOL[act])
        report(key + ("mean",), a["mean"], b["mean"], tol=TOL[F32])
        report(key + ("rstd",), a["rstd"], b["rstd"], tol=TOL[F32])
        for k in ("dword", "dtyp"):
            report(key + (k,), a[k], b[k], rtol=TAB[act][0], atol=TAB[act][1])
        for k in ("dpos", "dgamma", "dbeta"):
            report(key + (k,), a[k], b[k], tol=GRAD[act])

    for name, role, H in LAYOUT_RUNS:
        embed(R.layout_case(name, role, H), F32, ("layout", name, role, H))
    embed(R.high_id_case(), F32, ("high_id",))
    for act in (F32, BF16):
        embed(R.zipf_case(), act, ("zipf", NAME[act]))
        for P, Lt, H in EDGE_SHAPES:
            embed(edge_case(P, Lt, H), act, ("edge", (P, Lt, H), NAME[act]))
    for act, W, _ in VIT_WIDTHS:
        for P, gg in VIT_SHAPES:
            d = R.vit_inputs(P, gg, W, 1)
            a, b = R.vit_embed_ref(d, torch.float32, act), R.vit_embed_ref(d, R.F64, act)
            key = ("vit", NAME[act], W, (P, gg))
            for k in ("x", "y", "dpo"):
                report(key + (k,), a[k], b[k], tol=TOL[act] * 2)
            for k in VIT_GRADS:
                report(key + (k,), a[k], b[k], tol=GRAD[act])
    k = max(worst, key=worst.get)
    print(f"{len(worst)} outputs; the largest fp32 miss is {worst[k]:.3g} at {k}")
