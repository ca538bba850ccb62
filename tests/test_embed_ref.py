"""The references and run layouts that tests/test_embed_edges_gpu.py relies on, checked on the CPU:
the layouts reach the cases of the chunked table gradient they are there for, the float64
references agree with torch autograd, and the seeds of the table cases give reference rows that
stand out of the tolerance (so a dropped or doubled piece of a run cannot hide in it)."""
import pytest
import torch

import embed_ref as R

F64 = torch.float64


def _reach(names):
    cases, joins, last = set(), set(), False
    for n in names:
        c = R.chunk_cases(R.LAYOUTS[n])
        cases |= c["cases"]
        joins |= c["joins"]
        last |= c["last_row_join"]
    return cases, joins, last


def test_layouts_have_the_sizes_of_the_table():
    n = {k: sum(v) for k, v in R.LAYOUTS.items()}
    assert n == dict(a=192, b=192, c=194, d=128, e=336, f1=1, f63=63, f65=65, g=193)
    for k, v in n.items():
        P, Lt = R.LAYOUT_SHAPE[v]
        assert P * Lt == v


def test_layouts_cover_every_chunk_case():
    cases, joins, last = _reach(R.LAYOUTS)
    real = {(b, e, f) for pad, b, e, f in cases if not pad}
    # a full chunk: all four (began, ends)
    assert {(b, e, "full") for b in (False, True) for e in (False, True)} <= real
    # a partial chunk is the last one, so nothing in it continues: both cases that can occur
    assert {(b, e) for b, e, f in real if f == "partial"} == {(True, True), (False, True)}
    assert not any(f == "partial" and not e for _, _, e, f in cases)
    # the padding run: starts a crossing, fills a whole chunk inside it, ends it
    pad = {(b, e) for p, b, e, f in cases if p}
    assert {(True, False), (False, False), (False, True)} <= pad
    assert {1, 2, 3} <= joins
    assert last


def test_each_layout_reaches_what_it_is_there_for():
    T, F = True, False
    a = R.chunk_cases(R.LAYOUTS["a"])
    assert a["cases"] == {(F, T, T, "full")} and not a["joins"]  # exact fills: nothing crosses
    b = R.chunk_cases(R.LAYOUTS["b"])
    assert b["cases"] == {(F, T, T, "full")} and not b["joins"]
    c = R.chunk_cases(R.LAYOUTS["c"])
    assert c["joins"] == {3}
    assert {(F, T, F, "full"), (F, F, F, "full"), (F, F, T, "partial"), (F, T, T, "partial")} <= c["cases"]
    d = R.chunk_cases(R.LAYOUTS["d"])
    assert d["joins"] == {1} and d["last_row_join"]
    assert d["cases"] == {(T, T, T, "full"), (F, T, F, "full"), (F, F, T, "full")}
    e = R.chunk_cases(R.LAYOUTS["e"])
    assert e["joins"] == {3}
    assert {(T, T, F, "full"), (T, F, F, "full"), (T, F, T, "full"), (F, F, T, "partial")} <= e["cases"]
    assert R.chunk_cases(R.LAYOUTS["f1"])["cases"] == {(F, T, T, "partial")}
    assert R.chunk_cases(R.LAYOUTS["f63"])["cases"] == {(F, T, T, "partial")}
    f65 = R.chunk_cases(R.LAYOUTS["f65"])
    assert f65["cases"] == {(F, T, F, "full"), (F, F, T, "partial")} and f65["last_row_join"]
    assert R.chunk_cases(R.LAYOUTS["g"])["joins"] == {2}


def test_ids_from_counts_layout():
    counts = R.LAYOUTS["e"]
    ids = R.ids_from_counts(counts, 3)
    assert torch.bincount(ids, minlength=len(counts)).tolist() == counts
    assert torch.equal(ids, R.ids_from_counts(counts, 3))
    assert not torch.equal(ids, ids.sort().values)  # the rows of a run are scattered


def test_embed_ln_ref_agrees_with_autograd():
    d = R.embed_inputs(3, 7, 12, 9, 3, 1)
    d["ids"][0, :2] = 0
    ref = R.embed_ln_ref(d)
    P, Lt = d["ids"].shape
    w_, p_, t_, g_, b_ = (d[k].double().requires_grad_(True) for k in ("word", "pos", "typ", "gamma", "beta"))
    emb = torch.nn.functional.embedding
    posid = torch.arange(Lt)[None].expand(P, Lt)
    e = emb(d["ids"], w_, padding_idx=0) + emb(posid, p_, padding_idx=0) + emb(d["tt"], t_, padding_idx=0)
    y = torch.nn.functional.layer_norm(e, (12,), g_, b_, d["eps"])
    grads = torch.autograd.grad(y, (w_, p_, t_, g_, b_), d["dj"].double())
    tol = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref["y"], y.detach(), **tol)
    for name, g in zip(("dword", "dpos", "dtyp", "dgamma", "dbeta"), grads):
        torch.testing.assert_close(ref[name], g, **tol)
    assert not ref["dword"][0].any() and not ref["dpos"][0].any() and not ref["dtyp"][0].any()
    assert not ref["dpos"][Lt:].any()


def test_embed_ln_ref_without_token_types():
    d = R.embed_inputs(2, 5, 8, 9, 2, 2, tt=None)
    z = dict(d, tt=torch.zeros_like(d["ids"]))
    a, b = R.embed_ln_ref(d), R.embed_ln_ref(z)
    for k in a:
        assert torch.equal(a[k], b[k])
    assert not a["dtyp"].any()


@pytest.mark.parametrize("gg", [1, 4])
def test_vit_embed_ref_agrees_with_autograd(gg):
    P, W = 3, 12
    d = R.vit_inputs(P, gg, W, 3)
    ref = R.vit_embed_ref(d)
    ntok = 1 + 2 * gg
    po_, c_, p_, g_, b_ = (d[k].double().requires_grad_(True) for k in ("po", "cls", "pos", "gamma", "beta"))
    xx = torch.cat([c_.expand(P, 1, W), po_.view(P, 2 * gg, W)], 1)
    pe = torch.cat([p_, p_[:gg]], 0)
    y = torch.nn.functional.layer_norm(xx + pe, (W,), g_, b_, d["eps"])
    grads = torch.autograd.grad(y, (po_, c_, p_, g_, b_), d["dy"].double().view(P, ntok, W))
    tol = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref["y"], y.detach(), **tol)
    for name, g in zip(("dpo", "dcls", "dpos", "dgamma", "dbeta"), grads):
        torch.testing.assert_close(ref[name], g, **tol)
    # position row gg belongs to token gg alone, the rows below it to two tokens
    dx = ref["dx"]
    torch.testing.assert_close(ref["dpos"][gg], dx[:, gg].sum(0), **tol)
    for r in range(gg):
        torch.testing.assert_close(ref["dpos"][r], (dx[:, r] + dx[:, r + gg + 1]).sum(0), **tol)


def test_vit_embed_ref_bf16_normalises_the_stored_x():
    d = R.vit_inputs(2, 1, 16, 4)
    ref = R.vit_embed_ref(d, act=torch.bfloat16)
    assert torch.equal(ref["x"], ref["x"].bfloat16().double())
    y, _, _ = R.layer_norm(ref["x"], d["gamma"].double(), d["beta"].double(), d["eps"])
    assert torch.equal(ref["y"], y)


def test_vit_im2col_ref_is_a_gather():
    g = R.gen(5)
    images = torch.randn(2, 3, 3, 8, 8, generator=g)
    pairs = torch.tensor([[[0, 1], [2, 0]], [[1, 2], [2, 1]]])
    out = R.vit_im2col_ref(images, pairs, 4).view(2, 2, 2, 4, 3, 4, 4)
    # batch 1, pair 0, second image (= image 2), patch (1, 0), channel 2, kernel row 3
    assert torch.equal(out[1, 0, 1, 2, 2, 3], images[1, 2, 2, 4 + 3, 0:4])


# -------------------------------------------------------------------------------------------------
# every occurring id's reference row is more than 100 tolerances away from zero
# -------------------------------------------------------------------------------------------------
F32_TAB = (1e-5, 1e-4)  # rtol, atol of test_embed_table_grad_fixed_order
BF16_ATOL = 5e-2


def _margins(d, act=torch.float32):
    ref = R.embed_ln_ref(d, act=act)
    out = [("dword", ref["dword"], d["ids"])]
    if d["tt"] is not None:
        out.append(("dtyp", ref["dtyp"], d["tt"]))
    return out


@pytest.mark.parametrize("name", list(R.LAYOUTS))
@pytest.mark.parametrize("role", ["word", "type"])
def test_layout_rows_stand_out(name, role):
    for H in (8, 768) if name in ("c", "e") else (8,):
        for what, table, ids in _margins(R.layout_case(name, role, H)):
            assert R.row_margin(table, ids, *F32_TAB) > 100, (H, what)


def test_high_id_and_zipf_rows_stand_out():
    for what, table, ids in _margins(R.high_id_case()):
        assert R.row_margin(table, ids, *F32_TAB) > 100, what
    d = R.zipf_case()
    assert int((d["ids"] == 0).sum()) > 128 and int((d["ids"] == 1).sum()) > 64  # runs of chunks
    assert int((torch.bincount(d["ids"].reshape(-1)) == 1).sum()) > 300          # and single rows
    for what, table, ids in _margins(d):
        assert R.row_margin(table, ids, *F32_TAB) > 100, what
    # bf16: rtol = 2e-2 alone makes 100 tolerances more than any row, so the condition is taken on
    # the absolute part: every occurring row has max |.| > 100 * 5e-2
    for what, table, ids in _margins(d, act=torch.bfloat16):
        assert R.row_margin(table, ids, 0.0, BF16_ATOL) > 100, what
