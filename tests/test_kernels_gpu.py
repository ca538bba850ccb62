"""Per-kernel numerics: each HIP kernel (through the C ABI) against a plain fp32 PyTorch reference.

fp32 kernels (exact-fp32 MFMA) are held to ~1e-5 relative; bf16 kernels to bf16 rounding of
inputs/outputs (~1e-2 relative).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multimodal_sequencing_amd import _native as nat

DEV = "cuda"
TOL = {torch.float32: (2e-5, 2e-5), torch.bfloat16: (2e-2, 2e-2)}


def _close(a, b, dtype, scale=1.0):
    rt, at = TOL[dtype]
    a = a.float()
    b = b.float()
    err = (a - b).abs().max().item()
    ref = b.abs().max().item() + 1e-6
    assert err <= at * scale + rt * scale * ref, f"max err {err} vs ref max {ref}"


def _q(x, dtype):
    return x.to(dtype).float()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", [(256, 128, 64), (300, 200, 136), (77, 96, 520), (1, 2, 768),
                                   (513, 768, 768)])
@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("fast", [1, 3, 0, 4])
def test_gemm_nt_epilogues(dtype, M, N, K, act, fast):
    nat.gemm_set_fast(fast)
    g = torch.Generator(device="cpu").manual_seed(M * 7 + N + K + act)
    A = torch.randn(M, K, generator=g).to(DEV, dtype)
    Bm = torch.randn(N, K, generator=g).to(DEV, dtype) * 0.1
    bias = torch.randn(N, generator=g).to(DEV)
    resid = torch.randn(M, N, generator=g).to(DEV, dtype)
    C = torch.empty(M, N, device=DEV, dtype=dtype)
    aux = torch.empty(M, N, device=DEV, dtype=dtype) if act else None
    nat.gemm(A, Bm, C, M, N, K, bias=bias, act=act, aux=aux, resid=resid)
    z = A.float() @ Bm.float().t() + bias
    acts = {0: lambda x: x, 1: lambda x: torch.nn.functional.gelu(x), 2: lambda x: x * torch.sigmoid(1.702 * x),
            3: torch.tanh, 4: lambda x: torch.nn.functional.gelu(x, approximate="tanh")}
    ref = acts[act](z) + resid.float()
    _close(C, ref, dtype, scale=max(1.0, math.sqrt(K) / 8))
    if act:
        _close(aux, z, dtype, scale=max(1.0, math.sqrt(K) / 8))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (200, 96, 300), (768, 768, 1026), (2, 520, 77),
                                   (768, 3072, 4100), (136, 264, 64)])
@pytest.mark.parametrize("fast", [1, 3, 0])
def test_gemm_tn_accumulate(dtype, M, N, K, fast):
    nat.gemm_set_fast(fast)
    # dW[M][N] += sum_k dY[k][M] X[k][N]  (wgrad layout)
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    dY = torch.randn(K, M, generator=g).to(DEV, dtype)
    X = torch.randn(K, N, generator=g).to(DEV, dtype)
    C0 = torch.randn(M, N, generator=g).to(DEV)
    C = C0.clone()
    nat.gemm(dY, X, C, M, N, K, trans=1, accumulate=True)
    ref = C0 + dY.float().t() @ X.float()
    _close(C, ref, dtype, scale=max(1.0, math.sqrt(K) / 8))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gemm_dact_and_batched(dtype):
    nat.gemm_set_fast(1)
    g = torch.Generator(device="cpu").manual_seed(3)
    M, Nn, K, Bt = 96, 64, 128, 3
    A = torch.randn(Bt, M, K, generator=g).to(DEV, dtype)
    Bm = torch.randn(Nn, K, generator=g).to(DEV, dtype) * 0.1
    z = torch.randn(Bt, M, Nn, generator=g).to(DEV, dtype)
    C = torch.empty(Bt, M, Nn, device=DEV, dtype=dtype)
    nat.gemm(A, Bm, C, M, Nn, K, batch=Bt, sA=M * K, sB=0, sC=M * Nn, act=1, dact=z)
    zz = z.float().requires_grad_(True)
    gz = torch.autograd.grad(torch.nn.functional.gelu(zz).sum(), zz)[0]
    ref = (A.float() @ Bm.float().t()) * gz
    _close(C, ref, dtype, scale=2.0)


def test_gemm_fast_strided_batched():
    # batched NT with a row stride > K and non-multiple-of-128 M (visn_fc into the joint rows)
    nat.gemm_set_fast(1)
    Bt, M, K, Nn, ldc = 3, 200, 128, 192, 192
    g = torch.Generator(device="cpu").manual_seed(9)
    A = torch.randn(Bt, M, K, generator=g).to(DEV, torch.bfloat16)
    W = torch.randn(Nn, K, generator=g).to(DEV, torch.bfloat16)
    C = torch.zeros(Bt, M + 50, Nn, device=DEV, dtype=torch.bfloat16)
    nat.gemm(A, W, C[:, 50:], M, Nn, K, batch=Bt, sA=M * K, sC=(M + 50) * Nn)
    ref = A.float() @ W.float().t()
    _close(C[:, 50:], ref, torch.bfloat16, scale=2.0)
    assert C[:, :50].abs().max().item() == 0


@pytest.mark.parametrize("fast", [1, 4])
def test_gemm_big_tile_path(fast):
    # >= 256 256x256 tiles (here 130 x 4) selects the 256^2 NT kernel by default; ragged M edge, GELU + aux +
    # residual epilogue; mode 4 also runs it batched with strides
    nat.gemm_set_fast(fast)
    M, Nn, K = 33000 + 77, 1024, 256
    g = torch.Generator(device="cpu").manual_seed(10)
    A = torch.randn(M, K, generator=g).to(DEV, torch.bfloat16)
    W = (torch.randn(Nn, K, generator=g) * 0.1).to(DEV, torch.bfloat16)
    bias = torch.randn(Nn, generator=g).to(DEV)
    resid = torch.randn(M, Nn, generator=g).to(DEV, torch.bfloat16)
    C = torch.empty(M, Nn, device=DEV, dtype=torch.bfloat16)
    aux = torch.empty_like(C)
    nat.gemm(A, W, C, M, Nn, K, bias=bias, act=1, aux=aux, resid=resid)
    z = A.float() @ W.float().t() + bias
    _close(aux, z, torch.bfloat16, scale=2.0)
    _close(C, torch.nn.functional.gelu(z) + resid.float(), torch.bfloat16, scale=2.0)
    if fast == 4:
        Bt, Mb = 3, 300
        Ab = torch.randn(Bt, Mb, K, generator=g).to(DEV, torch.bfloat16)
        Cb = torch.zeros(Bt, Mb + 20, Nn, device=DEV, dtype=torch.bfloat16)
        nat.gemm(Ab, W, Cb[:, 20:], Mb, Nn, K, batch=Bt, sA=Mb * K, sC=(Mb + 20) * Nn)
        _close(Cb[:, 20:], Ab.float() @ W.float().t(), torch.bfloat16, scale=2.0)
        assert Cb[:, :20].abs().max().item() == 0


@pytest.fixture(autouse=True)
def _restore_gemm_path():
    yield
    nat.gemm_set_fast(1)


def _attn_ref(qkv, P, T, heads, bias, scale):
    H = heads * 64
    q, k, v = qkv.float().view(P, T, 3, heads, 64).unbind(2)
    s = torch.einsum("pqhd,pkhd->phqk", q, k) * scale
    if bias is not None:
        s = s + bias[:, None, None, :]
    a = torch.softmax(s, -1)
    return torch.einsum("phqk,pkhd->pqhd", a, v).reshape(P * T, H)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("P,T,heads,masked", [(2, 64, 1, False), (3, 129, 2, True), (2, 33, 2, True),
                                              (1, 513, 12, True), (2, 393, 2, False), (1, 1, 1, False),
                                              (2, 127, 1, True), (2, 144, 2, True), (1, 272, 3, False),
                                              (1, 145, 2, True), (1, 65, 2, True), (2, 192, 1, False),
                                              (1, 128, 2, True), (1, 17, 1, False)])
@pytest.mark.parametrize("fast", [1, 0, 2])
def test_attention_fwd_bwd(dtype, P, T, heads, masked, fast):
    nat.attn_set_fast(fast)
    g = torch.Generator(device="cpu").manual_seed(P * T + heads)
    H = heads * 64
    qkv = torch.randn(P * T, 3 * H, generator=g).to(DEV, dtype)
    bias = None
    if masked:
        m = (torch.rand(P, T, generator=g) > 0.3).float()
        m[:, 0] = 1
        bias = ((1 - m) * -10000.0).to(DEV)
    scale = 1 / 8
    out = torch.empty(P * T, H, device=DEV, dtype=dtype)
    lse = torch.empty(P, heads, T, device=DEV)
    nat.attn_fwd(P, T, heads, qkv, 3 * H, 0, H, 2 * H, bias, scale, out, H, lse)
    qf = qkv.float().requires_grad_(True)
    ref = _attn_ref(qf, P, T, heads, bias, scale)
    _close(out, ref, dtype)
    dout = torch.randn(P * T, H, generator=g).to(DEV, dtype)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty(P, heads, T, device=DEV)
    nat.attn_bwd(P, T, heads, qkv, 3 * H, 0, H, 2 * H, bias, scale, out, H, dout, H, lse, delta,
               dqkv, 3 * H)
    (ref_g,) = torch.autograd.grad(ref, qf, dout.float())
    _close(dqkv, ref_g, dtype, scale=2.0)
    nat.attn_set_fast(1)


@pytest.mark.parametrize("profile", ["ramp_up", "ramp_gentle", "ramp_down", "jump"])
@pytest.mark.parametrize("bias_mode", ["none", "first_tile_masked", "zeros"])
@pytest.mark.parametrize("fast", [1, 2])
@pytest.mark.parametrize("T", [300, 265])
def test_attention_rescale_and_zero_bias_tiles(profile, bias_mode, fast, T):
    """bf16 fast kernels: the running max moves only when a row's tile max exceeds it by > 8
    (log2) and all-zero-bias key tiles skip the bias add. Scores that climb across key tiles
    (several rescales mid-sequence), climb gently (~3.8 log2 per tile: the forward's fast
    exponentials are refused for a tile sum > 2^8 and the tile redone by the max path, which then
    rescales only every other tile), fall (none after the first tile) or jump, with a key bias
    masked only inside the first tile (later tiles take the zero-bias path). T = 265 leaves 9
    rows in the last query block: the forward's tail path, whose four waves see very different
    running maxima on their key chunks before the merge."""
    P, heads = 2, 2
    H = heads * 64
    g = torch.Generator(device="cpu").manual_seed(11)
    q, k, v = (torch.randn(3, P, T, heads, 64, generator=g) * 0.3).unbind(0)
    u = torch.nn.functional.normalize(torch.randn(64, generator=g), dim=0)
    pos = torch.arange(T, dtype=torch.float32) / T
    # score(q, key) ~ amp(key) * scale: ramps spanning ~54 log2 units (several rescales) and a
    # jump of ~36 log2 units at key 200
    if profile == "ramp_up":
        amp = 300.0 * pos
    elif profile == "ramp_gentle":
        amp = 100.0 * pos * T / 300.0
    elif profile == "ramp_down":
        amp = 300.0 * (1 - pos)
    else:
        amp = torch.where(torch.arange(T) >= 200, 200.0, 0.0)
    q = q + 3.0 * u
    k = k + amp[None, :, None, None] * u / 3.0
    qkv = torch.stack([q, k, v], 2).reshape(P * T, 3 * H).to(DEV, torch.bfloat16)
    bias = None
    if bias_mode == "first_tile_masked":
        b = torch.zeros(P, T)
        b[:, 10:20] = -10000.0
        bias = b.to(DEV)
    elif bias_mode == "zeros":
        bias = torch.zeros(P, T, device=DEV)
    scale = 1 / 8
    out = torch.empty(P * T, H, device=DEV, dtype=torch.bfloat16)
    lse = torch.empty(P, heads, T, device=DEV)
    nat.attn_set_fast(fast)
    nat.attn_fwd(P, T, heads, qkv, 3 * H, 0, H, 2 * H, bias, scale, out, H, lse)
    nat.attn_set_fast(1)
    qf = qkv.float().requires_grad_(True)
    ref = _attn_ref(qf, P, T, heads, bias, scale)
    _close(out, ref, torch.bfloat16)
    qq, kk, _ = qkv.float().view(P, T, 3, heads, 64).unbind(2)
    sc = torch.einsum("pqhd,pkhd->phqk", qq, kk) * scale
    if bias is not None:
        sc = sc + bias[:, None, None, :]
    torch.testing.assert_close(lse, torch.logsumexp(sc, -1), rtol=1e-3, atol=1e-3)
    dout = torch.randn(P * T, H, generator=g).to(DEV, torch.bfloat16)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty(P, heads, T, device=DEV)
    nat.attn_bwd(P, T, heads, qkv, 3 * H, 0, H, 2 * H, bias, scale, out, H, dout, H, lse, delta,
                 dqkv, 3 * H)
    (ref_g,) = torch.autograd.grad(ref, qf, dout.float())
    _close(dqkv, ref_g, torch.bfloat16, scale=2.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,cols,eps", [(100, 768, 1e-12), (7, 128, 1e-5), (300, 96, 1e-6),
                                           (64, 1536, 1e-12), (33, 2048, 1e-5), (17, 1100, 1e-6),
                                           (70001, 768, 1e-12)])  # > 512 blocks: rpb > 64
def test_layernorm(dtype, rows, cols, eps):
    g = torch.Generator(device="cpu").manual_seed(rows + cols)
    x = (torch.randn(rows, cols, generator=g) * 2 + 0.5).to(DEV, dtype)
    gamma = (1 + 0.1 * torch.randn(cols, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(cols, generator=g)).to(DEV)
    y = torch.empty_like(x)
    mean = torch.empty(rows, device=DEV)
    rstd = torch.empty(rows, device=DEV)
    nat.layernorm_fwd(rows, cols, x, nat.rows(cols), gamma, beta, eps, y, nat.rows(cols), mean, rstd)
    xf = x.float().requires_grad_(True)
    gf = gamma.clone().requires_grad_(True)
    bf = beta.clone().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(xf, (cols,), gf, bf, eps)
    _close(y, ref, dtype)
    dy = torch.randn(rows, cols, generator=g).to(DEV, dtype)
    dres = torch.randn(rows, cols, generator=g).to(DEV, dtype)
    dx = torch.empty_like(x)
    dg = torch.ones(cols, device=DEV)
    db = torch.ones(cols, device=DEV)
    nat.layernorm_bwd(rows, cols, dy, nat.rows(cols), x, nat.rows(cols), mean, rstd, gamma, dx,
                    nat.rows(cols), dres, nat.rows(cols), dg, db)
    rdx, rdg, rdb = torch.autograd.grad(ref, (xf, gf, bf), dy.float())
    _close(dx, rdx + dres.float(), dtype, scale=2.0)
    _close(dg, rdg + 1, torch.float32, scale=10.0 if dtype == torch.float32 else 500.0)
    _close(db, rdb + 1, torch.float32, scale=10.0 if dtype == torch.float32 else 500.0)


@pytest.mark.parametrize("dtype,rows,cols,mode", [
    (torch.bfloat16, 70001, 768, "drop"),   # joint LN2 / LN1: sums of the masked copy (fast kernel)
    (torch.bfloat16, 4099, 768, "dres"),    # ViT LN2: sums of dx with the residual (fast kernel)
    (torch.bfloat16, 300, 256, "plain"),    # fast kernel, one 256-column chunk
    (torch.bfloat16, 517, 1024, "drop"),    # cols 1024: the separate column-sum pass
    (torch.float32, 333, 768, "drop"),      # fp32 parity mode: generic kernel + column-sum pass
    (torch.bfloat16, 129, 96, "dres")])     # generic kernel (cols not a multiple of 256)
def test_layernorm_bwd_column_sums(dtype, rows, cols, mode):
    """mmseq_layernorm_bwd_ex: the LN backward outputs are unchanged and dsum accumulates the
    column sums of the gradient it writes for the next GEMM (dx_drop, else dx with dres), as stored;
    bitwise repeatable."""
    g = torch.Generator(device="cpu").manual_seed(rows * 3 + cols)
    x = (torch.randn(rows, cols, generator=g) * 2 + 0.5).to(DEV, dtype)
    gamma = (1 + 0.1 * torch.randn(cols, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(cols, generator=g)).to(DEV)
    y = torch.empty_like(x)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    nat.layernorm_fwd(rows, cols, x, nat.rows(cols), gamma, beta, 1e-12, y, nat.rows(cols), mean, rstd)
    dy = torch.randn(rows, cols, generator=g).to(DEV, dtype)
    dres = torch.randn(rows, cols, generator=g).to(DEV, dtype) if mode == "dres" else None
    d = nat.drop(0.1, 7, 11) if mode == "drop" else None

    def run(dsum):
        dx, dxd = torch.empty_like(x), torch.empty_like(x) if d is not None else None
        dg, db = torch.zeros(cols, device=DEV), torch.zeros(cols, device=DEV)
        nat.layernorm_bwd(rows, cols, dy, nat.rows(cols), x, nat.rows(cols), mean, rstd, gamma, dx,
                          nat.rows(cols), dres, nat.rows(cols), dg, db, dx_drop=dxd, drop_dx=d,
                          dsum=dsum, dsum_with_dres=dres is not None and dxd is None)
        return dx, dxd, dg, db

    dx0, dxd0, dg0, db0 = run(None)
    acc = torch.full((cols,), 0.5, device=DEV)
    dx1, dxd1, dg1, db1 = run(acc)
    assert torch.equal(dx1, dx0) and (dxd0 is None or torch.equal(dxd1, dxd0))
    torch.testing.assert_close(dg1, dg0, rtol=1e-6, atol=1e-5)
    torch.testing.assert_close(db1, db0, rtol=1e-6, atol=1e-5)
    summed = (dxd0 if dxd0 is not None else dx0).double().sum(0)
    tol = 1e-6 * float(summed.abs().max()) + 1e-3
    assert float((acc.double() - 0.5 - summed).abs().max()) < tol
    acc2 = torch.full((cols,), 0.5, device=DEV)
    run(acc2)
    assert torch.equal(acc2, acc)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_transpose_cast_batch(dtype):
    """mmseq_transpose_cast_batch: several fp32 matrices (ragged edges, odd widths, an unaligned
    source offset) transposed into one flat buffer in one launch, exactly as the cast of their
    transposes."""
    shapes = [(768, 768), (2304, 768), (130, 70), (1, 5), (3072, 768), (64, 3), (97, 128)]
    g = torch.Generator(device="cpu").manual_seed(5)
    src = torch.randn(sum(r * c for r, c in shapes) + 64 * len(shapes) + 2, generator=g).to(DEV)
    dst = torch.full((sum(r * c for r, c in shapes) + 64 * len(shapes),), 7.0, device=DEV, dtype=dtype)
    desc, so, do_, tiles = [], 2, 0, 0  # source offset 2: the unaligned (scalar) path
    for r, c in shapes:
        desc.append([r, c, so, do_, tiles])
        tiles += ((r + 63) // 64) * ((c + 63) // 64)
        so += r * c + (64 if so % 64 == 0 else 62)
        do_ += r * c + 64
    nat.transpose_cast_batch(torch.tensor(desc, dtype=torch.int64, device=DEV), tiles, src, dst)
    for (r, c, so, do_, _) in desc:
        want = src[so:so + r * c].view(r, c).t().contiguous().to(dtype)
        assert torch.equal(dst[do_:do_ + r * c].view(c, r), want)


def test_layernorm_strided_rows():
    # write the visual half of a [P][T][H] joint buffer in place (two-level strides)
    P, Lt, Tv, H = 3, 5, 7, 64
    x = torch.randn(P * Tv, H, device=DEV)
    joint = torch.zeros(P, Lt + Tv, H, device=DEV)
    g1 = torch.ones(H, device=DEV)
    b0 = torch.zeros(H, device=DEV)
    mean = torch.empty(P * Tv, device=DEV)
    rstd = torch.empty(P * Tv, device=DEV)
    nat.layernorm_fwd(P * Tv, H, x, nat.rows(H), g1, b0, 1e-12, joint[:, Lt:], nat.rows(H, (Lt + Tv) * H, Tv),
                    mean, rstd)
    ref = torch.nn.functional.layer_norm(x, (H,), eps=1e-12).view(P, Tv, H)
    torch.testing.assert_close(joint[:, Lt:], ref, rtol=1e-5, atol=1e-5)
    assert joint[:, :Lt].abs().max().item() == 0


def test_small_attention():
    B, T, heads, d = 3, 5, 8, 16
    g = torch.Generator(device="cpu").manual_seed(0)
    q, k, v = (torch.randn(B, T, heads * d, generator=g).to(DEV) for _ in range(3))
    m = torch.ones(B, T)
    m[1, 3:] = 0
    bias = ((1 - m) * -10000.0).to(DEV)
    out = torch.empty_like(q)
    probs = torch.empty(B, heads, T, T, device=DEV)
    nat.small_attn_fwd(B, T, heads, d, q, k, v, bias, d ** -0.5, out, probs)
    qf, kf, vf = (t.clone().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("bqhd,bkhd->bhqk", qf.view(B, T, heads, d), kf.view(B, T, heads, d)) * d ** -0.5
    a = torch.softmax(s + bias[:, None, None, :], -1)
    ref = torch.einsum("bhqk,bkhd->bqhd", a, vf.view(B, T, heads, d)).reshape(B, T, heads * d)
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-5)
    do = torch.randn_like(q)
    dq, dk, dv = (torch.empty_like(q) for _ in range(3))
    nat.small_attn_bwd(B, T, heads, d, q, k, v, probs, do, d ** -0.5, dq, dk, dv)
    rq, rk, rv = torch.autograd.grad(ref, (qf, kf, vf), do)
    for a_, b_ in ((dq, rq), (dk, rk), (dv, rv)):
        torch.testing.assert_close(a_, b_, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_span_pool(dtype):
    P, Lt, H = 6, 17, 96
    g = torch.Generator(device="cpu").manual_seed(1)
    top = torch.randn(P, Lt + 4, H, generator=g).to(DEV, dtype)  # ld_pair > Lt*H (joint rows)
    score = torch.randn(P, Lt, generator=g).to(DEV)
    sep = torch.tensor([[3, 9], [7, 16], [1, 2], [5, 12], [8, 16], [2, 16]], device=DEV)
    probs = torch.empty(P, 2, Lt, device=DEV)
    mix = torch.empty(P, 2, H, device=DEV)
    nat.span_pool_fwd(P, Lt, H, top, (Lt + 4) * H, score, sep, probs, mix)
    tf = top[:, :Lt].float().clone().requires_grad_(True)
    sf = score.clone().requires_grad_(True)
    pos = torch.arange(Lt, device=DEV)[None]
    m0 = ((pos >= 1) & (pos <= sep[:, :1])).float()
    m1 = ((pos > sep[:, :1]) & (pos <= sep[:, 1:])).float()
    sel = torch.stack([m0, m1], 1)
    a = torch.softmax(sel * sf[:, None] + (1 - sel) * -10000.0, -1)
    ref = a @ tf
    _close(mix, ref, dtype)
    dmix = torch.randn(P, 2, H, generator=g).to(DEV)
    dscore = torch.empty(P, Lt, device=DEV)
    dtop = torch.zeros_like(top)
    nat.span_pool_bwd(P, Lt, H, top, (Lt + 4) * H, probs, sep, dmix, dscore, dtop)
    rt, rs = torch.autograd.grad(ref, (tf, sf), dmix)
    _close(dtop[:, :Lt], rt, dtype)
    _close(dscore, rs, torch.float32, scale=5.0 if dtype == torch.float32 else 500.0)


def test_pointer_fwd_bwd():
    B, Nn, H = 3, 5, 64
    g = torch.Generator(device="cpu").manual_seed(2)
    q = torch.randn(B, Nn, H, generator=g).to(DEV)
    key = torch.randn(B, Nn, Nn, H, generator=g).to(DEV)
    okey = torch.randn(B, Nn, H, generator=g).to(DEV)
    w = torch.randn(H, generator=g).to(DEV) * 0.2
    wb = torch.tensor([0.3], device=DEV)
    target = torch.stack([torch.randperm(Nn, generator=g) for _ in range(B)]).to(DEV)
    tgt_len = torch.tensor([5, 4, 5], device=DEV)
    pointed = torch.zeros(B, Nn, Nn, dtype=torch.uint8)
    for b in range(B):
        for t in range(1, Nn):
            pointed[b, t] = pointed[b, t - 1]
            pointed[b, t, target[b, t - 1]] = 1
    pointed = pointed.to(DEV)
    logp = torch.empty(B, Nn, Nn, device=DEV)
    nll = torch.empty(B, Nn, device=DEV)
    nat.pointer_fwd(B, Nn, H, q, key, okey, w, wb, pointed, tgt_len, target, logp, nll)
    qf, kf, of, wf = (t.clone().requires_grad_(True) for t in (q, key, okey, w))
    e = torch.tanh(qf[:, :, None] + kf + of[:, None]) @ wf + wb
    valid = torch.arange(Nn, device=DEV)[None] < tgt_len[:, None]
    e = e.masked_fill(pointed == 1, -1e9).masked_fill(~valid[:, None, :], -1e9)
    lp = torch.log_softmax(e, -1)
    rn = -lp.gather(-1, target[:, :, None]).squeeze(-1) * valid
    torch.testing.assert_close(logp, lp, rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(nll, rn, rtol=1e-5, atol=1e-5)
    dn = torch.randn(B, Nn, generator=g).to(DEV)
    dq, dkey = torch.empty_like(q), torch.empty_like(key)
    dok, dw, dwb = torch.zeros_like(okey), torch.zeros_like(w), torch.zeros(1, device=DEV)
    nat.pointer_bwd(B, Nn, H, q, key, okey, w, logp, pointed, tgt_len, target, dn, dq, dkey, dok, dw,
                    dwb)
    rq, rk, ro, rw = torch.autograd.grad(rn, (qf, kf, of, wf), dn)
    for a_, b_ in ((dq, rq), (dkey, rk), (dok, ro), (dw, rw)):
        torch.testing.assert_close(a_, b_, rtol=1e-4, atol=1e-5)


def test_adamw_matches_torch():
    n = 10000
    g = torch.Generator(device="cpu").manual_seed(4)
    p = torch.randn(n, generator=g).to(DEV)
    grad = torch.randn(n, generator=g).to(DEV)
    m = torch.zeros(n, device=DEV)
    v = torch.zeros(n, device=DEV)
    ss = torch.empty(1, device=DEV)
    nat.sumsq(grad, ss)
    torch.testing.assert_close(ss[0], (grad ** 2).sum(), rtol=1e-5, atol=1e-3)
    # transformers-3.4 AdamW (trainers/train.py:185): eps added to sqrt(v) BEFORE bias correction,
    # step = lr * sqrt(1 - b2^t) / (1 - b1^t); decoupled decay p -= lr * wd * p after the update
    pr, mr, vr = p.double().clone(), torch.zeros(n, dtype=torch.float64, device=DEV), \
        torch.zeros(n, dtype=torch.float64, device=DEV)
    shadow = torch.empty(n, device=DEV, dtype=torch.bfloat16)
    lr, wd = 1e-3, 0.01
    for step in range(1, 4):
        nat.adamw(p, grad, m, v, None, lr, 0.9, 0.999, 1e-8, wd, step, 1.0, ss, shadow)
        gr = grad.double() * min(1.0, 1.0 / (ss[0].double().sqrt().item() + 1e-6))
        mr = 0.9 * mr + 0.1 * gr
        vr = 0.999 * vr + 0.001 * gr * gr
        st = lr * math.sqrt(1 - 0.999 ** step) / (1 - 0.9 ** step)
        pr = pr - st * mr / (vr.sqrt() + 1e-8)
        pr = pr - lr * wd * pr
    torch.testing.assert_close(p, pr.float(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(shadow.float(), p.bfloat16().float())


def test_colsum_and_cast():
    x = torch.randn(1000, 300, device=DEV).bfloat16()
    out = torch.ones(300, device=DEV)
    nat.colsum(x, 1000, 300, 300, out, accumulate=True)
    torch.testing.assert_close(out, x.float().sum(0) + 1, rtol=1e-4, atol=1e-3)
    w = torch.randn(70, 130, device=DEV)
    wt = torch.empty(130, 70, device=DEV, dtype=torch.bfloat16)
    nat.transpose_cast(w, wt)
    torch.testing.assert_close(wt, w.t().bfloat16())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_embed_ln_fwd_bwd(dtype):
    P, Lt, Tv, H, V = 4, 9, 5, 128, 50
    T = Lt + Tv
    g = torch.Generator(device="cpu").manual_seed(5)
    ids = torch.randint(0, V, (P, Lt), generator=g).to(DEV)
    ids[0, :3] = 0
    tt = torch.zeros(P, Lt, dtype=torch.long, device=DEV)
    word = torch.randn(V, H, generator=g).to(DEV)
    pos = torch.randn(20, H, generator=g).to(DEV)
    typ = torch.randn(1, H, generator=g).to(DEV)
    gam = (1 + 0.1 * torch.randn(H, generator=g)).to(DEV)
    bet = (0.1 * torch.randn(H, generator=g)).to(DEV)
    joint = torch.zeros(P, T, H, device=DEV, dtype=dtype)
    mean = torch.empty(P * Lt, device=DEV)
    rstd = torch.empty(P * Lt, device=DEV)
    nat.embed_ln_fwd(P, Lt, H, ids, tt, word, pos, typ, gam, bet, 1e-12, joint, T * H, mean, rstd)
    w_, p_, t_, g_, b_ = (x.clone().requires_grad_(True) for x in (word, pos, typ, gam, bet))
    posid = torch.arange(Lt, device=DEV)[None].expand(P, Lt)
    e = (torch.nn.functional.embedding(ids, w_, padding_idx=0)
         + torch.nn.functional.embedding(posid, p_, padding_idx=0)
         + torch.nn.functional.embedding(tt, t_, padding_idx=0))
    ref = torch.nn.functional.layer_norm(e, (H,), g_, b_, 1e-12)
    _close(joint[:, :Lt], ref, dtype)
    dj = torch.randn(P, T, H, generator=g).to(DEV, dtype)
    dw, dp, dty = torch.zeros_like(word), torch.zeros_like(pos), torch.zeros_like(typ)
    dg, db = torch.zeros_like(gam), torch.zeros_like(bet)
    nat.embed_ln_bwd(P, Lt, H, ids, tt, word, pos, typ, gam, mean, rstd, dj, T * H, dw, dp, dty,
                     dg, db)
    rw, rp, rt, rg, rb = torch.autograd.grad(ref, (w_, p_, t_, g_, b_), dj[:, :Lt].float())
    for a_, b2 in ((dw, rw), (dp, rp), (dty, rt), (dg, rg), (db, rb)):
        _close(a_, b2, torch.float32, scale=10.0 if dtype == torch.float32 else 300.0)
    assert dw.abs().sum() > 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_embed_table_grad_fixed_order(dtype):
    """The word / token-type table gradients in a fixed order (rows grouped by id, summed in row
    order; no float atomics): ids 1 and 2 make runs that cross many 64-row chunks of the sorted
    order, most other ids occur once, id 0 (padding_idx) never gets a gradient, type id 1 does;
    equal to a float64 index_add and bitwise equal across calls."""
    P, Lt, Tv, H = 64, 40, 3, 256
    T = Lt + Tv
    g = torch.Generator(device="cpu").manual_seed(11)
    V = 3000
    ids = torch.randint(3, V, (P, Lt), generator=g)
    ids[torch.rand(P, Lt, generator=g) < 0.3] = 1
    ids[torch.rand(P, Lt, generator=g) < 0.2] = 2
    ids[torch.rand(P, Lt, generator=g) < 0.05] = 0
    ids = ids.to(DEV)
    tt = (torch.rand(P, Lt, generator=g) < 0.5).long().to(DEV)
    word = torch.randn(V, H, generator=g).to(DEV)
    pos = torch.randn(Lt, H, generator=g).to(DEV)
    typ = torch.randn(2, H, generator=g).to(DEV)
    gam = (1 + 0.1 * torch.randn(H, generator=g)).to(DEV)
    bet = (0.1 * torch.randn(H, generator=g)).to(DEV)
    joint = torch.zeros(P, T, H, device=DEV, dtype=dtype)
    mean = torch.empty(P * Lt, device=DEV)
    rstd = torch.empty(P * Lt, device=DEV)
    nat.embed_ln_fwd(P, Lt, H, ids, tt, word, pos, typ, gam, bet, 1e-12, joint, T * H, mean, rstd)
    dj = torch.randn(P, T, H, generator=g).to(DEV, dtype)
    runs = []
    for _ in range(2):
        dw, dp, dty = torch.zeros_like(word), torch.zeros_like(pos), torch.zeros_like(typ)
        dg, db = torch.zeros_like(gam), torch.zeros_like(bet)
        nat.embed_ln_bwd(P, Lt, H, ids, tt, word, pos, typ, gam, mean, rstd, dj, T * H, dw, dp, dty,
                         dg, db)
        runs.append((dw, dty))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    w_, t_ = word.double().requires_grad_(True), typ.double().requires_grad_(True)
    posid = torch.arange(Lt, device=DEV)[None].expand(P, Lt)
    e = (torch.nn.functional.embedding(ids, w_, padding_idx=0)
         + torch.nn.functional.embedding(posid, pos.double(), padding_idx=0)
         + torch.nn.functional.embedding(tt, t_, padding_idx=0))
    ref = torch.nn.functional.layer_norm(e, (H,), gam.double(), bet.double(), 1e-12)
    rw, rt = torch.autograd.grad(ref, (w_, t_), dj[:, :Lt].double())
    dw, dty = runs[0]
    assert not dw[0].any() and not dty[0].any()  # padding_idx rows
    tol = dict(rtol=1e-5, atol=1e-4) if dtype == torch.float32 else dict(rtol=2e-2, atol=5e-2)
    torch.testing.assert_close(dw.double(), rw, **tol)
    torch.testing.assert_close(dty.double(), rt, **tol)
    assert dw[1].abs().sum() > 0 and dty[1].abs().sum() > 0


@pytest.mark.parametrize("dtype,W", [(torch.float32, 64), (torch.bfloat16, 64), (torch.bfloat16, 768),
                                     (torch.bfloat16, 1024)])
def test_vit_im2col_embed_fwd_bwd(dtype, W):
    """W = 64: the generic kernels; bf16 with W % 256 == 0: the 16-byte half-wave kernels and dpos /
    dcls from column sums over the pairs (config 3 / 5 widths)."""
    B, Nst, R, ps = 2, 3, 32, 8
    g = torch.Generator(device="cpu").manual_seed(6)
    images = torch.randn(B, Nst, 3, R, R, generator=g).to(DEV)
    pairs = torch.tensor([[[0, 1], [2, 0]], [[1, 2], [2, 1]]], device=DEV)
    npair = 2
    P = B * npair
    gg = (R // ps) ** 2
    ntok = 1 + 2 * gg
    patches = torch.empty(P * 2 * gg, 3 * ps * ps, device=DEV, dtype=dtype)
    nat.vit_im2col(B, Nst, npair, R, ps, images, pairs, patches)
    imgs = images[torch.arange(B)[:, None, None].to(DEV), pairs].reshape(P * 2, 3, R, R)
    ref_p = torch.nn.functional.unfold(imgs, ps, stride=ps).transpose(1, 2).reshape(P * 2 * gg, -1)
    _close(patches, ref_p, dtype)
    po = torch.randn(P * 2 * gg, W, generator=g).to(DEV, dtype)
    cls = torch.randn(W, generator=g).to(DEV)
    pos = torch.randn(gg + 1, W, generator=g).to(DEV)
    gam = (1 + 0.1 * torch.randn(W, generator=g)).to(DEV)
    bet = (0.1 * torch.randn(W, generator=g)).to(DEV)
    x = torch.empty(P * ntok, W, device=DEV, dtype=dtype)
    y = torch.empty_like(x)
    mean = torch.empty(P * ntok, device=DEV)
    rstd = torch.empty_like(mean)
    nat.vit_embed_fwd(P, ntok, W, gg, po, cls, pos, gam, bet, 1e-5, x, y, mean, rstd)
    po_, c_, p_, g_, b_ = (t.float().clone().requires_grad_(True) for t in (po, cls, pos, gam, bet))
    xx = torch.cat([c_.expand(P, 1, W), po_.view(P, 2 * gg, W)], 1)
    pe = torch.cat([p_, p_[:gg]], 0)
    ref = torch.nn.functional.layer_norm(xx + pe, (W,), g_, b_, 1e-5)
    _close(y.view(P, ntok, W), ref, dtype, scale=2.0)
    dy = torch.randn(P * ntok, W, generator=g).to(DEV, dtype)
    dpo = torch.empty_like(po)
    dcls, dpos = torch.zeros_like(cls), torch.zeros_like(pos)
    dg, db = torch.zeros_like(gam), torch.zeros_like(bet)
    nat.vit_embed_bwd(P, ntok, W, gg, dy, x, mean, rstd, gam, dpo, dcls, dpos, dg, db)
    r = torch.autograd.grad(ref, (po_, c_, p_, g_, b_), dy.float().view(P, ntok, W))
    _close(dpo, r[0], dtype, scale=2.0)
    for a_, b2 in ((dcls, r[1]), (dpos, r[2]), (dg, r[3]), (db, r[4])):
        _close(a_, b2, torch.float32, scale=10.0 if dtype == torch.float32 else 300.0)


@pytest.mark.parametrize("M,Nn,K", [(33000 + 77, 1024, 256), (256 * 3 + 5, 768, 768),
                                    (2048, 2304, 128), (164160 // 8, 768, 3072)])
@pytest.mark.parametrize("epi", ["plain", "gelu_aux", "qgelu_aux", "drop_resid", "dgelu", "dqgelu",
                                 "accum"])
@pytest.mark.parametrize("variant", [4, 5, 6])
def test_gemm256_persistent(M, Nn, K, epi, variant):
    """Persistent 256x256 NT kernel (mode 4 forces it) vs the fp32 reference, and bit-for-bit
    the same dropout mask as the 128x128 path (mode 2) on the same descriptor."""
    g = torch.Generator(device="cpu").manual_seed(M + Nn + K)
    A = torch.randn(M, K, generator=g).to(DEV, torch.bfloat16)
    W = (torch.randn(Nn, K, generator=g) * 0.1).to(DEV, torch.bfloat16)
    bias = torch.randn(Nn, generator=g).to(DEV)
    resid = torch.randn(M, Nn, generator=g).to(DEV, torch.bfloat16)
    z_in = torch.randn(M, Nn, generator=g).to(DEV, torch.bfloat16)
    c0 = torch.randn(M, Nn, generator=g).to(DEV, torch.bfloat16)
    drop = nat.drop(0.1, 77, 1234) if epi == "drop_resid" else None
    act = {"gelu_aux": 1, "qgelu_aux": 2, "dgelu": 1, "dqgelu": 2}.get(epi, 0)
    outs = []
    for mode in (variant, 2):
        nat.gemm_set_fast(mode)
        C = c0.clone()
        aux = torch.empty_like(C) if epi.endswith("aux") else None
        nat.gemm(A, W, C, M, Nn, K, bias=bias if epi in ("gelu_aux", "qgelu_aux", "drop_resid") else None,
                 act=act, aux=aux, dact=z_in if epi.startswith("d") and epi != "drop_resid" else None,
                 resid=resid if epi == "drop_resid" else None, accumulate=epi == "accum", drop=drop)
        outs.append((C, aux))
    torch.cuda.synchronize()
    z = A.float() @ W.float().t()
    acts = {1: torch.nn.functional.gelu, 2: lambda x: x * torch.sigmoid(1.702 * x)}
    if epi == "plain":
        ref = z
    elif epi.endswith("aux"):
        z = z + bias
        ref = acts[act](z)
        _close(outs[0][1], z, torch.bfloat16, scale=4.0)
    elif epi == "drop_resid":
        ref = None
    elif epi == "accum":
        ref = z + c0.float()
    else:
        zz = z_in.float().requires_grad_(True)
        gz = torch.autograd.grad(acts[act](zz).sum(), zz)[0]
        ref = z * gz
    if ref is not None:
        _close(outs[0][0], ref, torch.bfloat16, scale=4.0)
    # identical epilogue math on both paths: at most one bf16 ulp apart (accumulation order)
    d = (outs[0][0].float() - outs[1][0].float()).abs()
    tol = 2e-2 * outs[1][0].float().abs() + 2e-2 * math.sqrt(K) / 8
    assert bool((d <= tol).all()), f"max diff {d.max().item()}"
    if drop is not None:
        # the dropped positions (== resid exactly) coincide
        m4 = outs[0][0] == resid
        m2 = outs[1][0] == resid
        assert (m4 != m2).float().mean().item() < 1e-4


@pytest.mark.parametrize("M,Nn,K", [(33000 + 77, 1024, 256), (256 * 3 + 5, 768, 768),
                                    (2048, 2304, 128), (70001, 768, 384), (4096, 3072, 768)])
@pytest.mark.parametrize("epi", ["plain", "gelu_aux", "qgelu_aux", "gelu", "drop_resid", "resid",
                                 "drop", "dgelu", "dqgelu", "accum"])
def test_gemm_pingpong_equals_8wave(M, Nn, K, epi):
    """The ping-pong NT kernel (MMSEQ_GEMM_PINGPONG: two 4-wave groups on 256 x 128 tiles) runs
    the same 16x16x32 MFMA sequence per output as the 8-wave 256 x 256 kernel and the same
    epilogue math: outputs (and the GELU pre-activation) bit for bit equal, edge tiles included."""
    g = torch.Generator(device="cpu").manual_seed(M * 7 + Nn + K)
    A = torch.randn(M, K, generator=g).to(DEV, torch.bfloat16)
    W = (torch.randn(Nn, K, generator=g) * 0.1).to(DEV, torch.bfloat16)
    bias = torch.randn(Nn, generator=g).to(DEV)
    resid = torch.randn(M, Nn, generator=g).to(DEV, torch.bfloat16)
    z_in = torch.randn(M, Nn, generator=g).to(DEV, torch.bfloat16)
    c0 = torch.randn(M, Nn, generator=g).to(DEV, torch.bfloat16)
    drop = nat.drop(0.1, 77, 1234) if epi.startswith("drop") else None
    act = {"gelu_aux": 1, "qgelu_aux": 2, "gelu": 1, "dgelu": 1, "dqgelu": 2}.get(epi, 0)
    outs = []
    for mode in (6, 4):
        nat.gemm_set_fast(mode)
        C = c0.clone()
        aux = torch.full_like(C, 3.0) if epi.endswith("aux") else None
        nat.gemm(A, W, C, M, Nn, K, bias=bias if epi not in ("plain", "accum", "dgelu", "dqgelu") else None,
                 act=act, aux=aux, dact=z_in if epi in ("dgelu", "dqgelu") else None,
                 resid=resid if epi.endswith("resid") else None, accumulate=epi == "accum", drop=drop)
        outs.append((C, aux))
    nat.gemm_set_fast(1)
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]), float((outs[0][0].float() - outs[1][0].float()).abs().max())
    if outs[0][1] is not None:
        assert torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("trans,M,N,K", [(1, 1, 768, 38400), (1, 768, 768, 38400), (1, 130, 96, 5000),
                                         (0, 100, 768, 4096), (0, 3, 5, 2049)])
def test_gemm_fp32_splitk(trans, M, N, K):
    """Skinny fp32 GEMMs with a long K take the split-K generic path (slabs + ordered reduce)."""
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    if trans:
        A = torch.randn(K, M, generator=g).to(DEV)
        B = torch.randn(K, N, generator=g).to(DEV)
        ref0 = A.t() @ B
    else:
        A = torch.randn(M, K, generator=g).to(DEV)
        B = torch.randn(N, K, generator=g).to(DEV)
        ref0 = A @ B.t()
    C0 = torch.randn(M, N, generator=g).to(DEV)
    C = C0.clone()
    nat.gemm(A, B, C, M, N, K, trans=trans, accumulate=True)
    C2 = C0.clone()
    nat.gemm(A, B, C2, M, N, K, trans=trans, accumulate=True)
    assert torch.equal(C, C2)  # fixed-order reduction: bitwise reproducible
    ref = C0.double() + (A.double().t() @ B.double() if trans else A.double() @ B.double().t())
    err = (C.double() - ref).abs().max().item()
    assert err <= 1e-5 * math.sqrt(K) * (1 + ref.abs().max().item()) / 8, err


@pytest.mark.parametrize("M,N,K", [(80, 768, 768), (16, 3072, 768), (80, 768, 3072), (400, 3080, 768),
                                   (7, 36, 300)])
@pytest.mark.parametrize("epi", ["bias_gelu_aux", "resid", "dact", "drop", "acc"])
def test_gemm_fp32_splitk_epilogue(M, N, K, epi):
    """fp32 GEMMs with few output tiles (the BERSON head) split K and apply the epilogue in the
    ordered reduction: same results as the unfused ops, bitwise reproducible."""
    g = torch.Generator(device="cpu").manual_seed(M * 7 + N + K)
    A = torch.randn(M, K, generator=g).to(DEV)
    B = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    R = torch.randn(M, N, generator=g).to(DEV)
    z = (A.double() @ B.double().t())
    outs = []
    for _ in range(2):
        C = R.clone() if epi == "acc" else torch.empty(M, N, device=DEV)
        aux = torch.empty(M, N, device=DEV)
        kw = {}
        if epi == "bias_gelu_aux":
            kw = dict(bias=bias, act=1, aux=aux)
        elif epi == "resid":
            kw = dict(bias=bias, resid=R)
        elif epi == "dact":
            kw = dict(act=1, dact=R)
        elif epi == "drop":
            kw = dict(bias=bias, drop=nat.drop(0.1, 11, 5))
        elif epi == "acc":
            kw = dict(accumulate=True)
        nat.gemm(A, B, C, M, N, K, **kw)
        outs.append((C, aux))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0])
    C, aux = outs[0]
    zb = z + bias.double()
    if epi == "bias_gelu_aux":
        ref = torch.nn.functional.gelu(zb)
        torch.testing.assert_close(aux.double(), zb, rtol=1e-5, atol=1e-5)
    elif epi == "resid":
        ref = zb + R.double()
    elif epi == "dact":
        x = R.double().requires_grad_(True)
        (gx,) = torch.autograd.grad(torch.nn.functional.gelu(x).sum(), x)
        ref = z * gx
    elif epi == "drop":
        y = torch.empty(M, N, device=DEV)
        nat.dropout(zb.float().contiguous(), y, nat.drop(0.1, 11, 5))  # same (seed, stream, index)
        ref = y.double()
    else:
        ref = z + R.double()
    torch.testing.assert_close(C.double(), ref, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("M,N,K", [(768, 3072, 20000), (2304, 768, 4100), (768, 768, 164), (40, 96, 300),
                                   (3072, 768, 1000)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_gemm_wgrad_fused_bias(M, N, K, dtype):
    """mmseq_gemm_wgrad: dW += dY^T X and db += colsum(dY) in one pass (split-K, fused column sums
    on the bf16 256x256 TN kernel; fallback path otherwise); deterministic."""
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    dY = torch.randn(K, M, generator=g).to(DEV, dtype)
    X = torch.randn(K, N, generator=g).to(DEV, dtype)
    W0 = torch.randn(M, N, generator=g).to(DEV)
    b0 = torch.randn(M, generator=g).to(DEV)
    outs = []
    for _ in range(2):
        gW, gb = W0.clone(), b0.clone()
        nat.gemm_wgrad(dY, X, gW, gb)
        outs.append((gW, gb))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    refW = W0.double() + dY.double().t() @ X.double()
    refb = b0.double() + dY.double().sum(0)
    tol = 1e-5 if dtype == torch.float32 else 1e-4
    errW = (outs[0][0].double() - refW).abs().max().item()
    errb = (outs[0][1].double() - refb).abs().max().item()
    assert errW <= tol * math.sqrt(K) * (1 + refW.abs().max().item()), errW
    assert errb <= tol * math.sqrt(K) * (1 + refb.abs().max().item()), errb


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("R,ps,ld", [(32, 8, 192), (32, 8, 256), (56, 14, 640), (28, 14, 588),
                                     (64, 32, 3072)])
def test_vit_im2col_any_patch_padded(dtype, R, ps, ld):
    """Patch gather for every ViT patch size (ViT-L/14: K = 588 padded to 640 for the GEMM,
    the pad columns zero)."""
    B, Nst = 2, 3
    g = torch.Generator(device="cpu").manual_seed(R + ps + ld)
    images = torch.randn(B, Nst, 3, R, R, generator=g).to(DEV)
    pairs = torch.tensor([[[0, 1], [2, 0]], [[1, 2], [2, 1]]], device=DEV)
    P = B * 2
    gg = (R // ps) ** 2
    K = 3 * ps * ps
    patches = torch.full((P * 2 * gg, ld), 7.0, device=DEV, dtype=dtype)
    nat.vit_im2col(B, Nst, 2, R, ps, images, pairs, patches)
    imgs = images[torch.arange(B)[:, None, None].to(DEV), pairs].reshape(P * 2, 3, R, R)
    ref_p = torch.nn.functional.unfold(imgs, ps, stride=ps).transpose(1, 2).reshape(P * 2 * gg, -1)
    _close(patches[:, :K], ref_p, dtype)
    if ld > K:
        assert float(patches[:, K:].abs().max()) == 0.0
