"""Every GEMM epilogue x activation on ALL of bf16: one single-tile GEMM pushes each of the 65 536
bf16 bit patterns through an epilogue as an exactly known pre-activation, and the result is held
to the error bound of the implementation that (variant, act, direction) is documented to use
(tests/act_curve_ref.py: `interval_ok` with the bounds re-derived in test_act_curve_ref.py).

  forward     M = N = K = 256, A = identity, B[n][k] = pattern n * 256 + k, no bias, alpha 1:
              z[m][n] = B[n][m] exactly (one non-zero term per sum), C = act(z); aux_out = z.
  derivative  A[m][0] = 2^((m mod 3) - 1), B[n][0] = 1, all else 0: the product is that power of
              two; dact = the pattern table, C[m][n] = A[m][0] * act'(pattern m * 256 + n), and E
              scales by the same power of two.

On D (finite, |x| <= 8192) the rule must hold; off D (|x| up to 3.4e38; the 256 Inf / NaN patterns
are replaced by 0) every result must be finite. Each test prints the smallest E its results need
(act_curve_ref.needed_E; DESIGN.md records the figures of an MI355X run).
"""
import numpy as np
import pytest
import torch

import act_curve_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import native_raw as raw
    from multimodal_sequencing_amd import _native as nat

DEV = "cuda"
F32, BF16 = 0, 1
GELU, QGELU, TANH, GTANH = R.GELU_ERF, R.QUICKGELU, R.TANH, R.GELU_TANH
TOL_F32 = 2e-5  # TOL[torch.float32] of test_kernels_gpu.py: |err| <= 2e-5 (1 + |ref|)

# (variant, act, direction) -> the implementation the source routes it to, for bf16 output
# (gemm.hip launch_fast / gemm_common.h epilogue4; gemm256.hip epi8 and mmseq_gemm256_nt):
#   "as"    act_fwd_fast / act_bwd_fast, GELU: Abramowitz-Stegun erf      (common.h)
#   "rcp"   act_fwd_fast / act_bwd_fast, QuickGELU: x * rcp(1 + exp)      (common.h)
#   "sig"   gelu_sig8 forward, gelu_sig_grad derivative                   (common.h)
#   "table" the LDS derivative table dtab_fill / dtab_index               (gemm256.hip)
#   "libm"  act_fwd / act_bwd                                             (common.h)
# Variants 0 (generic), 1 (auto: one 256 x 256 tile stays on the 128 x 128 kernel) and 3 (ring) end
# in epilogue4; 4 (gemm256_nt_kernel) and 6 (gemm_pp_kernel) use gelu_sig8 forward and the table
# backward; 5 (gemm_nt_2b_kernel) has no table. A change of routing has to change this table.
IMPL = {}
for _v in (0, 1, 3):
    for _d in ("fwd", "bwd"):
        IMPL[(_v, GELU, _d)] = "as"
        IMPL[(_v, QGELU, _d)] = "rcp"
        IMPL[(_v, TANH, _d)] = "libm"
        IMPL[(_v, GTANH, _d)] = "libm"
for _v in (4, 6):
    IMPL[(_v, GELU, "fwd")] = "sig"
    IMPL[(_v, QGELU, "fwd")] = "rcp"
    IMPL[(_v, GELU, "bwd")] = "table"
    IMPL[(_v, QGELU, "bwd")] = "table"
IMPL[(5, GELU, "fwd")] = "sig"
IMPL[(5, GELU, "bwd")] = "sig"
IMPL[(5, QGELU, "fwd")] = "rcp"
IMPL[(5, QGELU, "bwd")] = "rcp"
CASES = sorted(k[:2] for k in IMPL if k[2] == "fwd")  # 6 x 2 + 3 x 2 (variant, act)

BITS, REPLACED = R.all_bf16()         # [n][k] = pattern n * 256 + k
X = R.bits_to_f64(BITS)
FINITE = ~REPLACED
IN_D = R.domain(X) & FINITE
ROWSCALE = np.ldexp(1.0, (np.arange(256) % 3) - 1)[:, None]  # A[m][0] of the derivative form

_ref_cache = {}


def ref64(act, direction):
    """act(X) / act'(X) in float64, computed once per (act, direction)."""
    k = (act, direction)
    if k not in _ref_cache:
        _ref_cache[k] = (R.act64 if direction == "fwd" else R.dact64)(act, X)
    return _ref_cache[k]


def _dev_bf16(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(DEV).view(torch.bfloat16)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


_tensors = {}


def T(name):
    """Device operands shared by the tests (built once, never written)."""
    if not _tensors:
        eye = torch.eye(256)
        col = torch.zeros(256, 256)
        col[:, 0] = 1.0
        a_pow = torch.zeros(256, 256, dtype=torch.float64)
        a_pow[:, 0] = torch.from_numpy(ROWSCALE[:, 0])
        tab = _dev_bf16(BITS)
        _tensors.update(
            eye=eye.to(DEV, torch.bfloat16), eye32=eye.to(DEV), col=col.to(DEV, torch.bfloat16),
            col32=col.to(DEV), apow=a_pow.to(DEV, torch.bfloat16), apow32=a_pow.float().to(DEV),
            tab=tab, tab32=tab.float(), zeros=torch.zeros(256, 256, device=DEV, dtype=torch.bfloat16),
            zeros32=torch.zeros(256, 256, device=DEV))
    return _tensors[name]


def _gemm(A, B, C, act, variant, code, aux=None, dact=None, resid=None, ws=None):
    p = raw.p
    raw.call("mmseq_gemm", 0, 256, 256, 256, 1, p(A), 256, 0, p(B), 256, 0, p(C), 256, 0, None, act,
             p(aux), p(dact), p(resid), 256, 0, 1.0, 0, code, code, None, variant, p(ws),
             0 if ws is None else ws.numel() * 4)


def check_bf16(got_bits, ref, impl_key, what, scale=1.0, x=X, in_d=IN_D, finite=FINITE):
    """interval_ok on D with E[impl_key] * scale, finiteness wherever the input is finite; prints
    the smallest E (per unit of scale) that the results need."""
    got = R.bits_to_f64(got_bits)
    assert np.isfinite(got[finite]).all(), \
        f"{what}: non-finite result for the finite input {x[finite & ~np.isfinite(got)][0]!r}"
    E = R.E[impl_key]
    need = np.where(in_d, R.needed_E(got, ref) / scale, 0.0)
    i = np.unravel_index(int(need.argmax()), need.shape)
    print(f"[act-curve] {what}: bound {impl_key[0]} E = {E:.4g}; needs E >= {need[i]:.4g} "
          f"(at x = {x[i]!r})")
    bad = in_d & ~R.interval_ok(got, ref, E * scale)
    assert not bad.any(), (
        f"{what}: {int(bad.sum())} inputs outside rne_bf16(ref -+ {E:.4g}); worst x = {x[i]!r}: "
        f"got {got[i]!r}, exact {ref[i]!r}, needs E = {need[i]:.4g}")


def check_aux(aux_bits, z, what):
    aux = R.bits_to_f64(aux_bits)
    same = aux == z  # as floats: -0 counts as +0, a NaN never equals
    assert same.all(), f"{what}: aux_out differs from the pre-activation at z = {z[~same][0]!r}"


# =================================================================================================
# mmseq_gemm, bf16
# =================================================================================================
@pytest.mark.parametrize("mode", ["plain", "aux", "resid"])
@pytest.mark.parametrize("variant,act", CASES)
def test_gemm_bf16_forward_curve(variant, act, mode):
    """mode resid: a residual of zeros (the operand-reading XIN instantiations of the 256-wide
    kernels)."""
    C = torch.full((256, 256), float("nan"), device=DEV, dtype=torch.bfloat16)
    aux = torch.full_like(C, float("nan")) if mode == "aux" else None
    _gemm(T("eye"), T("tab"), C, act, variant, BF16, aux=aux,
          resid=T("zeros") if mode == "resid" else None)
    torch.cuda.synchronize()
    key = (IMPL[(variant, act, "fwd")], act, "fwd")
    what = f"gemm bf16 variant {variant} {R.ACT_NAMES[act]} forward ({mode})"
    # C[m][n] = act(z[m][n]), z[m][n] = B[n][m]: transpose back to the pattern table's order
    check_bf16(_bits(C).T, ref64(act, "fwd"), key, what)
    if aux is not None:
        check_aux(_bits(aux).T, X, what)


@pytest.mark.parametrize("variant,act", CASES)
def test_gemm_bf16_derivative_curve(variant, act):
    C = torch.full((256, 256), float("nan"), device=DEV, dtype=torch.bfloat16)
    _gemm(T("apow"), T("col"), C, act, variant, BF16, dact=T("tab"))
    torch.cuda.synchronize()
    key = (IMPL[(variant, act, "bwd")], act, "bwd")
    check_bf16(_bits(C), ROWSCALE * ref64(act, "bwd"), key,
               f"gemm bf16 variant {variant} {R.ACT_NAMES[act]} derivative", scale=ROWSCALE)


# =================================================================================================
# mmseq_gemm, fp32 in / out (libm act_fwd / act_bwd), the pattern table widened to fp32
# =================================================================================================
def check_f32(got, ref, what, scale=1.0):
    got = got.double().cpu().numpy()
    assert np.isfinite(got[FINITE]).all(), f"{what}: non-finite result for a finite input"
    err = np.where(IN_D, np.abs(got - ref) / (1.0 + np.abs(ref)) / scale, 0.0)
    i = np.unravel_index(int(err.argmax()), err.shape)
    print(f"[act-curve] {what}: max |err| / (1 + |ref|) = {err[i]:.4g} (at x = {X[i]!r}); "
          f"bound {TOL_F32:.1g}")
    assert err[i] <= TOL_F32, f"{what}: x = {X[i]!r}: got {got[i]!r}, exact {ref[i]!r}"


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("act", [GELU, QGELU, TANH, GTANH])
@pytest.mark.parametrize("variant", [0, 1])
def test_gemm_f32_curve(variant, act, direction):
    """variant 1 is given a split-K workspace (the fixed-order reduction then applies the
    epilogue, splitk_epi_kernel), variant 0 none (the GEMM kernel's own epilogue)."""
    ws = None
    if variant == 1:
        nbytes = nat.lib().mmseq_gemm_workspace_size(256, 256, 256)
        ws = torch.full((max(nbytes // 4, 4),), float("nan"), device=DEV)
    C = torch.full((256, 256), float("nan"), device=DEV)
    what = f"gemm fp32 variant {variant} {R.ACT_NAMES[act]} {direction}"
    if direction == "fwd":
        aux = torch.full_like(C, float("nan"))
        _gemm(T("eye32"), T("tab32"), C, act, variant, F32, aux=aux, ws=ws)
        torch.cuda.synchronize()
        check_f32(C.t(), ref64(act, "fwd"), what)
        same = aux.t().double().cpu().numpy() == X
        assert same.all(), f"{what}: aux_out differs from the pre-activation at {X[~same][0]!r}"
    else:
        _gemm(T("apow32"), T("col32"), C, act, variant, F32, dact=T("tab32"), ws=ws)
        torch.cuda.synchronize()
        check_f32(C, ROWSCALE * ref64(act, "bwd"), what, scale=ROWSCALE)


# =================================================================================================
# mmseq_act_fwd / mmseq_act_bwd (elementwise, libm), n = 65 536
# =================================================================================================
@pytest.mark.parametrize("act", [GELU, QGELU, TANH, GTANH])
@pytest.mark.parametrize("code", [BF16, F32])
def test_act_fwd_bwd_curve(code, act):
    x = T("tab") if code == BF16 else T("tab32")
    dy = (T("apow")[:, :1] if code == BF16 else T("apow32")[:, :1]).expand(256, 256).contiguous()
    y = torch.full_like(x, float("nan"))
    dz = torch.full_like(x, float("nan"))
    nat.act_fwd(x, y, act)
    nat.act_bwd(x, dy, dz, act)
    torch.cuda.synchronize()
    name = f"act_{{}} {'bf16' if code == BF16 else 'fp32'} {R.ACT_NAMES[act]}"
    if code == BF16:
        check_bf16(_bits(y), ref64(act, "fwd"), ("libm", act, "fwd"), name.format("fwd"))
        check_bf16(_bits(dz), ROWSCALE * ref64(act, "bwd"), ("libm", act, "bwd"),
                   name.format("bwd"), scale=ROWSCALE)
    else:
        check_f32(y, ref64(act, "fwd"), name.format("fwd"))
        check_f32(dz, ROWSCALE * ref64(act, "bwd"), name.format("bwd"), scale=ROWSCALE)


# =================================================================================================
# mmseq_gemm_mxfp8_ex (the F8 instantiations of gemm256_nt_kernel), M = N = K = 256
# =================================================================================================
E4M3_ONE = 0x38
E8M0_ONE = 127


def _mx(first_col):
    """An MX-fp8 [256][256] operand with unit scales: e4m3 1.0 in the first K-element of every row
    (first_col) or all zero."""
    q = torch.zeros(256, 256, dtype=torch.uint8, device=DEV)
    if first_col:
        q[:, 0] = E4M3_ONE
    sc = torch.full((nat.lib().mmseq_mxfp8_scale_bytes(256, 256),), E8M0_ONE, dtype=torch.uint8,
                    device=DEV)
    return nat.MXFP8(q, sc, 256, 256)


@pytest.mark.parametrize("mode", ["aux", "resid", "q8"])
@pytest.mark.parametrize("act", [GELU, QGELU])
def test_gemm_mxfp8_forward_curve(act, mode):
    """A = 0, so the pre-activation is bias[n]: 256 patterns per call, and ALL 256 chunks of the
    pattern table are looped (the Inf / NaN slots hold 0), one call each. mode q8: the MX-fp8
    output's bf16 copy (epi8_q8)."""
    a, b = _mx(False), _mx(False)
    bias = T("tab32")
    got = torch.empty(256, 256, device=DEV, dtype=torch.bfloat16)
    auxs = torch.empty_like(got)
    c = torch.empty_like(got)
    aux = torch.empty_like(got) if mode in ("aux", "q8") else None
    rows_equal = torch.ones((), dtype=torch.bool, device=DEV)
    for r in range(256):
        c.fill_(float("nan"))
        nat.gemm_mxfp8_ex(a, b, c, bias=bias[r], act=act, aux=aux,
                          resid=T("zeros") if mode == "resid" else None, q8=mode == "q8")
        ci = c.view(torch.int16)
        rows_equal &= (ci == ci[:1]).all()
        got[r].copy_(c[0])
        if aux is not None:
            auxs[r].copy_(aux[0])
    torch.cuda.synchronize()
    assert bool(rows_equal), "rows of one call differ although every row has the same pre-activation"
    key = ("sig" if act == GELU else "rcp", act, "fwd")
    what = f"gemm_mxfp8_ex {R.ACT_NAMES[act]} forward ({mode})"
    check_bf16(_bits(got), ref64(act, "fwd"), key, what)
    if aux is not None:
        check_aux(_bits(auxs), X, what)


@pytest.mark.parametrize("q8", [False, True])
@pytest.mark.parametrize("act", [GELU, QGELU])
def test_gemm_mxfp8_derivative_curve(act, q8):
    """The first K-element of every row of A and B is e4m3 1.0 with unit scales: the product is 1
    and C = act'(dact) from the derivative table."""
    a, b = _mx(True), _mx(True)
    c = torch.full((256, 256), float("nan"), device=DEV, dtype=torch.bfloat16)
    nat.gemm_mxfp8_ex(a, b, c, act=act, dact=T("tab"), q8=q8)
    torch.cuda.synchronize()
    check_bf16(_bits(c), ref64(act, "bwd"), ("table", act, "bwd"),
               f"gemm_mxfp8_ex {R.ACT_NAMES[act]} derivative ({'q8' if q8 else 'bf16'})")
