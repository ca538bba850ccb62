"""The activation implementations of the bf16 GEMM epilogues (csrc/common.h, gemm256.hip),
emulated operation by operation in fp32 numpy over every bf16 input against float64: re-derives
the error bounds that tests/act_curve_ref.py stores for the GPU tests, and shows that the
acceptance rule `interval_ok` with those bounds rejects a coefficient moved by 1 % and a
derivative table indexed one binade off.

The emulation uses correctly rounded exp / exp2 / reciprocal where the GPU has 1-ulp v_exp_f32 /
v_rcp_f32 (hence the factor 1.25 in act_curve_ref.E) and a float64 product-sum rounded once for
fmaf.
"""
import numpy as np
import pytest

import act_curve_ref as R

f32 = np.float32
L2E = f32(1.4426950408889634)


def _fma(a, b, c):
    return (np.float64(a) * np.float64(b) + np.float64(c)).astype(f32)


def _exp(x):      # __expf
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(np.float64(x)).astype(f32)


def _exp2(x):     # __builtin_amdgcn_exp2f
    with np.errstate(over="ignore", under="ignore"):
        return np.exp2(np.float64(x)).astype(f32)


def _rcp(x):      # __builtin_amdgcn_rcpf
    with np.errstate(divide="ignore", over="ignore"):
        return (f32(1.0) / x).astype(f32)


# --- gelu_sig / gelu_sig8 / gelu_sig_grad --------------------------------------------------------
SIG_C = (1.59501577, 7.40112921e-2, -7.03033584e-4)


def emu_gelu_sig(x, c=SIG_C):
    x = x.astype(f32)
    k0, k1, k2 = (f32(-f32(ci) * L2E) for ci in c)
    xc = np.clip(x, f32(-9), f32(9))
    x2 = xc * xc
    q = xc * _fma(x2, _fma(x2, k2, k1), k0)
    return x * _rcp(f32(1) + _exp2(q))


def emu_gelu_sig_grad(x, c=SIG_C):
    x = x.astype(f32)
    c0, c1, c2 = (f32(ci) for ci in c)
    xc = np.clip(x, f32(-9), f32(9))
    x2 = xc * xc
    q = xc * _fma(x2, _fma(x2, f32(-c2 * L2E), f32(-c1 * L2E)), f32(-c0 * L2E))
    sg = _rcp(f32(1) + _exp2(q))
    dp = _fma(x2, _fma(x2, f32(5) * c2, f32(3) * c1), c0)
    return _fma(xc * _fma(-sg, sg, sg), dp, sg)


# --- act_fwd_fast / act_bwd_fast -----------------------------------------------------------------
AS_C = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)


def _erf_and_gauss(x, c=AS_C):
    ax = np.abs(x)
    t = _rcp(_fma(f32(0.3275911), ax, f32(1)))
    poly = _fma(f32(c[4]), t, f32(c[3]))
    poly = _fma(poly, t, f32(c[2]))
    poly = _fma(poly, t, f32(c[1]))
    poly = _fma(poly, t, f32(c[0]))
    poly = poly * t
    with np.errstate(over="ignore"):
        e = _exp(-ax * ax)
    return np.copysign(_fma(-poly, e, f32(1)), x), e


def emu_as_gelu(x, c=AS_C):
    x = x.astype(f32)
    er, _ = _erf_and_gauss(x * f32(0.70710678118654752), c)
    return f32(0.5) * x * (f32(1) + er)


def emu_as_dgelu(x, c=AS_C):
    x = x.astype(f32)
    er, e = _erf_and_gauss(x * f32(0.70710678118654752), c)
    return _fma(f32(0.39894228040143268) * x, e, f32(0.5) * (f32(1) + er))


def _sigmoid_rcp(x, k=1.702):
    with np.errstate(over="ignore"):
        return _rcp(f32(1) + _exp(f32(-k) * x))


def emu_rcp_qgelu(x, k=1.702):
    x = x.astype(f32)
    with np.errstate(invalid="ignore"):
        return x * _sigmoid_rcp(x, k)


def emu_rcp_dqgelu(x, k=1.702, old_order=False):
    x = x.astype(f32)
    s = _sigmoid_rcp(x, k)
    with np.errstate(over="ignore", invalid="ignore"):
        if old_order:  # the form before this test existed: ((1.702 x) s) (1 - s)
            return s + f32(k) * x * s * (f32(1) - s)
        return s + x * (f32(k) * (s * (f32(1) - s)))


# --- the LDS derivative table (gemm256.hip dtab_fill / dtab_index) --------------------------------
DT_LO = 117 << 7
DT_N = 13 * 128


def emu_table(act, bits, shift=0):
    """act'(z) as the dgrad epilogues read it: the table entry of the bf16 pattern, clamped to
    2^-10 <= |z| <= 7.96875. The entries are libm-exact (float64 rounded to fp32 here). `shift`
    moves the index by that many entries (128 = one binade) to show that the test sees it."""
    u = bits.astype(np.int64)
    a = np.clip((u & 0x7FFF) - DT_LO + shift, 0, DT_N - 1)
    entry = ((u >> 15) << 15) | (a + DT_LO)
    return R.dact64(act, R.bits_to_f64(entry)).astype(f32)


# --- the sweep ------------------------------------------------------------------------------------
BITS, REPLACED = R.all_bf16()
X = R.bits_to_f64(BITS)
IN_D = R.domain(X) & ~REPLACED
FINITE = ~REPLACED
X32 = X.astype(f32)


def _maxerr(got, ref):
    err = np.abs(np.float64(got) - ref)[IN_D]
    return float(err.max())


ROWS = [
    (("sig", R.GELU_ERF, "fwd"), lambda: emu_gelu_sig(X32)),
    (("sig", R.GELU_ERF, "bwd"), lambda: emu_gelu_sig_grad(X32)),
    (("as", R.GELU_ERF, "fwd"), lambda: emu_as_gelu(X32)),
    (("as", R.GELU_ERF, "bwd"), lambda: emu_as_dgelu(X32)),
    (("rcp", R.QUICKGELU, "fwd"), lambda: emu_rcp_qgelu(X32)),
    (("rcp", R.QUICKGELU, "bwd"), lambda: emu_rcp_dqgelu(X32)),
    (("table", R.GELU_ERF, "bwd"), lambda: emu_table(R.GELU_ERF, BITS)),
    (("table", R.QUICKGELU, "bwd"), lambda: emu_table(R.QUICKGELU, BITS)),
]


def _ref(key):
    return (R.act64 if key[2] == "fwd" else R.dact64)(key[1], X)


@pytest.mark.parametrize("key,emu", ROWS, ids=["-".join(map(str, k)) for k, _ in ROWS])
def test_emulated_bound_is_the_stored_one(key, emu):
    """The stored EMULATED[key] bounds the emulation's maximum error over D and is not slack,
    E[key] is 1.25 x that, the emulated values pass interval_ok with E[key] everywhere on D, and
    every finite input gives a finite output."""
    got = emu()
    err = _maxerr(got, _ref(key))
    at = float(X[IN_D][np.argmax(np.abs(np.float64(got) - _ref(key))[IN_D])])
    print(f"{key}: emulated max |err| on D = {err:.4g} at x = {at:.6g}; stored {R.EMULATED[key]:.4g}")
    # the stored figures carry two to four digits: not above the last printed digit, and within
    # 2 % below it, but for the A&S GELU' (this fma-faithful emulation: 2.28e-7; one without fma:
    # 2.68e-7; the stored 2.8e-7 is the figure the bound was set with)
    assert err <= 1.02 * R.EMULATED[key], (err, R.EMULATED[key])
    assert err >= (0.8 if key == ("as", R.GELU_ERF, "bwd") else 0.98) * R.EMULATED[key]
    assert R.E[key] == 1.25 * R.EMULATED[key]
    ok = R.interval_ok(R.rne_bf16(np.float64(got)), _ref(key), R.E[key])
    assert ok[IN_D].all()
    assert np.isfinite(got[FINITE]).all()


def test_quickgelu_derivative_old_order_overflows():
    """((1.702 x) s) (1 - s) is inf * 0 = NaN for finite |x| >~ 2e38; s (1 - s) first is finite."""
    old = emu_rcp_dqgelu(X32, old_order=True)
    assert np.isnan(old[FINITE]).any()
    assert np.isfinite(emu_rcp_dqgelu(X32)[FINITE]).all()


def _emu_dgelu_tanh(x, stable):
    """act_bwd(GELU_TANH) of csrc/common.h: `stable` is the form in the source (0.5 (1 + tanh u) and
    1 - tanh^2 u from exp(-2 |u|), x clamped to +-16), the other the textbook one with tanhf."""
    k, c = f32(0.79788456080286536), f32(0.044715)
    x = x.astype(f32)
    with np.errstate(all="ignore"):
        if not stable:
            u = k * (x + c * x * x * x)
            t = np.tanh(np.float64(u)).astype(f32)
            return (f32(0.5) * (f32(1) + t)
                    + f32(0.5) * x * (f32(1) - t * t) * k * (f32(1) + f32(3) * c * x * x))
        x = np.clip(x, f32(-16), f32(16))
        u = k * (x + c * x * x * x)
        e = _exp(f32(-2) * np.abs(u))
        r = _rcp(f32(1) + e)
        s = np.where(u >= 0, r, e * r)
        return s + f32(0.5) * x * (f32(4) * e * r * r) * k * (f32(1) + f32(3) * c * x * x)


def test_gelu_tanh_derivative_form():
    """1 - t * t with t = tanhf(u) cancels near |t| = 1 and the factor x k (1 + 3 c x^2) / 2 makes
    5.4e-7 of it at x = -5.16 (above E_LIBM, which an MI355X run showed too), and x * x overflows
    into 0 * inf = NaN from |x| ~ 1.8e19; the form in the source stays below E_LIBM and finite."""
    ref = R.dact64(R.GELU_TANH, X)
    old = _emu_dgelu_tanh(X32, False)
    new = _emu_dgelu_tanh(X32, True)
    assert _maxerr(old, ref) > R.E_LIBM and np.isnan(old[FINITE]).any()
    assert _maxerr(new, ref) < 0.5 * R.E_LIBM and np.isfinite(new[FINITE]).all()
    assert R.interval_ok(R.rne_bf16(np.float64(new)), ref, R.E_LIBM)[IN_D].all()
    assert not R.interval_ok(R.rne_bf16(np.float64(old)), ref, R.E_LIBM)[IN_D].all()


def test_rne_bf16_and_interval_rule():
    # every bf16 value is a fixed point; a value half a quantum up goes to the even neighbour
    assert np.array_equal(R.rne_bf16(X[FINITE]), X[FINITE])
    assert R.rne_bf16(1.0 + 2.0 ** -8) == 1.0              # tie -> even (1.0)
    assert R.rne_bf16(1.0 + 3 * 2.0 ** -8) == 1.0 + 2.0 ** -6  # tie -> even
    assert R.rne_bf16(1.0 + 2.0 ** -8 + 2.0 ** -30) == 1.0 + 2.0 ** -7
    assert R.rne_bf16(2.0 ** -133 * 0.49) == 0.0 and R.rne_bf16(2.0 ** -133 * 0.51) == 2.0 ** -133
    assert np.isinf(R.rne_bf16(3.4e38)) and R.rne_bf16(3.39e38) == R.bits_to_f64(0x7F7F)
    # E = 0 demands the correctly rounded value, -0 counts as +0, NaN never passes
    assert R.interval_ok(1.0, 1.001, 0.0) and not R.interval_ok(1.0 + 2.0 ** -7, 1.001, 0.0)
    assert R.interval_ok(-0.0, 0.0, 0.0) and R.interval_ok(0.0, -1e-50, 0.0)
    assert not R.interval_ok(np.nan, 0.0, 1.0)
    # E widens by exactly what it says: 1.0039 rounds to 1 + 2^-7 only once ref + E passes the tie
    tie = 1.0 + 2.0 ** -8
    assert not R.interval_ok(1.0 + 2.0 ** -7, tie - 3e-5, 2e-5)
    assert R.interval_ok(1.0 + 2.0 ** -7, tie - 1e-5, 2e-5)
    # needed_E is the E at which the rule starts to accept
    for got, ref in ((1.0 + 2.0 ** -7, tie - 3e-5), (1.0, tie + 1e-4), (1.0, 1.001)):
        e = float(R.needed_E(got, ref))
        assert R.interval_ok(got, ref, e * 1.0001 + 1e-300)
        assert e == 0.0 or not R.interval_ok(got, ref, e * 0.999)


def test_all_bf16_table():
    assert BITS.shape == (256, 256) and int(REPLACED.sum()) == 256
    n, k = 0x3F, 0x80
    assert BITS[n, k] == 0x3F80 and X[n, k] == 1.0
    assert not np.isfinite(R.bits_to_f64(np.arange(65536)[REPLACED.ravel()])).any()
    assert (BITS[REPLACED] == 0).all() and np.isfinite(X).all()


MUTATIONS = [
    ("sig fwd c0 +1%", ("sig", R.GELU_ERF, "fwd"),
     lambda: emu_gelu_sig(X32, (SIG_C[0] * 1.01,) + SIG_C[1:])),
    ("sig fwd c1 +1%", ("sig", R.GELU_ERF, "fwd"),
     lambda: emu_gelu_sig(X32, (SIG_C[0], SIG_C[1] * 1.01, SIG_C[2]))),
    ("sig bwd c0 +1%", ("sig", R.GELU_ERF, "bwd"),
     lambda: emu_gelu_sig_grad(X32, (SIG_C[0] * 1.01,) + SIG_C[1:])),
    ("A&S fwd a1 +1%", ("as", R.GELU_ERF, "fwd"),
     lambda: emu_as_gelu(X32, (AS_C[0] * 1.01,) + AS_C[1:])),
    ("A&S bwd a5 +1%", ("as", R.GELU_ERF, "bwd"),
     lambda: emu_as_dgelu(X32, AS_C[:4] + (AS_C[4] * 1.01,))),
    ("QuickGELU fwd 1.702 +1%", ("rcp", R.QUICKGELU, "fwd"), lambda: emu_rcp_qgelu(X32, 1.702 * 1.01)),
    ("QuickGELU bwd 1.702 +1%", ("rcp", R.QUICKGELU, "bwd"), lambda: emu_rcp_dqgelu(X32, 1.702 * 1.01)),
    ("GELU' table one binade up", ("table", R.GELU_ERF, "bwd"),
     lambda: emu_table(R.GELU_ERF, BITS, 128)),
    ("GELU' table one binade down", ("table", R.GELU_ERF, "bwd"),
     lambda: emu_table(R.GELU_ERF, BITS, -128)),
    ("QuickGELU' table one binade up", ("table", R.QUICKGELU, "bwd"),
     lambda: emu_table(R.QUICKGELU, BITS, 128)),
    ("GELU' table one entry up", ("table", R.GELU_ERF, "bwd"),
     lambda: emu_table(R.GELU_ERF, BITS, 1)),
    ("sig fwd held to the A&S bound", ("as", R.GELU_ERF, "fwd"), lambda: emu_gelu_sig(X32)),
    ("sig grad held to the table's exact GELU' at E = A&S", ("as", R.GELU_ERF, "bwd"),
     lambda: emu_gelu_sig_grad(X32)),
]


@pytest.mark.parametrize("what,key,emu", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_rule_rejects_mutation(what, key, emu):
    """A subtly wrong implementation (or the right one under another implementation's bound: a
    changed routing) fails interval_ok on D at the stored E; the norm-wise 2e-2 (1 + max|ref|)
    tolerance of the GEMM tests accepts all of them but the table shifted by a whole binade."""
    got = R.rne_bf16(np.float64(emu()))
    ref = _ref(key)
    bad = ~R.interval_ok(got, ref, R.E[key]) & IN_D
    print(f"{what}: {int(bad.sum())} of {int(IN_D.sum())} inputs rejected")
    assert bad.any()
    if "binade" not in what:  # (a whole binade off is 0.2 wrong below |z| = 2: that much shows)
        near = IN_D & (np.abs(X) <= 16)  # where the GEMM tests' randn pre-activations lie
        assert np.abs(got - ref)[near].max() <= 2e-2 * (1 + np.abs(ref[near]).max())
