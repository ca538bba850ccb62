"""Float64 references of the activations of include/mmseq.h and the acceptance rule for a bf16
result of an approximation whose absolute error E is known.

The rule (`interval_ok`): a bf16 result `got` of a function whose exact value is `ref` is accepted
iff  rne_bf16(ref - E) <= got <= rne_bf16(ref + E).  With E = 0 that is the correctly rounded
value; E is the approximation's own absolute error before the final rounding and nothing else, so
the rule is as sharp at 1e-3 as at 100 (an abs/rel tolerance that lets bf16 rounding through near
100 lets errors of 0.4 through).

`E[...]` are the constants the GPU tests import: 1.25 x the maximum error of each implementation
over the domain D (finite bf16, |x| <= 8192), emulated in fp32 numpy from the source formulas
against float64 (tests/test_act_curve_ref.py holds the emulations and re-derives `EMULATED`). The
quarter of margin is for v_exp_f32 / v_rcp_f32 being 1-ulp approximations where the emulation uses
correctly rounded ones.
"""
import math

import numpy as np

# mmseq_act
NONE, GELU_ERF, QUICKGELU, TANH, GELU_TANH = 0, 1, 2, 3, 4
ACT_NAMES = {GELU_ERF: "gelu", QUICKGELU: "quickgelu", TANH: "tanh", GELU_TANH: "gelu_tanh"}

D_MAX = 8192.0  # the domain D on which the bounds hold: finite bf16 values with |x| <= D_MAX

_erf = np.frompyfunc(math.erf, 1, 1)
_K = math.sqrt(2.0 / math.pi)
_C = 0.044715


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def act64(act, x):
    """act(x) in float64 (definitions: include/mmseq.h mmseq_act and its reference sites)."""
    x = _f64(x)
    with np.errstate(over="ignore", under="ignore"):
        if act == GELU_ERF:
            return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)).astype(np.float64))
        if act == QUICKGELU:
            return x / (1.0 + np.exp(-1.702 * x))
        if act == TANH:
            return np.tanh(x)
        if act == GELU_TANH:
            return 0.5 * x * (1.0 + np.tanh(_K * (x + _C * x * x * x)))
    assert act == NONE
    return x.copy()


def dact64(act, x):
    """d act / dx at x in float64."""
    x = _f64(x)
    with np.errstate(over="ignore", under="ignore"):
        if act == GELU_ERF:
            cdf = 0.5 * (1.0 + _erf(x / math.sqrt(2.0)).astype(np.float64))
            return cdf + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
        if act == QUICKGELU:
            s = 1.0 / (1.0 + np.exp(-1.702 * x))
            return s + 1.702 * x * (s * (1.0 - s))
        if act == TANH:
            t = np.tanh(x)
            return 1.0 - t * t
        if act == GELU_TANH:
            t = np.tanh(_K * (x + _C * x * x * x))
            return 0.5 * (1.0 + t) + 0.5 * x * ((1.0 - t * t) * (_K * (1.0 + 3.0 * _C * x * x)))
    assert act == NONE
    return np.ones_like(x)


def bits_to_f64(bits):
    """bf16 bit patterns (any integer array) -> their values as float64."""
    b = np.asarray(bits).astype(np.uint32) & 0xFFFF
    with np.errstate(invalid="ignore"):  # signalling NaN patterns
        return (b << 16).view(np.float32).astype(np.float64)


def all_bf16():
    """(bits, replaced): the 65 536 bf16 patterns as a uint16 [256][256] table, entry [n][k] = the
    pattern n * 256 + k, with the 256 Inf / NaN patterns replaced by 0; `replaced` marks those."""
    bits = np.arange(65536, dtype=np.uint32).reshape(256, 256)
    replaced = (bits & 0x7F80) == 0x7F80
    bits = np.where(replaced, 0, bits).astype(np.uint16)
    return bits, replaced


def domain(x):
    """The mask of D: finite with |x| <= D_MAX."""
    x = _f64(x)
    return np.isfinite(x) & (np.abs(x) <= D_MAX)


def rne_bf16(x64):
    """float64 -> the nearest bf16 value, ties to even (8 significant bits, fp32's exponent range,
    subnormals kept, overflow to inf), returned as float64. One rounding: not via fp32."""
    x = _f64(x64)
    out = x.copy()
    fin = np.isfinite(x)
    _, ex = np.frexp(np.where(fin, x, 0.0))        # |x| = m 2^ex, m in [0.5, 1)
    e = np.maximum(ex - 1, -126)                    # floor(log2 |x|), subnormals share 2^-126
    quantum = np.ldexp(1.0, e - 7)
    r = np.rint(np.where(fin, x, 0.0) / quantum) * quantum  # both steps exact but the rint
    r = np.where(np.abs(r) >= 2.0 ** 128, np.copysign(np.inf, r), r)
    out[fin] = r[fin]
    return out


def interval_ok(got_bf16, ref64, E):
    """Element-wise: rne_bf16(ref - E) <= got <= rne_bf16(ref + E), compared as floats (-0 == +0;
    a NaN in `got` fails). got_bf16: the values of bf16 results; E: scalar or array, >= 0."""
    got = _f64(got_bf16)
    ref = _f64(ref64)
    E = _f64(E)
    with np.errstate(invalid="ignore"):
        return (rne_bf16(ref - E) <= got) & (got <= rne_bf16(ref + E))


# Maximum absolute error over D of each implementation in csrc/common.h / gemm256.hip, emulated in
# fp32 (tests/test_act_curve_ref.py re-derives every entry). Key: (implementation, act, direction).
EMULATED = {
    ("sig", GELU_ERF, "fwd"): 2.533e-5,     # gelu_sig / gelu_sig8, at x ~ 3.06
    ("sig", GELU_ERF, "bwd"): 1.099e-4,     # gelu_sig_grad, at x ~ 0.93
    ("as", GELU_ERF, "fwd"): 4.4e-7,        # act_fwd_fast: Abramowitz-Stegun erf
    ("as", GELU_ERF, "bwd"): 2.8e-7,        # act_bwd_fast
    ("rcp", QUICKGELU, "fwd"): 6.3e-7,      # act_fwd_fast: x * rcp(1 + exp)
    ("rcp", QUICKGELU, "bwd"): 9.4e-7,      # act_bwd_fast
    ("table", GELU_ERF, "bwd"): 7.79e-4,    # dtab: clamped at 2^-10 and 7.96875; at z = 0
    ("table", QUICKGELU, "bwd"): 8.31e-4,   # at z = 0
}
E = {k: 1.25 * v for k, v in EMULATED.items()}
# libm act_fwd / act_bwd (fp32 erff / tanhf / exp): held to this absolute error before rounding
E_LIBM = 4e-7
for _a in (GELU_ERF, QUICKGELU, TANH, GELU_TANH):
    for _d in ("fwd", "bwd"):
        E[("libm", _a, _d)] = E_LIBM


def _bf16_key(v):
    """bf16 values -> integers that order like the values (neighbours differ by 1)."""
    b = (np.asarray(v, dtype=np.float64).astype(np.float32).view(np.uint32) >> 16).astype(np.int64)
    return np.where(b & 0x8000, -(b & 0x7FFF), b)


def _bf16_from_key(k):
    b = np.where(k < 0, (-k) | 0x8000, k).astype(np.uint32)
    return (b << 16).view(np.float32).astype(np.float64)


def needed_E(got_bf16, ref64):
    """The smallest E with which interval_ok accepts each element (0 where `got` is the correctly
    rounded value): the distance from ref to the rounding boundary of got's bf16 cell. A lower
    bound of the error the implementation had before its result was rounded; what a GPU run can
    measure from bf16 outputs. got and ref finite."""
    got = _f64(got_bf16)
    ref = _f64(ref64)
    best = rne_bf16(ref)
    k = _bf16_key(got)
    toward = np.where(got > best, -1, 1)  # the neighbour of got on ref's side
    boundary = 0.5 * (got + _bf16_from_key(k + toward))
    return np.where(got == best, 0.0, np.abs(boundary - ref))
