"""CPU self-check of the attention accuracy metric (tests/attn_accuracy.py): the bound of
FACTOR x the bf16 emulation's own per-row error accepts the emulation and rejects torch
implementations that are wrong in the ways a fast kernel goes wrong."""
import pytest
import torch

import attn_accuracy as acc

P, HEADS, T, SCALE = 2, 2, 145, 1 / 8


def _case(pattern="random30", p_drop=0.0):
    gen = torch.Generator().manual_seed(5)
    q, k, v, dout = (t.double() for t in acc.make_inputs(P, T, HEADS, gen))
    bias = acc.key_bias(pattern, P, T, gen)
    keep = None
    if p_drop:
        keep = (torch.rand(P, HEADS, T, T, generator=gen) >= p_drop).double() / (1 - p_drop)
    ref = acc.reference(q, k, v, bias, SCALE, keep, dout)
    emu = acc.emulate(q, k, v, bias, SCALE, keep, dout)
    return (q, k, v, bias, keep, dout), ref, emu


@pytest.mark.parametrize("pattern", ["none", "random30", "first_tile", "last_tile", "one_key"])
@pytest.mark.parametrize("p_drop", [0.0, 0.1])
def test_emulation_is_accepted_and_small(pattern, p_drop):
    _, ref, emu = _case(pattern, p_drop)
    res = acc.judge(emu, ref, emu)
    for n, (k, e) in res.items():
        if pattern == "one_key" and n in ("dq", "dk"):
            continue  # zero reference: absolute row norms, not relative errors
        assert k <= 0.01, (n, k)  # bf16 rounding at a handful of sites: well under 1 % per row
    torch.testing.assert_close(emu["lse"], ref["lse"], rtol=1e-3, atol=1e-3)


def _rejected(got, ref, emu, name):
    with pytest.raises(AssertionError, match=name + ": kernel row error"):
        acc.judge(got, ref, emu)


def test_last_key_dropped_is_rejected():
    (q, k, v, bias, keep, dout), ref, emu = _case()
    bias = bias.clone()
    bias[:, -1] = 0.0  # the last key counts in the reference ...
    ref = acc.reference(q, k, v, bias, SCALE, keep, dout)
    emu = acc.emulate(q, k, v, bias, SCALE, keep, dout)
    got = acc.emulate(q, k[:, :, :-1], v[:, :, :-1], bias[:, :-1], SCALE, keep, dout)  # ... not here
    z = torch.zeros(P, HEADS, 1, 64, dtype=torch.float64)
    got["dk"], got["dv"] = torch.cat([got["dk"], z], 2), torch.cat([got["dv"], z], 2)
    _rejected(got, ref, emu, "out")


def test_scaled_dq_is_rejected():
    _, ref, emu = _case()
    got = dict(emu)
    got["dq"] = acc.bf(emu["dq"] * 0.97)
    _rejected(got, ref, emu, "dq")
    assert acc.judge({**emu, "dq": emu["dq"]}, ref, emu)["dq"][0] < 0.01


def test_bias_ignored_on_one_key_is_rejected():
    (q, k, v, bias, keep, dout), ref, emu = _case()
    j = int((bias[0] != 0).nonzero()[0])
    b2 = bias.clone()
    b2[0, j] = 0.0
    _rejected(acc.emulate(q, k, v, b2, SCALE, keep, dout), ref, emu, "out")


def test_swapped_heads_are_rejected():
    _, ref, emu = _case()
    got = dict(emu)
    got["out"] = emu["out"].flip(1)
    _rejected(got, ref, emu, "out")


def test_bleed_between_sequences_is_rejected():
    _, ref, emu = _case("none")
    got = dict(emu)
    got["dv"] = emu["dv"].clone()
    got["dv"][1, :, 3] = emu["dv"][0, :, 3]  # one key row of sequence 1 takes sequence 0's dV
    _rejected(got, ref, emu, "dv")


def test_zero_reference_tensor_is_held_to_fp32_noise():
    """one_key: dQ and dK are zero in exact arithmetic. fp32-sized noise passes, a value of the
    size of an ordinary gradient does not, and a masked key's dK must be exactly zero."""
    _, ref, emu = _case("one_key")
    assert float(ref["dq"].abs().max()) == 0.0 and float(ref["dk"].abs().max()) == 0.0
    noisy = dict(emu)
    noisy["dq"] = 1e-7 * ref["dq_terms"]
    acc.judge(noisy, ref, emu)
    for wrong in (1e-3 * ref["dq_terms"], torch.full_like(ref["dq"], 1e-3)):
        with pytest.raises(AssertionError, match="dq: reference is zero"):
            acc.judge({**emu, "dq": wrong}, ref, emu)
    dk = emu["dk"].clone()
    dk[0, 0, 0, 0] = 1e-30 if float(ref["dk_terms"][0, 0, 0].abs().max()) == 0.0 else 1.0
    with pytest.raises(AssertionError, match="dk: reference is zero"):
        acc.judge({**emu, "dk": dk}, ref, emu)
