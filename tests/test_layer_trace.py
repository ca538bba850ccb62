"""Which C-ABI entries each precision / placement mode of the encoder launches, in which order and
with which arguments — pinned on the CPU against a recorded trace.

`_native.lib` is replaced by a fake whose functions record the call and return 0 (4096 for the
int64_t size queries); `_native._dev`, `_native._stream` and `_native.gemm_workspace` by stand-ins
that need no device. An `LXRTModel(device="cpu")` is then driven through `encode_joint` (and a
backward) in every mode of kernels.BertLayerFn / VitBlockFn: bf16 / fp32 training, bf16 eval, the
last layer on the text rows, fused MX-fp8 eval, its K % 128 FFN-only form (128-wide model), ViT-only
and mixed placement, fp8 training with and without fp8 dgrad. Nothing touches a GPU or the built
library.

A record is the entry name followed by one item per argument: integers as they are, floats as the
hex of their float32 value, pointers as 0 (null) / 1, an mmseq_rows as its three fields, a dropout
descriptor as [hex(p), stream] or null (the seed counts forward passes and is left out). The
expected traces are tests/golden/layer_trace.json: the distinct records once, and per scenario the
list of their indices. Equality is exact: a differing record is a behaviour change. Regenerate
(only for an intended change of the launches) with

    python tests/test_layer_trace.py --write
"""
import ctypes
import json
import os
import struct
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "layer_trace.json")

# the smallest shapes at which every path is still eligible: widths % 256 == 0 and ViT rows
# P * Tv = 48 * 9 = 432 >= 256 for the fp8 forms; two joint layers (the layer-to-layer MX-fp8
# hand-off and the last-layer text-rows path both occur)
MAIN = dict(hidden=256, heads=4, inter=1024, vit=256)
NARROW = dict(hidden=128, heads=2, inter=384, vit=128)  # K % 128 only: the FFN-only fp8 fallback
B, NST, LT, RES = 8, 3, 24, 32

# name -> (shape, compute dtype, train (forward + backward), text_rows, fp8_forward kwargs or None)
SCENARIOS = {
    "bf16_train": (MAIN, torch.bfloat16, True, False, None),
    "bf16_train_rows": (MAIN, torch.bfloat16, True, True, None),
    "bf16_eval_rows": (MAIN, torch.bfloat16, False, True, None),
    "fp32_train_rows": (MAIN, torch.float32, True, True, None),
    "fp8_eval": (MAIN, torch.bfloat16, False, False, {}),
    "fp8_eval_rows": (MAIN, torch.bfloat16, False, True, {}),
    "fp8_eval_vit_only": (MAIN, torch.bfloat16, False, False, {"sites": "FP8_VIT_ONLY"}),
    "fp8_eval_mixed": (MAIN, torch.bfloat16, False, False, {"sites": ("qkv", "vit.fc1")}),
    "fp8_train_rows": (MAIN, torch.bfloat16, True, True, {"training": True}),
    "fp8_train_dgrad": (MAIN, torch.bfloat16, True, False, {"training": True, "dgrad": True}),
    "fp8_eval_128": (NARROW, torch.bfloat16, False, False, {}),
}


def _f32hex(v):
    return struct.pack("<f", v).hex()


def _item(ctype, v):
    from multimodal_sequencing_amd import _native as N
    if ctype is N.Rows:
        return [int(v.ld), int(v.bstride), int(v.rpb)]
    if ctype is N._dp:
        return None if v is None else [_f32hex(v._obj.p), int(v._obj.stream)]
    if ctype is ctypes.c_void_p:
        return int(bool(getattr(v, "value", v)))
    if ctype in (ctypes.c_float, ctypes.c_double):
        return _f32hex(v) if ctype is ctypes.c_float else struct.pack("<d", v).hex()
    return int(v)


class FakeLib:
    """Stands in for the loaded library: every entry of _native._SIGS records its call."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        from multimodal_sequencing_amd import _native as N
        res, argtypes = N._SIGS[name]  # an entry the binding does not declare: KeyError

        def entry(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            self.calls.append([name] + [_item(t, a) for t, a in zip(argtypes, args)])
            return 4096 if res is ctypes.c_int64 else (b"" if res is ctypes.c_char_p else 0)
        return entry


def install(setattr_):
    """Replace the library and the three device helpers of _native through setattr_(obj, name,
    value) (monkeypatch.setattr in the tests); returns the fake library."""
    from multimodal_sequencing_amd import _native as N
    fake = FakeLib()
    ws = torch.empty(1024)
    setattr_(N, "lib", lambda: fake)
    setattr_(N, "_dev", lambda *ts: None)
    setattr_(N, "_stream", lambda: None)
    setattr_(N, "gemm_workspace", lambda device, stream=None: ws)
    return fake


def _inputs():
    g = torch.Generator(device="cpu").manual_seed(11)
    npair = NST * (NST - 1)
    P = B * npair
    ids = torch.randint(3, 64, (P, LT), generator=g)
    mask = torch.ones(P, LT, dtype=torch.long)
    mask[1::2, LT - 5:] = 0  # ragged: every other pair is padded
    images = torch.randn(B, NST, 3, RES, RES, generator=g)
    pairs = torch.tensor([[i, j] for i in range(NST) for j in range(NST) if i != j])
    return ids, mask, images, pairs[None].expand(B, npair, 2).contiguous()


def run_scenario(name, fake):
    """The trace (list of records) of one scenario; the fake library must be installed."""
    from multimodal_sequencing_amd import _native as N
    from multimodal_sequencing_amd import kernels as K
    from multimodal_sequencing_amd.lxrt import LXRTConfig, LXRTModel
    shape, dtype, train, text_rows, f8 = SCENARIOS[name]
    cfg = LXRTConfig(vocab_size=64, hidden_size=shape["hidden"], num_hidden_layers=2,
                     num_attention_heads=shape["heads"], intermediate_size=shape["inter"],
                     max_position_embeddings=40)
    vision = dict(width=shape["vit"], layers=1, patch=16, res=RES, embed=128)
    m = LXRTModel(cfg, device="cpu", compute_dtype=dtype, vision=vision)
    m.train(train)
    ids, mask, images, pairs = _inputs()
    rows_on, sel = K.ROWS["on"], dict(N._sel)
    K.ROWS["on"] = True
    N._sel.update(gemm=N.GEMM_AUTO, attn=1)
    del fake.calls[:]
    try:
        if f8 is not None and f8.get("sites") == "FP8_VIT_ONLY":
            f8 = dict(f8, sites=K.FP8_VIT_ONLY)
        with K.fp8_forward(f8 is not None, **(f8 or {})):
            with torch.enable_grad() if train else torch.no_grad():
                x, _ = m.encode_joint(ids, mask, None, images, pairs, text_rows=text_rows)
                if train:
                    x.float().sum().backward()
    finally:
        K.ROWS["on"] = rows_on
        N._sel.update(sel)
    return list(fake.calls)


def _pack(traces):
    """{scenario: [record, ...]} -> the fixture: distinct records once + index lists."""
    index, records, scen = {}, [], {}
    for name, calls in traces.items():
        ids = []
        for c in calls:
            key = json.dumps(c)
            if key not in index:
                index[key] = len(records)
                records.append(c)
            ids.append(index[key])
        scen[name] = ids
    return {"records": records, "scenarios": scen}


def _dump(fix, path):
    with open(path, "w") as f:
        f.write('{"records": [\n')
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in fix["records"]))
        f.write('\n], "scenarios": {\n')
        f.write(",\n".join(f'{json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}'
                           for k, v in fix["scenarios"].items()))
        f.write("\n}}\n")


_GOLD = []


def _golden():
    if not _GOLD:
        with open(FIXTURE) as f:
            _GOLD.append(json.load(f))
    return _GOLD[0]


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_layer_call_trace(name, monkeypatch):
    gold = _golden()
    assert set(gold["scenarios"]) == set(SCENARIOS)
    fake = install(monkeypatch.setattr)
    got = run_scenario(name, fake)
    want = [gold["records"][i] for i in gold["scenarios"][name]]
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"{name}: call {k} differs:\n got  {a}\n want {b}"
    assert len(got) == len(want), (name, len(got), len(want),
                                   [c[0] for c in (got if len(got) > len(want) else want)[min(len(got), len(want)):]])


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    fake = install(setattr)
    fix = _pack({name: run_scenario(name, fake) for name in SCENARIOS})
    if "--write" in sys.argv:
        _dump(fix, FIXTURE)
    n = sum(len(v) for v in fix["scenarios"].values())
    print(f"{len(SCENARIOS)} scenarios, {n} calls, {len(fix['records'])} distinct records")
