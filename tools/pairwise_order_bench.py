"""Decoding from the pairwise head: what the subset DP and the pairwise scorer cost beside the
encode and beside the enumerations, and how the decodes agree on the decisive story sets.

    python tools/pairwise_order_bench.py [--stories 32] [--rounds 5] [--log FILE]

Part 1a, config 3 (bf16, eval, N = 5, T = 513), seeded synthetic stories, one process: device
events around the encode, berson.pairwise_order_batch (weights + mmseq_pairwise_order),
berson.pairwise_score_orders over all 120 orders and berson.joint_order_batch, in that order within
a pass; the passes repeat --rounds times after two warm-up passes and the median of each segment
is reported.

Part 1b, decoder inputs from beam_batch_ref.random_case (fp32, no encoder, H = 768), one call per
window between two device events, two warm-up rounds, the median of --rounds: at N = 9, B = 1 and
8, the DP (the whole Python call, and mmseq_pairwise_order alone on weights made before) beside
the pairwise scoring of all 362 880 orders and beside the prefix-tree enumeration
of their pointer scores; the DP alone at N = 12 (tables in the workspace), B = 1 and 32.

Part 2, the two 16-story decisive sets (tests/golden decisive_config3_bf16w, seeds 312 / 313, bf16),
not timed: in how many stories the beam, exact, pairwise and joint orders and the legacy
topological sort coincide, and the mean |before_pointer - before_pairwise| between the exact
pointer posterior's and the pairwise distribution's precedence marginals.
Nothing is gated on these times. Prints one JSON line (and writes it to --log).
"""
import argparse
import itertools
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import torch  # noqa: E402

import beam_batch_ref as R  # noqa: E402
import bench  # noqa: E402
import order_score_ref as S  # noqa: E402
from counter_init import counter_state_dict  # noqa: E402
from make_golden_real import real_inputs, scale_decisive  # noqa: E402
from multimodal_sequencing_amd import _native as NV  # noqa: E402
from multimodal_sequencing_amd import berson, model_zoo  # noqa: E402

SETS = ("decisive_config3_bf16w", "decisive_config3_bf16w_s313")


class Head:
    """What the berson decoders read of a model: the head's f32 weights and a cache dict."""
    pairwise_loss_lam = 0.6

    def __init__(self, case):
        self._w = {k: v.cuda().contiguous() for k, v in case["p"].items()}
        self.store = self

    def f32(self, name):
        return self._w[name]


def dev_enc(case):
    def dev(v):
        return tuple(dev(x) for x in v) if isinstance(v, tuple) else (None if v is None else v.cuda())
    return tuple(dev(v) for v in S.enc(case))


def timed(fns, rounds, warm=2):
    """fns: name -> callable; one window per call -> name -> median ms of `rounds` windows."""
    ms = {k: [] for k in fns}
    for r in range(warm + rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= warm:
                ms[k].append(e0.elapsed_time(e1))
    return {k: round(statistics.median(v), 3) for k, v in ms.items()}


def config3(a, dev):
    preset = model_zoo.PRESETS["config3"]
    N = preset["N"]
    m = model_zoo.build_preset("config3", device=dev, dtype=torch.bfloat16, seed=0).eval()
    data = bench.synthetic_batch(a.stories, N, preset["per_seq"], 50265, 224, dev, seed=2000)
    perms = torch.tensor(list(itertools.permutations(range(N))), dtype=torch.int64, device=dev)
    inp = berson._batch_inputs(m, data)
    names = ("encode_ms", "pairwise_order_ms", "pairwise_score_ms", "joint_ms")
    ms = {k: [] for k in names}
    with torch.no_grad():
        for r in range(a.rounds + 2):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
            ev[0].record()
            enc = m.encode(**inp)
            ev[1].record()
            post = berson.pairwise_order_batch(m.args, m, enc)
            ev[2].record()
            pnll = berson.pairwise_score_orders(m.args, m, enc, perms)
            ev[3].record()
            berson.joint_order_batch(m.args, m, enc)
            ev[4].record()
            torch.cuda.synchronize()
            if r >= 2:  # two warm-up passes (allocator, workspaces, kernel selection)
                for i, k in enumerate(names):
                    ms[k].append(ev[i].elapsed_time(ev[i + 1]))
    out = {k: round(statistics.median(v), 3) for k, v in ms.items()}
    e = out["encode_ms"]
    out.update({k.replace("_ms", "_over_encode"): round(out[k] / e, 5) for k in names[1:]})
    idx, best, _ = berson.exact_from_scores(pnll)
    out["dp_order_is_argmin_of_scores"] = bool(torch.equal(perms[idx], post["order"]))
    out["dp_pnll_minus_min_score_max_abs"] = float((best - post["pnll"]).abs().max())
    return out


def kernel_alone(enc):
    """-> a callable that launches mmseq_pairwise_order alone, on weights and buffers made before."""
    w = berson.pairwise_weights(enc[7])
    B, N = w.shape[0], w.shape[1]
    out = {name: torch.empty((B,) + (N,) * nn, dtype=dtype, device=w.device)
           for name, dtype, nn in NV.PAIRWISE_OUTPUTS}
    ws = torch.empty(NV.pairwise_order_workspace(B, N) // 4, device=w.device)
    return lambda: NV.pairwise_order(w, out, ws)


def random_cases(a):
    out = {}
    H = 768
    with torch.no_grad():
        for B in (1, 8):
            case = R.random_case(B, 9, H, R.SEED)
            head, enc = Head(case), dev_enc(case)
            nll, perms = berson.enumerate_orders_batch(None, head, enc, return_orders=True)
            ms = timed({"dp_ms": lambda: berson.pairwise_order_batch(None, head, enc),
                        "dp_kernel_ms": kernel_alone(enc),
                        "score_all_ms": lambda: berson.pairwise_score_orders(None, head, enc, perms),
                        "tree_ms": lambda: berson.enumerate_orders_batch(None, head, enc)},
                       a.rounds)
            post = berson.pairwise_order_batch(None, head, enc)
            idx, best, _ = berson.exact_from_scores(
                berson.pairwise_score_orders(None, head, enc, perms))
            ms["orders"] = int(perms.shape[0])
            ms["dp_order_is_argmin_of_scores"] = bool(torch.equal(perms[idx], post["order"]))
            out[f"N9_B{B}"] = ms
        for B in (1, 32):
            case = R.random_case(B, 12, 16, R.SEED)
            head, enc = Head(case), dev_enc(case)
            out[f"N12_B{B}"] = timed(
                {"dp_ms": lambda: berson.pairwise_order_batch(None, head, enc),
                 "dp_kernel_ms": kernel_alone(enc)}, a.rounds)
    return out


def decisive(name):
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", name + ".json")))
    m = model_zoo.build_from_golden(meta["config"], device="cuda", dtype=torch.bfloat16)
    cw = scale_decisive(counter_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}),
                        name)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in cw.items()})
    m.eval()
    ids, labels, images = real_inputs(meta["input_seed"], meta["config"])
    inputs = {"input_ids": torch.from_numpy(ids), "labels": torch.from_numpy(labels),
              "images": torch.from_numpy(images).cuda()}
    with torch.no_grad():
        enc = m.encode(**berson._batch_inputs(m, inputs))
        got = {"beam": berson.beam_decode_batch(m.args, m, enc)[0].tolist(),
               "exact": berson.exact_order_batch(m.args, m, enc)[0].tolist(),
               "joint": berson.joint_order_batch(m.args, m, enc)[0].tolist()}
        pw = berson.pairwise_order_batch(m.args, m, enc)
        pointer = berson.order_posterior_batch(m.args, m, enc, source="exact")
    got["pairwise"] = pw["order"].tolist()
    got["topological"] = [berson.topological_order_host(w) for w in pw["w"].cpu()]
    B = len(got["beam"])
    out = {"stories": B}
    for x, y in itertools.combinations(("beam", "exact", "pairwise", "joint", "topological"), 2):
        out[f"{x}_eq_{y}"] = sum(got[x][b] == got[y][b] for b in range(B))
    out["mean_abs_before_pointer_minus_pairwise"] = round(
        float((pointer["before"] - pw["before"]).abs().mean()), 4)
    out["mean_entropy_pointer_nats"] = round(float(pointer["entropy"].mean()), 4)
    out["mean_entropy_pairwise_nats"] = round(float(pw["entropy"].mean()), 4)
    out["mean_pairwise_margin"] = round(float(pw["margin"].mean()), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stories", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"workload": f"config3: pairwise decode of {a.stories} stories, bf16, N=5; random N=9 / "
                       "N=12 cases",
           "device": torch.cuda.get_device_name(0), "stories": a.stories, "rounds": a.rounds}
    res["config3"] = config3(a, dev)
    res["random"] = random_cases(a)
    res["decisive_sets"] = {name: decisive(name) for name in SETS}
    line = json.dumps(res)
    print(line)
    if a.log:
        with open(a.log, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
