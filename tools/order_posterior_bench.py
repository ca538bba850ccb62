"""Posterior over orders: what the new calls cost beside the encode, and what the minimum-risk
decodes change on the decisive story sets.

    python tools/order_posterior_bench.py [--stories 32] [--samples 256] [--rounds 5]

Part 1, config 3 (bf16, eval, N = 5, T = 513), seeded synthetic stories, one process: device
events around the encode, the scoring of all 120 orders (berson.score_orders_batch), the posterior
reduction over them (berson.order_posterior), a draw of --samples ancestral samples
(berson.sample_orders_batch) and the reduction over those, in that order within a pass; the passes
repeat --rounds times after two warm-up passes and the median of each segment is reported.

Part 2, the two 16-story decisive sets (tests/golden decisive_config3_bf16w, seeds 312 / 313, bf16):
per set, in how many stories the mbr_acc / mbr_tau order differs from the MAP order over all 120
orders, and the expected accuracy / tau of both orders under the posterior. Nothing is timed.
Prints one JSON line.
"""
import argparse
import itertools
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from counter_init import counter_state_dict  # noqa: E402
from make_golden_real import real_inputs, scale_decisive  # noqa: E402
from multimodal_sequencing_amd import berson, model_zoo  # noqa: E402

SETS = ("decisive_config3_bf16w", "decisive_config3_bf16w_s313")


def timings(a, dev):
    preset = model_zoo.PRESETS["config3"]
    N = preset["N"]
    m = model_zoo.build_preset("config3", device=dev, dtype=torch.bfloat16, seed=0).eval()
    data = bench.synthetic_batch(a.stories, N, preset["per_seq"], 50265, 224, dev, seed=2000)
    perms = torch.tensor(list(itertools.permutations(range(N))), dtype=torch.int64, device=dev)
    inp = berson._batch_inputs(m, data)
    names = ("encode_ms", "score_ms", "posterior_ms", "sample_ms", "sample_posterior_ms")
    ms = {k: [] for k in names}
    with torch.no_grad():
        for r in range(a.rounds + 2):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
            ev[0].record()
            enc = m.encode(**inp)
            ev[1].record()
            nll = berson.score_orders_batch(m.args, m, enc, perms)
            ev[2].record()
            post = berson.order_posterior(perms, nll)
            ev[3].record()
            orders, snll = berson.sample_orders_batch(m.args, m, enc, a.samples, seed=r)
            ev[4].record()
            spost = berson.order_posterior(orders, snll, mode="uniform")
            ev[5].record()
            torch.cuda.synchronize()
            if r >= 2:  # two warm-up passes (allocator, workspaces, kernel selection)
                for i, k in enumerate(names):
                    ms[k].append(ev[i].elapsed_time(ev[i + 1]))
    out = {k: round(statistics.median(v), 3) for k, v in ms.items()}
    e = out["encode_ms"]
    out.update({k.replace("_ms", "_over_encode"): round(out[k] / e, 4) for k in names[1:]})
    out["largest_abs_logz_exact"] = round(float(post["logz"].abs().max()), 6)
    out["sample_vs_exact_position_max_diff"] = round(
        float((spost["position"] - post["position"]).abs().max()), 4)
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
    post = berson.berson_order_posterior(m.args, m, None, inputs, source="exact")
    orders = post["orders"].cpu().numpy()
    pos, bef = post["position"].cpu().numpy(), post["before"].cpu().numpy()
    N = orders.shape[1]
    out = {"stories": int(pos.shape[0])}
    for kind in ("acc", "tau"):
        idx, mp = post[f"mbr_{kind}_index"].cpu().numpy(), post["map_index"].cpu().numpy()
        gains = []
        for b in range(pos.shape[0]):
            o = orders[mp[b]]
            if kind == "acc":
                g = sum(float(pos[b, t, o[t]]) for t in range(N)) / N
            else:
                g = sum(float(bef[b, o[i], o[j]]) - float(bef[b, o[j], o[i]])
                        for i in range(N) for j in range(i + 1, N)) / (N * (N - 1) / 2)
            gains.append(g)
        out[f"mbr_{kind}_differs_from_map"] = int((idx != mp).sum())
        out[f"mean_exp_{kind}_of_mbr"] = round(float(post[f"exp_{kind}"].mean()), 4)
        out[f"mean_exp_{kind}_of_map"] = round(float(np.mean(gains)), 4)
    out["mean_map_prob"] = round(float(post["map_prob"].mean()), 4)
    out["mean_entropy_nats"] = round(float(post["entropy"].mean()), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stories", type=int, default=32)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"workload": f"config3: posterior over 120 orders / {a.samples} samples of "
                       f"{a.stories} stories, bf16, N=5",
           "device": torch.cuda.get_device_name(0), "stories": a.stories, "samples": a.samples,
           "rounds": a.rounds}
    res.update(timings(a, dev))
    res["decisive_sets"] = {name: decisive(name) for name in SETS}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
