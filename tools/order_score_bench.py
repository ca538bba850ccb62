"""Scoring candidate orders: one encode + berson.score_orders_batch over all N! orders against
today's route, a full model forward with labels = the order once per candidate, on the same
seeded stories, in one process, alternating.

    python tools/order_score_bench.py [--stories 32] [--forward-orders 6] [--rounds 3]

config 3: bf16, eval, N = 5 (120 orders), T = 513. Both routes are warmed first. Every timing
window is a host clock around whole passes, each pass ending in a device synchronise, repeated
until the window exceeds --min-window seconds; the windows of the two routes alternate and the
median window of each is reported. The full-forward route is timed on --forward-orders of the 120
orders (evenly spaced through the list) and reported per order; its 120-order cost is that times
120, no more measured than that. The scoring call's share of the encode is taken with device
events around the two calls. Prints one JSON line.
"""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from multimodal_sequencing_amd import berson, model_zoo  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stories", type=int, default=32)
    ap.add_argument("--forward-orders", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-window", type=float, default=1.0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    preset = model_zoo.PRESETS["config3"]
    N = preset["N"]
    m = model_zoo.build_preset("config3", device=dev, dtype=torch.bfloat16, seed=0).eval()
    data = bench.synthetic_batch(a.stories, N, preset["per_seq"], 50265, 224, dev, seed=2000)
    perms = list(itertools.permutations(range(N)))
    K = len(perms)
    perms_dev = torch.tensor(perms, dtype=torch.int64, device=dev)
    picks = [perms[i * K // a.forward_orders] for i in range(a.forward_orders)]
    labels = [torch.tensor([list(p)] * a.stories) for p in picks]

    def scored():
        with torch.no_grad():
            enc = m.encode(**berson._batch_inputs(m, data))
            out = berson.score_orders_batch(m.args, m, enc, perms_dev)
        torch.cuda.synchronize()
        return out

    def forwards():
        out = []
        with torch.no_grad():
            for lab in labels:
                m({**data, "labels": lab})
                out.append(m.last_loss_terms[0])
        torch.cuda.synchronize()
        return out

    def window(fn, orders):
        n, t0 = 0, time.perf_counter()
        while True:
            fn()
            n += 1
            dt = time.perf_counter() - t0
            if dt > a.min_window:
                return a.stories * orders * n / dt

    for _ in range(2):  # warm both routes (allocator, workspaces, kernel selection)
        nll = scored()
        forwards()
    rates = {"scored": [], "forward": []}
    for _ in range(a.rounds):
        rates["scored"].append(window(scored, K))
        rates["forward"].append(window(forwards, len(picks)))
    sc, fw = statistics.median(rates["scored"]), statistics.median(rates["forward"])

    enc_ms, score_ms = [], []
    with torch.no_grad():
        inp = berson._batch_inputs(m, data)
        for _ in range(5):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            enc = m.encode(**inp)
            ev[1].record()
            berson.score_orders_batch(m.args, m, enc, perms_dev)
            ev[2].record()
            torch.cuda.synchronize()
            enc_ms.append(ev[0].elapsed_time(ev[1]))
            score_ms.append(ev[1].elapsed_time(ev[2]))
    e, s = statistics.median(enc_ms), statistics.median(score_ms)
    # the two routes on the same candidates: the forward's mean pointer loss over the batch x
    # (N - 1) against the mean of the scorer's NLLs (bf16 encoders at different batch contents
    # are the same here: both see all stories at once)
    fw_mean = [float(x) * (N - 1) for x in forwards()]
    sc_mean = [float(nll[:, perms.index(p)].mean()) for p in picks]
    print(json.dumps({
        "workload": f"config3: score {K} orders of {a.stories} stories, bf16, N={N}",
        "device": torch.cuda.get_device_name(0), "stories": a.stories, "orders": K,
        "scored_story_orders_per_s": round(sc, 1), "forward_story_orders_per_s": round(fw, 1),
        "ratio": round(sc / fw, 2),
        "windows_scored": [round(x, 1) for x in rates["scored"]],
        "windows_forward": [round(x, 1) for x in rates["forward"]],
        "forward_orders_timed": len(picks),
        "forward_ms_per_order": round(1e3 * a.stories / fw, 3),
        "encode_ms": round(e, 3), "score_ms": round(s, 3), "score_over_encode": round(s / e, 4),
        "largest_mean_nll_difference": round(max(abs(x - y) for x, y in zip(fw_mean, sc_mean)), 6)}))


if __name__ == "__main__":
    main()
