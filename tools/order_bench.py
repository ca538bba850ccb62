"""Ordering throughput: the per-story path (berson.berson_pointer_network, one encode of 20 or 72
pairs and a host-driven beam search per story) against the batched path
(berson.berson_pointer_network_batch: one encode of the whole batch and one device-resident
mmseq_beam_search), on the same seeded stories, in one process, alternating.

    python tools/order_bench.py [--config 3|5] [--stories 32] [--batch 32] [--rounds 3]

config 3: bf16, N = 5, T = 513, beam 16 (the benchmark's model); config 5: N = 9, H = 1024.
Both paths are warmed first. Every timing window is a host clock around whole passes over the
stories, each pass ending in a device synchronise, repeated until the window exceeds
--min-window seconds; the windows of the two paths alternate and the median window of each is
reported. The batched path's split into encode and decode is taken with device events around the
two calls. Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from multimodal_sequencing_amd import berson, model_zoo  # noqa: E402
from multimodal_sequencing_amd.process_inputs import prepare_berson_inputs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3, choices=(3, 5))
    ap.add_argument("--stories", type=int, default=32)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-window", type=float, default=1.0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    name = f"config{a.config}"
    preset = model_zoo.PRESETS[name]
    m = model_zoo.build_preset(name, device=dev, dtype=torch.bfloat16, seed=0).eval()
    m.args.beam_size = 16
    data = bench.synthetic_batch(a.stories, preset["N"], preset["per_seq"], 50265, 224, dev,
                                 seed=2000)
    chunks = [{k: v[o:o + a.batch] for k, v in data.items()} for o in range(0, a.stories, a.batch)]
    singles = [{k: v[b:b + 1] for k, v in data.items()} for b in range(a.stories)]

    def per_story():
        out = [berson.berson_pointer_network(m.args, m, None, s) for s in singles]
        torch.cuda.synchronize()
        return out

    def batched():
        out = [o for c in chunks for o in berson.berson_pointer_network_batch(m.args, m, None, c)]
        torch.cuda.synchronize()
        return out

    def window(fn):
        n, t0 = 0, time.perf_counter()
        while True:
            fn()
            n += 1
            dt = time.perf_counter() - t0
            if dt > a.min_window:
                return a.stories * n / dt

    for _ in range(2):  # warm both paths (allocator, workspaces, kernel selection)
        one, many = per_story(), batched()
    rates = {"per_story": [], "batched": []}
    for _ in range(a.rounds):
        rates["per_story"].append(window(per_story))
        rates["batched"].append(window(batched))
    ps, bt = statistics.median(rates["per_story"]), statistics.median(rates["batched"])

    # the batched path's two parts, device events around encode and decode of one chunk
    enc_ms, dec_ms = [], []
    with torch.no_grad():
        c = chunks[0]
        inp = prepare_berson_inputs(c["input_ids"], c["labels"], m.n_steps, device=m.device_)
        inp["images"] = c["images"].to(m.device_, torch.float32).contiguous()
        for _ in range(5):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            enc = m.encode(**inp)
            ev[1].record()
            berson.beam_decode_batch(m.args, m, enc)
            ev[2].record()
            torch.cuda.synchronize()
            enc_ms.append(ev[0].elapsed_time(ev[1]))
            dec_ms.append(ev[1].elapsed_time(ev[2]))
    e, d = statistics.median(enc_ms), statistics.median(dec_ms)
    print(json.dumps({
        "workload": f"{name}: order {a.stories} stories, bf16, N={preset['N']}, beam 16",
        "device": torch.cuda.get_device_name(0), "stories": a.stories, "batch": a.batch,
        "per_story_stories_per_s": round(ps, 2), "batched_stories_per_s": round(bt, 2),
        "ratio": round(bt / ps, 3),
        "windows_per_story": [round(x, 2) for x in rates["per_story"]],
        "windows_batched": [round(x, 2) for x in rates["batched"]],
        "batched_chunk_stories": int(c["input_ids"].shape[0]),
        "encode_ms": round(e, 3), "decode_ms": round(d, 3), "decode_over_encode": round(d / e, 4),
        "orders_equal": sum(x == y for x, y in zip(one, many)), "orders_total": len(one)}))


if __name__ == "__main__":
    main()
