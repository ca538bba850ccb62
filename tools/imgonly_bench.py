"""Image-only against text+image config 3 (ViT-B/16, H = 768, N = 5, 60 tokens per step), B
stories, bf16, in one process, the two models alternating:

  train  trainer.train_step (dropout on, fused AdamW), steps/s and stories/s: host clock around
         whole steps ending in a device synchronise, windows of at least --min-window seconds,
         the median window of each model;
  order  berson_pointer_network_batch (decode="beam", eval mode), stories/s, timed the same way.

    python tools/imgonly_bench.py [--batch 32] [--rounds 3] [--min-window 2.0] [--out FILE]

The image-only model runs the pair-sequence ViT (20 pairs x 393 tokens per story) and the head over
all 393 rows; the text+image model runs the same ViT, then 12 joint layers over 513 rows, and the
head over the 120 text rows. Prints one JSON line and writes it to --out (default
profiles/imgonly_bench.log). No threshold is asserted: the numbers are recorded in DESIGN §6.15.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from multimodal_sequencing_amd import model_zoo  # noqa: E402
from multimodal_sequencing_amd.berson import berson_pointer_network_batch  # noqa: E402
from multimodal_sequencing_amd.trainer import FusedAdamW, train_step  # noqa: E402

PRESETS = {"imgonly": "config3_imgonly", "text_image": "config3"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-window", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imgonly_bench.log"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B = a.batch
    p = model_zoo.PRESETS["config3"]
    batch = bench.synthetic_batch(B, p["N"], p["per_seq"], p["joint"]["vocab_size"], 224, dev,
                                  seed=4000)
    models = {k: model_zoo.build_preset(v, device=dev, dtype=torch.bfloat16) for k, v in
              PRESETS.items()}
    opts = {k: FusedAdamW(m.stores(), lr=1e-5, warmup=0, total_steps=10 ** 6)
            for k, m in models.items()}

    def train(k):
        models[k].train()
        loss = train_step(models[k], opts[k], [batch])
        torch.cuda.synchronize()
        return float(loss)

    def order(k):
        models[k].eval()
        out = berson_pointer_network_batch(models[k].args, models[k], None, batch)
        torch.cuda.synchronize()
        return out

    def window(fn, k):
        n, t0 = 0, time.perf_counter()
        while True:
            fn(k)
            n += 1
            dt = time.perf_counter() - t0
            if dt > a.min_window:
                return n / dt

    out = {"workload": f"config 3 (ViT-B/16, H=768, N=5, 60 tok/step), B={B}, bf16: image-only "
                       "(Tv=393, no joint stack) vs text+image (T=120+393, 12 joint layers)",
           "device": torch.cuda.get_device_name(0), "batch": B}
    for what, fn in (("train", train), ("order", order)):
        last = {k: [fn(k) for _ in range(2)][-1] for k in PRESETS}  # warm both
        rates = {k: [] for k in PRESETS}
        for _ in range(a.rounds):
            for k in PRESETS:
                rates[k].append(window(fn, k))
        for k in PRESETS:
            r = statistics.median(rates[k])
            out[f"{what}_{k}"] = {"calls_per_s": round(r, 3), "stories_per_s": round(r * B, 1),
                                  "windows": [round(x, 3) for x in rates[k]]}
            if what == "train":
                out[f"{what}_{k}"]["loss"] = round(last[k], 4)
        out[f"{what}_imgonly_over_text_image"] = round(
            out[f"{what}_imgonly"]["calls_per_s"] / out[f"{what}_text_image"]["calls_per_s"], 3)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
