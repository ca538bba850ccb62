"""Headline benchmark: multimodal fine-tuning steps/sec (fwd+bwd+optimizer) at N = 5 story steps,
pair sequence 512 (120 text + 393 ViT-B/16 tokens), BASELINE config 3 (1 GPU) / config 4 (DP).

One "step" = one optimizer step of the reference train loop (trainers/train.py:275-363) over a
per-GPU batch of B stories (B = 32, config 3), all 20 ordered pairs per story, bf16 compute with
fp32 master weights; synthetic seeded inputs already resident in HBM; random-init weights of the
exact architecture. Data parallel (config 4): one process per GPU, each rank takes its B stories
of the global batch by the DistributedSampler rule (train.py:158-161), gradients are averaged by
RCCL all-reduces issued from the layer backwards (trainer.GradAllReduce).

`value` is the whole-job aggregate: per-GPU-batch training steps per second summed over the
ranks, i.e. (stories/s over all GPUs) / B. With weak scaling (B fixed per GPU) the optimizer
step rate is `optimizer_steps_per_s` (= value / n_gpus), reported beside it.

Launch: `python bench.py --gpus N` re-launches itself under torch.distributed.run with N
processes (before touching the GPU) when WORLD_SIZE is not set; the driver's form
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
      --master-port P bench.py --gpus N --steps K --warmup W
runs directly. Rank 0 prints ONE JSON line.

A plain run does only what the headline needs: set-up, warm-up, the timed steps, the result line.
`--full` adds every other leg: HIP events around the bf16 NT GEMM launches of the timed steps (the
`roofline` entry), the eval forward in bf16 and MX-fp8 (`forward`), config 2, the RN50 backbone,
config 5 and the CPU oracle baseline; --no-gemm-timer, --fwd-steps 0, --no-config2, --no-rn50,
--no-config5 and --no-cpu-baseline drop single legs of it.
`--dump-outputs DIR` writes what the last timed step handed its caller (dump_outputs) as .npy
files: the inputs are seeded, so two builds of the library can be compared array for array.
"""
import argparse
import json
import re
import math
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from multimodal_sequencing_amd import _native as N  # noqa: E402
if os.environ.get("MMSEQ_BENCH_LIB"):  # A/B runs on one box: another build of the library
    N.LIB_PATH = os.environ["MMSEQ_BENCH_LIB"]
from multimodal_sequencing_amd import kernels as K  # noqa: E402
from multimodal_sequencing_amd import model_zoo  # noqa: E402
from multimodal_sequencing_amd.trainer import (FusedAdamW, GradAllReduce,  # noqa: E402
                                               distributed_indices, train_step)

PEAK_BF16_TFLOPS = 2500.0  # MI355X dense bf16 MFMA (MI355X_MICROARCH.md chip table)


def story_flops(Pst, Lt, Tv, H, Lj, W, Lv, patch, E, ff=4):
    """SURVEY §8(d) algorithmic fwd FLOPs per story (2 FLOP / MAC)."""
    npatch = Tv - 1
    T = Lt + Tv
    vit = 2 * (npatch * 3 * patch * patch * W + Lv * (12 * Tv * W * W + 2 * Tv * Tv * W) + Tv * W * E)
    joint = 2 * Lj * (12 * T * H * H + 2 * T * T * H)
    visn = 2 * Tv * E * H
    head = 2 * Pst * Lt * H * H + 2 * Pst * Lt * H
    return Pst * (vit + visn + joint) + head


def rows_layer_saving(Pst, Lt, Tv, H):
    """Forward FLOPs per story the text-rows last joint layer (kernels.ROWS) does not
    execute: the full layer 2 (12 T H^2 + 2 T^2 H) minus QKV over all T rows, attention for the
    Lt text queries against T keys, and the output projection + FFN on the Lt rows."""
    T = Lt + Tv
    full = 2 * (12 * T * H * H + 2 * T * T * H)
    rows = 2 * (3 * T * H * H + 9 * Lt * H * H + 2 * Lt * T * H)
    return Pst * (full - rows)


def synthetic_story(idx, Nst, per_seq, vocab, res, seed):
    """Story `idx` of the synthetic dataset: each step = <s>(0) + k ids
    ~ U[3, vocab) + </s>(2), labels = argsort(randperm(N)), images ~ N(0, 1). A pure function of
    (seed, idx), so any rank materialises exactly its own shard."""
    g = torch.Generator(device="cpu").manual_seed(seed * 1000003 + idx)
    k = per_seq - 2
    content = torch.randint(3, vocab, (Nst, k), generator=g)
    steps = torch.cat([torch.zeros(Nst, 1, dtype=torch.long), content,
                       torch.full((Nst, 1), 2, dtype=torch.long)], -1)
    labels = torch.argsort(torch.randperm(Nst, generator=g))
    images = torch.randn(Nst, 3, res, res, generator=g)
    return steps.view(Nst * per_seq), labels, images


def synthetic_batch(B, Nst, per_seq, vocab, res, device, seed, indices=None):
    """Batch of the stories `indices` (default 0..B-1) of the seeded synthetic dataset."""
    indices = list(range(B)) if indices is None else list(indices)
    ids, labels, images = zip(*(synthetic_story(i, Nst, per_seq, vocab, res, seed)
                                for i in indices))
    return {"input_ids": torch.stack(ids), "labels": torch.stack(labels),
            "images": torch.stack(images).to(device)}


class GemmTimer:
    """Records HIP events around every bf16 NT GEMM launch (the dominant kernel) on the stream it
    is launched on, to report achieved TFLOP/s per launch live from the timed region."""

    def __init__(self):
        self.recs = []
        self.on = False
        self._orig = N.gemm

    def install(self):
        orig = self._orig
        timer = self

        def wrapped(A, B, C, M, Nn, K, **kw):
            if timer.on and kw.get("trans", 0) == 0 and A.dtype == torch.bfloat16:
                s = torch.cuda.current_stream()
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record(s)
                orig(A, B, C, M, Nn, K, **kw)
                e1.record(s)
                bt = kw.get("batch", 1)
                # algorithmic HBM bytes: A, B, C once (+ residual / dact / aux tensors), bf16
                extra = sum(1 for k in ("resid", "dact", "aux") if kw.get(k) is not None)
                if kw.get("accumulate"):
                    extra += 1
                byts = 2.0 * bt * (M * K + Nn * K + M * Nn * (1 + extra))
                timer.recs.append((e0, e1, 2.0 * M * Nn * K * bt, byts))
            else:
                orig(A, B, C, M, Nn, K, **kw)

        N.gemm = wrapped
        import multimodal_sequencing_amd.kernels as Kmod
        Kmod.N.gemm = wrapped

    def summary(self):
        if not self.recs:
            return None
        t = sum(r[0].elapsed_time(r[1]) for r in self.recs) * 1e-3
        f = sum(r[2] for r in self.recs)
        b = sum(r[3] for r in self.recs)
        n = len(self.recs)
        return {"launches": n, "avg_us": t / n * 1e6, "avg_gflop": f / n / 1e9,
                "achieved_tflops": f / t / 1e12, "avg_alg_bytes": b / n}


DUMP_SAMPLE = 1 << 20  # elements kept of every flat buffer (2 stores x 3 buffers x 4 MB = 24 MB)


def dump_outputs(directory, loss, opt):
    """What train_step hands its caller after the last timed step, as float32 <name>.npy: the mean
    loss it returns and, from the buffers it updates in place, DUMP_SAMPLE elements of every flat
    store's fp32 master weights and AdamW moments at fixed seeded positions (the gradients are
    zero again when the step returns; the moments carry them)."""
    import numpy as np
    os.makedirs(directory, exist_ok=True)

    def save(name, t):
        np.save(os.path.join(directory, name + ".npy"), t.detach().float().cpu().numpy())

    save("loss", loss.reshape(1))
    for i, s in enumerate(opt.stores):
        n = s.master.numel()
        if n > DUMP_SAMPLE:
            g = torch.Generator(device="cpu").manual_seed(424243 + i)
            idx = torch.randint(0, n, (DUMP_SAMPLE,), generator=g).to(s.master.device)
        else:
            idx = torch.arange(n, device=s.master.device)
        save(f"store{i}_master", s.master[idx])
        save(f"store{i}_exp_avg", opt.m[i][idx])
        save(f"store{i}_exp_avg_sq", opt.v[i][idx])


def _newest_profile(pattern):
    import glob

    def order(f):  # r<round>_v<version>: numeric, so v10 sorts after v9
        m = re.match(r"r(\d+)_v(\d+)_", os.path.basename(f))
        return (int(m.group(1)), int(m.group(2))) if m else (-1, -1)
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)), key=order)
    return files[-1] if files else None


def measured_peak():
    """Dense bf16 MFMA rate measured on MI355X by tools/mfma_peak (random register operands,
    every SIMD issuing back to back): the best of its two MFMA shapes, or None."""
    f = _newest_profile("r*_mfma_peak.json")
    try:
        d = json.load(open(f))
        return max(d["bf16_16x16x32_tflops"], d["bf16_32x32x16_tflops"]), os.path.relpath(f, ROOT)
    except (TypeError, OSError, KeyError, ValueError):
        return None, None


def pmc_mfma_util(group="gemm256_nt"):
    """MFMA busy fraction of the roofline kernel from the newest committed PMC pass
    (tools/pmc_mfma.py: SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 x 4 SIMD x CUs))."""
    f = _newest_profile("r*_pmc_mfma_util.json")
    try:
        return json.load(open(f))[group]["mfma_util_mean"], os.path.relpath(f, ROOT)
    except (TypeError, OSError, KeyError, ValueError):
        return None, None


def pmc_traffic(group="gemm256_nt"):
    """Per-launch HBM traffic of the roofline kernel from the newest committed rocprofv3 --pmc
    summary (profiles/r*_pmc_traffic.json, made by tools/pmc_traffic.py: FETCH_SIZE x 2 +
    WRITE_SIZE, the gfx950 corrections of MI355X_MICROARCH.md), or None."""
    import glob
    def order(f):  # r<round>_v<version>: numeric, so v10 sorts after v9
        m = re.match(r"r(\d+)_v(\d+)_", os.path.basename(f))
        return (int(m.group(1)), int(m.group(2))) if m else (-1, -1)
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")), key=order)
    if not files:
        return None, None
    try:
        d = json.load(open(files[-1]))
        return d[group]["traffic_bytes"], os.path.relpath(files[-1], ROOT)
    except (OSError, KeyError, ValueError):
        return None, None


def profile_nt_launches():
    """Average duration of the bf16 NT GEMM's launches (every gemm256_nt_kernel instantiation with
    F8 = false) in the newest committed default-workload kernel statistics (profiles/rN_vM_kernel_stats.csv,
    rocprofv3 --kernel-trace --stats of this bench via tools/profile_round.sh): the profile-side
    figure beside the live HIP-event one, so the line's roofline follows from the file it cites."""
    import csv
    import glob

    def order(f):
        m = re.match(r"r(\d+)_v(\d+)_kernel_stats\.csv$", os.path.basename(f))
        return (int(m.group(1)), int(m.group(2))) if m else None
    files = [f for f in glob.glob(os.path.join(ROOT, "profiles", "r*_v*_kernel_stats.csv")) if order(f)]
    if not files:
        return None
    f = max(files, key=order)
    calls, ns = 0, 0.0
    try:
        for row in csv.DictReader(open(f)):
            m = re.search(r"gemm256_nt_kernel<([^>]*)>", row["Name"])
            if m and m.group(1).split(",")[-1].strip() == "false":
                calls += int(row["Calls"])
                ns += float(row["TotalDurationNs"])
    except (OSError, KeyError, ValueError):
        return None
    return (ns / calls / 1e3, calls, os.path.relpath(f, ROOT)) if calls else None


def _physical_cores():
    try:
        import psutil
        n = psutil.cpu_count(logical=False)
        if n:
            return n
    except ImportError:
        pass
    return os.cpu_count() or 1


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(preset, timed=3):
    """The CPU oracle (fp32 PyTorch restatement, oracle/berson_oracle.py) on host cores, by the
    BASELINE.md protocol: B = 1 story of the same config, eval mode, 1 warm-up, then the median
    of `timed` fwd+bwd iterations, torch threads = physical cores (capped at this job's
    16-CPU share of the box)."""
    from oracle import berson_oracle as O
    threads = max(1, min(16, _physical_cores()))
    torch.set_num_threads(threads)
    m = model_zoo.build_preset(preset, device="cpu", dtype=torch.float32)
    p = model_zoo.PRESETS[preset]
    data = synthetic_batch(1, p["N"], p["per_seq"], 50265, 224, "cpu", seed=7)
    cfg = {"N": p["N"], "heads": p["joint"]["num_attention_heads"], "inter_heads": 8,
           "text_only": p["vision"] is None, "vit_heads": None}
    times = []
    for it in range(1 + timed):
        params = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
        t0 = time.perf_counter()
        loss, _, _ = O.forward_loss(params, data["input_ids"].numpy(), data["labels"].numpy(),
                                    data["images"], cfg)
        loss.backward()
        dt = time.perf_counter() - t0
        print(f"[bench] cpu_baseline iteration {it} ({'warm-up' if it == 0 else 'timed'}): "
              f"{dt:.1f} s", file=sys.stderr, flush=True)
        if it > 0:
            times.append(dt)
    med = sorted(times)[len(times) // 2]
    return {"value": 1.0 / med, "unit": "stories/s (fwd+bwd, fp32)", "cores": threads,
            "kind": "port", "s_per_story": med,
            "sample": f"1 story ({p['N']} steps, {p['N'] * (p['N'] - 1)} pairs) fwd+bwd of the "
                      f"oracle, eval mode, 1 warm-up + median of {timed} "
                      f"({', '.join(f'{t:.1f}' for t in times)} s) on {threads} threads "
                      f"of {_cpu_model()}"}


def bench_config2(batch, steps, warmup, dev):
    """BASELINE config 2 (image-only MRM pretraining, scripts/wikihow_image_only_pretrain.sh):
    B stories of 5 synthetic 224^2 images per step, 2 sub-sampled per story into one ViT-B/16
    sequence, MRM loss + AdamW (lr 1e-5, warmup 1000), bf16, train mode. Per-step host draws as
    the reference's np.random calls. Forward FLOPs per story: ViT 73.2 GF + visn_fc
    + the LM head over 393 tokens to 30522 words (18.4 GF)."""
    from multimodal_sequencing_amd.pretraining import build_config2
    m = build_config2(device=dev, dtype=torch.bfloat16, seed=0)
    m.train()
    opt = FusedAdamW(m.stores(), lr=1e-5, warmup=1000, total_steps=warmup + steps)
    data = synthetic_batch(batch, 5, 10, 30522, 224, dev, seed=2000)

    def step():
        loss = m(data)[0]
        loss.backward()
        opt.step()
        m.zero_grad()
        return loss

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()  # steps ~10 ms each: at least 30 so the rate is not timer/host noise
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    g = 224 // 16
    Tv = 1 + 2 * g * g
    vit = 2 * (2 * g * g * 3 * 16 * 16 * 768 + 12 * (12 * Tv * 768 * 768 + 2 * Tv * Tv * 768)
               + Tv * 768 * 512)
    fwd = vit + 2 * Tv * 512 * 768 + 2 * Tv * 768 * 768 + 2 * Tv * 768 * 30522
    del m, opt
    torch.cuda.empty_cache()
    return {"workload": "config2: image-only MRM pretraining, ViT-B/16 over 2 of 5 images "
                        f"(T={Tv}), LM head to 30522 words, B={batch}, bf16, train mode",
            "steps_per_s": steps / dt, "ms_per_step": dt / steps * 1e3,
            "stories_per_s": batch * steps / dt,
            "fwd_tflops": batch * steps / dt * fwd / 1e12,
            "note": "the MRM loss has an exactly-zero ViT gradient (pretraining.py docstring): "
                    "backward = visn_fc + heads; AdamW updates every parameter",
            "loss": float(loss.item())}


def bench_config5(stories, micro, steps, warmup, dev):
    """BASELINE config 5 shape on one GPU (scripts/recipeqa_finetune.sh): ViT-L/14 (patch 14,
    1024 wide, 24 layers) + RoBERTa-large-shaped 24 x 1024 joint encoder, N = 9 steps -> 72 pairs
    per story, 128 tokens per step -> T = 256 + 513 = 769: the full training step in bf16 and with
    the fp8 forward GEMMs (kernels.fp8_forward(training=True): QKV / O / FC1 / FC2 of every ViT block
    and joint layer on v_mfma_scale_f32_16x16x128_f8f6f4, backward bf16), plus the eval forward (no
    grad) in bf16 and MX-fp8: stories/s, speedups and the fp8 - bf16 loss differences."""
    preset = model_zoo.PRESETS["config5"]
    m = model_zoo.build_preset("config5", device=dev, dtype=torch.bfloat16, seed=0)
    opt = FusedAdamW(m.stores(), lr=5e-6, warmup=100, total_steps=3 * (warmup + steps))
    data = synthetic_batch(stories, preset["N"], preset["per_seq"], 50265, 224, dev, seed=3000)
    mbs = [{k: v[o:o + micro] for k, v in data.items()} for o in range(0, stories, micro)]
    Nst, per = preset["N"], preset["per_seq"]
    V = m.bert.vision
    g = 224 // V["patch"]
    Tv = 1 + 2 * g * g
    J = preset["joint"]
    fwd = story_flops(Nst * (Nst - 1), 2 * per, Tv, J["hidden_size"], J["num_hidden_layers"],
                      V["width"], V["layers"], V["patch"], V["embed"])
    train = {}
    for name, fp8, dg in (("bf16", False, False), ("mxfp8_fwd", True, False),
                          ("mxfp8_fwd_dgrad", True, True)):
        m.train()
        with K.fp8_forward(fp8, training=True, dgrad=dg):
            for _ in range(warmup):
                train_step(m, opt, mbs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = train_step(m, opt, mbs)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        train[name] = {"steps_per_s": steps / dt, "ms_per_step": dt / steps * 1e3,
                       "stories_per_s": stories * steps / dt,
                       "model_tflops": stories * steps / dt * 3 * fwd / 1e12,
                       "model_flops_util": stories * steps / dt * 3 * fwd / 1e12 / PEAK_BF16_TFLOPS,
                       "loss": float(loss.item())}
    m.eval()
    fwd_legs = {}
    with torch.no_grad():
        for name, fp8, sites in (("bf16", False, None), ("mxfp8", True, None),
                                 ("mxfp8_vit_only", True, K.FP8_VIT_ONLY)):
            with K.fp8_forward(fp8, sites=sites):
                for _ in range(2):
                    lv = m(mbs[0])[0]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    for mb in mbs:
                        lv = m(mb)[0]
                torch.cuda.synchronize()
                fdt = time.perf_counter() - t0
            fwd_legs[name] = {"stories_per_s": stories * steps / fdt,
                              "tflops": stories * steps / fdt * fwd / 1e12,
                              "loss": float(lv.item())}
    fwd_legs["mxfp8_speedup"] = fwd_legs["mxfp8"]["stories_per_s"] / fwd_legs["bf16"]["stories_per_s"]
    fwd_legs["mxfp8_loss_rel_diff"] = (abs(fwd_legs["mxfp8"]["loss"] - fwd_legs["bf16"]["loss"]) /
                                       max(1e-12, abs(fwd_legs["bf16"]["loss"])))
    # the mixed placement the per-site error budget picks: ViT on the fp8 MFMA, joint
    # encoder bf16 (ordering margins within 2x of bf16's error instead of 11x)
    fwd_legs["mxfp8_vit_only_speedup"] = (fwd_legs["mxfp8_vit_only"]["stories_per_s"] /
                                          fwd_legs["bf16"]["stories_per_s"])
    del m, opt, mbs, data
    torch.cuda.empty_cache()
    out = {"workload": f"config5 shape: ViT-L/14 + 24x1024 joint encoder + BERSON, N={Nst}, "
                       f"{Nst * (Nst - 1)} pairs/story, pair seq {2 * per}+{Tv}={2 * per + Tv}, "
                       f"{stories} stories/step in micro-batches of {micro}, train mode (dropout), 1 GPU; "
                       f"the last joint layer runs on the text rows only"
                       f"{' (in bf16 under fp8_forward)' if K.ROWS['on'] else ' (off: MMSEQ_ROWS=0)'}",
           **train["bf16"], "fwd_tflop_per_story": fwd / 1e12,
           "loss_note": "the three training legs run one after another on one model and optimizer "
                        "(bf16, then mxfp8_fwd, then mxfp8_fwd_dgrad), so each leg's loss is after "
                        "a different number of updates and the training losses are not comparable "
                        "across legs; eval_forward's two losses are (same weights, same batch)",
           "train_mxfp8_forward": dict(train["mxfp8_fwd"], speedup=train["mxfp8_fwd"]["steps_per_s"] /
                                       train["bf16"]["steps_per_s"],
                                       mode="kernels.fp8_forward(training=True): the four encoder "
                                            "GEMMs of every layer's forward on the MX-fp8 MFMA, "
                                            "backward bf16 (runs after the bf16 steps, same optimizer)"),
           "train_mxfp8_forward_dgrad": dict(train["mxfp8_fwd_dgrad"],
                                             speedup=train["mxfp8_fwd_dgrad"]["steps_per_s"] /
                                             train["bf16"]["steps_per_s"],
                                             mode="fp8_forward(training=True, dgrad=True): also the "
                                                  "four data-gradient GEMMs of every layer on the "
                                                  "MX-fp8 MFMA (dY quantised per call); weight "
                                                  "gradients bf16"),
           "eval_forward": fwd_legs}
    return out


def bench_config3_rn50(stories, micro, steps, warmup, dev):
    """The reference's default backbone (--clip_model_name RN50, train.py:1011-1019) with the
    config-3 joint encoder: CLIP ModifiedResNet-50 over each story's 5 images (the product runs the
    convolutions once per unique image; the reference, once per pair slot: 8x the work), attention
    pool over each pair's two images (99 tokens), 12 x 768 joint encoder over T = 120 + 99, BERSON,
    full bf16 training step with train-mode BatchNorm."""
    m = model_zoo.build_preset("config3_rn50", device=dev, dtype=torch.bfloat16, seed=0)
    m.train()
    preset = model_zoo.PRESETS["config3_rn50"]
    opt = FusedAdamW(m.stores(), lr=5e-6, warmup=100, total_steps=warmup + steps)
    data = synthetic_batch(stories, preset["N"], preset["per_seq"], 50265, 224, dev, seed=4000)
    mbs = [{k: v[o:o + micro] for k, v in data.items()} for o in range(0, stories, micro)]
    for _ in range(warmup):
        train_step(m, opt, mbs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = train_step(m, opt, mbs)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del m, opt, mbs, data
    torch.cuda.empty_cache()
    return {"workload": f"config3_rn50: CLIP RN50 (224^2, unique images) + 12x768 joint encoder + "
                        f"BERSON, N=5, 20 pairs/story, pair seq 120+99=219, {stories} stories/step "
                        f"in micro-batches of {micro}, bf16, train mode, 1 GPU",
            "steps_per_s": steps / dt, "ms_per_step": dt / steps * 1e3,
            "stories_per_s": stories * steps / dt, "loss": float(loss.item())}


def _relaunch(args):
    """`--gpus N` without a torchrun environment: start N ranks under torch.distributed.run as
    a child process (nothing here has touched the GPU) and return its exit code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={args.gpus}", "--master-addr=127.0.0.1", f"--master-port={port}",
           os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.run(cmd, env=env).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", default="config3")
    ap.add_argument("--batch", type=int, default=32, help="stories per GPU per step")
    ap.add_argument("--micro", type=int, default=32,
                    help="stories per micro-batch (default: the whole per-GPU batch in one pass; "
                         "16 measured 1.8%% slower on the same box, profiles/r2_v14_micro_ab.txt)")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary legs (GEMM roofline events, eval forward, config 2, "
                         "RN50, config 5, CPU baseline); the --no-* flags and --fwd-steps 0 drop "
                         "single legs of it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's outputs (loss, sampled "
                         "weights and AdamW moments) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-gemm-timer", action="store_true")
    ap.add_argument("--fwd-micro", type=int, default=0,
                    help="stories per forward-leg call (0: the whole per-GPU batch)")
    ap.add_argument("--fwd-steps", type=int, default=3,
                    help="forward-only passes timed after the training steps (north-star check)")
    ap.add_argument("--bucket-mb", type=float, default=64.0,
                    help="DP all-reduce bucket cap (MB of fp32 grads)")
    ap.add_argument("--no-config2", action="store_true", help="skip the config-2 leg")
    ap.add_argument("--no-config5", action="store_true", help="skip the config-5 leg")
    ap.add_argument("--no-rn50", action="store_true", help="skip the RN50-backbone leg")
    ap.add_argument("--dist-backend", default="nccl",
                    help="nccl (= RCCL, one GPU per rank); gloo only to rehearse several ranks "
                         "sharing one GPU (RCCL refuses duplicate devices)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(_relaunch(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    ndev = torch.cuda.device_count()
    if args.dist_backend == "nccl" and world > ndev:
        raise SystemExit(f"bench.py: {world} ranks but {ndev} GPUs (RCCL needs one GPU per rank)")
    torch.cuda.set_device(local % ndev)
    dev = torch.device("cuda", local % ndev)
    if world > 1:
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.dist_backend)
        assert dist.get_world_size() == args.gpus

    preset = model_zoo.PRESETS[args.config]
    model = model_zoo.build_preset(args.config, device=dev, dtype=torch.bfloat16, seed=0)
    model.train()  # dropout p = 0.1 at every reference site, counter-based masks
    model.bert.dropout_seed = 1 + rank
    stores = model.stores()
    # the reference's schedule: warmup 100 (wikihow_finetune.sh), t_total = the run length
    opt = FusedAdamW(stores, lr=5e-6, warmup=100, total_steps=args.warmup + args.steps)
    reducer = None
    if world > 1:
        units, begin = model.ddp_units()
        reducer = GradAllReduce(stores, bucket_mb=args.bucket_mb, units=units, begin_units=begin)
    # this rank's shard of the global batch (DistributedSampler rule over world * B stories)
    shard = distributed_indices(args.batch * world, world, rank)
    data = synthetic_batch(args.batch, preset["N"], preset["per_seq"], 50265, 224, dev,
                           seed=1000, indices=shard)
    mbs = []
    for o in range(0, args.batch, args.micro):
        mbs.append({k: v[o:o + args.micro] for k, v in data.items()})

    timer = GemmTimer()
    if args.full and not args.no_gemm_timer:
        timer.install()
    for _ in range(args.warmup):
        train_step(model, opt, mbs, reducer)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    timer.on = True
    if reducer is not None:
        reducer.timing = True
    t0 = time.perf_counter()
    loss = None
    for _ in range(args.steps):
        loss = train_step(model, opt, mbs, reducer)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    timer.on = False
    ar_stats = None
    if reducer is not None:
        reducer.timing = False
        mine = reducer.timing_summary() or {}
        every = [None] * world
        dist.all_gather_object(every, mine)
        ar_stats = {"buckets_per_step": mine.get("buckets"),
                    "issued_during_backward": mine.get("issued_in_backward"),
                    "exposed_ms_per_step_by_rank": [e.get("exposed_ms_mean") for e in every],
                    "exposed_ms_max_by_rank": [e.get("exposed_ms_max") for e in every],
                    "definition": "GPU time the compute stream waits inside GradAllReduce.finish() "
                                  "after the last backward kernel (HIP events around the waits), "
                                  "mean over the timed steps"}
    if world > 1:
        t = torch.tensor([dt], device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, loss, opt)

    # North-star forward check (stories/s_fwd x fwd FLOP/story / peak): the same
    # batch, eval mode (no dropout), no autograd graph, timed like the training steps.
    fwd_dt = None
    if args.full and args.fwd_steps > 0:
        model.eval()
        # inference keeps no activations for a backward: the whole per-GPU batch in one pass
        # (--fwd-micro stories per call), bigger GEMMs and half the launches of the training split
        fm = max(1, min(args.fwd_micro or args.batch, args.batch))
        fbs = [{k: v[o:o + fm] for k, v in data.items()} for o in range(0, args.batch, fm)]
        with torch.no_grad():
            for b in fbs:
                model(b)
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            torch.cuda.synchronize()
            f0 = time.perf_counter()
            for _ in range(args.fwd_steps):
                for b in fbs:
                    model(b)
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            torch.cuda.synchronize()
            fwd_dt = time.perf_counter() - f0
            floss = {"bf16": float(model(fbs[0])[0])}
            # the same forward with the MX-fp8 encoder GEMMs (kernels.fp8_forward: QKV, O, FC1, FC2
            # of every ViT block and joint layer on v_mfma_scale_f32_16x16x128_f8f6f4); the
            # first pass quantises the weights
            with K.fp8_forward(True):
                for b in fbs:
                    model(b)
                torch.cuda.synchronize()
                if world > 1:
                    dist.barrier()
                torch.cuda.synchronize()
                f0 = time.perf_counter()
                for _ in range(args.fwd_steps):
                    for b in fbs:
                        model(b)
                torch.cuda.synchronize()
                if world > 1:
                    dist.barrier()
                torch.cuda.synchronize()
                fwd8_dt = time.perf_counter() - f0
                floss["mxfp8"] = float(model(fbs[0])[0])
        model.train()
        if world > 1:
            t = torch.tensor([fwd_dt, fwd8_dt], device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            fwd_dt, fwd8_dt = t[0].item(), t[1].item()

    Nst, per = preset["N"], preset["per_seq"]
    Pst = Nst * (Nst - 1)
    J = preset["joint"]
    V = model.bert.vision
    g = 224 // V["patch"]
    Tv = 1 + 2 * g * g
    Lt = 2 * per
    fwd = story_flops(Pst, Lt, Tv, J["hidden_size"], J["num_hidden_layers"], V["width"],
                      V["layers"], V["patch"], V["embed"])
    # FLOPs actually executed: the text-rows last joint layer skips its visual rows' work
    fwd_exec = fwd - (rows_layer_saving(Pst, Lt, Tv, J["hidden_size"]) if K.ROWS["on"] else 0)
    stories = args.batch * args.steps * world
    steps_s = args.steps * world / dt
    out = {
        "metric": "multimodal steps/sec (fwd+bwd) at N=5 steps, seq=512, ViT-B/16; 1/2/4/8 GPU",
        "value": steps_s, "unit": "steps/s",
        "value_definition": f"aggregate {args.batch}-story per-GPU training steps (fwd+bwd+"
                            "all-reduce+AdamW) per second summed over all GPUs = stories_per_s / "
                            f"{args.batch}",
        "optimizer_steps_per_s": args.steps / dt,
        "n_gpus": world, "steps": args.steps,
        "dist_backend": dist.get_backend() if world > 1 else None,
        "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
        "data": "synthetic (seeded token ids U[3,50265), N(0,1) 224x224 images), random-init "
                "weights, train mode (dropout 0.1)",
        "config": {"workload": f"{args.config}: ViT-B/16 + 12x768 joint encoder + BERSON, "
                               f"N={Nst} steps, {Pst} pairs/story, pair seq {Lt}+{Tv}={Lt + Tv}",
                   "global_batch": args.batch * world, "stories_per_gpu": args.batch,
                   "micro_batch": args.micro, "seq_len": Lt + Tv, "parallelism": f"dp{world}",
                   "allreduce": (f"{'RCCL' if args.dist_backend == 'nccl' else args.dist_backend} "
                                 f"mean all-reduce in <= {args.bucket_mb:g} MB buckets issued "
                                 "from the layer backwards") if world > 1 else None},
        "stories_per_s": stories / dt,
        "model_tflops": stories / dt * 3 * fwd / 1e12,
        "model_flops_util": stories / dt * 3 * fwd / 1e12 / PEAK_BF16_TFLOPS,
        "executed_flops_util": stories / dt * 3 * fwd_exec / 1e12 / PEAK_BF16_TFLOPS,
        "flops_note": "model FLOPs = the reference's computation (SURVEY 8d); executed = without the "
                      "last joint layer's visual rows, which the text-rows layer does not compute",
        "loss": float(loss.item()) if loss is not None else None,
    }
    if ar_stats is not None:
        out["allreduce"] = ar_stats
    _mpk, _ = measured_peak()
    if _mpk:  # stories/s x (fwd+bwd FLOP/story) / measured peak
        out["model_flops_util_of_measured_peak"] = stories / dt * 3 * fwd / 1e12 / _mpk
    if fwd_dt is not None:
        fst = args.batch * args.fwd_steps * world / fwd_dt
        mpk, _src = measured_peak()
        out["forward"] = {"stories_per_s": fst, "ms_per_batch": fwd_dt / args.fwd_steps * 1e3,
                          "stories_per_call": fm,
                          "tflops": fst * fwd / 1e12,
                          "mfma_frac": fst * fwd / 1e12 / PEAK_BF16_TFLOPS,
                          "mfma_frac_executed": fst * fwd_exec / 1e12 / PEAK_BF16_TFLOPS,
                          "mfma_frac_of_measured_peak": (fst * fwd / 1e12 / mpk) if mpk else None,
                          "mode": "eval (no dropout), torch.no_grad, full model forward incl. "
                                  "BERSON head + loss; ViT + joint encoder are >99.9% of FLOPs"}
        f8 = args.batch * args.fwd_steps * world / fwd8_dt
        out["forward"]["mxfp8"] = {
            "stories_per_s": f8, "tflops": f8 * fwd / 1e12, "speedup_vs_bf16": f8 / fst,
            "loss_bf16": floss["bf16"], "loss_mxfp8": floss["mxfp8"],
            "loss_rel_diff": abs(floss["mxfp8"] - floss["bf16"]) / max(1e-12, abs(floss["bf16"])),
            "mode": "the same forward under kernels.fp8_forward(): the four encoder GEMMs of every "
                    "ViT block and joint layer on the MX-fp8 MFMA (tests/test_fp8_gpu.py)"}
    gs = timer.summary()
    if gs:
        traffic, tsrc = pmc_traffic()
        if (args.config, args.batch, args.micro) != ("config3", 32, 32):
            traffic, tsrc = None, None  # the committed PMC pass profiles the default workload
        mpeak, msrc = measured_peak()
        util, usrc = pmc_mfma_util()
        if (args.config, args.batch, args.micro) != ("config3", 32, 32):
            util, usrc = None, None
        out["roofline"] = {"bound": "mfma", "kernel": "gemm256_nt_kernel (bf16 NT: fwd + dgrad)",
                           "achieved": gs["achieved_tflops"], "peak": PEAK_BF16_TFLOPS,
                           "unit": "TFLOP/s", "frac": gs["achieved_tflops"] / PEAK_BF16_TFLOPS,
                           "peak_measured": mpeak, "peak_measured_source": msrc,
                           "frac_of_measured": (gs["achieved_tflops"] / mpeak) if mpeak else None,
                           "mfma_busy_pmc": util, "mfma_busy_source": usrc,
                           "traffic": traffic, "traffic_unit": "bytes per launch (PMC)",
                           "traffic_source": tsrc,
                           "algorithmic_bytes_per_launch": gs["avg_alg_bytes"],
                           "launches": gs["launches"],
                           "avg_launch_us": gs["avg_us"], "avg_gflop_per_launch": gs["avg_gflop"],
                           "frac_source": "HIP events around every launch inside this run's timed region"}
        prof = profile_nt_launches()
        if prof and (args.config, args.batch, args.micro) == ("config3", 32, 32):
            pus, pcalls, psrc = prof
            out["roofline"].update({
                "frac_profile": gs["avg_gflop"] * 1e9 / (pus * 1e-6) / 1e12 / PEAK_BF16_TFLOPS,
                "profile_avg_launch_us": pus, "profile_launches": pcalls, "profile_source": psrc,
                "frac_profile_note": "the same average GFLOP per launch over the average duration of "
                                     "the bf16 gemm256_nt_kernel launches in the cited rocprofv3 kernel "
                                     "statistics (a separate, profiled run of this workload)"})
    legs = args.full and world == 1  # the secondary legs: one GPU, --full only
    if legs and not args.no_config2:
        try:
            out["config2"] = bench_config2(32, max(30, args.steps), max(3, args.warmup), dev)
        except Exception as e:  # a secondary leg: reported, never required for the headline
            out["config2"] = {"error": repr(e)}
    if legs and not args.no_rn50:
        try:
            out["config3_rn50"] = bench_config3_rn50(32, 16, max(2, args.steps), 1, dev)
        except Exception as e:  # a secondary leg: reported, never required for the headline
            out["config3_rn50"] = {"error": repr(e)}
    if legs and not args.no_config5:
        try:
            out["config5"] = bench_config5(4, 2, 2, 1, dev)
        except Exception as e:
            out["config5"] = {"error": repr(e)}
    if legs and not args.no_cpu_baseline:
        try:
            out["cpu_baseline"] = cpu_baseline(args.config)
            out["cpu_baseline"]["tflops"] = out["cpu_baseline"]["value"] * 3 * fwd / 1e12
        except Exception as e:  # the baseline is reported, never required for the GPU number
            out["cpu_baseline"] = {"value": None, "error": repr(e)}
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
