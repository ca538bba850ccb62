"""The evaluation head of the text+image pretraining stage at its stated size (vocab 50265, H = 768,
bf16), in one process, the variants alternating call by call:

  kernel  over one row-padded logit buffer [M][50304] with M = 48 (one evaluation batch of 4
          stories at mlm_probability 0.1) and M = 512:
            eval        mmseq_xent_eval at k = 5 with totals: lse, loss, rank, top-5 in ONE pass
            fwd         (a) mmseq_xent_fwd alone: what training pays for lse and the loss
            fwd_torch   (b) mmseq_xent_fwd, then torch.topk and the rank by comparison and sum in
                        torch: the same quantities from parts that existed before (three more
                        passes and [M][V] temporaries; torch's tie rule, not the kernel's)
  batch   a whole LXRTPretraining.evaluate_batch against model(batch) under no_grad, eval mode,
          B = 4 stories, for each objective

    python tools/pretrain_eval_bench.py [--iters 30] [--batch 4] [--part all|kernel|batch]

Device events around each call, median after warm-up. The buffer (4.8 MB at M = 48) stays
cache-resident between calls, as it is in the product, where the decoder GEMM has just written it.
Nothing here asserts a threshold. Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from multimodal_sequencing_amd import _native as N  # noqa: E402
from multimodal_sequencing_amd.pretraining import MM_OBJECTIVES, build_pretrain_mm  # noqa: E402

IGNORE = -100
V, K_TOP = 50265, 5


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def alternate(variants, iters, warm=5):
    """{name: median ms}, the variants called in turn so that none owns a clock state."""
    ms = {k: [] for k in variants}
    for it in range(warm + iters):
        for k, fn in variants.items():
            t = timed(fn)
            if it >= warm:
                ms[k].append(t)
    return {k: round(statistics.median(v), 4) for k, v in ms.items()}


def kernel_part(M, dev, iters):
    ld = (V + 63) // 64 * 64
    g = torch.Generator().manual_seed(M)
    logits = (torch.randn(M, ld, generator=g) * 2).to(torch.bfloat16).to(dev)
    labels = torch.randint(0, V, (M,), generator=g).to(dev)
    lse, row = torch.empty(M, device=dev), torch.empty(M, device=dev)
    stats = torch.empty(2, device=dev)
    rank = torch.empty(M, dtype=torch.int32, device=dev)
    idx = torch.empty(M, K_TOP, dtype=torch.int32, device=dev)
    val = torch.empty(M, K_TOP, device=dev)
    totals = torch.zeros(4, dtype=torch.float64, device=dev)
    cols = torch.arange(V, device=dev)[None, :]

    def ev():
        N.xent_eval(logits, V, labels, IGNORE, K_TOP, lse, row, rank, idx, val, totals, stats)

    def fwd():
        N.xent_fwd(logits, V, labels, IGNORE, lse, row, stats)

    def fwd_torch():
        N.xent_fwd(logits, V, labels, IGNORE, lse, row, stats)
        x = logits[:, :V]
        top = torch.topk(x, K_TOP, dim=1)
        gold = x.gather(1, labels[:, None])
        r = (x > gold).sum(1) + ((x == gold) & (cols < labels[:, None])).sum(1)
        return top, r

    out = alternate({"eval": ev, "fwd": fwd, "fwd_torch": fwd_torch}, iters)
    out["eval_over_fwd"] = round(out["eval"] / out["fwd"], 3)
    out["eval_over_fwd_torch"] = round(out["eval"] / out["fwd_torch"], 3)
    return out


def batch_part(B, dev, iters):
    import pretrain_bench
    m = build_pretrain_mm(device=dev, dtype=torch.bfloat16, seed=0).eval()
    Nst, per_seq = 5, 60
    batch = pretrain_bench.make_batch(B, Nst, per_seq, V, dev, seed=3000)
    g = torch.Generator().manual_seed(1)
    ids = batch["input_ids"]
    special = (ids == 0) | (ids == 1) | (ids == 2)
    pick = (torch.rand(ids.shape, generator=g) < 0.1) & ~special  # mlm_probability 0.1
    batch["masked_lm_labels"] = torch.where(pick, ids, torch.full_like(ids, IGNORE))
    Tv = 1 + 2 * (224 // 16) ** 2
    every = list(m.multimodal_pretrain_objectives)
    out = {}
    for obj in MM_OBJECTIVES:
        m.multimodal_pretrain_objectives = [obj]
        draws = m.draw_mm(B, Nst, Tv, rng=np.random.RandomState(7))
        m.multimodal_pretrain_objectives = every
        b = dict(batch, draws=draws)
        rows = {}

        def model():
            with torch.no_grad():
                m(b)

        def evaluate():
            rows["n"] = m.evaluate_batch(b, topk=K_TOP)[3]["mlm"]["rows"].numel()

        ms = alternate({"model_no_grad": model, "evaluate_batch": evaluate}, iters, warm=3)
        ms["labelled_rows"] = rows["n"]
        ms["evaluate_over_model"] = round(ms["evaluate_batch"] / ms["model_no_grad"], 3)
        out[obj] = ms
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--part", choices=["all", "kernel", "batch"], default="all",
                    help="kernel: the part to run under a kernel trace for device-side durations")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"workload": f"masked-LM evaluation head, vocab {V}, bf16, k = {K_TOP}; times in ms",
           "device": torch.cuda.get_device_name(0)}
    if a.part in ("all", "kernel"):
        out["kernel"] = {f"M={M}": kernel_part(M, dev, a.iters) for M in (48, 512)}
    if a.part in ("all", "batch"):
        out["batch"] = batch_part(a.batch, dev, max(a.iters // 3, 5))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
