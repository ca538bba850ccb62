"""Text+image pretraining step (pretraining.build_pretrain_mm: ViT-B/16 + 12 x 768, vocab 50265,
N = 5 steps of 60 tokens, T = 120 + 393) at B stories, bf16, dropout on, full trainer.train_step,
for each objective, with the masked-LM head in two modes, in one process:

  (a) labelled  the product path (kernels.MlmLossFn): the labelled rows are compacted, transform
                and tied decoder run on them only, mmseq_xent_fwd / _bwd fuse the loss;
  (b) all_rows  a baseline built here from parts that existed before: every text row through the
                transform (LinearFn / LayerNormFn) and the decoder (N.gemm into the row-padded
                buffer, NT dgrad and TN wgrad GEMMs), the loss by torch's cross_entropy.

    python tools/pretrain_bench.py [--batch 32] [--rounds 3] [--min-window 2.0]

steps/s: host clock around whole train steps ending in a device synchronise, in windows of at least
--min-window seconds, the two modes alternating, the median window of each. mlm_head_ms: device
events around the head's forward + backward alone (a detached lang_output of the step's shape and
the step's labels), median of 7 after warm-up. Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from multimodal_sequencing_amd import _native as N  # noqa: E402
from multimodal_sequencing_amd import kernels as K  # noqa: E402
from multimodal_sequencing_amd.pretraining import MM_OBJECTIVES, build_pretrain_mm  # noqa: E402
from multimodal_sequencing_amd.trainer import FusedAdamW, train_step  # noqa: E402

IGNORE = -100


class AllRowsDecoderFn(torch.autograd.Function):
    """logits [rows][ld] = h W^T + b for every row (N.gemm, ld = vocab rounded up to 64, padding
    columns zero); backward: NT dgrad, TN wgrad into the word table + bias."""

    @staticmethod
    def forward(ctx, h, anchor, wstore, wname, bstore, bname):
        h = h.contiguous()
        W = wstore.w(wname)
        V = W.shape[0]
        ld = (V + 63) // 64 * 64
        out = torch.zeros(h.shape[0], ld, device=h.device, dtype=h.dtype)
        N.gemm(h, W, out, h.shape[0], V, h.shape[1], ldc=ld, bias=bstore.f32(bname))
        ctx.save_for_backward(h)
        ctx.meta = (wstore, wname, bstore, bname, V)
        return out

    @staticmethod
    def backward(ctx, dl):
        (h,) = ctx.saved_tensors
        wstore, wname, bstore, bname, V = ctx.meta
        dl = dl.contiguous()
        ld = dl.shape[1]
        gW, gb = wstore.g(wname), bstore.g(bname)
        V8 = V // 8 * 8
        N.gemm_wgrad(dl, h, gW[:V8], gb[:V8], lddy=ld)
        if V8 < V:
            N.gemm_wgrad(dl[:, V8:], h, gW[V8:], gb[V8:], lddy=ld)
        dh = torch.empty_like(h)
        N.gemm(dl, K._decoder_wt(wstore, wname), dh, h.shape[0], h.shape[1], ld)
        return dh, None, None, None, None, None


def all_rows_mlm(lang_output, labels, ignore_index, anchor, head_store, word_store,
                 wname="embeddings.word_embeddings.weight", prefix="cls.predictions."):
    x = lang_output.reshape(-1, lang_output.shape[-1])
    t = K.LinearFn.apply(x, anchor, head_store, prefix + "transform.dense.weight",
                         prefix + "transform.dense.bias", K.GELU)
    t = K.LayerNormFn.apply(t, anchor, head_store, prefix + "transform.LayerNorm", 1e-12)
    logits = AllRowsDecoderFn.apply(t, anchor, word_store, wname, head_store, prefix + "bias")
    V = word_store.w(wname).shape[0]
    return torch.nn.functional.cross_entropy(logits[:, :V].float(),
                                             labels.reshape(-1).to(logits.device),
                                             ignore_index=ignore_index)


LABELLED = K.MlmLossFn.apply
MODES = {"labelled": LABELLED, "all_rows": all_rows_mlm}


def make_batch(B, Nst, per_seq, vocab, dev, seed):
    data = bench.synthetic_batch(B, Nst, per_seq, vocab, 224, dev, seed=seed)
    ids = data["input_ids"]
    g = torch.Generator().manual_seed(seed + 1)
    special = (ids == 0) | (ids == 1) | (ids == 2)
    pick = (torch.rand(ids.shape, generator=g) < 0.15) & ~special  # BERT's 15 % masking rate
    labels = torch.where(pick, ids, torch.full_like(ids, IGNORE))
    return {"input_ids": ids, "attention_mask": (ids != 1).long(), "token_type_ids": None,
            "masked_lm_labels": labels, "images": data["images"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-window", type=float, default=2.0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = build_pretrain_mm(device=dev, dtype=torch.bfloat16, seed=0).train()
    opt = FusedAdamW(m.stores(), lr=1e-5, warmup=0, total_steps=10 ** 6)
    B, Nst, per_seq = a.batch, 5, 60
    batch = make_batch(B, Nst, per_seq, 50265, dev, seed=3000)
    Tv = 1 + 2 * (224 // 16) ** 2
    out = {"workload": f"text+image pretraining step, ViT-B/16 + 12x768, vocab 50265, B={B}, "
                       f"T={2 * per_seq}+{Tv}, bf16, dropout on",
           "device": torch.cuda.get_device_name(0), "batch": B, "objectives": {}}
    every = list(m.multimodal_pretrain_objectives)
    for obj in MM_OBJECTIVES:
        m.multimodal_pretrain_objectives = [obj]  # the draws of this objective, every step
        draws = m.draw_mm(B, Nst, Tv, rng=np.random.RandomState(7))
        m.multimodal_pretrain_objectives = every
        b = dict(batch, draws=draws)

        def step(mode):
            K.MlmLossFn.apply = staticmethod(MODES[mode])
            loss = train_step(m, opt, [b])
            torch.cuda.synchronize()
            return float(loss)

        def window(mode):
            n, t0 = 0, time.perf_counter()
            while True:
                step(mode)
                n += 1
                dt = time.perf_counter() - t0
                if dt > a.min_window:
                    return n / dt

        losses = {k: [step(k) for _ in range(2)][-1] for k in MODES}  # warm both
        rates = {k: [] for k in MODES}
        for _ in range(a.rounds):
            for k in MODES:
                rates[k].append(window(k))
        # the head alone: a detached lang_output of the step's shape, the sub-sampled labels
        from multimodal_sequencing_amd.pretraining import subsample_text
        labels = subsample_text(batch["input_ids"], batch["attention_mask"], None,
                                batch["masked_lm_labels"], draws["sub_idx"], Nst, 0, 1, IGNORE)[3]
        lang = (torch.randn(B, 2 * per_seq, 768, device=dev) * 0.5).to(torch.bfloat16)
        head_ms = {k: [] for k in MODES}
        for it in range(10):
            for k in MODES:
                x = lang.clone().requires_grad_()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                loss = MODES[k](x, labels, IGNORE, m._anchor, m.store, m.bert.store)
                loss.backward()
                ev[1].record()
                torch.cuda.synchronize()
                if it >= 3:
                    head_ms[k].append(ev[0].elapsed_time(ev[1]))
        m.zero_grad()
        ra, rb = (statistics.median(rates[k]) for k in ("labelled", "all_rows"))
        ha, hb = (statistics.median(head_ms[k]) for k in ("labelled", "all_rows"))
        out["objectives"][obj] = {
            "labelled_rows": int((labels != IGNORE).sum()), "text_rows": int(labels.numel()),
            "steps_per_s_labelled": round(ra, 3), "steps_per_s_all_rows": round(rb, 3),
            "steps_ratio": round(ra / rb, 3),
            "windows_labelled": [round(x, 3) for x in rates["labelled"]],
            "windows_all_rows": [round(x, 3) for x in rates["all_rows"]],
            "mlm_head_ms_labelled": round(ha, 3), "mlm_head_ms_all_rows": round(hb, 3),
            "mlm_head_ratio": round(hb / ha, 2), "loss_labelled": round(losses["labelled"], 4),
            "loss_all_rows": round(losses["all_rows"], 4)}
    K.MlmLossFn.apply = staticmethod(LABELLED)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
