"""Golden fixtures of the text+image pretraining stage (scripts/wikihow_pretrain.sh: MLM + one of
image_swapping / patch_based_image_swapping / patch_based_mrm_classification per batch), generated
by running the REFERENCE in this container. Test infrastructure only: the .npz / .json it writes
travel, the reference never does. Same probe-only shims and counter-based weights as
make_golden.py / make_golden_pretrain.py.

Reference path: LXRTPretraining(multimodal_img_part=False, multimodal_text_part=False,
multimodal_pretrain_objectives=[objective], pretraining=True, mlm_ignore_index=-100)
(models/CLIP/src/lxrt/modeling.py:1601-1734) .forward(batch with masked_lm_labels) (:1734-2484).

Every np.random draw of the forward (choice / rand / randint / shuffle) goes through a recording
wrapper; the .json holds the stream in call order (what LXRTPretraining.draw must consume, call by
call) and the .npz the structured draws (what the model takes as `draws`). The draw seed is searched
so that every fixture holds at least one swapped and one unswapped story (ISP, PISP) and, for PISP,
one story whose patch count is 0; the .json names those stories.

pretrain_mm_real_pisp is the stage at its stated size (REAL_MM, B = 2): inputs regenerated from the
seed, outputs only (losses, pooled output, the logsumexp of every labelled LM row and four rows in
full, per parameter the gradient norm and 2 x 1024 samples as make_golden_real.grad_samples).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pretrain_mm.py [isp|pisp|mrm|real ...]
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_pretrain import BASE2  # noqa: E402  (sizes of the tiny fixtures)

# the stage at its stated size (scripts/wikihow_pretrain.sh with ViT-B/16): T = 120 + 393 = 513
REAL_MM = {
    "B": 2, "N": 5, "per_seq": 60,
    "vit": {"embed": 512, "res": 224, "layers": 12, "width": 768, "patch": 16},
    "joint": {"vocab": 50265, "hidden": 768, "layers": 12, "heads": 12, "inter": 3072,
              "max_pos": 514},
}
REAL_ROWS = 4  # labelled LM rows stored in full (the first four)

OBJECTIVES = {"isp": "image_swapping", "pisp": "patch_based_image_swapping",
              "mrm": "patch_based_mrm_classification"}
IGNORE = -100


def mm_inputs(cfg, seed):
    """ids [B][N * per_seq] (<s> tokens </s> per step), attention mask, masked_lm_labels on ~30 % of
    the non-special tokens with at least one per step (so every sub-sample keeps one), images."""
    g = np.random.RandomState(seed)
    B, N, ps = cfg["B"], cfg["N"], cfg["per_seq"]
    ids = np.ones((B, N * ps), dtype=np.int64)
    labels = np.full((B, N * ps), IGNORE, dtype=np.int64)
    for b in range(B):
        for s in range(N):
            k = ps - 2
            ids[b, s * ps:(s + 1) * ps] = [0] + list(g.randint(3, cfg["joint"]["vocab"], size=k)) + [2]
            pick = g.rand(k) < 0.3
            pick[g.randint(0, k)] = True
            for t in np.nonzero(pick)[0]:
                labels[b, s * ps + 1 + t] = g.randint(3, cfg["joint"]["vocab"])
    R = cfg["vit"]["res"]
    images = g.standard_normal((B, N, 3, R, R)).astype(np.float32)
    return ids, (ids != 1).astype(np.int64), labels, images


def mm_token_types(cfg):
    """token_type_ids [B][N * per_seq] of the tiny fixtures: type 1 on every odd step, so that the
    sub-sampling of the types (:2008-2011) and the type table's gradient are pinned too (with
    token_type_ids None every token has type 0, whose row is the table's padding_idx: the
    reference's gradient of the whole table is then exactly zero)."""
    B, N, ps = cfg["B"], cfg["N"], cfg["per_seq"]
    return np.tile(np.repeat(np.arange(N, dtype=np.int64) % 2, ps), (B, 1))


def build_reference(cfg, objective):
    import make_golden_pretrain as MP
    import models.CLIP.src.lxrt.modeling as lx
    MP.build_reference(cfg)  # installs the CLIP shims for this size (its model is discarded)
    J = cfg["joint"]
    bcfg = lx.BertConfig(J["vocab"], hidden_size=J["hidden"], num_hidden_layers=J["layers"],
                         num_attention_heads=J["heads"], intermediate_size=J["inter"],
                         max_position_embeddings=J["max_pos"], type_vocab_size=2)
    return lx.LXRTPretraining(bcfg, visual_losses="obj", multimodal_text_part=False,
                              multimodal_img_part=False, cls_id=0, sep_id=2, pad_id=1,
                              max_story_length=cfg["N"], mlm_ignore_index=IGNORE,
                              multimodal_pretrain_objectives=[objective],
                              clip_model_name="ViT-B/16", pretraining=True)


class Recorder:
    """np.random.choice / rand / randint / shuffle backed by a seeded RandomState, every call
    appended to `stream` as [kind, value]."""

    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)
        self.stream = []

    def choice(self, a, size=None, replace=True, p=None):
        out = self.rs.choice(a, size, replace=replace, p=p)
        self.stream.append(["choice", np.asarray(out).tolist()])
        return out

    def rand(self, *shape):
        out = self.rs.rand(*shape)
        self.stream.append(["rand", np.asarray(out).tolist()])
        return out

    def randint(self, low, high=None, size=None):
        out = self.rs.randint(low, high, size)
        self.stream.append(["randint", np.asarray(out).tolist()])
        return out

    def shuffle(self, x):
        self.rs.shuffle(x)
        self.stream.append(["shuffle", np.asarray(x).tolist()])

    def __enter__(self):
        self.saved = (np.random.choice, np.random.rand, np.random.randint, np.random.shuffle)
        np.random.choice, np.random.rand = self.choice, self.rand
        np.random.randint, np.random.shuffle = self.randint, self.shuffle
        return self

    def __exit__(self, *exc):
        np.random.choice, np.random.rand, np.random.randint, np.random.shuffle = self.saved


def structure(kind, stream, B, g2):
    """The recorded stream as the structured draws the model takes."""
    it = iter(stream)

    def take(k):
        kind_, val = next(it)
        assert kind_ == k, (kind_, k)
        return val

    out = {"objective": take("choice")[0]}
    out["sub_idx"] = np.array([sorted(take("choice")) for _ in range(B)], np.int64)
    Tv = 1 + 2 * g2
    if kind == "isp":
        swap = []
        for _ in range(B):
            swap.append(take("rand") > 0.5)
            if swap[-1]:
                assert sorted(take("choice")) == [0, 1]
        out["swap"] = np.array(swap, np.uint8)
    elif kind == "pisp":
        take("randint")  # drawn before the loop and overwritten (:896)
        count, src = [], np.tile(np.arange(Tv, dtype=np.int64), (B, 1))
        sel = []
        for _ in range(B):
            count.append(take("randint"))
            cur = []
            for _j in range(2):
                cur.append(take("choice"))
                take("choice")  # selected_patches_j: drawn, never used
            sel.append(cur)
        swap = []
        for b in range(B):
            swap.append(take("rand") > 0.5)
            if swap[-1]:
                assert sorted(take("choice")) == [0, 1]
                x, y = np.array(sel[b][0], np.int64), np.array(sel[b][1], np.int64)
                src[b, y], src[b, x] = x, y
        out.update(count=np.array(count, np.int64), swap=np.array(swap, np.uint8), patch_src=src)
    else:
        masks = []
        for _ in range(B):
            masks.append(sorted(take("choice")) + sorted(take("choice")))  # (no redraw: asserted below)
        out["mask_idx"] = np.array(masks, np.int64)
        out["shuffle"] = np.array([take("shuffle") for _ in range(B)], np.int64)
    assert next(it, None) is None, "unconsumed draws"
    return out


def wanted(kind, d):
    if kind == "mrm":
        return True
    ok = 0 < int(d["swap"].sum()) < len(d["swap"])
    if kind == "pisp":
        ok = ok and bool((d["count"] == 0).any()) and bool((d["count"][d["swap"] == 1] > 0).any())
    return ok


PART_BYTES = 900 << 10  # every committed file stays below 1 MiB


def save_parts(name, out):
    """name.npz holds everything but the gradients; the "g..." arrays (g:: full gradients, or gn:: /
    gh:: / gs:: norms and samples, and grad_norm) are packed, in order, into
    name_g0.npz, name_g1.npz, ... of at most PART_BYTES (uncompressed) each. load_parts merges."""
    for f in os.listdir(HERE):
        if f.startswith(name + "_g") and f.endswith(".npz"):
            os.remove(os.path.join(HERE, f))
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"),
                        **{k: v for k, v in out.items() if not k.startswith("g")})
    part, size, k = {}, 0, 0
    for key in [x for x in out if x.startswith("g")] + [None]:
        if part and (key is None or size + out[key].nbytes > PART_BYTES):
            np.savez_compressed(os.path.join(HERE, f"{name}_g{k}.npz"), **part)
            part, size, k = {}, 0, k + 1
        if key is not None:
            part[key] = out[key]
            size += out[key].nbytes


def load_parts(name):
    d = dict(np.load(os.path.join(HERE, f"{name}.npz")))
    k = 0
    while os.path.exists(os.path.join(HERE, f"{name}_g{k}.npz")):
        d.update(np.load(os.path.join(HERE, f"{name}_g{k}.npz")))
        k += 1
    return d


def run(kind, cfg, seed, real=False):
    from counter_init import counter_state_dict
    objective = OBJECTIVES[kind]
    torch.manual_seed(seed)
    m = build_reference(cfg, objective)
    sd = m.state_dict()
    cw = counter_state_dict({k: tuple(v.shape) for k, v in sd.items()})
    cw["cls.predictions.decoder.weight"] = cw["bert.embeddings.word_embeddings.weight"]
    m.load_state_dict({k: torch.from_numpy(v) for k, v in cw.items()})
    m.eval()
    ids, mask, labels, images = mm_inputs(cfg, seed + 1)
    types = None if real else mm_token_types(cfg)
    B = cfg["B"]
    g2 = (cfg["vit"]["res"] // cfg["vit"]["patch"]) ** 2
    ce_calls, inter = [], {}
    ce_forward = torch.nn.CrossEntropyLoss.forward

    def rec_ce(self, inp, tgt):
        ce_calls.append((inp.detach().clone(), tgt.detach().clone()))
        return ce_forward(self, inp, tgt)

    pre = m.bert.register_forward_pre_hook(lambda mod, a: inter.__setitem__("bert_in", a))
    post = m.bert.register_forward_hook(lambda mod, i, o: inter.__setitem__("bert", o))
    torch.nn.CrossEntropyLoss.forward = rec_ce
    try:
        for draw_seed in range(seed + 2, seed + 200):
            ce_calls.clear()
            m.zero_grad()
            batch = {"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(mask),
                     "token_type_ids": None if types is None else torch.from_numpy(types),
                     "masked_lm_labels": torch.from_numpy(labels),
                     "images": torch.from_numpy(images).double()}
            with Recorder(draw_seed) as rec:
                total, losses, answer = m(batch)
            d = structure(kind, rec.stream, B, g2)
            if real or wanted(kind, d):  # (the forced stories are the tiny fixtures' business)
                break
        else:
            raise RuntimeError("no draw seed gives the wanted stories")
    finally:
        torch.nn.CrossEntropyLoss.forward = ce_forward
        pre.remove()
        post.remove()
    total.backward()
    out = {k: (v if k != "objective" else np.array(v)) for k, v in d.items()}
    out.update(loss=np.array(total.item(), np.float64), losses=losses.detach().numpy(),
               answer_score=answer.numpy())
    if not real:  # the real-shape inputs are regenerated from the seed (mm_inputs)
        out.update(input_ids=ids, attention_mask=mask, token_type_ids=types,
                   masked_lm_labels=labels, images=images)
    sub_ids, sub_types, sub_mask = inter["bert_in"][:3]
    if sub_types is not None:
        out["sub::token_type_ids"] = sub_types.numpy()
    mlm_in, mlm_tgt = ce_calls[-1]  # the masked-LM term is the last CrossEntropy of the forward
    assert mlm_in.shape[-1] == cfg["joint"]["vocab"]
    out["sub::input_ids"] = sub_ids.numpy()
    out["sub::attention_mask"] = sub_mask.numpy()
    out["sub::masked_lm_labels"] = mlm_tgt.view(B, -1).numpy()
    res = inter["bert"]
    out["i::pooled"] = res[-1].detach().numpy()
    out["i::mlm_loss"] = losses.detach().numpy()[0, 1]
    if real:  # the LM head on the labelled rows: every logsumexp, the first REAL_ROWS rows in full
        rows = torch.nonzero(mlm_tgt != IGNORE).view(-1)
        out["i::mlm_rows"] = rows.numpy()
        out["i::mlm_lse"] = torch.logsumexp(mlm_in[rows].double(), -1).numpy()
        out["i::mlm_logit_rows"] = mlm_in[rows[:REAL_ROWS]].numpy()
    obj_calls = ce_calls[:-1]
    if kind == "mrm":
        assert len(obj_calls) == B
        out["i::objective_logits"] = np.stack([c[0].numpy() for c in obj_calls])
        out["i::objective_labels"] = np.stack([c[1].numpy() for c in obj_calls])
        out["i::mrm_targets"] = res[0][0].detach().numpy()
    else:
        assert len(obj_calls) == 1
        out["i::objective_logits"] = obj_calls[0][0].numpy()
        out["i::objective_labels"] = obj_calls[0][1].numpy()
    gsq, with_grad = 0.0, []
    from make_golden_real import grad_samples
    for k, p in m.named_parameters():
        if p.grad is not None:
            g = p.grad.detach().double()
            gsq += float((g ** 2).sum())
            if real:
                out["gn::" + k] = np.array(float(g.norm()), np.float64)
                out["gh::" + k], out["gs::" + k] = grad_samples(g.float().numpy())
            else:
                out["g::" + k] = g.float().numpy()
            if float(g.abs().max()) > 0:
                with_grad.append(k)
    out["grad_norm"] = np.array(gsq ** 0.5, np.float64)
    name = f"pretrain_mm_real_{kind}" if real else f"pretrain_mm_tiny_{kind}"
    save_parts(name, out)
    meta = {"config": cfg, "seed": seed, "draw_seed": draw_seed, "objective": objective,
            "mlm_ignore_index": IGNORE, "loss": float(total.item()),
            "shapes": {k: list(v.shape) for k, v in m.state_dict().items()},
            "parameter_order": [k for k, _ in m.named_parameters()],
            "nonzero_grad": with_grad, "stream": rec.stream,
            "generator": "tests/golden/make_golden_pretrain_mm.py (reference run in-process, eval "
                         "mode, np.random draws recorded)"}
    if kind != "mrm":
        meta["swapped_stories"] = np.nonzero(d["swap"])[0].tolist()
        meta["unswapped_stories"] = np.nonzero(d["swap"] == 0)[0].tolist()
    if kind == "pisp":
        meta["zero_count_stories"] = np.nonzero(d["count"] == 0)[0].tolist()
    with open(os.path.join(HERE, f"{name}.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(name, "draw seed", draw_seed, "loss", total.item(), "losses", losses.tolist(),
          "grad_norm", gsq ** 0.5, "params with grad", len(with_grad), "of",
          len(meta["parameter_order"]))


def main():
    import make_golden as MG
    MG._install_shims()
    torch.set_num_threads(8)
    for kind in sys.argv[1:] or list(OBJECTIVES):
        if kind == "real":
            run("pisp", REAL_MM, 560, real=True)
        else:
            run(kind, BASE2, 520 + 10 * list(OBJECTIVES).index(kind))


if __name__ == "__main__":
    main()
