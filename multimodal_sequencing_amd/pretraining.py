"""Pretraining: LXRTPretraining for the image-only MRM stage (BASELINE config 2,
multimodal_img_part with the patch_based_mrm_classification objective, described first) and for
the text+image stage that follows it (multimodal_img_part = multimodal_text_part = False, the
section "Text+image stage" below).

Drop-in for models/CLIP/src/lxrt/modeling.py LXRTPretraining (:1601-1734 construction,
:1734-2484 forward) on the path trainers/run_pretraining.py runs for
scripts/wikihow_image_only_pretrain.sh: same constructor kwargs, `model(batch)` ->
(total_loss, losses [1, n], answer_score), same state-dict names (the LM decoder is tied to the
word embeddings as in the reference).

Per story:
  * 2 of the N images are sub-sampled (:1979-1985) and encoded as ONE CLIP-ViT sequence of
    1 + 2 g^2 tokens (img_len = 2, the pos-embed quirk) — on device, by index, no copies;
  * 5 patch features per image are zeroed and their visn_fc features kept as targets
    (:948-1009); visn_fc on the masked sequence; pooler = dense(token 0), no tanh (:1125-1137);
  * BertPreTrainingHeads over every visual token (:1217-1227, :2247): the LM head to the vocab is
    one bf16 MFMA GEMM against the word table (computed as the reference does, not in the loss);
    the answer head on the pooled output (:2249-2250);
  * MRM classification (:2309-2351): each masked output is paired with every shuffled target,
    scored by a BertLMPredictionHead of width 2H with a 1-row decoder, cross-entropy against the
    inverse permutation, summed over stories, x 0.2.

The reference draws every random choice from np.random at run time; here they are explicit
(`draws`: sub_idx [B, 2], mask_idx [B, 10], shuffle [B, 10]) or drawn from `self.rng` in the
reference's order and distributions (SURVEY §8c determinism).

Gradient structure (exact, also true of the reference): the masked positions' ViT features are
zeroed BEFORE visn_fc and only those positions (and the detached targets) enter the loss, so the
loss's gradient with respect to the ViT is identically zero (the reference's autograd still runs
the ViT backward on zeros; the fixture's ViT gradients are all 0). The ViT output therefore enters
visn_fc detached, and the ViT parameters receive their exact (zero) gradient without the pass.

Text+image stage (scripts/wikihow_pretrain.sh). Per batch ONE objective is
drawn (:1817) from the subset of image_swapping (ISP), patch_based_image_swapping (PISP) and
patch_based_mrm_classification (MRM) the model was built with, and the masked-LM term is added:
  * the batch is masked afresh every step by `mask_tokens_sentence` (trainers/train_utils.py:
    19-66 as the counter-based kernel mmseq_mlm_mask: ids in place, labels out, on the device);
  * 2 of the N steps are sub-sampled, images by index and their tokens / mask / types / labels
    (:1979-2032) where the batch lives: device tensors by `subsample_text_device`
    (mmseq_subsample_text) followed by the labelled-row compaction (mmseq_rows_compact), with ONE
    read-back of two integers per step (bad stories, labelled rows); host tensors by
    `subsample_text` on the host, as before;
  * ISP (:2034-2053): rand() > 0.5 "swaps" the two images, label 0 (the reference keeps a view of
    one image while overwriting it, so a swapped story holds the first image twice), else label
    1; loss CrossEntropy(image_swapping_mlp(pooled));
  * PISP (:885-942): a row permutation of the ViT output (kernels.RowsGatherFn) before visn_fc;
  * MRM (:948-1009, :2309-2351): as above, except that the masked rows are zeroed by the row
    kernel's keep mask (every other row keeps its gradient into the ViT) and the masked outputs
    are the joint encoder's visual rows;
  * encoder: LXRTModel.encode_joint(visual_row_op=...); ISP / PISP use only the text rows and
    the pooled output, so the last layer runs on the text rows;
  * MLM (:2423-2428): kernels.MlmLossFn on the labelled rows only; the tied decoder's weight
    gradient accumulates into the word-embedding gradient.
`draw_mm` makes every np.random call of the reference in its order (the fixtures record the
stream); total = objective + MLM, losses = [[objective, mlm]].
"""
import copy
import os
from types import SimpleNamespace

import numpy as np
import torch
from torch import nn

from . import _native as N
from . import kernels as K
from .checkpoint import lxrt_from_pretrained, save_pretrained
from .lxrt import LXRTConfig, LXRTModel, _mark_stale
from .params import ParamStore, Spec, attach_tree, linear_specs, ln_specs, normal, zeros

OBJ_ID_NUM = 1600  # param.py:68 (VISUAL_CONFIG.obj_id_num, BertVisualObjHead 'obj' decoder)


def _pretrain_head_specs(H, vocab, std=0.02, num_answers=2):
    p = "cls.predictions."
    sp = [Spec(p + "bias", (vocab,), zeros)]
    sp += linear_specs(p + "transform.dense", H, H, std=std) + ln_specs(p + "transform.LayerNorm", H)
    sp += linear_specs("cls.seq_relationship", H, 2, std=std)
    o = "obj_predict_head."
    sp += linear_specs(o + "transform.dense", H, H, std=std) + ln_specs(o + "transform.LayerNorm", H)
    sp += linear_specs(o + "decoder_dict.obj", H, OBJ_ID_NUM, std=std, transpose=False)
    a = "answer_head.logit_fc."
    sp += linear_specs(a + "0", H, 2 * H, std=std) + ln_specs(a + "2", 2 * H)
    sp += linear_specs(a + "3", 2 * H, num_answers, std=std)
    m = "patch_based_mrm_classification_head."
    sp += [Spec(m + "bias", (1,), zeros)]
    sp += linear_specs(m + "transform.dense", 2 * H, 2 * H, std=std)
    sp += ln_specs(m + "transform.LayerNorm", 2 * H)
    sp += [Spec(m + "decoder.weight", (1, 2 * H), normal(std), transpose=True)]
    return sp


ISP, PISP, MRM = "image_swapping", "patch_based_image_swapping", "patch_based_mrm_classification"
MM_OBJECTIVES = (ISP, PISP, MRM)  # the reference's constructor order (:1647-1657, :1704-1714)


def _mm_head_specs(H, vocab, objectives, std=0.02, num_answers=2):
    """Heads of the text+image stage: the objectives' own (in the reference's constructor order),
    then BertPreTrainingHeads, the object head and the answer head as in config 2."""
    sp = []
    if ISP in objectives:
        sp += linear_specs("image_swapping_mlp", H, 2, std=std)
    if PISP in objectives:
        sp += linear_specs("patch_based_image_swapping_mlp", H, 2, std=std)
    base = _pretrain_head_specs(H, vocab, std, num_answers)
    m = "patch_based_mrm_classification_head."
    if MRM in objectives:
        sp += [x for x in base if x.name.startswith(m)]
    return sp + [x for x in base if not x.name.startswith(m)]


def subsample_text(input_ids, attention_mask, token_type_ids, masked_lm_labels, sub_idx, n_steps,
                   cls_id, pad_id, ignore_index):
    """The text of the sub-sampled steps (:1986-2032), on the host: step k of a story runs from its
    k-th cls token to the next one (the last step: L // n_steps tokens); the kept steps are
    concatenated and padded to L // n_steps * 2 with pad_id / 0 / 0 / ignore_index.
    All tensors int64 [B][L] (token_type_ids may be None); sub_idx [B][2] ascending. Returns
    (input_ids, attention_mask, token_type_ids or None, masked_lm_labels), each [B][pad]."""
    ids = torch.as_tensor(input_ids).cpu()
    B, L = ids.shape
    per, n_sub = L // n_steps, len(sub_idx[0])
    pad = per * n_sub
    gather = torch.full((B, pad), -1, dtype=torch.int64)
    for b in range(B):
        cls_pos = torch.nonzero(ids[b] == cls_id).view(-1).tolist()
        at = 0
        for k in (int(x) for x in sub_idx[b]):
            if k >= len(cls_pos):
                raise ValueError(f"story {b}: step {k} of {len(cls_pos)} cls tokens")
            start = cls_pos[k]
            end = start + per if k == n_steps - 1 else cls_pos[k + 1]
            if at + end - start > pad or end > L:
                raise ValueError(f"story {b}: the sub-sampled steps exceed {pad} tokens")
            gather[b, at:at + end - start] = torch.arange(start, end)
            at += end - start
    valid, idx = gather >= 0, gather.clamp(min=0)

    def take(t, fill):
        if t is None:
            return None
        t = torch.as_tensor(t).cpu()
        return torch.where(valid, t.gather(1, idx), torch.full_like(idx, fill).to(t.dtype))

    return (take(ids, pad_id), take(attention_mask, 0), take(token_type_ids, 0),
            take(masked_lm_labels, ignore_index))


def subsample_text_device(input_ids, attention_mask, token_type_ids, masked_lm_labels, sub_idx,
                          n_steps, cls_id, pad_id, ignore_index, device="cuda", status=None):
    """`subsample_text` on the device (mmseq_subsample_text): the same arguments and returns, the
    tensors on the device (that of input_ids when it is a device tensor, else host tensors are
    copied to `device` first). Raises ValueError naming the number of stories for which the host
    function raises. With `status` (int32 [>= 1] on the device, zeroed by the caller) the bad-story
    count is added to status[0] and NOT read back here: the caller reads it with whatever else the
    step needs, and raises."""
    ids = torch.as_tensor(input_ids)
    dev = ids.device if ids.is_cuda else torch.device(device)

    def on(t):
        if t is None:
            return None
        return torch.as_tensor(t).to(dev, torch.int64, non_blocking=True).contiguous()

    ids, mask, tt, lab = on(ids), on(attention_mask), on(token_type_ids), on(masked_lm_labels)
    sub = on(np.asarray(sub_idx, np.int64) if not torch.is_tensor(sub_idx) else sub_idx)
    B, L = ids.shape
    pad = L // n_steps * sub.shape[1]
    out = [None if t is None else torch.empty(B, pad, dtype=torch.int64, device=dev)
           for t in (ids, mask, tt, lab)]
    own = status is None
    if own:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    N.subsample_text(ids, mask, tt, lab, sub, n_steps, int(cls_id), int(pad_id), int(ignore_index),
                     out[0], out[1], out[2], out[3], status)
    if own:
        _raise_bad_stories(int(status.item()))
    return tuple(out)


def _raise_bad_stories(bad):
    if bad:
        raise ValueError(f"{bad} stor{'y' if bad == 1 else 'ies'} whose sub-sampled steps lack a "
                         "cls token or exceed the padded length (lxrt/modeling.py:1986-2032)")


_MASK_CALLS = [0]  # process-wide: mask_tokens_sentence(seed=None) never repeats a key


def mask_tokens_sentence(inputs, tokenizer, args, seed=None, device="cuda", stream_id=None):
    """Drop-in for trainers/train_utils.py:19-66 on the device (kernels.mlm_mask): 80 % [MASK],
    10 % random word, 10 % unchanged over the tokens selected with args.mlm_probability; reads
    tokenizer.pad_token / mask_token (convert_tokens_to_ids), len(tokenizer), args.cls_id and
    args.mlm_ignore_index. `inputs`: int64 [B][L]; a device tensor is masked IN PLACE, a host one
    is copied to `device` first. Returns (inputs, labels), both on the device. seed=None draws a
    fresh key from a process-wide counter (successive calls differ); an explicit seed reproduces
    the bits. `stream_id` (with an explicit seed) selects another counter stream of that seed: the
    evaluation loop masks step s on stream 2 + s; None is stream 0."""
    pad_id = tokenizer.convert_tokens_to_ids(tokenizer.pad_token)
    mask_id = tokenizer.convert_tokens_to_ids(tokenizer.mask_token)
    t = torch.as_tensor(inputs)
    if not t.is_cuda:
        t = t.to(device, torch.int64).contiguous()
    if t.dtype != torch.int64 or t.dim() != 2 or not t.is_contiguous():
        raise ValueError("mask_tokens_sentence: inputs must be contiguous int64 [B][L]")
    if seed is None:
        if stream_id is not None:
            raise ValueError("mask_tokens_sentence: stream_id needs an explicit seed")
        _MASK_CALLS[0] += 1
        seed, stream_id = _MASK_CALLS[0], 1  # stream 1: apart from every explicit seed's stream 0
    elif stream_id is None:
        stream_id = 0
    labels = K.mlm_mask(t, pad_id, args.cls_id, mask_id, len(tokenizer), args.mlm_ignore_index,
                        args.mlm_probability, seed, stream_id)
    return t, labels


class LXRTPretraining(nn.Module):
    MASK_NUM = 5  # pb_mrm_cls_mask_num (:1694)
    MRM_SCALE = 0.2  # :2347
    from_pretrained = classmethod(lxrt_from_pretrained)  # roberta/lm_head remaps (checkpoint.py)
    save_pretrained = save_pretrained

    def __init__(self, config, task_mask_lm=True, task_matched=True, task_obj_predict=True,
                 visual_losses="", task_qa=True, num_answers=2, device="cuda",
                 compute_dtype=torch.bfloat16, seed=0, vision=None, **kwargs):
        super().__init__()
        if not kwargs.get("multimodal_img_part", False):
            self._init_mm(config, num_answers, device, compute_dtype, seed, vision, task_qa, kwargs)
            return
        objectives = list(kwargs.get("multimodal_pretrain_objectives") or [])
        if objectives != ["patch_based_mrm_classification"]:
            raise NotImplementedError(
                f"pretraining objectives {objectives}: only patch_based_mrm_classification "
                "(scripts/wikihow_image_only_pretrain.sh) is built")
        self.config = config
        self.multimodal_img_part = True
        self.multimodal_pretrain_objectives = objectives
        self.cls_id, self.sep_id = kwargs.get("cls_id", 0), kwargs.get("sep_id", 2)
        self.pad_id = kwargs.get("pad_id", 1)
        self.task_qa = task_qa
        inner_kw = {k: v for k, v in kwargs.items()
                    if k in ("cls_id", "sep_id", "max_story_length", "clip_model_name")}
        self.bert = LXRTModel(config, multimodal_img_part=True, device=device,
                              compute_dtype=compute_dtype, vision=vision, seed=seed, **inner_kw)
        H = config.hidden_size
        self.store = ParamStore(_pretrain_head_specs(H, config.vocab_size,
                                                     config.initializer_range, num_answers),
                                device, compute_dtype)
        self.store.init_weights(seed=seed + 7)
        # the reference builds the MRM head before BertPreTrainingHeads (lxrt/modeling.py:1713,
        # 1724-1728): registration order = named_parameters() order
        mrm = "patch_based_mrm_classification_head."
        attach_tree(self, self.store.params, order=lambda names: (
            [n for n in names if n.startswith(mrm)] + [n for n in names if not n.startswith(mrm)]))
        # tied LM decoder (:1164-1167): the word table registered under both names
        attach_tree(self, {"cls.predictions.decoder.weight":
                           self.bert.store.params["embeddings.word_embeddings.weight"]})
        self._anchor = torch.zeros((), device=device, requires_grad=True)
        self.register_load_state_dict_post_hook(_mark_stale)
        self.rng = np.random.RandomState(seed)
        self.device_ = torch.device(device)
        self.last_prediction_scores = None
        self.last_seq_relationship = None

    def _init_mm(self, config, num_answers, device, compute_dtype, seed, vision, task_qa, kwargs):
        """The text+image stage (scripts/wikihow_pretrain.sh): MLM + one of ISP / PISP / MRM per
        batch over the joint encoder; multimodal_img_part = multimodal_text_part = False."""
        objectives = list(kwargs.get("multimodal_pretrain_objectives") or [])
        bad = [o for o in objectives if o not in MM_OBJECTIVES]
        if bad or not objectives:
            raise NotImplementedError(
                f"pretraining objectives {bad or objectives}: the text+image stage builds "
                f"{', '.join(MM_OBJECTIVES)}")
        if kwargs.get("multimodal_text_part", False):
            raise NotImplementedError("text-only pretraining (multimodal_text_part) is not built")
        vis = vision if isinstance(vision, dict) else None
        if (vis or {}).get("type") == "rn50" or str(kwargs.get("clip_model_name", "")).startswith("RN"):
            raise NotImplementedError("RN50 as the pretraining backbone is not built (ViT only)")
        self.config = config
        self.multimodal_img_part = False
        self.multimodal_pretrain_objectives = objectives
        self.cls_id, self.sep_id = kwargs.get("cls_id", 0), kwargs.get("sep_id", 2)
        self.pad_id = kwargs.get("pad_id", 1)
        self.mlm_ignore_index = kwargs.get("mlm_ignore_index", -1)
        self.max_story_length = kwargs.get("max_story_length", 5)
        self.task_qa = task_qa
        inner_kw = {k: v for k, v in kwargs.items()
                    if k in ("cls_id", "sep_id", "max_story_length", "clip_model_name",
                             "multimodal_pretrain_objectives")}
        self.bert = LXRTModel(config, device=device, compute_dtype=compute_dtype, vision=vision,
                              seed=seed, **inner_kw)
        self.store = ParamStore(_mm_head_specs(config.hidden_size, config.vocab_size, objectives,
                                               config.initializer_range, num_answers),
                                device, compute_dtype)
        self.store.init_weights(seed=seed + 7)
        attach_tree(self, self.store.params)  # spec order = the reference's registration order
        attach_tree(self, {"cls.predictions.decoder.weight":
                           self.bert.store.params["embeddings.word_embeddings.weight"]})
        self._anchor = torch.zeros((), device=device, requires_grad=True)
        self.register_load_state_dict_post_hook(_mark_stale)
        self.rng = np.random.RandomState(seed)
        self.device_ = torch.device(device)
        self.last_objective = None
        self.last_objective_logits = self.last_objective_labels = None
        self.last_pooled = self.last_mrm_targets = None

    def stores(self):
        return [self.bert.store, self.store]

    def zero_grad(self, set_to_none=False):
        for s in self.stores():
            s.zero_grad()

    def ddp_units(self):
        """(units, begin_stores) for trainer.GradAllReduce: the heads and visn_fc finish together;
        no per-layer units (the ViT gradient is exactly zero, see the module docstring). The
        text+image stage: the inner model's per-layer spans, the head store completing as a whole
        before the inner model's backward begins (as BertForOrdering.ddp_units)."""
        if not self.multimodal_img_part:
            return {id(self.bert.store): self.bert.grad_units()}, [self.store]
        return {}, []

    # ------------------------------------------------------------------------------------
    def draw(self, B, N, Tv, rng=None):
        """The reference's np.random draws (:1981, :983-987, :2322-2323) for a batch of B
        stories of N images with Tv visual tokens (1 + 2 g^2), from `rng` (default self.rng)."""
        rng = rng or self.rng
        per = Tv // 2  # visn_per_seq_len (:955)
        sub_idx, mask_idx, shuffle = [], [], []
        for _ in range(B):
            sub_idx.append(sorted(rng.choice(N, 2, replace=False)))
        for _ in range(B):
            m = []
            for start in range(1, Tv, per):
                m += sorted(rng.choice(list(range(start, start + per)), self.MASK_NUM,
                                            replace=False))
            mask_idx.append(m)
        for _ in range(B):
            idx = np.arange(self.MASK_NUM * 2)
            rng.shuffle(idx)
            shuffle.append(idx)
        return {"sub_idx": np.asarray(sub_idx, np.int64), "mask_idx": np.asarray(mask_idx, np.int64),
                "shuffle": np.asarray(shuffle, np.int64)}

    def draw_mm(self, B, N, Tv, rng=None):
        """The reference's np.random draws of one text+image batch, in its call order and
        distributions: the objective (:1817), 2 of N images per story (:1981), then the
        objective's own. ISP (:2038-2050): rand() > 0.5 swaps. PISP (:889-939): the two patch ranges
        are [0, 1 + g^2) (the class token included) and [1 + g^2, 1 + 2 g^2); a count in
        [0, g^2) per story, preceded by one that is overwritten; per range one selection that is
        used and one that is not; then rand() > 0.5 swaps the selections row for row
        (`patch_src`: the row of the ViT output each row is taken from). MRM (:983-990, :2322):
        as config 2, with the redraw while more than 60 % of a selection repeats the one before."""
        rng = rng or self.rng
        d = {"objective": str(rng.choice(self.multimodal_pretrain_objectives, 1, replace=False)[0])}
        d["sub_idx"] = np.asarray([sorted(rng.choice(N, 2, replace=False)) for _ in range(B)],
                                  np.int64)
        obj = d["objective"]

        def swapped():
            if rng.rand() > 0.5:
                rng.choice(2, 2, replace=False)  # always the pair (0, 1) once sorted
                return 1
            return 0

        if obj == ISP:
            d["swap"] = np.asarray([swapped() for _ in range(B)], np.uint8)
        elif obj == PISP:
            patch_len = Tv // 2
            ranges = [list(range(0, 1 + patch_len)), list(range(1 + patch_len, Tv))]
            rng.randint(0, patch_len)
            count, sel = [], []
            for _ in range(B):
                count.append(int(rng.randint(0, patch_len)))
                cur = []
                for r in ranges:
                    cur.append(np.asarray(rng.choice(r, count[-1], replace=False), np.int64))
                    rng.choice(r, count[-1], replace=False)
                sel.append(cur)
            d["count"] = np.asarray(count, np.int64)
            d["swap"] = np.asarray([swapped() for _ in range(B)], np.uint8)
            src = np.tile(np.arange(Tv, dtype=np.int64), (B, 1))
            for b in range(B):
                if d["swap"][b]:
                    x, y = sel[b]
                    src[b, y], src[b, x] = x, y
            d["patch_src"] = src
        else:
            per = Tv // 2
            masks = []
            for _ in range(B):
                m, prev = [], None
                for start in range(1, Tv, per):
                    choices = list(range(start, start + per))
                    cur = rng.choice(choices, self.MASK_NUM, replace=False)
                    while prev is not None and \
                            sum(int(x) in set(int(p) for p in prev) for x in cur) / len(cur) > 0.6:
                        cur = rng.choice(choices, self.MASK_NUM, replace=False)
                    prev = cur
                    m += sorted(int(x) for x in cur)
                masks.append(m)
            d["mask_idx"] = np.asarray(masks, np.int64)
            sh = []
            for _ in range(B):
                idx = np.arange(self.MASK_NUM * 2)
                rng.shuffle(idx)
                sh.append(np.asarray(idx, np.int64))
            d["shuffle"] = np.asarray(sh, np.int64)
        return d

    def _lin(self, x, store, name, act=0, bias=True):
        return K.LinearFn.apply(x, self._anchor, store, name + ".weight",
                                name + ".bias" if bias else None, act)

    def _ln(self, x, store, name, eps=1e-12):
        return K.LayerNormFn.apply(x, self._anchor, store, name, eps)

    def forward(self, input_ids, token_type_ids=None, attention_mask=None, masked_lm_labels=None,
                visual_feats=None, pos=None, obj_labels=None, matched_label=None, ans=None,
                draws=None):
        """:1734-2484 for the image-only MRM objective. `input_ids` may be the batch dict
        (input_ids, attention_mask, images [B, N, 3, R, R]); `draws` the explicit random
        choices (else drawn from self.rng)."""
        return self._forward_any(input_ids, token_type_ids, attention_mask, masked_lm_labels,
                                 visual_feats, draws, None)

    def evaluate_batch(self, batch, topk=5, totals=None):
        """One evaluation batch of either stage: (loss, losses, answer, stats) under no_grad, the
        first three with the bits `model(batch)` gives on the same batch and draws under no_grad
        in eval mode (the same kernels run; only the masked-LM loss's pass is the evaluating
        instantiation, mmseq_xent_eval). Raises in train mode (dropout would make the statistics
        those of another network). `batch`: the dict `forward` takes. stats, text+image stage:
          mlm                kernels.mlm_eval's dict over the labelled rows (rows, labels, lse,
                             loss_row, rank, topk_idx / topk_logit [rows][topk], mean_loss)
          seq_len            Lt: mlm["rows"] = story * Lt + position in the sub-sampled text
          objective, objective_logits, objective_labels, objective_loss
          objective_correct, objective_count   device int64 scalars (arg-max of the head's scores:
                             [B] decisions for ISP / PISP, [B][10] for MRM)
        `totals` (f64 [4] on the device) accumulates (sum of NLL, labelled tokens, rank 0,
        rank < topk) over the calls. The image-only stage has no masked-LM term: its stats hold the
        MRM head's objective_* entries only."""
        if self.training:
            raise RuntimeError("evaluate_batch needs the model in eval mode: call model.eval()")
        if not isinstance(batch, dict):
            raise TypeError("evaluate_batch takes the batch dict that forward takes")
        ev = {"topk": int(topk), "totals": totals, "stats": {}}
        with torch.no_grad():
            loss, losses, answer = self._forward_any(batch, None, None, None, None, None, ev)
        return loss, losses, answer, ev["stats"]

    def _forward_any(self, input_ids, token_type_ids, attention_mask, masked_lm_labels,
                     visual_feats, draws, ev):
        """forward's body; `ev` (evaluate_batch's request) also collects the statistics."""
        if isinstance(input_ids, dict):
            batch = input_ids
            visual_feats = batch.get("images")
            draws = batch.get("draws", draws)
            if not self.multimodal_img_part:
                input_ids, token_type_ids = batch.get("input_ids"), batch.get("token_type_ids")
                attention_mask = batch.get("attention_mask")
                masked_lm_labels = batch.get("masked_lm_labels")
        if not self.multimodal_img_part:
            return self._forward_mm(input_ids, token_type_ids, attention_mask, masked_lm_labels,
                                    visual_feats, draws, ev)
        images = visual_feats.to(self.device_, torch.float32).contiguous()
        B, Nimg = images.shape[:2]
        inner = self.bert
        st_in, st = inner.store, self.store
        for s in self.stores():
            if s.shadow_stale:
                s.refresh_shadows()
        V = inner.vision
        g = images.shape[-1] // V["patch"]
        Tv = 1 + 2 * g * g
        if draws is None:
            draws = self.draw(B, Nimg, Tv)
        dev = self.device_
        sub_idx = torch.as_tensor(np.asarray(draws["sub_idx"]), dtype=torch.int64)
        mask_idx = torch.as_tensor(np.asarray(draws["mask_idx"]), dtype=torch.int64)
        shuffle = np.asarray(draws["shuffle"], dtype=np.int64)
        nm = mask_idx.shape[1]
        sub_idx = sub_idx.to(dev).view(B, 1, 2).contiguous()
        mask_idx = mask_idx.to(dev)
        D = inner.new_dropouts()
        ph = self.config.hidden_dropout_prob
        # CLIP ViT over the two sub-sampled images of each story (img_len = 2)
        with torch.no_grad():  # only vout.detach() is used: the blocks skip their saves
            vout, Tv = inner.visual_forward(images, sub_idx)  # [B * Tv, E]
        E = vout.shape[-1]
        # MRM masking (:948-1009): targets = visn_fc(features at the masked patches), the
        # sequence fed on has them zeroed; the ViT's gradient is exactly zero (docstring)
        vseq = vout.detach().view(B, Tv, E)
        bidx = torch.arange(B, device=dev)[:, None]
        gt = vseq[bidx, mask_idx]  # [B, nm, E]
        keep = torch.ones(B, Tv, 1, device=dev, dtype=vseq.dtype)
        keep[bidx, mask_idx] = 0
        vmasked = vseq * keep
        vf = "encoder.visn_fc."
        visn = K.dropout(self._ln(self._lin(vmasked, st_in, vf + "visn_fc"), st_in,
                                  vf + "visn_layer_norm"), D.site(ph, "pt_visn_fc"))
        targets = K.dropout(self._ln(self._lin(gt.contiguous(), st_in, vf + "visn_fc"), st_in,
                                     vf + "visn_layer_norm"), D.site(ph, "pt_visn_fc_gt"))
        H = visn.shape[-1]
        # pooler (:1575-1578 with img_part): dense(token 0), no tanh
        pooled = self._lin(visn[:, 0].contiguous(), st_in, "pooler.dense")
        # BertPreTrainingHeads (:2247): LM head over every visual token + seq_relationship
        self.last_prediction_scores = self._lm_head(visn.reshape(B * Tv, H)).view(B, Tv, -1)
        self.last_seq_relationship = self._lin(pooled, st, "cls.seq_relationship")
        # answer head (:2249-2250): Linear(H, 2H) + GeLU + LN + Linear(2H, 2)
        a = "answer_head.logit_fc."
        answer = self._lin(self._ln(self._lin(pooled, st, a + "0", act=K.GELU), st, a + "2"),
                           st, a + "3")
        # MRM classification (:2309-2351)
        masked = visn[bidx, mask_idx]  # [B, nm, H], positions ascending = target order
        shuf = torch.as_tensor(shuffle, device=dev)
        tshuf = targets[bidx, shuf]  # mask_patch_gt[i][indices]
        qa = torch.cat([masked[:, :, None, :].expand(B, nm, nm, H),
                        tshuf[:, None, :, :].expand(B, nm, nm, H)], -1)  # [B, j, k, 2H]
        m = "patch_based_mrm_classification_head."
        hdn = self._ln(self._lin(qa.contiguous(), st, m + "transform.dense", act=K.GELU), st,
                       m + "transform.LayerNorm")
        scores = K.LinearFn.apply(hdn, self._anchor, st, m + "decoder.weight", m + "bias", 0)
        scores = scores.view(B, nm, nm).float()
        labels = torch.as_tensor(np.argsort(shuffle, axis=1), device=dev)  # indices_argsort
        logp = torch.log_softmax(scores, -1)
        ce = -logp.gather(-1, labels[:, :, None]).squeeze(-1).mean(-1)  # CrossEntropyLoss per story
        mrm = ce.sum() * self.MRM_SCALE
        losses = mrm.detach().view(1, 1)
        if ev is not None:
            ev["stats"].update(_objective_stats(MRM, scores, labels, mrm))
        return mrm, losses, answer.detach()

    def _forward_mm(self, input_ids, token_type_ids, attention_mask, masked_lm_labels, images,
                    draws, ev=None):
        """:1734-2484 for the text+image stage: one objective per batch + the masked-LM term.
        Returns (total_loss, [[objective_loss, mlm_loss]], answer_score). A device `input_ids`
        takes the device input path (attention_mask, token_type_ids and masked_lm_labels must then
        be on that device); host tensors go through the host sub-sampling."""
        if masked_lm_labels is None or images is None:
            raise ValueError("the text+image stage needs masked_lm_labels and images: "
                             "pretraining.mask_tokens_sentence(input_ids, tokenizer, args) masks a "
                             "batch on the device and returns the labels")
        dev = self.device_
        on_device = torch.is_tensor(input_ids) and input_ids.is_cuda
        if on_device:
            for name, t in (("attention_mask", attention_mask), ("token_type_ids", token_type_ids),
                            ("masked_lm_labels", masked_lm_labels)):
                if t is not None and not (torch.is_tensor(t) and t.device == input_ids.device):
                    raise ValueError(f"input_ids is on {input_ids.device}: {name} must be there too")
        images = images.to(dev, torch.float32).contiguous()
        B, Nimg = images.shape[:2]
        inner = self.bert
        st_in, st = inner.store, self.store
        for s in self.stores():
            if s.shadow_stale:
                s.refresh_shadows()
        g = images.shape[-1] // inner.vision["patch"]
        Tv = 1 + 2 * g * g
        if draws is None:
            draws = self.draw_mm(B, Nimg, Tv)
        obj = str(np.asarray(draws["objective"]).reshape(-1)[0])
        if obj not in self.multimodal_pretrain_objectives:
            raise ValueError(f"objective {obj} was not built into this model")
        self.last_objective = obj
        sub_idx = np.asarray(draws["sub_idx"], np.int64)
        if attention_mask is None:
            attention_mask = torch.ones_like(torch.as_tensor(input_ids))
        # sub-sampling: integer work, the images are only indexed (mmseq_vit_im2col)
        mlm_rows = None
        if on_device:
            # a device batch stays there: sub-sampling and the labelled-row compaction are two
            # kernels whose counts (bad stories, labelled rows) come back in ONE read
            status = torch.zeros(2, dtype=torch.int32, device=input_ids.device)
            ids, mask, tt, labels = subsample_text_device(
                input_ids, attention_mask, token_type_ids, masked_lm_labels, sub_idx, Nimg,
                self.cls_id, self.pad_id, self.mlm_ignore_index, status=status)
            src, lab = K.compact_rows(labels, self.mlm_ignore_index, status[1:])
            bad, n_rows = status.tolist()
            _raise_bad_stories(bad)
            mlm_rows = (src[:n_rows], lab[:n_rows])
        else:
            ids, mask, tt, labels = subsample_text(input_ids, attention_mask, token_type_ids,
                                                   masked_lm_labels, sub_idx, Nimg, self.cls_id,
                                                   self.pad_id, self.mlm_ignore_index)
        pairs = torch.as_tensor(sub_idx).clone()
        if obj == ISP:
            # :2042-2046 keeps a VIEW of image y while overwriting it, so a "swapped" story holds
            # image x twice (the fixtures record it)
            swap = torch.as_tensor(np.asarray(draws["swap"]).astype(bool))
            pairs[:, 1] = torch.where(swap, pairs[:, 0], pairs[:, 1])
            obj_labels = (~swap).long()
        elif obj == PISP:
            obj_labels = (~torch.as_tensor(np.asarray(draws["swap"]).astype(bool))).long()
        pairs = pairs.to(dev).view(B, 1, 2).contiguous()
        row_op, mask_rows = None, None
        base = torch.arange(B, dtype=torch.int64)[:, None] * Tv
        if obj == PISP:
            src = (base + torch.as_tensor(np.asarray(draws["patch_src"], np.int64))).view(-1)
            src = src.to(dev, torch.int32)
            row_op = lambda vout, _tv: K.RowsGatherFn.apply(vout, src, None)  # noqa: E731
        elif obj == MRM:
            mask_idx = torch.as_tensor(np.asarray(draws["mask_idx"], np.int64))
            nm = mask_idx.shape[1]
            mask_rows = (base + mask_idx).view(-1)
            keep = torch.ones(B * Tv, dtype=torch.uint8)
            keep[mask_rows] = 0
            keep = keep.to(dev)
            ident = torch.arange(B * Tv, dtype=torch.int32, device=dev)
            gt_rows = mask_rows.to(dev, torch.int32)
            stash = {}

            def row_op(vout, _tv):
                # targets: the (detached) features at the masked patches; the sequence fed on has
                # those rows zeroed, every other row keeps its gradient into the ViT
                stash["gt"] = K.RowsGatherFn.apply(vout.detach(), gt_rows, None)
                return K.RowsGatherFn.apply(vout, ident, keep)
        D = inner.new_dropouts()
        ph = self.config.hidden_dropout_prob
        joint, Lt = inner.encode_joint(ids.to(dev), mask.to(dev),
                                       None if tt is None else tt.to(dev), images, pairs, drops=D,
                                       text_rows=obj != MRM, visual_row_op=row_op)
        H = joint.shape[-1]
        lang = joint[:, :Lt]
        # pooler (:1125-1137): dense(lang[:, 0]), no tanh
        pooled = self._lin(lang[:, 0].contiguous(), st_in, "pooler.dense")
        self.last_pooled = pooled.detach()
        a = "answer_head.logit_fc."
        answer = self._lin(self._ln(self._lin(pooled, st, a + "0", act=K.GELU), st, a + "2"),
                           st, a + "3")
        if obj == MRM:
            vf = "encoder.visn_fc."
            targets = K.dropout(self._ln(self._lin(stash["gt"], st_in, vf + "visn_fc"), st_in,
                                         vf + "visn_layer_norm"), D.site(ph, "pt_visn_fc_gt"))
            targets = targets.view(B, nm, H)
            self.last_mrm_targets = targets.detach()
            T = joint.shape[1]
            out_rows = (torch.arange(B, dtype=torch.int64)[:, None] * T + Lt + mask_idx).view(-1)
            masked = K.RowsGatherFn.apply(joint, out_rows.to(dev, torch.int32), None).view(B, nm, H)
            shuffle = np.asarray(draws["shuffle"], dtype=np.int64)
            bidx = torch.arange(B, device=dev)[:, None]
            tshuf = targets[bidx, torch.as_tensor(shuffle, device=dev)]
            qa = torch.cat([masked[:, :, None, :].expand(B, nm, nm, H),
                            tshuf[:, None, :, :].expand(B, nm, nm, H)], -1)
            m = "patch_based_mrm_classification_head."
            hdn = self._ln(self._lin(qa.contiguous(), st, m + "transform.dense", act=K.GELU), st,
                           m + "transform.LayerNorm")
            scores = K.LinearFn.apply(hdn, self._anchor, st, m + "decoder.weight", m + "bias", 0)
            scores = scores.view(B, nm, nm).float()
            obj_labels = torch.as_tensor(np.argsort(shuffle, axis=1))
            logp = torch.log_softmax(scores, -1)
            ce = -logp.gather(-1, obj_labels.to(dev)[:, :, None]).squeeze(-1).mean(-1)
            obj_loss = ce.sum() * self.MRM_SCALE
        else:
            scores = self._lin(pooled, st, obj + "_mlp").float()
            obj_loss = torch.nn.functional.cross_entropy(scores, obj_labels.to(dev))
        self.last_objective_logits, self.last_objective_labels = scores.detach(), obj_labels
        if ev is None:
            mlm = K.MlmLossFn.apply(lang, labels, self.mlm_ignore_index, self._anchor, st, st_in,
                                    rows=mlm_rows)
        else:  # the same gather, transform and decoder GEMM; the loss's pass also ranks
            stats = ev["stats"]
            stats["mlm"] = K.mlm_eval(lang, labels, self.mlm_ignore_index, st, st_in, ev["topk"],
                                      rows=mlm_rows, totals=ev["totals"])
            stats["seq_len"] = Lt
            stats.update(_objective_stats(obj, scores, obj_labels.to(dev), obj_loss))
            mlm = stats["mlm"]["mean_loss"]
        total = obj_loss + mlm
        losses = torch.stack([obj_loss.detach(), mlm.detach()]).view(1, 2)
        return total, losses, answer.detach()

    def _lm_head(self, x):
        """BertLMPredictionHead (:1157-1173): transform (dense + erf-GELU + LN 1e-12) and the tied
        decoder + bias as one MFMA GEMM into a row-padded buffer (ld = vocab rounded up to 64)."""
        st, st_in = self.store, self.bert.store
        p = "cls.predictions."
        h = self._ln(self._lin(x, st, p + "transform.dense", act=K.GELU), st, p + "transform.LayerNorm")
        Wd = st_in.w("embeddings.word_embeddings.weight")  # [V, H] compute dtype (tied)
        V = Wd.shape[0]
        ldc = (V + 63) // 64 * 64
        out = torch.empty(h.shape[0], ldc, device=h.device, dtype=h.dtype)
        with torch.no_grad():  # not in the loss (masked_lm_labels is None for img_part)
            N.gemm(h.detach(), Wd, out, h.shape[0], V, h.shape[-1], ldc=ldc,
                   bias=st.f32(p + "bias"))
        return out[:, :V]


def _objective_stats(obj, scores, labels, loss):
    """Accuracy of an objective head from its scores ([B][2] for ISP / PISP, [B][10][10] for MRM)
    and labels ([B] / [B][10]); tiny, so the arg-max stays a torch op as the head's loss does."""
    correct = (scores.detach().argmax(-1) == labels).sum()
    return {"objective": obj, "objective_logits": scores.detach(), "objective_labels": labels,
            "objective_loss": loss.detach(), "objective_correct": correct,
            "objective_count": torch.tensor(labels.numel(), device=correct.device)}


def fill_mask(model, batch, k=5, tokenizer=None):
    """What the model puts at the masks of one text+image batch (the dict `forward` takes, masked
    by mask_tokens_sentence). Per labelled position, in row order, a dict of device tensors:
    story [n], position [n] (in the sub-sampled text), gold [n], ids [n][k] ordered by (logit
    descending, id ascending), probs [n][k] = exp(topk_logit - lse), rank [n], loss_row [n]; with
    a tokenizer also tokens / gold_tokens (convert_ids_to_tokens). A convenience over
    evaluate_batch."""
    _, _, _, stats = model.evaluate_batch(batch, topk=k)
    if "mlm" not in stats:
        raise ValueError("fill_mask needs the text+image stage (the image-only stage has no "
                         "masked-LM head in its loss)")
    m, Lt = stats["mlm"], stats["seq_len"]
    rows = m["rows"].long()
    out = {"story": rows // Lt, "position": rows % Lt, "gold": m["labels"],
           "ids": m["topk_idx"].long(), "probs": torch.exp(m["topk_logit"] - m["lse"][:, None]),
           "rank": m["rank"], "loss_row": m["loss_row"]}
    if tokenizer is not None:
        out["tokens"] = [tokenizer.convert_ids_to_tokens(r) for r in out["ids"].tolist()]
        out["gold_tokens"] = tokenizer.convert_ids_to_tokens(out["gold"].tolist())
    return out


def pretrain_evaluate(args, model, load_and_cache_examples, tokenizer, prefix="", seed=0, topk=5):
    """trainers/run_pretraining.py:377-511 (`evaluate`, as scripts/wikihow_pretrain.sh runs it with
    --do_eval --evaluate_during_training --max_eval_steps 200) for LXRTPretraining: the per-task
    loop (:384-386), SequentialSampler and eval_batch_size = per_gpu_eval_batch_size *
    max(1, n_gpu) (:391-395), model.eval() (:416), the batch to the device (:417), masking by
    mask_tokens_sentence for the text+image stage (:433-437), max_eval_steps (:480-483), the mean
    of the per-batch losses (:485) and the results written sorted as "%s = %s\n" into
    <output_dir>/<prefix>/eval_results.txt (:502-509).
    `load_and_cache_examples(args, [task], tokenizer, evaluate=True)` returns a map-style dataset
    of tuples (input_ids, attention_mask, token_type_ids, labels, ..., images).

    Beyond the reference, whose :493-497 writes "{task}_perplexity": 0.0 under "# TODO:
    Perplexity." and reports no accuracy: {task}_perplexity = exp(sum of NLL / labelled tokens)
    over the whole evaluation (0.0 for the image-only stage, which has no masked-LM term),
    {task}_mlm_loss, _mlm_acc, _mlm_acc_top{topk}, _mlm_tokens, and per objective drawn at least
    once {task}_{objective}_acc, _loss, _batches.

    An evaluation is a pure function of (weights, data, seed): step s is masked with `seed` on
    counter stream 2 + s and the model's draws come from a local RandomState(seed), so model.rng
    and the process-wide mask counter are untouched and training resumes on the stream it would
    have had. Everything accumulates on the device and is read back once per task."""
    from torch.utils.data import DataLoader, SequentialSampler
    results = {}
    dev = model.device_
    mm = not model.multimodal_img_part
    objectives = list(model.multimodal_pretrain_objectives)
    for task, out_dir in zip(args.task_names, [args.output_dir] * len(args.task_names)):
        dataset = load_and_cache_examples(args, [task], tokenizer, evaluate=True)
        if not os.path.exists(out_dir) and getattr(args, "local_rank", -1) in (-1, 0):
            os.makedirs(out_dir)
        args.eval_batch_size = args.per_gpu_eval_batch_size * max(1, getattr(args, "n_gpu", 1))
        loader = DataLoader(dataset, sampler=SequentialSampler(dataset),
                            batch_size=args.eval_batch_size)
        rng = np.random.RandomState(seed)
        totals = torch.zeros(4, dtype=torch.float64, device=dev)
        loss_sum = torch.zeros((), dtype=torch.float64, device=dev)
        # per objective: correct decisions, decisions, summed loss, batches
        per_obj = torch.zeros(len(objectives), 4, dtype=torch.float64, device=dev)
        steps = 0
        for batch in loader:
            model.eval()
            images = batch[-1]
            B, Nimg = images.shape[:2]
            g = images.shape[-1] // model.bert.vision["patch"]
            inputs = {"images": images}
            if mm:
                ids = batch[0].to(dev, torch.int64).contiguous()
                ids, lm_labels = mask_tokens_sentence(ids, tokenizer, args, seed=seed,
                                                      stream_id=2 + steps)
                inputs.update(input_ids=ids, masked_lm_labels=lm_labels,
                              attention_mask=batch[1].to(dev))
                if getattr(args, "replace_token_type_embeddings", False) and \
                        getattr(args, "model_type", "roberta") in ("bert", "roberta"):
                    inputs["token_type_ids"] = batch[2].to(dev)
                inputs["draws"] = model.draw_mm(B, Nimg, 1 + 2 * g * g, rng=rng)
            else:
                inputs["input_ids"] = batch[0]
                inputs["draws"] = model.draw(B, Nimg, 1 + 2 * g * g, rng=rng)
            loss, _, _, stats = model.evaluate_batch(inputs, topk=topk,
                                                     totals=totals if mm else None)
            loss_sum += loss.double()
            o = objectives.index(stats["objective"])
            per_obj[o] += torch.stack([stats["objective_correct"].double(),
                                       stats["objective_count"].double(),
                                       stats["objective_loss"].double(),
                                       torch.ones((), dtype=torch.float64, device=dev)])
            steps += 1
            if getattr(args, "max_eval_steps", 0) > 0 and steps >= args.max_eval_steps:
                break
        # the one read-back of the task
        flat = torch.cat([loss_sum.view(1), totals, per_obj.view(-1)]).tolist()
        loss_sum_h, tot, po = flat[0], flat[1:5], np.asarray(flat[5:]).reshape(-1, 4)
        result = {f"{task}_loss": loss_sum_h / max(steps, 1), f"{task}_perplexity": 0.0}
        if mm:
            tokens = tot[1]
            nll = tot[0] / tokens if tokens else float("nan")
            result.update({f"{task}_perplexity": float(np.exp(nll)), f"{task}_mlm_loss": nll,
                           f"{task}_mlm_acc": tot[2] / tokens if tokens else float("nan"),
                           f"{task}_mlm_acc_top{topk}": tot[3] / tokens if tokens else float("nan"),
                           f"{task}_mlm_tokens": int(tokens)})
        for name, (correct, count, lsum, nb) in zip(objectives, po):
            if nb:
                result.update({f"{task}_{name}_acc": correct / count,
                               f"{task}_{name}_loss": lsum / nb, f"{task}_{name}_batches": int(nb)})
        results.update(result)
    out_file = os.path.join(out_dir, prefix, "eval_results.txt")
    os.makedirs(os.path.dirname(out_file), exist_ok=True)
    with open(out_file, "w") as wr:
        for key in sorted(results):
            wr.write("%s = %s\n" % (key, str(results[key])))
    return results


def build_config2(device="cuda", dtype=torch.bfloat16, seed=0, vision="ViT-B/16", joint=None):
    """Config 2 (scripts/wikihow_image_only_pretrain.sh): bert-base-uncased sizes (vocab 30522,
    type vocab 2, 512 positions) around a CLIP ViT-B/16, N = 5 images per story."""
    from .lxrt import CLIP_VISION
    j = dict(vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12,
             intermediate_size=3072, max_position_embeddings=512, type_vocab_size=2)
    j.update(joint or {})
    vis = dict(vision) if isinstance(vision, dict) else dict(CLIP_VISION[vision])
    return LXRTPretraining(LXRTConfig(**j), visual_losses="obj", multimodal_text_part=False,
                           multimodal_img_part=True, cls_id=0, sep_id=2, pad_id=1,
                           max_story_length=5, mlm_ignore_index=-1,
                           multimodal_pretrain_objectives=["patch_based_mrm_classification"],
                           clip_model_name="ViT-B/16", pretraining=True, device=device,
                           compute_dtype=dtype, seed=seed, vision=vis)


def build_pretrain_mm(device="cuda", dtype=torch.bfloat16, seed=0, vision="ViT-B/16", joint=None,
                      objectives=MM_OBJECTIVES, N=5):
    """The text+image stage (scripts/wikihow_pretrain.sh): RoBERTa-base sizes (vocab 50265) around
    a CLIP ViT-B/16, N = 5 steps of 60 tokens, MLM + ISP / PISP / MRM, mlm_ignore_index -100."""
    from .lxrt import CLIP_VISION
    j = dict(vocab_size=50265, hidden_size=768, num_hidden_layers=12, num_attention_heads=12,
             intermediate_size=3072, max_position_embeddings=514, type_vocab_size=1)
    j.update(joint or {})
    vis = dict(vision) if isinstance(vision, dict) else dict(CLIP_VISION[vision])
    return LXRTPretraining(LXRTConfig(**j), visual_losses="obj", multimodal_text_part=False,
                           multimodal_img_part=False, cls_id=0, sep_id=2, pad_id=1,
                           max_story_length=N, mlm_ignore_index=-100,
                           multimodal_pretrain_objectives=list(objectives),
                           clip_model_name="ViT-B/16", pretraining=True, device=device,
                           compute_dtype=dtype, seed=seed, vision=vis)
