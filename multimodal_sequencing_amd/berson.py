"""BERSON ordering head: BertForOrdering, HierarchicalAttention, TransformerInterEncoder, the
pointer-network decoder, losses, and beam-search ordering.

Drop-in for models/berson/modeling_bert.py (BertForOrdering :825-1402, HierarchicalAttention
:666-817, beam_search_pointer :1411-1552, berson_pointer_network :1405-1408) and
models/berson/{encoder,neural,generator}.py: same constructor / forward contract
(`model(inputs) -> (loss,)`), same state-dict names.

What changes is HOW: no per-pair Python loops and no device->host syncs inside the forward —
the span pooling, pointer scoring and small attention run as HIP kernels, the pair<->sentence
scatters use static index maps for the fixed story length N, and the pointer decoder's mask
bookkeeping is vectorised over time steps. The head is tiny (< 0.1 % of FLOPs) and runs in fp32.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _native as N_
from . import kernels as K
from .checkpoint import JsonConfigMixin, berson_from_pretrained, save_pretrained
from .params import ParamStore, Spec, attach_tree, linear_specs, ln_specs, normal, uniform, zeros
from .process_inputs import pairs_generator, prepare_berson_inputs


class BersonConfig(JsonConfigMixin, SimpleNamespace):
    """models/berson/configuration_bert.py:77-113 (the fields the head reads) plus the
    PretrainedConfig attributes (configuration_utils.py:46-58) that from_pretrained kwargs may
    override (train.py:2010-2011 passes num_labels and finetuning_task)."""

    def __init__(self, hidden_size=768, num_labels=1, initializer_range=0.02,
                 hidden_dropout_prob=0.1, **kw):
        for k, v in (("finetuning_task", None), ("output_attentions", False),
                     ("output_hidden_states", False), ("torchscript", False),
                     ("use_bfloat16", False), ("pruned_heads", {})):
            kw.setdefault(k, v)
        super().__init__(hidden_size=hidden_size, num_labels=num_labels,
                         initializer_range=initializer_range,
                         hidden_dropout_prob=hidden_dropout_prob, **kw)


def _head_specs(H, args, num_labels, std):
    ff, L = args.ff_size, args.inter_layers
    sp = linear_specs("classifier", H, num_labels, std=std)
    for i in range(L):
        b = f"encoder.transformer_inter.{i}."
        for n in ("linear_keys", "linear_values", "linear_query", "final_linear"):
            sp += linear_specs(b + "self_attn." + n, H, H, std=std)
        sp += linear_specs(b + "feed_forward.w_1", H, ff, std=std)
        sp += linear_specs(b + "feed_forward.w_2", ff, H, std=std)
        sp += ln_specs(b + "feed_forward.layer_norm", H)
        sp += ln_specs(b + "layer_norm", H)
    sp += ln_specs("encoder.layer_norm", H)
    sp += linear_specs("key_linear", 2 * H, H, std=std)
    sp += linear_specs("query_linear", H, H, std=std)
    sp += linear_specs("tanh_linear", H, 1, std=std)
    b = 1.0 / math.sqrt(H)  # nn.LSTM default init (re-initialised normal by _init_weights? no:
    # BertPreTrainedModel._init_weights touches Linear/Embedding/LayerNorm only)
    sp += [Spec("decoder.weight_ih_l0", (4 * H, H), uniform(b), transpose=True),
           Spec("decoder.weight_hh_l0", (4 * H, H), uniform(b), transpose=True),
           Spec("decoder.bias_ih_l0", (4 * H,), uniform(b)),
           Spec("decoder.bias_hh_l0", (4 * H,), uniform(b))]
    t = "two_level_encoder."
    sp += [Spec(t + "linear_in_2.weight", (1, H), normal(std), transpose=True)]
    sp += linear_specs(t + "sentence_tran", H, H, std=std)
    sp += linear_specs(t + "sentence_tran_2", H, 1, std=std)
    for n in ("pairwise_relationship", "h1_relationship", "h2_relationship"):
        sp += linear_specs(t + n, H, 2, std=std)
    sp += [Spec("pw_k.weight", (H, 4 * (H + 2)), normal(std), transpose=True)]
    return sp


class BertForOrdering(nn.Module):
    base_model_prefix = "bert"  # modeling_bert.py:462
    from_pretrained = classmethod(berson_from_pretrained)  # modeling_utils.py:208-428
    save_pretrained = save_pretrained  # modeling_utils.py:190-204

    def __init__(self, config, args, inner_model=None, tokenizer=None, load_inner_model=False,
                 device="cuda", seed=1, **kw):
        super().__init__()
        self.config = config
        self.args = args
        self.tokenizer = tokenizer
        H = config.hidden_size
        self.hidden_size = H
        self.pairwise_loss_lam = getattr(args, "pairwise_loss_lam", 0.6)
        self.n_steps = args.max_story_length
        self.store = ParamStore(_head_specs(H, args, getattr(config, "num_labels", 1),
                                            getattr(config, "initializer_range", 0.02)),
                                device, torch.float32)
        self.store.init_weights(seed=seed)
        # the inner model's slot comes first, as in the reference (`self.bert` is set before the
        # head at modeling_bert.py:860-866): named_parameters() order is what a reference-written
        # optimizer.pt indexes by position (trainer.FusedAdamW.load_state_dict)
        self.add_module("bert", inner_model)
        attach_tree(self, self.store.params)
        self._anchor = torch.zeros((), device=device, requires_grad=True)
        self.device_ = torch.device(device)
        self._maps = {}
        self.hidden_dropout_prob = getattr(config, "hidden_dropout_prob", 0.1)  # :677
        self.para_dropout = getattr(args, "para_dropout", 0.1)  # train.py:2014, :881
        self._drops = K.EVAL
        from .lxrt import _mark_stale
        self.register_load_state_dict_post_hook(_mark_stale)

    # ------------------------------------------------------------------------------------
    def ddp_units(self):
        """(units, begin_stores) for trainer.GradAllReduce: the inner model's per-layer spans;
        the head store completes as a whole before the inner model's backward begins."""
        units = {}
        if self.bert is not None:
            units[id(self.bert.store)] = self.bert.grad_units()
        return units, [self.store]

    def stores(self):
        return [self.bert.store, self.store] if self.bert is not None else [self.store]

    def zero_grad(self, set_to_none=False):  # keep the flat-buffer grad views alive
        for s in self.stores():
            s.zero_grad()

    def equip(self, critic):  # modeling_bert.py:916 (NLLLoss(reduction='none') is built in)
        self.critic = critic

    def _static_maps(self, N):
        """Index maps for the fixed story length (replace the host loops at :766-792)."""
        if N not in self._maps:
            pairs, npair = pairs_generator(N)
            E = 2 * (N - 1)
            slot = [[] for _ in range(N)]
            for j, (a, c) in enumerate(pairs):
                slot[a].append(2 * j)
                slot[c].append(2 * j + 1)
            dev = self.device_
            self._maps[N] = dict(
                slot=torch.tensor(slot, device=dev).view(N * E),  # into mix.view(B, 2*npair, H)
                pair_flat=torch.tensor([a * N + c for a, c in pairs], device=dev),
                E=E, npair=npair)
        return self._maps[N]

    def _lin(self, x, name, act=0, bias=True):
        return K.LinearFn.apply(x, self._anchor, self.store, name + ".weight",
                                name + ".bias" if bias else None, act)

    def _ln(self, x, name, eps):
        return K.LayerNormFn.apply(x, self._anchor, self.store, name, eps)

    # ------------------------------------------------------------------------------------
    def forward(self, inputs):
        """BertForOrdering.forward (:937-941): inputs = {input_ids [B][L], labels [B][N],
        images [B][N][3][R][R] (optional), ...} -> (loss,)."""
        return self._forward(**_batch_inputs(self, inputs, non_blocking=True))

    @property
    def img_part(self):
        """args.multimodal_img_part: the image-only model (no text, no joint stack)."""
        return bool(getattr(self.args, "multimodal_img_part", False))

    def encode(self, input_ids, attention_mask=None, token_type_ids=None, pairs_list=None,
               passage_length=None, pairs_num=None, sep_positions=None, ground_truth=None,
               mask_cls=None, pairwise_labels=None, cuda=None, head_mask=None, images=None):
        """:1239-1366 — returns the same 10-tuple as the reference."""
        B, npair, Lt = input_ids.shape
        N = mask_cls.shape[1]
        H = self.hidden_size
        P = B * npair
        mp = self._static_maps(N)
        if self.store.shadow_stale:  # transposed fp32 weight shadows for the head's dgrad GEMMs
            self.store.refresh_shadows()
        D = self.bert.new_dropouts()
        D.training = D.training and self.training
        self._drops = D
        ph = self.hidden_dropout_prob
        inner_img = bool(getattr(self.bert, "img_part", False))
        if self.img_part != inner_img:
            raise ValueError(f"args.multimodal_img_part = {self.img_part} but the inner model was "
                             f"built with multimodal_img_part = {inner_img}: the "
                             "head would pool rows of the wrong modality")
        if self.img_part:
            if images is None:
                raise ValueError("an image-only model (multimodal_img_part) needs images")
            # :1284-1290 with lxrt:1576-1582: lang_feats IS visn_feats [P][Tv][H]; kept in the
            # compute dtype (the span pool and sentence_tran read bf16 rows, no fp32 copy)
            rows, Lt = self.bert.encode_visual(images, pairs_list, drops=D)
            top = rows
            cls_pooled = rows[:, 0].float()  # the class-token row, not the pooler's output
            # :1326-1328 shifts sep_positions in place by [Tv // 2 - 1, Tv - 2] -> [g^2 - 1, 2 g^2]
            # from [0, 1]: the last patch of the first image is pooled with the second image.
            # Built out of place here: the caller's tensor is left as it was.
            if ("sep_shift", Lt) not in self._maps:
                self._maps[("sep_shift", Lt)] = torch.tensor([Lt // 2 - 1, Lt - 2],
                                                             device=self.device_)
            sep_positions = sep_positions + self._maps[("sep_shift", Lt)]
        else:
            joint, Lt = self.bert.encode_joint(input_ids.reshape(P, Lt),
                                               attention_mask.reshape(P, Lt),
                                               token_type_ids.reshape(P, Lt),
                                               images if not self.bert.text_part else None,
                                               pairs_list, drops=D, text_rows=True)
            rows = joint[:, :Lt]
            top = rows.float()  # lang_feats (:1289), fp32 for the head
            cls_pooled = top[:, 0]  # :1290
        # ---- HierarchicalAttention (:686-817) -------------------------------------------
        t = "two_level_encoder."
        if rows.dtype == torch.bfloat16:  # the head's one large GEMM on the bf16 MFMA kernels
            st = K.LinearLowpFn.apply(rows, self._anchor, self.store,
                                      t + "sentence_tran.weight", t + "sentence_tran.bias", K.TANH)
        else:
            st = self._lin(top, t + "sentence_tran", act=K.TANH)
        score = self._lin(st, t + "sentence_tran_2")
        mix = K.SpanPoolFn.apply(top, score.view(P, Lt), sep_positions.reshape(P, 2).contiguous(),
                                 D.site(ph, "span"))  # :735
        sample = mix.view(B, 2 * npair, H)[:, mp["slot"]].view(B, N, mp["E"], H)
        q2 = K.LinearFn.apply(sample, self._anchor, self.store, t + "linear_in_2.weight", None, 0)
        wts = torch.softmax(q2.view(B, N, mp["E"]), -1)
        final = (wts.unsqueeze(-1) * sample).sum(2)  # [B, N, H]
        cls_score = self._lin(cls_pooled, t + "pairwise_relationship")  # [P, 2]
        cls_mat = torch.zeros(B, N * N, H, device=top.device)
        cls_mat = cls_mat.index_copy(1, mp["pair_flat"], cls_pooled.view(B, npair, H))
        cs_mat = torch.zeros(B, N * N, 2, device=top.device)
        cs_mat = cs_mat.index_copy(1, mp["pair_flat"], cls_score.view(B, npair, 2))
        cls_mat = cls_mat.view(B, N, N, H)
        cs_mat = cs_mat.view(B, N, N, 2)
        # h1/h2_relationship outputs are computed but never used downstream (:751-757, :1016):
        # they do not affect loss or gradients, so they are not evaluated here.
        # ---- encode tail (:1338-1357) -------------------------------------------------------
        mcf = mask_cls.float()
        clean = final * mcf[:, :, None]
        para = self._inter_encoder(clean, mcf) * mcf[:, :, None]
        plen = passage_length.float()
        para_vec = para.sum(1) / (plen + 1e-20)[:, None]
        hcn = (para_vec.unsqueeze(0), torch.zeros_like(para_vec).unsqueeze(0))
        okey = self._lin(torch.cat([clean, para], -1), "key_linear")
        return (clean, para, hcn, okey, cls_pooled, cls_mat, cls_score, cs_mat, cs_mat, cs_mat)

    def _inter_encoder(self, top_vecs, mask):
        """TransformerInterEncoder (encoder.py:46-61) + TransformerEncoderLayer (:20-30)."""
        x = top_vecs * mask[:, :, None]
        key_bias = ((1.0 - mask) * -10000.0).contiguous()  # neural.py:210-213 with mask = 1 - m
        heads = self.args.heads
        D = self._drops
        pd = self.para_dropout
        for i in range(self.args.inter_layers):
            b = f"encoder.transformer_inter.{i}."
            h = self._ln(x, b + "layer_norm", 1e-6) if i != 0 else x
            q = self._lin(h, b + "self_attn.linear_query")
            k = self._lin(h, b + "self_attn.linear_keys")
            v = self._lin(h, b + "self_attn.linear_values")
            ctx = K.SmallAttnFn.apply(q, k, v, key_bias, heads, D.site(pd, "inter_att", i))
            # encoder.py:28 and neural.py:31-33
            out = K.dropout(self._lin(ctx, b + "self_attn.final_linear"),
                            D.site(pd, "inter_ctx", i)) + x
            inter = K.dropout(self._lin(self._ln(out, b + "feed_forward.layer_norm", 1e-6),
                                        b + "feed_forward.w_1", act=K.GELU_TANH),
                              D.site(pd, "inter_ff1", i))
            f = K.dropout(self._lin(inter, b + "feed_forward.w_2"), D.site(pd, "inter_ff2", i))
            x = f + out
        return self._ln(x, "encoder.layer_norm", 1e-6)

    def _lstm_gx(self, x):
        """x W_ih^T + b_ih for every decoder input at once (one GEMM, not one per step)."""
        return K.LinearFn.apply(x, self._anchor, self.store, "decoder.weight_ih_l0",
                                "decoder.bias_ih_l0", 0)

    def _lstm_step(self, gx, h, c):
        """nn.LSTM single step (gate order i, f, g, o) from precomputed input gates: the h GEMM
        and one fused cell kernel (sigmoid/tanh gates, c', h')."""
        gh = K.LinearFn.apply(h, self._anchor, self.store, "decoder.weight_hh_l0",
                              "decoder.bias_hh_l0", 0)
        return K.LstmCellFn.apply(gx, gh, c)

    def _forward(self, input_ids, attention_mask=None, token_type_ids=None, pairs_list=None,
                 passage_length=None, pairs_num=None, sep_positions=None, ground_truth=None,
                 mask_cls=None, pairwise_labels=None, cuda=None, head_mask=None, images=None):
        """:943-1237 — pointer decoder + pointer NLL + 0.6 * pairwise NLL."""
        (doc, _para, hcn, okey, _cls, cls_mat, cls_score, cs_mat, _h1, _h2) = self.encode(
            input_ids, attention_mask, token_type_ids, pairs_list, passage_length, pairs_num,
            sep_positions, ground_truth, mask_cls, pairwise_labels, cuda, head_mask, images)
        target = ground_truth
        tgt_len = passage_length
        B, N = target.shape
        H = self.hidden_size
        dev = doc.device
        ar = torch.arange(N, device=dev)
        valid = ar[None] < tgt_len[:, None]  # [B, N]
        # pointed_before[b][t][j] = j in target[b, :t]  (cumulative masks of :1027-1050)
        onehot = F.one_hot(target, N).to(torch.int64)  # [B, N(t), N(j)]
        pointed = (onehot.cumsum(1) - onehot).clamp_(max=1)  # exclusive prefix
        base = (1 - torch.eye(N, dtype=torch.int64, device=dev))[None] * valid[:, :, None] * \
            valid[:, None, :]
        alive = 1 - pointed  # rows/cols of already-pointed sentences are zeroed (:1036-1037)
        rela_mask = base[:, None] * alive[:, :, :, None] * alive[:, :, None, :]  # [B,t,i,j]
        rela = torch.cat([cls_mat, torch.softmax(cs_mat, -1)], -1)  # rela_encode (:919-925)
        hist = rela  # history_encode with cls_score_matrix_nn for both (:1016)
        live = rela[:, None] * rela_mask[..., None].to(rela.dtype)  # [B, t, i, j, H+2]
        forw = live.mean(3)  # rela_vec.mean(2) per t (:1061)
        back = live.mean(2)  # rela_vec.mean(1) per t (:1062)
        bidx = torch.arange(B, device=dev)[:, None]
        prev1 = torch.cat([target.new_zeros(B, 1), target[:, :-1]], 1)
        prev2 = torch.cat([target.new_zeros(B, 2), target[:, :-2]], 1)[:, :N]
        l1 = hist[bidx, prev1]  # [B, t, j, H+2] row target[t-1] (:1043, :1053)
        l2 = hist[bidx, prev2]
        l1 = l1 * (ar >= 1).to(l1.dtype)[None, :, None, None]
        l2 = l2 * (ar >= 2).to(l2.dtype)[None, :, None, None]
        pw_info = torch.cat([l1, l2, forw, back], -1)  # [B, t, j, 4(H+2)]
        pw_keys = K.LinearFn.apply(pw_info, self._anchor, self.store, "pw_k.weight", None, 0)
        dec_in = torch.cat([doc.new_zeros(B, 1, H), doc[bidx, target[:, :-1]]], 1)  # :998-1002
        h, c = hcn[0][0], hcn[1][0]
        gx = self._lstm_gx(dec_in)  # [B, N, 4H]
        outs = []
        for t in range(N):
            h, c = self._lstm_step(gx[:, t], h, c)
            outs.append(h)
        query = self._lin(torch.stack(outs, 1), "query_linear")
        nll, _logp = K.PointerFn.apply(query, pw_keys, okey, self._anchor, self.store,
                                       "tanh_linear.weight", "tanh_linear.bias",
                                       pointed.to(torch.uint8).contiguous(), tgt_len.contiguous(),
                                       target.contiguous())
        l_ptr = (nll.sum(-1) / (tgt_len.float() + 1e-20 - 1)).sum() / B  # :1140-1142
        npair = pairwise_labels.shape[1]
        lc = torch.log_softmax(cls_score, -1)
        pnll = -lc.gather(-1, pairwise_labels.reshape(-1, 1)).view(B, npair)
        pmask = (torch.arange(npair, device=dev)[None] < pairs_num[:, None]).float()
        l_pair = ((pnll * pmask).sum(-1) / (pairs_num.float() + 1e-20)).sum() / B  # :1145-1172
        self.last_loss_terms = (l_ptr.detach(), l_pair.detach())  # (pointer, pairwise) losses
        return (l_ptr + l_pair * self.pairwise_loss_lam,)

    # ------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, prev_y, prev_h, prev_c, original_keys, pointed, rela, rela_mask, hist, l1_idx,
             l2_idx):
        """BertForOrdering.step (:1368-1402) for a beam of candidates."""
        h, c = self._lstm_step(self._lstm_gx(prev_y), prev_h, prev_c)
        q = self._lin(h, "query_linear")[:, None]  # [beam, 1, H]
        nb, T = pointed.shape
        zeros = rela.new_zeros(nb, T, rela.shape[-1])
        left1 = hist[torch.arange(nb), l1_idx] if l1_idx is not None else zeros
        left2 = hist[torch.arange(nb), l2_idx] if l2_idx is not None else zeros
        rela = rela * rela_mask[..., None].to(rela.dtype)
        pw = torch.cat([left1, left2, rela.mean(2), rela.mean(1)], -1)
        keys = K.LinearFn.apply(pw, self._anchor, self.store, "pw_k.weight", None, 0)
        e = torch.tanh(q + keys + original_keys)
        e = K.LinearFn.apply(e, self._anchor, self.store, "tanh_linear.weight",
                             "tanh_linear.bias", 0).squeeze(-1)
        e = e.masked_fill(pointed.bool(), -1e9)
        return h, c, torch.log_softmax(e, -1), rela


@torch.no_grad()
def beam_search_pointer(args, model, input_ids, attention_mask=None, token_type_ids=None,
                        pairs_list=None, passage_length=None, pairs_num=None, sep_positions=None,
                        ground_truth=None, mask_cls=None, pairwise_labels=None, cuda=None,
                        head_mask=None, images=None):
    """:1411-1552 + generator.py Beam (B = 1). Ties in the k-smallest selection break toward the
    lowest flat index (deterministic); returns the ordering as a list of ints."""
    enc = model.encode(
        input_ids, attention_mask, token_type_ids, pairs_list, passage_length, pairs_num,
        sep_positions, ground_truth, mask_cls, pairwise_labels, cuda, head_mask, images)
    return _beam_decode_story(args, model, enc, 0)[0]


@torch.no_grad()
def _beam_decode_story(args, model, enc, b):
    """The host-driven beam search over story b of an encode() tuple -> (order, best score)."""
    (sent, _p, dec_init, okeys, _cls, cls_mat, _cs, cs_mat, _h1, _h2) = enc
    T = int(sent.shape[1])
    doc = sent[b]
    okeys = okeys[b:b + 1]
    H = doc.shape[-1]
    dev = doc.device
    rela = torch.cat([cls_mat[b:b + 1], torch.softmax(cs_mat[b:b + 1], -1)], -1)
    hist = rela.clone()
    W = getattr(args, "beam_size", 16)
    cands, scores, hyps = [[]], [0.0], []
    valid = W
    h, c = dec_init[0][0][b:b + 1], dec_init[1][0][b:b + 1]
    rela_mask = (1 - torch.eye(T, dtype=torch.int64, device=dev))[None]
    pointed = torch.zeros(1, T, dtype=torch.int64, device=dev)
    x = torch.zeros(1, H, device=dev)
    for t in range(T - 1):
        nb = len(cands)
        l1_idx = l2_idx = None
        if t > 0:
            index = torch.tensor([cd[-1] for cd in cands], device=dev)
            x = doc[index]
            ar = torch.arange(nb, device=dev)
            pointed = pointed.clone()
            pointed[ar, index] = 1
            rela_mask = rela_mask.clone()
            rela_mask[ar, :, index] = 0
            rela_mask[ar, index] = 0
            l1_idx = index
            if t > 1:
                l2_idx = torch.tensor([cd[-2] for cd in cands], device=dev)
        h, c, logp, rela = model.step(x, h, c, okeys, pointed, rela, rela_mask, hist, l1_idx, l2_idx)
        score = (-logp + torch.tensor(scores, device=dev)[:, None]).float().cpu()
        flat = score.reshape(-1).numpy()
        k = min(valid, flat.size)
        order = np.lexsort((np.arange(flat.size), flat))[:k]
        new_c, new_s, remain = [], [], []
        for ix in order:
            bi, ti = int(ix) // T, int(ix) % T
            cand = cands[bi] + [ti]
            if len(cand) == T - 1:
                hyps.append((cand, float(flat[ix])))
            else:
                remain.append(bi)
                new_c.append(cand)
                new_s.append(float(flat[ix]))
        valid -= k - len(remain)
        if valid == 0:
            break
        ri = torch.tensor(remain, dtype=torch.long, device=dev)
        h, c = h[ri], c[ri]
        pointed, rela_mask, rela, hist = pointed[ri], rela_mask[ri], rela[ri], hist[ri]
        cands, scores = new_c, new_s
    best, best_score = sorted(hyps, key=lambda z: z[1])[0]
    return best + sorted(set(range(T)) - set(best))[:1], best_score


def _decoder_inputs(model, enc):
    """An encode() tuple -> (B, N, H, ins), `ins` the six inputs every decoder wrapper of _native
    takes first: doc, okey, hist = (cls_mat, softmax(cs_mat)), h0, c0 (contiguous) and the nine
    decoder weights. For the no-grad entries; OrderScoreFn takes the tensors with their graph."""
    (sent, _p, dec_init, okeys, _cls, cls_mat, _cs, cs_mat, _h1, _h2) = enc
    B, N, H = sent.shape
    hist = torch.cat([cls_mat, torch.softmax(cs_mat, -1)], -1).contiguous()
    return B, N, H, (sent.contiguous(), okeys.contiguous(), hist, dec_init[0][0].contiguous(),
                     dec_init[1][0].contiguous(), [model.store.f32(n) for n in K.ORDER_WEIGHTS])


def _fit_chunk(size_fn, n, low=1, cap=None):
    """-> (count, bytes): the largest count, halving from n down to `low`, whose workspace of
    size_fn(count) bytes fits `cap` (default: SCORE_WS_CAP, read at call time); `low` is taken
    whatever it needs (a single candidate is always tried). bytes 0 = unsupported shape."""
    if cap is None:
        cap = SCORE_WS_CAP
    while n > low:
        nbytes = size_fn(n)
        if 0 < nbytes <= cap:
            return n, nbytes
        n = max(low, (n + 1) // 2)
    return low, size_fn(low)


@torch.no_grad()
def beam_decode_batch(args, model, enc):
    """Every story of an encode() tuple through ONE mmseq_beam_search (the beam state stays on
    the device, nothing synchronises until the caller reads the result) -> (order int64 [B][N],
    best score f32 [B]) on the device. Where the ABI reports the shape unsupported, the stories
    go through the per-story decoder one by one."""
    B, N, H = enc[0].shape
    W = int(getattr(args, "beam_size", 16))
    dev = enc[0].device
    order = torch.empty(B, N, dtype=torch.int64, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    nbytes = N_.beam_workspace(B, N, H, W)
    st = N_.EUNSUPPORTED
    if nbytes > 0:
        ws = K._cached_ws(model, "_beam_ws", (B, N, H, W), nbytes, dev)
        st = N_.beam_search(*_decoder_inputs(model, enc)[3], W, order, score, ws)
    if st == N_.EUNSUPPORTED:
        res = [_beam_decode_story(args, model, enc, b) for b in range(B)]
        order = torch.tensor([r[0] for r in res], dtype=torch.int64, device=dev)
        score = torch.tensor([r[1] for r in res], dtype=torch.float32, device=dev)
    return order, score


@torch.no_grad()
def beam_search_pointer_batch(args, model, input_ids, attention_mask=None, token_type_ids=None,
                              pairs_list=None, passage_length=None, pairs_num=None,
                              sep_positions=None, ground_truth=None, mask_cls=None,
                              pairwise_labels=None, cuda=None, head_mask=None, images=None):
    """beam_search_pointer for B >= 1 stories: one encode at the batched shape, one device-resident
    decode, one device-to-host copy of the orders -> list of B orderings. The best hypotheses'
    scores stay on the device in `model.last_beam_scores` ([B] f32)."""
    enc = model.encode(
        input_ids, attention_mask, token_type_ids, pairs_list, passage_length, pairs_num,
        sep_positions, ground_truth, mask_cls, pairwise_labels, cuda, head_mask, images)
    order, model.last_beam_scores = beam_decode_batch(args, model, enc)
    return order.tolist()


def berson_pointer_network(args, model, tokenizer, inputs):
    """:1405-1408 — ordering indices for one story."""
    return beam_search_pointer(args, model, **_batch_inputs(model, inputs))


def _batch_inputs(model, inputs, non_blocking=False):
    """The berson_inputs dict (+ images on the device) of a story batch. An image-only model
    (args.multimodal_img_part) may get a batch without "input_ids" and "labels": the story count
    and N come from the images, the labels default to 0 .. N-1."""
    images = inputs.get("images")
    img_part = model.img_part
    if img_part:
        if images is None:
            raise ValueError("an image-only model (multimodal_img_part) needs inputs['images']")
        ids, labels = inputs.get("input_ids"), inputs.get("labels")
        if labels is None:
            labels = torch.arange(images.shape[1]).expand(images.shape[0], -1)
    else:
        ids, labels = inputs["input_ids"], inputs["labels"]
    berson = prepare_berson_inputs(ids, labels, model.n_steps, device=model.device_,
                                   img_part=img_part)
    if images is not None:
        images = images.to(model.device_, torch.float32, non_blocking=non_blocking).contiguous()
    berson["images"] = images
    return berson


def berson_pointer_network_batch(args, model, tokenizer, inputs, decode="beam", enumeration=None):
    """Ordering indices for the B >= 1 stories of `inputs` (same keys as berson_pointer_network)
    -> list of B lists. decode="beam": the device-resident beam search. decode="exact": the
    arg-min over all N! orders (exact_order_batch, N <= 7); `model.last_beam_scores` then holds
    the exact optimum's scores. decode="mbr_acc" / "mbr_tau": the order with the largest expected
    positional accuracy / Kendall's tau under the decoder's own distribution
    (order_posterior_batch: all N! orders for N <= 7, above that args.mbr_samples (256) ancestral
    samples with seed args.mbr_seed (0)); `model.last_beam_scores` then holds the chosen orders'
    pointer NLLs. berson_evaluate takes any of them as its `pointer_network_batch`, e.g.
    functools.partial(berson_pointer_network_batch, decode="mbr_tau").
    enumeration (default args.order_enumeration, else "flat") says how all N! orders are scored:
    "flat" as above; "tree": through the prefix tree (enumerate_orders_batch), which carries
    decode="exact" and the exact posterior of "mbr_*" up to N = TREE_MAX_N = 9; above that "exact"
    raises and "mbr_*" samples as with "flat".
    decode="pairwise": the exact optimum of the pairwise head (pairwise_order_batch, N <= 12);
    `model.last_beam_scores` then holds its pnll. decode="joint": the arg-min over all N! orders
    of the model's own training loss J (joint_order_batch), enumerated as for "exact";
    `model.last_beam_scores` then holds J."""
    if decode not in ("beam", "exact", "mbr_acc", "mbr_tau", "pairwise", "joint"):
        raise ValueError("decode must be 'beam', 'exact', 'mbr_acc' or 'mbr_tau', 'pairwise' or "
                         f"'joint', got {decode!r}")
    if enumeration is None:
        enumeration = getattr(args, "order_enumeration", "flat")
    if enumeration not in ("flat", "tree"):
        raise ValueError(f"enumeration must be 'flat' or 'tree', got {enumeration!r}")
    tree = enumeration == "tree"
    berson = _batch_inputs(model, inputs)
    if decode == "beam":
        return beam_search_pointer_batch(args, model, **berson)
    with torch.no_grad():
        enc = model.encode(**berson)
        if decode == "exact":
            order, model.last_beam_scores, _ = exact_order_batch(
                args, model, enc, method="tree" if tree else "flat")
            return order.tolist()
        if decode == "pairwise":
            post = pairwise_order_batch(args, model, enc)
            model.last_beam_scores = post["pnll"]
            return post["order"].tolist()
        if decode == "joint":
            order, model.last_beam_scores, _ = joint_order_batch(
                args, model, enc, method="tree" if tree else "flat")
            return order.tolist()
        N = enc[0].shape[1]
        if tree:
            source = "tree" if N <= TREE_MAX_N else "sample"
        else:
            source = "exact" if N <= EXACT_MAX_N else "sample"
        post = order_posterior_batch(args, model, enc, source=source,
                                     samples=int(getattr(args, "mbr_samples", 256)),
                                     seed=int(getattr(args, "mbr_seed", 0)))
        idx = post[decode + "_index"].to(torch.int64).clamp_(min=0)
        model.last_beam_scores = post["nll"].gather(1, idx[:, None])[:, 0]
    return post[decode + "_order"].tolist()


# ------------------------------------------------------------------------------------------------
# Scoring candidate orders, n-best and exact decode on ONE encoder output.
SCORE_WS_CAP = 256 << 20  # bytes of mmseq_order_score workspace per call; above it K is chunked
EXACT_MAX_N = 7           # 7! = 5040 candidates per story
TREE_MAX_N = 9            # 9! = 362880 leaves of the prefix tree (mmseq_order_tree)


def check_orders(orders, B, N):
    """Host-side validation of candidate orders given as a list or a CPU tensor -> int64 CPU tensor
    [K][N] or [B][K][N]. Every candidate must be a permutation of 0 .. N-1; a ValueError names
    the first one that is not."""
    try:
        o = torch.as_tensor(orders)
    except (ValueError, TypeError) as e:  # ragged lists
        raise ValueError(f"orders: every candidate must hold N = {N} entries ({e})") from None
    if o.dtype.is_floating_point or o.dtype == torch.bool:
        raise ValueError(f"orders must hold integers, got {o.dtype}")
    o = o.to(torch.int64)
    if o.dim() not in (2, 3) or o.shape[-1] != N or o.shape[-2] < 1:
        raise ValueError(f"orders must be [K][{N}] or [{B}][K][{N}] with K >= 1, got "
                         f"{tuple(o.shape)}")
    if o.dim() == 3 and o.shape[0] != B:
        raise ValueError(f"orders [B][K][N] must hold B = {B} stories, got {o.shape[0]}")
    flat = o.reshape(-1, N)
    ok = (flat.sort(-1).values == torch.arange(N)).all(-1)
    if not bool(ok.all()):
        i = int((~ok).nonzero()[0])
        K = o.shape[-2]
        where = f"candidate {i % K}" + (f" of story {i // K}" if o.dim() == 3 else "")
        row = flat[i].tolist()
        why = "an entry outside 0 .. N-1" if min(row) < 0 or max(row) >= N else "a repeated entry"
        raise ValueError(f"orders: {where} = {row} is no permutation of 0 .. {N - 1}: {why}")
    return o.contiguous()


@torch.no_grad()
def score_orders_host(args, model, enc, orders, return_steps=False, chunk=128):
    """Teacher-forced pointer NLL of candidate orders in torch, built on `model.step` (the
    per-story decoder's step, :1368-1402): the second scorer beside mmseq_order_score and what
    score_orders_batch falls back to where the ABI reports the shape unsupported. `orders` as for
    score_orders_batch (a device tensor is copied to the host and validated) -> nll f32 [B][K]
    (and the per-step terms [B][K][N-1]) on the encoder output's device."""
    (sent, _p, dec_init, okeys, _cls, cls_mat, _cs, cs_mat, _h1, _h2) = enc
    B, N, H = sent.shape
    dev = sent.device
    o = check_orders(orders.cpu() if torch.is_tensor(orders) else orders, B, N).to(dev)
    Kn = o.shape[-2]
    nll = torch.zeros(B, Kn, dtype=torch.float32, device=dev)
    steps = torch.zeros(B, Kn, max(N - 1, 0), dtype=torch.float32, device=dev)
    for b in range(B if N > 1 else 0):
        hist1 = torch.cat([cls_mat[b:b + 1], torch.softmax(cs_mat[b:b + 1], -1)], -1)
        for k0 in range(0, Kn, chunk):
            cand = (o if o.dim() == 2 else o[b])[k0:k0 + chunk]
            k = cand.shape[0]
            ar = torch.arange(k, device=dev)
            hist = hist1.expand(k, -1, -1, -1).contiguous()
            rela = hist.clone()
            h = dec_init[0][0][b:b + 1].expand(k, -1).contiguous()
            c = dec_init[1][0][b:b + 1].expand(k, -1).contiguous()
            rela_mask = (1 - torch.eye(N, dtype=torch.int64, device=dev))[None].repeat(k, 1, 1)
            pointed = torch.zeros(k, N, dtype=torch.int64, device=dev)
            x = torch.zeros(k, H, dtype=sent.dtype, device=dev)
            total = torch.zeros(k, dtype=torch.float32, device=dev)
            for t in range(N - 1):
                l1_idx = l2_idx = None
                if t > 0:
                    l1_idx = cand[:, t - 1]
                    x = sent[b][l1_idx]
                    pointed[ar, l1_idx] = 1
                    rela_mask[ar, :, l1_idx] = 0
                    rela_mask[ar, l1_idx] = 0
                    if t > 1:
                        l2_idx = cand[:, t - 2]
                h, c, logp, rela = model.step(x, h, c, okeys[b:b + 1], pointed, rela, rela_mask,
                                              hist, l1_idx, l2_idx)
                step = -logp.float().gather(1, cand[:, t:t + 1])[:, 0]
                steps[b, k0:k0 + k, t] = step
                total = total + step
            nll[b, k0:k0 + k] = total
    return (nll, steps) if return_steps else nll


def _device_orders(orders, B, N, dev):
    """Candidate orders for a device entry: a device tensor is checked for shape only (no
    synchronisation), anything else is validated on the host (check_orders) and copied."""
    if torch.is_tensor(orders) and orders.is_cuda:
        o = orders
        if o.dtype != torch.int64 or o.dim() not in (2, 3) or o.shape[-1] != N or \
                o.shape[-2] < 1 or (o.dim() == 3 and o.shape[0] != B):
            raise ValueError(f"orders must be int64 [K][{N}] or [{B}][K][{N}] with K >= 1, got "
                             f"{o.dtype} {tuple(o.shape)}")
        return o
    return check_orders(orders, B, N).to(dev)


def _score_chunk(B, N, H, Kn):
    """-> (candidates per call, workspace bytes) of mmseq_order_score under SCORE_WS_CAP."""
    return _fit_chunk(lambda k: N_.order_score_workspace(B, N, H, k), Kn)


@torch.no_grad()
def score_orders_batch(args, model, enc, orders, return_steps=False):
    """Teacher-forced pointer NLL of K candidate orders for every story of an encode() tuple
    through mmseq_order_score: what `model({**inputs, "labels": order})` reports as the pointer
    loss x (N - 1), without the encoder. `orders`: a list or tensor [K][N] (one list for all
    stories) or [B][K][N]. A list or CPU tensor is validated here (ValueError naming the
    candidate); a device tensor is not synchronised on, and a candidate in it that is no
    permutation comes back as +inf. -> nll f32 [B][K] on the device, with return_steps=True also
    the per-step terms [B][K][N-1].

    The workspace is cached on the model like the beam's. Its size grows with B*K*H, so K is
    split (halved until it fits) into chunks whose workspace stays within SCORE_WS_CAP = 256 MiB
    per call (B = 32, H = 768, all 120 orders of N = 5 need 90 MiB: one call; the 5040 orders of
    N = 7 at H = 1024 go in chunks of 158). Where the ABI reports the shape
    unsupported (N > 16) the candidates go through score_orders_host."""
    B, N, H = enc[0].shape
    dev = enc[0].device
    o = _device_orders(orders, B, N, dev)
    Kn = int(o.shape[-2])
    kc, nbytes = _score_chunk(B, N, H, Kn)
    if nbytes == 0:
        return score_orders_host(args, model, enc, o, return_steps)
    nll = torch.empty(B, Kn, dtype=torch.float32, device=dev)
    steps = torch.empty(B, Kn, N - 1, dtype=torch.float32, device=dev) if return_steps else None
    ins = _decoder_inputs(model, enc)[3]
    for k0, k, whole in K._chunks(Kn, kc):
        nb = nbytes if k == kc else N_.order_score_workspace(B, N, H, k)
        ws = K._cached_ws(model, "_score_ws", (B, N, H, k), nb, dev)
        o_c = o if whole else o[..., k0:k0 + k, :].contiguous()
        nll_c = nll if whole else torch.empty(B, k, dtype=torch.float32, device=dev)
        st_c = None
        if return_steps:
            st_c = steps if whole else torch.empty(B, k, N - 1, dtype=torch.float32, device=dev)
        N_._check_shape(N_.order_score(*ins, o_c.contiguous(), nll_c, st_c, ws),
                        "mmseq_order_score")
        if not whole:
            nll[:, k0:k0 + k] = nll_c
            if return_steps:
                steps[:, k0:k0 + k] = st_c
    return (nll, steps) if return_steps else nll


def berson_score_orders(args, model, tokenizer, inputs, orders, return_steps=False):
    """Pointer NLL of candidate orders for the B >= 1 stories of `inputs` (same keys as
    berson_pointer_network_batch): one encode, one scoring call -> score_orders_batch's result."""
    with torch.no_grad():
        enc = model.encode(**_batch_inputs(model, inputs))
        return score_orders_batch(args, model, enc, orders, return_steps)


# ------------------------------------------------------------------------------------------------
# Gradients of candidate-order scores and sequence-level losses.
def score_orders_grad(args, model, enc, orders):
    """score_orders_batch with a graph: nll f32 [B][K] of K candidate orders per story, attached
    to the graph of the encode() tuple `enc` (K.OrderScoreFn: mmseq_order_score forward, the same
    bits as score_orders_batch, mmseq_order_score_bwd backward). Gradients reach the encoder
    through doc, okey, cls_mat, cs_mat and the decoder's initial state, and the nine decoder
    weights through the head store. `orders` as for score_orders_batch; a candidate of a device
    tensor that is no permutation scores +inf and contributes no gradient. K is chunked so that
    the backward workspace stays within SCORE_WS_CAP. Where the ABI reports the shape unsupported
    (N > 16) the candidates go through score_orders_autograd."""
    (sent, _p, dec_init, okeys, _cls, cls_mat, _cs, cs_mat, _h1, _h2) = enc
    B, N, H = sent.shape
    o = _device_orders(orders, B, N, sent.device)
    if K.order_grad_chunk(B, N, H, int(o.shape[-2]), SCORE_WS_CAP)[1] == 0:
        return score_orders_autograd(args, model, enc, o)
    hist = torch.cat([cls_mat, torch.softmax(cs_mat, -1)], -1)
    return K.OrderScoreFn.apply(sent, okeys, hist, dec_init[0][0], dec_init[1][0], model._anchor,
                                model.store, o, SCORE_WS_CAP)


def score_orders_autograd(args, model, enc, orders):
    """The value and the gradients of score_orders_grad in torch only: the encoder output tiled K
    times through the training decoder's own Functions (LinearFn, LstmCellFn, PointerFn), i.e.
    _forward's pointer loop on B*K rows with labels = the candidates. It materialises
    [B*K][N][N][N][H+2] and projects hist once per (candidate, step, key): the fallback where
    mmseq_order_score_bwd reports the shape unsupported, and the cross-check of the tests. The
    candidates are validated on the host (a device tensor is copied there)."""
    (sent, _p, dec_init, okeys, _cls, cls_mat, _cs, cs_mat, _h1, _h2) = enc
    B, N, H = sent.shape
    dev = sent.device
    o = check_orders(orders.cpu() if torch.is_tensor(orders) else orders, B, N).to(dev)
    Kn = int(o.shape[-2])
    if N == 1:
        return sent.new_zeros(B, Kn) + 0.0 * sent.sum()
    target = (o[None].expand(B, -1, -1) if o.dim() == 2 else o).reshape(B * Kn, N)
    R = B * Kn

    def tile(x):
        return x[:, None].expand(B, Kn, *x.shape[1:]).reshape(R, *x.shape[1:])

    doc, okey = tile(sent), tile(okeys)
    hist = tile(torch.cat([cls_mat, torch.softmax(cs_mat, -1)], -1))
    ar = torch.arange(N, device=dev)
    onehot = F.one_hot(target, N).to(torch.int64)
    pointed = (onehot.cumsum(1) - onehot).clamp_(max=1)
    base = (1 - torch.eye(N, dtype=torch.int64, device=dev))[None]
    alive = 1 - pointed
    rela_mask = base[:, None] * alive[:, :, :, None] * alive[:, :, None, :]
    live = hist[:, None] * rela_mask[..., None].to(hist.dtype)
    forw, back = live.mean(3), live.mean(2)
    ridx = torch.arange(R, device=dev)[:, None]
    prev1 = torch.cat([target.new_zeros(R, 1), target[:, :-1]], 1)
    prev2 = torch.cat([target.new_zeros(R, 2), target[:, :-2]], 1)[:, :N]
    l1 = hist[ridx, prev1] * (ar >= 1).to(hist.dtype)[None, :, None, None]
    l2 = hist[ridx, prev2] * (ar >= 2).to(hist.dtype)[None, :, None, None]
    pw_keys = K.LinearFn.apply(torch.cat([l1, l2, forw, back], -1), model._anchor, model.store,
                               "pw_k.weight", None, 0)
    dec_in = torch.cat([doc.new_zeros(R, 1, H), doc[ridx, target[:, :-1]]], 1)
    h, c = tile(dec_init[0][0]), tile(dec_init[1][0])
    gx = model._lstm_gx(dec_in)
    outs = []
    for t in range(N):
        h, c = model._lstm_step(gx[:, t], h, c)
        outs.append(h)
    query = model._lin(torch.stack(outs, 1), "query_linear")
    tgt_len = torch.full((R,), N, dtype=torch.int64, device=dev)
    nll, _logp = K.PointerFn.apply(query, pw_keys, okey, model._anchor, model.store,
                                   "tanh_linear.weight", "tanh_linear.bias",
                                   pointed.to(torch.uint8).contiguous(), tgt_len, target.contiguous())
    return nll[:, :N - 1].sum(-1).view(B, Kn)


def order_gains(orders, gold, metric="tau"):
    """Per-candidate gain of orders int64 [K][N] or [B][K][N] against gold [B][N] -> f32 [B][K]:
    metric="acc" the share of positions that agree, "tau" Kendall's tau, both as
    evaluate.cal_result computes them per story (and as mmseq_order_posterior's gain_acc /
    gain_tau against a posterior that is a point mass on gold). N = 1: 1. A candidate that is no
    permutation gets some finite value; it is meant to weigh 0."""
    if metric not in ("tau", "acc"):
        raise ValueError(f"metric must be 'tau' or 'acc', got {metric!r}")
    B, N = gold.shape
    o = orders[None].expand(B, -1, -1) if orders.dim() == 2 else orders
    if metric == "acc":
        return (o == gold[:, None]).float().mean(-1)
    if N == 1:
        return torch.ones(o.shape[:2], dtype=torch.float32, device=gold.device)
    pos_o = o.clamp(0, N - 1).argsort(-1)  # position of every sentence in the candidate
    pos_g = gold.argsort(-1)[:, None]
    so = torch.sign(pos_o[..., :, None] - pos_o[..., None, :])
    sg = torch.sign(pos_g[..., :, None] - pos_g[..., None, :])
    upper = torch.triu(torch.ones(N, N, dtype=torch.bool, device=gold.device), 1)
    disc = ((so != sg) & upper).sum((-1, -2)).float()
    return 1.0 - 2.0 * disc / (N * (N - 1) / 2)


def order_loss(nll, orders, gold, kind, metric="tau", alpha=1.0, margin=1.0, refs=None):
    """A sequence-level loss over scored candidates, pure torch on nll [B][K] (differentiable),
    mean over stories. orders int64 [K][N] or [B][K][N], gold int64 [B][N].
      "risk":    sum_k softmax_k(-alpha nll) (1 - gain(order_k, gold)), gain by `metric`
                 (order_gains); a +inf score weighs 0.
      "set_nll": -logsumexp_{k in refs}(-nll_k) / (N - 1), the likelihood of a set of acceptable
                 orders; refs bool [B][K], by default the candidates equal to gold. Every story
                 needs at least one.
      "margin":  relu(margin + nll_gold - min_{k wrong} nll_k) / (N - 1), nll_gold the best score
                 in refs and wrong the candidates outside refs; 0 where there is no wrong one.
                 margin = 1.0 is the value of the reference's own ranking losses."""
    B, N = gold.shape
    if kind == "risk":
        w = torch.softmax(-alpha * nll, -1)
        return (w * (1.0 - order_gains(orders, gold, metric))).sum(-1).mean()
    if kind not in ("set_nll", "margin"):
        raise ValueError(f"kind must be 'risk', 'set_nll' or 'margin', got {kind!r}")
    if refs is None:
        o = orders[None].expand(B, -1, -1) if orders.dim() == 2 else orders
        refs = (o == gold[:, None]).all(-1)
    steps = max(N - 1, 1)
    inf = float("inf")
    if kind == "set_nll":
        return (-torch.logsumexp((-nll).masked_fill(~refs, -inf), -1) / steps).mean()
    right = nll.masked_fill(~refs, inf).amin(-1)
    wrong = nll.masked_fill(refs, inf).amin(-1)
    return (torch.relu(margin + right - wrong) / steps).mean()


def _candidate_set(orders):
    """orders int64 [B][K][N]: every row equal to an earlier row of its story becomes -1 (no
    permutation: it scores +inf and contributes no gradient), so the list is a set."""
    same = (orders[:, :, None] == orders[:, None, :]).all(-1)  # [B][K][K]
    Kn = orders.shape[1]
    earlier = torch.tril(torch.ones(Kn, Kn, dtype=torch.bool, device=orders.device), -1)
    dup = (same & earlier).any(-1)
    return torch.where(dup[..., None], torch.full_like(orders, -1), orders)


def sequence_loss(args, model, inputs, objective="risk", candidates="sample", samples=16, seed=0,
                  seq_lam=1.0, **loss_kw):
    """The training loss of `model(inputs)` plus a sequence-level term over a candidate list, from
    ONE encode -> (loss, terms):
        loss = l_ptr + pairwise_loss_lam * l_pair + seq_lam * l_seq
    l_ptr is the gold order's score / (N - 1) and l_pair the pairwise NLL, both as _forward
    computes them (:1140-1172, stories of full length N); l_seq = order_loss(objective, **loss_kw)
    over the candidates. The gold order is candidate 0; the others are `samples` ancestral
    samples (sample_orders_batch, seed), the beam's n-best list or all N! orders (N <= 7), chosen
    without a gradient; a repeat of an earlier candidate is taken out of the list. `terms` holds
    "ptr", "pair" and "seq", detached. trainer.train_step takes
    `lambda inp: (sequence_loss(args, model, inp, ...)[0],)` as its model."""
    import itertools
    if candidates not in ("sample", "nbest", "all"):
        raise ValueError(f"candidates must be 'sample', 'nbest' or 'all', got {candidates!r}")
    berson = _batch_inputs(model, inputs)
    enc = model.encode(**berson)
    gold = berson["ground_truth"]
    B, N = gold.shape
    dev = gold.device
    with torch.no_grad():
        if candidates == "sample":
            others, _nll = sample_orders_batch(args, model, enc, samples, seed)
        elif candidates == "nbest":
            others, _nll, _count = beam_nbest_batch(args, model, enc)
        else:
            if N > EXACT_MAX_N:
                raise ValueError(f"candidates='all' enumerates N! orders: N = {N} exceeds "
                                 f"{EXACT_MAX_N}")
            others = torch.tensor(list(itertools.permutations(range(N))), dtype=torch.int64,
                                  device=dev)[None].expand(B, -1, -1)
        orders = _candidate_set(torch.cat([gold[:, None], others], 1)).contiguous()
    nll = score_orders_grad(args, model, enc, orders)
    l_ptr = (nll[:, 0] / max(N - 1, 1)).sum() / B
    cls_score = enc[6]
    pairwise_labels, pairs_num = berson["pairwise_labels"], berson["pairs_num"]
    npair = pairwise_labels.shape[1]
    lc = torch.log_softmax(cls_score, -1)
    pnll = -lc.gather(-1, pairwise_labels.reshape(-1, 1)).view(B, npair)
    pmask = (torch.arange(npair, device=dev)[None] < pairs_num[:, None]).float()
    l_pair = ((pnll * pmask).sum(-1) / (pairs_num.float() + 1e-20)).sum() / B
    l_seq = order_loss(nll, orders, gold, objective, **loss_kw)
    terms = {"ptr": l_ptr.detach(), "pair": l_pair.detach(), "seq": l_seq.detach()}
    return l_ptr + model.pairwise_loss_lam * l_pair + seq_lam * l_seq, terms


def exact_from_scores(nll):
    """nll [B][K] -> (index of the smallest score [B], that score [B], second-smallest minus
    smallest [B]; inf where K = 1). Ties go to the LOWEST candidate index, stated here instead of
    left to argmin's choice among equals: the smallest index whose score equals the minimum."""
    B, Kn = nll.shape
    best = nll.min(1).values
    ar = torch.arange(Kn, device=nll.device)
    idx = torch.where(nll == best[:, None], ar, torch.full_like(ar, Kn)).min(1).values
    rest = nll.masked_fill(ar[None] == idx[:, None], float("inf"))
    return idx, best, rest.min(1).values - best


def _tree_rows(B, N, H):
    """-> (rows, workspace bytes) for mmseq_order_tree: the chunk cap, halving from the widest
    level's B * N! / 2 rows (unchunked) down to the minimum B * N, whose workspace fits
    SCORE_WS_CAP (the minimum is taken whatever it needs); bytes 0 = unsupported."""
    low = max(B * N, 1)
    return _fit_chunk(lambda rows: N_.order_tree_workspace(B, N, H, rows),
                      max(low, B * math.factorial(N) // 2), low)


@torch.no_grad()
def enumerate_orders_batch(args, model, enc, return_orders=False):
    """The pointer NLL of ALL N! orders for every story of an encode() tuple through ONE
    mmseq_order_tree: the prefix tree, every shared prefix stepped once -> nll f32 [B][N!] on the
    device, entry k the k-th order of itertools.permutations(range(N)) (score_orders_batch's
    result for that list, to fp32 GEMM rounding), with return_orders=True also that list, orders
    int64 [N!][N], unranked on the device and shared by all stories. N <= TREE_MAX_N = 9;
    ValueError above. The tree is walked in chunks of `rows` slot rows, the largest count whose
    workspace stays within SCORE_WS_CAP; the workspace is cached on the model like the beam's.
    A shape outside the ABI's limits raises _native.Unsupported."""
    B, N, H = enc[0].shape
    if N > TREE_MAX_N:
        raise ValueError(f"enumerate_orders_batch walks all N! orders: N = {N} exceeds "
                         f"{TREE_MAX_N}")
    dev = enc[0].device
    rows, nbytes = _tree_rows(B, N, H)
    if nbytes == 0:
        raise N_.Unsupported(f"enumerate_orders_batch: B={B} N={N} H={H} is outside "
                             "mmseq_order_tree's limits")
    Kn = math.factorial(N)
    nll = torch.empty(B, Kn, dtype=torch.float32, device=dev)
    orders = torch.empty(Kn, N, dtype=torch.int64, device=dev) if return_orders else None
    ws = K._cached_ws(model, "_tree_ws", (B, N, H, rows), nbytes, dev)
    N_._check_shape(N_.order_tree(*_decoder_inputs(model, enc)[3], rows, nll, orders, ws),
                    "mmseq_order_tree")
    return (nll, orders) if return_orders else nll


@torch.no_grad()
def exact_order_batch(args, model, enc, method="flat"):
    """The optimum over ALL N! orders (itertools.permutations order) for every story of an
    encode() tuple -> (order int64 [B][N], score f32 [B], margin f32 [B] = second-best minus
    best) on the device. Ties go to the lowest candidate index.
    method="flat": through one score_orders_batch; N <= 7; ValueError above.
    method="tree": through enumerate_orders_batch (the prefix tree); N <= TREE_MAX_N = 9."""
    import itertools
    if method not in ("flat", "tree"):
        raise ValueError(f"method must be 'flat' or 'tree', got {method!r}")
    B, N, _H = enc[0].shape
    if method == "tree":
        if N > TREE_MAX_N:
            raise ValueError(f"exact_order_batch(method='tree') enumerates N! orders: N = {N} "
                             f"exceeds {TREE_MAX_N}")
        nll, perms = enumerate_orders_batch(args, model, enc, return_orders=True)
        idx, best, margin = exact_from_scores(nll)
        return perms[idx], best, margin
    if N > EXACT_MAX_N:
        raise ValueError(f"exact_order_batch enumerates N! orders: N = {N} exceeds {EXACT_MAX_N}")
    perms = torch.tensor(list(itertools.permutations(range(N))), dtype=torch.int64,
                         device=enc[0].device)
    idx, best, margin = exact_from_scores(score_orders_batch(args, model, enc, perms))
    return perms[idx], best, margin


@torch.no_grad()
def beam_nbest_batch(args, model, enc):
    """Every finished hypothesis of the beam (mmseq_beam_search_nbest) for every story of an
    encode() tuple -> (orders int64 [B][W][N], scores f32 [B][W], count int32 [B]) on the device,
    ascending by score; entry 0 is beam_decode_batch's result. Rows count[b] .. W-1 hold -1 and
    +inf. W = args.beam_size. An unsupported shape raises (_native.Unsupported)."""
    B, N, H = enc[0].shape
    W = int(getattr(args, "beam_size", 16))
    dev = enc[0].device
    orders = torch.full((B, W, N), -1, dtype=torch.int64, device=dev)
    scores = torch.full((B, W), float("inf"), dtype=torch.float32, device=dev)
    count = torch.zeros(B, dtype=torch.int32, device=dev)
    nbytes = N_.beam_workspace(B, N, H, W)
    if nbytes == 0:
        raise N_.Unsupported(f"beam_nbest_batch: B={B} N={N} H={H} W={W} is outside "
                             "mmseq_beam_search's limits")
    ws = K._cached_ws(model, "_beam_ws", (B, N, H, W), nbytes, dev)
    N_._check_shape(N_.beam_search_nbest(*_decoder_inputs(model, enc)[3], W, orders, scores, count,
                                         ws), "mmseq_beam_search_nbest")
    return orders, scores, count


# ------------------------------------------------------------------------------------------------
# Posterior over orders, sampling and minimum-risk decode.
def _gather_orders(orders, index):
    """orders [K][N] or [B][K][N], index int32 [B] (-1: none) -> int64 [B][N], -1 rows for -1."""
    idx = index.to(torch.int64)
    safe = idx.clamp(min=0)
    rows = orders[safe] if orders.dim() == 2 else \
        orders.gather(1, safe[:, None, None].expand(-1, 1, orders.shape[-1]))[:, 0]
    return torch.where(idx[:, None] >= 0, rows, torch.full_like(rows, -1))


@torch.no_grad()
def order_posterior(orders, nll, mode="weights"):
    """Scored candidate orders -> their posterior (mmseq_order_posterior). orders: int64 device
    tensor [K][N] (one list for all stories) or [B][K][N]; nll f32 [B][K], +inf (or an order that
    is no permutation, such as the n-best list's -1 rows) = absent. mode="weights": p_k
    proportional to exp(-nll_k) (enumerations, n-best lists); "uniform": every valid row weighs
    the same (samples). -> dict of device tensors: logz, entropy, map_prob, exp_acc, exp_tau f32
    [B]; position, before f32 [B][N][N]; map_index, mbr_acc_index, mbr_tau_index int32 [B]; and
    the orders behind the three indices, map_order, mbr_acc_order, mbr_tau_order int64 [B][N]
    (gathered on the device; -1 where a story has no valid candidate). Nothing synchronises."""
    if mode not in N_.POSTERIOR_MODES:
        raise ValueError(f"mode must be 'weights' or 'uniform', got {mode!r}")
    if not (torch.is_tensor(orders) and torch.is_tensor(nll) and orders.is_cuda and nll.is_cuda):
        raise ValueError("order_posterior: orders and nll must be device tensors")
    if orders.dtype != torch.int64 or nll.dtype != torch.float32 or nll.dim() != 2 or \
            orders.dim() not in (2, 3) or orders.shape[-2] != nll.shape[1] or \
            (orders.dim() == 3 and orders.shape[0] != nll.shape[0]):
        raise ValueError("order_posterior: orders int64 [K][N] or [B][K][N] and nll f32 [B][K] "
                         f"expected, got {orders.dtype} {tuple(orders.shape)} and {nll.dtype} "
                         f"{tuple(nll.shape)}")
    B, N = nll.shape[0], orders.shape[-1]
    orders, nll = orders.contiguous(), nll.contiguous()
    out = {name: torch.empty((B,) + (N,) * nn, dtype=dtype, device=nll.device)
           for name, dtype, nn in N_.POSTERIOR_OUTPUTS}
    N_._check_shape(N_.order_posterior(orders, nll, N_.POSTERIOR_MODES[mode], out),
                    "mmseq_order_posterior")
    for name in ("map", "mbr_acc", "mbr_tau"):
        out[name + "_order"] = _gather_orders(orders, out[name + "_index"])
    return out


@torch.no_grad()
def sample_orders_batch(args, model, enc, samples, seed, stream_id=0, return_steps=False):
    """`samples` ancestral samples from the pointer decoder for every story of an encode() tuple
    (mmseq_order_sample) -> (orders int64 [B][S][N], nll f32 [B][S]) on the device, with
    return_steps=True also (u f32 [B][S][N-1], step_nlp f32 [B][S][N-1][N]): the uniforms drawn
    and the rows of -log p sampled from (+inf where pointed). Sample s of story b depends on
    (seed, stream_id, b, s) only: the first S' of S samples are the samples of a call for S'.
    S is split like score_orders_batch's K to keep the workspace within SCORE_WS_CAP. An
    unsupported shape (N > 16) raises _native.Unsupported: there is no host sampler."""
    B, N, H = enc[0].shape
    S = int(samples)
    if S < 1:
        raise ValueError(f"samples must be >= 1, got {samples}")
    dev = enc[0].device
    sc, nbytes = _fit_chunk(lambda s: N_.order_sample_workspace(B, N, H, s), S)
    if nbytes == 0:
        raise N_.Unsupported(f"sample_orders_batch: B={B} N={N} H={H} S={S} is outside "
                             "mmseq_order_sample's limits")
    orders = torch.empty(B, S, N, dtype=torch.int64, device=dev)
    nll = torch.empty(B, S, dtype=torch.float32, device=dev)
    u = steps = None
    if return_steps:
        u = torch.empty(B, S, max(N - 1, 0), dtype=torch.float32, device=dev)
        steps = torch.empty(B, S, max(N - 1, 0), N, dtype=torch.float32, device=dev)
    ins = _decoder_inputs(model, enc)[3]
    for s0, s, whole in K._chunks(S, sc):
        nb = nbytes if s == sc else N_.order_sample_workspace(B, N, H, s)
        ws = K._cached_ws(model, "_score_ws", (B, N, H, s), nb, dev)  # the scorer's layout and cache
        o_c = orders if whole else torch.empty(B, s, N, dtype=torch.int64, device=dev)
        n_c = nll if whole else torch.empty(B, s, dtype=torch.float32, device=dev)
        u_c = st_c = None
        if return_steps:
            u_c = u if whole else torch.empty(B, s, N - 1, dtype=torch.float32, device=dev)
            st_c = steps if whole else torch.empty(B, s, N - 1, N, dtype=torch.float32, device=dev)
        N_._check_shape(N_.order_sample(*ins, seed, stream_id, 0, s0, o_c, n_c, u_c, st_c, ws),
                        "mmseq_order_sample")
        if not whole:
            orders[:, s0:s0 + s] = o_c
            nll[:, s0:s0 + s] = n_c
            if return_steps:
                u[:, s0:s0 + s] = u_c
                steps[:, s0:s0 + s] = st_c
    return (orders, nll, u, steps) if return_steps else (orders, nll)


@torch.no_grad()
def order_posterior_batch(args, model, enc, source="exact", samples=256, seed=0):
    """The posterior over orders of every story of an encode() tuple -> order_posterior's dict
    plus "orders" and "nll", the candidates it was taken over.
    source="exact":  all N! orders (itertools.permutations order) through score_orders_batch;
                     logz is 0 up to rounding. N <= 7; ValueError above.
    source="nbest":  the beam's finished hypotheses (beam_nbest_batch); logz <= 0 is the log of
                     the mass the list covers, and the marginals are those of the list alone.
    source="sample": `samples` ancestral samples (sample_orders_batch, seed), weighted uniformly:
                     the unbiased estimate for N > 7, where the n-best list is a biased sample.
    source="tree":   all N! orders through the prefix tree (enumerate_orders_batch), the same
                     list and dict as "exact". N <= TREE_MAX_N = 9; ValueError above."""
    import itertools
    B, N, _H = enc[0].shape
    if source == "exact":
        if N > EXACT_MAX_N:
            raise ValueError(f"order_posterior_batch enumerates N! orders: N = {N} exceeds "
                             f"{EXACT_MAX_N}")
        orders = torch.tensor(list(itertools.permutations(range(N))), dtype=torch.int64,
                              device=enc[0].device)
        nll = score_orders_batch(args, model, enc, orders)
        mode = "weights"
    elif source == "tree":
        if N > TREE_MAX_N:
            raise ValueError(f"order_posterior_batch(source='tree') enumerates N! orders: N = {N} "
                             f"exceeds {TREE_MAX_N}")
        nll, orders = enumerate_orders_batch(args, model, enc, return_orders=True)
        mode = "weights"
    elif source == "nbest":
        orders, nll, _count = beam_nbest_batch(args, model, enc)
        mode = "weights"
    elif source == "sample":
        orders, nll = sample_orders_batch(args, model, enc, samples, seed)
        mode = "uniform"
    else:
        raise ValueError(f"source must be 'exact', 'nbest', 'sample' or 'tree', got {source!r}")
    post = order_posterior(orders, nll, mode)
    post["orders"], post["nll"] = orders, nll
    return post


def berson_order_posterior(args, model, tokenizer, inputs, source="exact", samples=256, seed=0):
    """The posterior over orders for the B >= 1 stories of `inputs` (same keys as
    berson_pointer_network_batch): one encode, then order_posterior_batch."""
    with torch.no_grad():
        enc = model.encode(**_batch_inputs(model, inputs))
        return order_posterior_batch(args, model, enc, source, samples, seed)


# ------------------------------------------------------------------------------------------------
# Decoding from the pairwise head, joint decode.
PAIRWISE_MAX_N = 12  # 2^12 = 4096 subsets per story (mmseq_pairwise_order)


@torch.no_grad()
def pairwise_weights(cs_mat):
    """cs_mat f32 [B][N][N][2] (enc[7]: the pairwise head's logits for "a before c" at [a][c]) ->
    w f32 [B][N][N], w[a][c] = log_softmax(cs[a][c])[1] + log_softmax(cs[c][a])[0]: the
    log-evidence of both pair views that a precedes c; diagonal 0. For an order o,
    pnll(o) = -sum_{i<j} w[o_i][o_j] is the numerator of the pairwise training loss with the
    labels o implies."""
    if cs_mat.dim() != 4 or cs_mat.shape[1] != cs_mat.shape[2] or cs_mat.shape[3] != 2:
        raise ValueError(f"cs_mat must be [B][N][N][2], got {tuple(cs_mat.shape)}")
    ls = torch.log_softmax(cs_mat.float(), -1)
    w = ls[..., 1] + ls[..., 0].transpose(1, 2)
    eye = torch.eye(cs_mat.shape[1], dtype=torch.bool, device=cs_mat.device)
    return w.masked_fill(eye[None], 0.0).contiguous()


@torch.no_grad()
def pairwise_order_batch(args, model, enc):
    """The pairwise head's own decode for every story of an encode() tuple, exactly, through ONE
    mmseq_pairwise_order (a DP over the 2^N subsets, not over N!) -> dict of device tensors:
    order int64 [B][N] (the arg-min of pnll, ties to the lexicographically smallest), pnll, margin
    (runner-up minus best), logz, entropy f32 [B] and position, before f32 [B][N][N], the exact
    marginals of Q(o) ~ exp(-pnll(o)) (order_posterior_batch's key names where the meanings
    coincide), plus "w", the weights they were taken over. N <= PAIRWISE_MAX_N = 12; ValueError
    above. Nothing synchronises; the workspace is cached on the model like the beam's."""
    w = pairwise_weights(enc[7])
    B, N = int(w.shape[0]), int(w.shape[1])
    if N > PAIRWISE_MAX_N:
        raise ValueError(f"pairwise_order_batch walks all 2^N subsets: N = {N} exceeds "
                         f"{PAIRWISE_MAX_N}")
    dev = w.device
    out = {name: torch.empty((B,) + (N,) * nn, dtype=dtype, device=dev)
           for name, dtype, nn in N_.PAIRWISE_OUTPUTS}
    nbytes = N_.pairwise_order_workspace(B, N)
    if nbytes == 0:
        raise N_.Unsupported(f"pairwise_order_batch: B={B} N={N} is outside "
                             "mmseq_pairwise_order's limits")
    cache = model.__dict__.setdefault("_pairwise_ws", {})
    ws = cache.get((B, N))
    if ws is None:
        ws = cache[(B, N)] = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    N_._check_shape(N_.pairwise_order(w, out, ws), "mmseq_pairwise_order")
    out["w"] = w
    return out


@torch.no_grad()
def pairwise_score_orders(args, model, enc, orders):
    """pnll of K candidate orders under the pairwise head for every story of an encode() tuple
    (mmseq_pairwise_score) -> f32 [B][K] on the device. `orders` as for score_orders_batch: a
    list or CPU tensor is validated here (check_orders); a device tensor is not synchronised on,
    and a candidate in it that is no permutation comes back as +inf. N > 16 raises
    _native.Unsupported."""
    w = pairwise_weights(enc[7])
    B, N = int(w.shape[0]), int(w.shape[1])
    if torch.is_tensor(orders) and orders.is_cuda:
        o = orders
        if o.dtype != torch.int64 or o.dim() not in (2, 3) or o.shape[-1] != N or \
                o.shape[-2] < 1 or (o.dim() == 3 and o.shape[0] != B):
            raise ValueError(f"orders must be int64 [K][{N}] or [{B}][K][{N}] with K >= 1, got "
                             f"{o.dtype} {tuple(o.shape)}")
        o = o.contiguous()
    else:
        o = check_orders(orders, B, N).to(w.device)
    pnll = torch.empty(B, int(o.shape[-2]), dtype=torch.float32, device=w.device)
    N_._check_shape(N_.pairwise_score(w, o, pnll), "mmseq_pairwise_score")
    return pnll


@torch.no_grad()
def joint_order_batch(args, model, enc, lam=None, method="flat"):
    """The order under which the model's own training loss is smallest, for every story of an
    encode() tuple: the arg-min over ALL N! orders (itertools.permutations order, ties to the
    lowest index) of J(o) = nll_ptr(o) / (N - 1) + lam * pnll(o) / (N (N - 1)), what
    `model({**inputs, "labels": o})` would report for that story -> (order int64 [B][N], J f32
    [B], margin f32 [B]) on the device. lam defaults to model.pairwise_loss_lam. The pointer part
    comes from score_orders_batch (method="flat", N <= 7) or enumerate_orders_batch ("tree",
    N <= 9), the pairwise part from pairwise_score_orders on the same list."""
    import itertools
    if method not in ("flat", "tree"):
        raise ValueError(f"method must be 'flat' or 'tree', got {method!r}")
    B, N, _H = enc[0].shape
    lam = float(model.pairwise_loss_lam if lam is None else lam)
    if method == "tree":
        if N > TREE_MAX_N:
            raise ValueError(f"joint_order_batch(method='tree') enumerates N! orders: N = {N} "
                             f"exceeds {TREE_MAX_N}")
        nll, perms = enumerate_orders_batch(args, model, enc, return_orders=True)
    else:
        if N > EXACT_MAX_N:
            raise ValueError(f"joint_order_batch enumerates N! orders: N = {N} exceeds "
                             f"{EXACT_MAX_N}")
        perms = torch.tensor(list(itertools.permutations(range(N))), dtype=torch.int64,
                             device=enc[0].device)
        nll = score_orders_batch(args, model, enc, perms)
    pnll = pairwise_score_orders(args, model, enc, perms)
    J = nll / max(N - 1, 1) + pnll * (lam / max(N * (N - 1), 1))
    idx, best, margin = exact_from_scores(J)
    return perms[idx], best, margin


def topological_order_host(w):
    """The legacy pairwise decode (trainers/eval.py topological_inference), restated for
    comparison: hard decisions, then a depth-first topological sort. w: [N][N] host values (lists,
    numpy or a CPU tensor) -> list of N steps. Edge a -> c where w[a][c] > w[c][a] (from the lower
    to the higher index where they are equal); every vertex's successors in ascending order;
    depth-first from vertex 0, 1, .. with no asserted head, a vertex going to the FRONT of the
    result when its successors are done. On a cyclic tournament the result depends on the
    traversal order alone."""
    w = [[float(x) for x in row] for row in w]
    N = len(w)
    succ = [[] for _ in range(N)]
    for a in range(N):
        for c in range(a + 1, N):
            if w[a][c] >= w[c][a]:
                succ[a].append(c)
            else:
                succ[c].append(a)
    seen, done = [False] * N, []

    def visit(v):
        seen[v] = True
        for u in succ[v]:
            if not seen[u]:
                visit(u)
        done.append(v)

    for v in range(N):
        if not seen[v]:
            visit(v)
    return done[::-1]
