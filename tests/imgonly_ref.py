"""float64 restatement of the image-only (multimodal_img_part) ordering head, from the visn_fc
output to the loss — TEST INFRASTRUCTURE ONLY.

The reference in this mode (models/berson/modeling_bert.py:1284-1293, 1316-1328) takes
top_vec = visn_feats [P][Tv][H] with Tv = 1 + 2 g^2, cls_pooled = visn_feats[:, 0] (the class-token
row), and shifts the pair's sep_positions [0, 1] by [Tv // 2 - 1, Tv - 2] to [g^2 - 1, 2 g^2]. With
HierarchicalAttention's masks (:711-712) span 1 is rows 1 .. g^2 - 1 and span 2 rows g^2 .. 2 g^2:
the last patch of the first image is pooled with the second image. `span_positions` states that
rule; everything after it is the shared head, taken from the CPU oracle's pieces in float64.
"""
import numpy as np
import torch

from oracle import berson_oracle as O


def span_positions(Tv):
    """Tv = 1 + 2 g^2 -> the two span ends [g^2 - 1, 2 g^2] HierarchicalAttention pools up to."""
    g2 = (Tv - 1) // 2
    assert Tv == 1 + 2 * g2
    return [g2 - 1, 2 * g2]


def span_rows(Tv):
    """The rows of the two spans under masks :711-712, as lists (for the tests' statements)."""
    s0, s1 = span_positions(Tv)
    return list(range(1, s0 + 1)), list(range(s0 + 1, s1 + 1))


def head_from_visn_fc(params, visn_fc, pair, inter_heads, lam=0.6):
    """params: reference state dict (any float dtype), visn_fc [P][Tv][H], pair: the pair::*
    tensors of prepare_berson_inputs(img_part=True) -> dict(sep, final_seq, cls_score,
    para_matrix, original_key, loss) in float64."""
    p = {k: (v.double() if v.is_floating_point() else v) for k, v in params.items()}
    top = torch.as_tensor(np.asarray(visn_fc)).double()
    P, Tv, H = top.shape
    B, npair = pair["pairs_list"].shape[:2]
    N = pair["mask_cls"].shape[1]
    assert P == B * npair
    sep = np.broadcast_to(np.asarray(span_positions(Tv), np.int64), (B, npair, 2))
    before = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        final, cls_mat, cls_score, cs_mat = O.hierarchical_attention(
            p, top, top[:, 0], np.asarray(pair["pairs_list"]), sep, N)
        mask_cls = torch.as_tensor(pair["mask_cls"])
        clean = final * mask_cls[:, :, None].double()
        para = O.inter_encoder(p, clean, mask_cls, inter_heads) * mask_cls[:, :, None]
        plen = torch.as_tensor(pair["passage_length"]).double()
        para_vec = para.sum(1) / (plen + 1e-20)[:, None]
        okey = O.linear(torch.cat([clean, para], -1), p, "key_linear")
        enc = dict(clean=clean, para=para, hcn=(para_vec, torch.zeros_like(para_vec)), okey=okey,
                   cls_mat=cls_mat, cls_score=cls_score, cs_mat=cs_mat)
        loss, _logp = O.pointer_forward(p, enc, pair, lam)
    finally:
        torch.set_default_dtype(before)
    return dict(sep=sep, final_seq=final, cls_score=cls_score, para_matrix=para,
                original_key=okey, loss=loss)
