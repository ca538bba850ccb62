"""The image-only span rule, pinned without a GPU: imgonly_ref's float64 restatement from the
reference's visn_fc output reproduces the reference's final_seq, cls_score and loss on the two tiny
fixtures (the real-shape fixture keeps visn_fc at a few rows only, so it cannot feed this)."""
import numpy as np
import pytest

from imgonly_ref import head_from_visn_fc, span_positions, span_rows
from imgonly_util import load_imgonly

TINY = ["imgonly_tiny", "imgonly_tiny_g3"]


def _pair(d):
    return {k[6:]: v for k, v in d.items() if k.startswith("pair::")}


@pytest.mark.parametrize("Tv,want", [(33, [15, 32]), (19, [8, 18]), (393, [195, 392])])
def test_span_positions(Tv, want):
    assert span_positions(Tv) == want
    first, second = span_rows(Tv)
    g2 = (Tv - 1) // 2
    assert first == list(range(1, g2)) and second == list(range(g2, 2 * g2 + 1))
    assert g2 in second  # the last patch of image 1 (row g^2) is pooled with image 2


@pytest.mark.parametrize("name", ["imgonly_tiny", "imgonly_tiny_g3", "imgonly_real_config3"])
def test_fixture_records_the_shifted_spans(name):
    meta, d, _ = load_imgonly(name, params=False)
    want = span_positions(meta["Tv"])
    assert (d["i::sep_used"] == np.asarray(want)).all()
    assert (d["pair::sep_positions"] == np.asarray([0, 1])).all()
    assert min(meta["margins"]) > 1e-3
    assert len(meta["nograd"]) == 24


@pytest.mark.parametrize("name", TINY)
def test_restatement_matches_reference(name):
    meta, d, params = load_imgonly(name)
    out = head_from_visn_fc(params, d["i::visn_fc"], _pair(d), meta["config"]["head"]["heads"])
    assert (out["sep"] == d["i::sep_used"]).all()
    np.testing.assert_allclose(out["final_seq"].numpy(), d["i::final_seq"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(out["cls_score"].numpy(), d["i::cls_score"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(float(out["loss"]), float(d["loss"]), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("name", TINY)
def test_unshifted_rule_does_not_match(name):
    """The check has teeth: pooling image 1's last patch with image 1 (the natural split
    [g^2, 2 g^2]) moves final_seq by far more than the tolerance."""
    import imgonly_ref as R
    meta, d, params = load_imgonly(name)
    real = R.span_positions
    R.span_positions = lambda Tv: [(Tv - 1) // 2, Tv - 1]
    try:
        out = head_from_visn_fc(params, d["i::visn_fc"], _pair(d), meta["config"]["head"]["heads"])
    finally:
        R.span_positions = real
    assert np.abs(out["final_seq"].numpy() - d["i::final_seq"]).max() > 1e-3
