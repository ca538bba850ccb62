"""The halving search behind every chunked decoder call (berson._fit_chunk): the counts it visits
and what it returns, pinned with a fake size function. No GPU and no library call."""
from multimodal_sequencing_amd import berson


def _search(size_fn, n, **kw):
    seen = []

    def size(k):
        seen.append(k)
        return size_fn(k)

    return berson._fit_chunk(size, n, **kw), seen


def test_halves_until_the_workspace_fits():
    got, seen = _search(lambda k: 10 * k, 24, cap=35)
    assert got == (3, 30)
    assert seen == [24, 12, 6, 3]


def test_a_single_candidate_is_always_tried():
    got, seen = _search(lambda k: 10 * k, 24, cap=5)
    assert got == (1, 10)
    assert seen == [24, 12, 6, 3, 2, 1]


def test_unsupported_shape_reports_zero_bytes():
    assert _search(lambda k: 0, 24, cap=35)[0] == (1, 0)


def test_whole_list_in_one_call_where_it_fits():
    got, seen = _search(lambda k: 10 * k, 24, cap=240)
    assert got == (24, 240)
    assert seen == [24]


def test_floor_above_one():
    got, seen = _search(lambda k: 10 * k, 60, low=6, cap=100)
    assert got == (8, 80)
    assert seen == [60, 30, 15, 8]


def test_floor_is_taken_whatever_it_needs():
    got, seen = _search(lambda k: 10 * k, 60, low=6, cap=10)
    assert got == (6, 60)
    assert seen == [60, 30, 15, 8, 6]


def test_default_cap_is_read_at_call_time(monkeypatch):
    assert berson._fit_chunk(lambda k: 10 * k, 24) == (24, 240)
    monkeypatch.setattr(berson, "SCORE_WS_CAP", 35)
    assert berson._fit_chunk(lambda k: 10 * k, 24) == (3, 30)
