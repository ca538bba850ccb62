"""The MLM masking scheme (include/mmseq.h mmseq_mlm_mask) on its numpy restatement alone
(tests/mlm_mask_ref.py), no GPU: rates, the 80 / 10 / 10 split, independence between neighbours at
the strides a [B][L] batch and a 64-lane wave make likely, uniform random words, independence
between keys.

2^22 sequential elements of random non-special ids (vocab 50265, pad 1, cls 0), the 12 keys
(seed s, stream s mod 3), s = 0 .. 11, and p in {0.1, 0.15, 0.8}. Every statistic is a count of
n trials that each succeed with a known probability q, and must lie within 5 standard deviations
sqrt(n q (1 - q)) of n q. The bound is derived, not tuned: about 1100 statistics are taken, and a
sound generator leaves all of them under 5 sigma with probability 1 - 1100 * 5.7e-7 > 0.999; the
scheme is deterministic, so the outcome is fixed. The restatement's worst is 3.3 sigma. With ONE
lowbias32 round (the dropout form) the lag-64 pair statistic reaches 7 sigma, which is why the
masking takes two.
"""
import numpy as np
import pytest

from mlm_mask_ref import MASK_THR, hashes, mlm_mask_ref, threshold

N = 1 << 22
VOCAB, PAD, CLS, MASK, IGNORE = 50265, 1, 0, 50264, -100
KEYS = [(s, s % 3) for s in range(12)]
PS = (0.1, 0.15, 0.8)
LAGS = (1, 2, 3, 4, 8, 60, 64, 120, 128, 300, 4096)
SIGMAS = 5.0


def _ids():
    return np.random.RandomState(2024).randint(2, VOCAB, size=N).astype(np.int64)


def _z(k, n, q):
    return (float(k) - n * q) / np.sqrt(n * q * (1.0 - q))


def test_statistics_within_five_sigma():
    ids = _ids()
    span = VOCAB - CLS - 1
    edges = [(b * span + 15) // 16 for b in range(17)]  # 16 bins over the span words from cls + 1
    worst = ("", 0.0)
    prev = {}
    count = 0

    def check(name, k, n, q):
        nonlocal worst, count
        z = _z(k, n, q)
        count += 1
        if abs(z) > abs(worst[1]):
            worst = (name, z)
        assert abs(z) <= SIGMAS, f"{name}: {k} of {n} at q = {q:.6f} is {z:+.2f} sigma"

    for seed, stream in KEYS:
        hashed = hashes(N, seed, stream)
        for p in PS:
            tag = f"seed {seed} stream {stream} p {p}"
            out, labels, sel, rep, rnd = mlm_mask_ref(ids, PAD, CLS, MASK, VOCAB, IGNORE, p, seed,
                                                      stream, hashed=hashed)
            q = threshold(p) / 65536.0
            qm = MASK_THR / 65536.0
            ns = int(sel.sum())
            # what the flags mean in the outputs
            assert np.array_equal(labels[sel], ids[sel]) and (labels[~sel] == IGNORE).all(), tag
            assert (out[rep] == MASK).all() and np.array_equal(out[~(rep | rnd)], ids[~(rep | rnd)])
            words = out[rnd]
            assert words.min() >= CLS + 1 and words.max() < VOCAB, tag
            check(tag + " selected", ns, N, q)
            check(tag + " replaced | selected", int(rep.sum()), ns, qm)
            check(tag + " random | selected", int(rnd.sum()), ns, (1 - qm) * 0.5)
            check(tag + " selected & replaced", int(rep.sum()), N, q * qm)
            for lag in LAGS:
                check(f"{tag} lag {lag}", int((sel[:-lag] & sel[lag:]).sum()), N - lag, q * q)
            hist = np.histogram(words - (CLS + 1), bins=edges)[0]
            assert hist.sum() == words.size
            for b in range(16):
                check(f"{tag} word bin {b}", int(hist[b]), words.size,
                      (edges[b + 1] - edges[b]) / span)
            if p in prev:  # against the key before: two seeds (and two streams)
                check(tag + " & previous key", int((sel & prev[p]).sum()), N, q * q)
            prev[p] = sel
    print(f"{count} statistics, worst: {worst[0]} at {worst[1]:+.2f} sigma")


def test_specials_never_change_and_extremes():
    rs = np.random.RandomState(7)
    ids = rs.randint(2, VOCAB, size=(64, 300)).astype(np.int64)
    ids[:, ::60] = CLS
    for b in range(64):
        ids[b, 300 - 4 * b:] = PAD  # ragged trailing padding, none in row 0
    special = (ids == PAD) | (ids == CLS)
    for p in (0.0, 0.15, 1.0):
        out, labels, sel, rep, rnd = mlm_mask_ref(ids, PAD, CLS, MASK, VOCAB, IGNORE, p, 3, 1)
        assert np.array_equal(out[special], ids[special]) and (labels[special] == IGNORE).all()
        assert not sel[special].any()
        assert np.array_equal(labels[sel], ids[sel])
        if p == 0.0:
            assert not sel.any() and np.array_equal(out, ids) and (labels == IGNORE).all()
        if p == 1.0:
            assert np.array_equal(sel, ~special)
        if rnd.any():
            assert out[rnd].min() >= CLS + 1 and out[rnd].max() < VOCAB
    # a vocabulary of 7: random words cover exactly [1, 7)
    small = rs.randint(2, 7, size=(8, 4096)).astype(np.int64)
    out, _, _, _, rnd = mlm_mask_ref(small, PAD, CLS, 6, 7, IGNORE, 1.0, 5, 0)
    assert sorted(set(out[rnd].tolist())) == [1, 2, 3, 4, 5, 6]


def test_same_key_same_bits_other_key_other_bits():
    ids = _ids()[:1 << 16]
    a = mlm_mask_ref(ids, PAD, CLS, MASK, VOCAB, IGNORE, 0.15, 9, 0)
    b = mlm_mask_ref(ids, PAD, CLS, MASK, VOCAB, IGNORE, 0.15, 9, 0)
    c = mlm_mask_ref(ids, PAD, CLS, MASK, VOCAB, IGNORE, 0.15, 10, 0)
    d = mlm_mask_ref(ids, PAD, CLS, MASK, VOCAB, IGNORE, 0.15, 9, 1)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(a[2], c[2]) and not np.array_equal(a[2], d[2])


def test_bad_arguments():
    ids = np.full((2, 3), 5, np.int64)
    for cls, vocab in ((0, 1), (6, 7), (-2, 7), (0, 1 << 31)):
        with pytest.raises(ValueError):
            mlm_mask_ref(ids, PAD, cls, MASK, vocab, IGNORE, 0.15, 0)
