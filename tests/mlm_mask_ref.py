"""numpy restatement of mmseq_mlm_mask (include/mmseq.h, csrc/inputs.hip): the counter-based MLM
masking of the text+image pretraining stage. No torch in the arithmetic; the kernel must reproduce
it bit for bit (tests/test_pretrain_inputs_gpu.py), and its statistics are checked on the CPU
(tests/test_mlm_mask_scheme.py).
"""
import numpy as np

M64 = (1 << 64) - 1
MASK_THR = 52429  # round(0.8 * 2^16)
RAND_THR = 32768


def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key_of(seed, stream_id):
    """(k0, k1) of csrc/common.h make_drop."""
    key = splitmix64((seed & M64) ^ splitmix64(0x5BD1E995 + (stream_id & 0xFFFFFFFF)))
    return key & 0xFFFFFFFF, (key >> 32) | 1


def _u32(x):
    return x & np.uint64(0xFFFFFFFF)


def lowbias32(x):
    """Wellons' lowbias32 on uint64 arrays holding 32-bit values."""
    x = x ^ (x >> np.uint64(16))
    x = _u32(x * np.uint64(0x7FEB352D))
    x = x ^ (x >> np.uint64(15))
    x = _u32(x * np.uint64(0x846CA68B))
    return x ^ (x >> np.uint64(16))


def hash2(h):
    m = _u32(h * np.uint64(0x9E3779B1))
    return m ^ (m >> np.uint64(16))


def threshold(p):
    t = int(np.floor(float(np.float32(p)) * 65536.0 + 0.5))
    return min(max(t, 0), 65536)


def hashes(n, seed, stream_id, rounds=2):
    """(h, h2, h3) of the flat elements 0 .. n-1, uint64 arrays of 32-bit values. rounds=1 is the
    dropout form, kept to show why the masking takes two."""
    k0, k1 = key_of(seed, stream_id)
    e = np.arange(n, dtype=np.uint64)
    lo, hi = _u32(e), e >> np.uint64(32)
    if rounds == 2:
        h = lowbias32(_u32(lowbias32(lo ^ np.uint64(k0)) + (hi ^ np.uint64(k1))))
    else:
        h = lowbias32(_u32((lo ^ np.uint64(k0)) + (hi ^ np.uint64(k1))))
    h2 = hash2(h)
    return h, h2, hash2(h2)


def mlm_mask_ref(ids, pad_id, cls_id, mask_id, vocab, ignore_index, p, seed, stream_id=0, rounds=2,
                 hashed=None):
    """ids int64 [B][L] (or flat) -> (masked ids, labels, selected, replaced, random), the last
    three bool arrays; the input is left unchanged. `hashed`: hashes(ids.size, seed, stream_id)
    when the caller runs several p over one key."""
    ids = np.asarray(ids, np.int64)
    if not (0 <= cls_id + 1 < vocab < (1 << 31)) or ids.size >= (1 << 31):
        raise ValueError("0 <= cls_id + 1 < vocab < 2^31 and B * L < 2^31 required")
    flat = ids.reshape(-1)
    h, h2, h3 = hashed if hashed is not None else hashes(flat.size, seed, stream_id, rounds)
    cand = (flat != pad_id) & (flat != cls_id)
    sel = cand & ((h & np.uint64(0xFFFF)) < np.uint64(threshold(p)))
    rep = sel & ((h >> np.uint64(16)) < np.uint64(MASK_THR))
    rnd = sel & ~rep & ((h2 & np.uint64(0xFFFF)) < np.uint64(RAND_THR))
    words = cls_id + 1 + ((h3 * np.uint64(vocab - cls_id - 1)) >> np.uint64(32)).astype(np.int64)
    out = np.where(rep, np.int64(mask_id), np.where(rnd, words, flat))
    labels = np.where(sel, flat, np.int64(ignore_index))
    s = ids.shape
    return out.reshape(s), labels.reshape(s), sel.reshape(s), rep.reshape(s), rnd.reshape(s)
