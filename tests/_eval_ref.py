"""What the evaluation tests share (tests/test_eval_cpu.py, tests/test_eval_gpu.py): the NumPy restatement of
``kws_eval_update_f32``'s counting given the posteriors, a float32 restatement of the softmax, float64 references."""
import numpy as np


def logits_for(seed, B, C, scale):
    """Seeded ``randn * scale`` float32 [B, C] and uniform truth labels int32 [B]."""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((B, C)) * scale).astype(np.float32)
    return z, rng.integers(0, C, B).astype(np.int32)


def softmax32(z):
    """The kernel's softmax in float32 NumPy: maximum, expf(z - m), the sum in index order, one reciprocal, one product."""
    z = np.asarray(z, dtype=np.float32)
    m = z.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):  # rows with a NaN or infinite logit: the callers leave them out
        e = np.exp(z - m, dtype=np.float32)
    s = np.zeros(len(z), np.float32)
    for i in range(z.shape[1]):
        s = (s + e[:, i]).astype(np.float32)
    inv = (np.float32(1.0) / s).astype(np.float32)
    return (e * inv[:, None]).astype(np.float32)


def softmax64(z):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def row_kinds(z, truth, C):
    """(used, ignored, nonfinite) row masks: the label is checked first, then the logits."""
    truth = np.asarray(truth, dtype=np.int64)
    ignored = (truth < 0) | (truth >= C)
    nonfinite = ~ignored & ~np.isfinite(z).all(axis=1)
    return ~ignored & ~nonfinite, ignored, nonfinite


def bins_of(p, K):
    """min(K - 1, int(p * K)) of float32 posteriors; the product is exact for a power of two."""
    x = (np.asarray(p, dtype=np.float32) * np.float32(K)).astype(np.float32)
    return np.minimum(K - 1, x.astype(np.int64))


def counts_from(p, z, truth, K):
    """``kws_eval_update_f32`` restated given the posteriors ``p`` float32 [B, C] of the logits ``z``: (counts int64[4],
    confusion [C, C], hist_pos [C, K], hist_neg [C, K]); the prediction is the first argmax of the logits."""
    z = np.asarray(z, dtype=np.float32)
    B, C = z.shape
    used, ignored, nonfinite = row_kinds(z, truth, C)
    t = np.asarray(truth, dtype=np.int64)[used]
    pred = np.argmax(z[used], axis=1) if used.any() else np.zeros(0, np.int64)
    confusion = np.zeros((C, C), np.int64)
    np.add.at(confusion, (t, pred), 1)
    pos, neg = np.zeros((C, max(K, 0)), np.int64), np.zeros((C, max(K, 0)), np.int64)
    if K > 0 and used.any():
        bins = bins_of(np.asarray(p)[used], K)
        cls = np.broadcast_to(np.arange(C), bins.shape)
        hit = cls == t[:, None]
        np.add.at(pos, (cls[hit], bins[hit]), 1)
        np.add.at(neg, (cls[~hit], bins[~hit]), 1)
    counts = np.array([used.sum(), (pred == t).sum(), ignored.sum(), nonfinite.sum()], np.int64)
    return counts, confusion, pos, neg
