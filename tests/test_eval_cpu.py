"""CPU tests of the evaluation report (kws.libs.evaluation.EvalReport): every figure it derives from the integer accumulators of
``kws_eval_update_f32`` against a direct count or the definition, on counts made in NumPy (tests/_eval_ref.py: a float32
softmax of seeded randn x {1, 5, 30} logits, N = 4099); and the loud failure of ``Evaluator`` without a GPU."""
import os
import re

import numpy as np
import pytest

import _eval_ref as ref
from conftest import PKG_ROOT

from kws.libs.evaluation import EvalReport

N = 4099


def problem(C, K, scale, seed=0):
    z, truth = ref.logits_for(1000 * C + K + int(scale) + seed, N, C, scale)
    p = ref.softmax32(z)
    counts, confusion, pos, neg = ref.counts_from(p, z, truth, K)
    loss = -np.log(np.maximum(ref.softmax64(z)[np.arange(N), truth], 1e-300)).sum()
    return z, truth, p, EvalReport(counts, loss, confusion, pos, neg)


def brute_counts(p, truth, c, K):
    """(TP_c(j), FP_c(j)) for j = 0..K by comparing every posterior with every threshold j / K; j = K: nothing is positive."""
    thr = np.arange(K, dtype=np.float64) / K
    above = p[:, c].astype(np.float64)[:, None] >= thr[None, :]
    is_c = (truth == c)[:, None]
    return np.append((above & is_c).sum(axis=0), 0), np.append((above & ~is_c).sum(axis=0), 0)


@pytest.mark.parametrize("scale", [1.0, 5.0, 30.0])
@pytest.mark.parametrize("K", [2, 16, 1024])
@pytest.mark.parametrize("C", [1, 2, 12, 64])
def test_roc_counts_and_curves_equal_brute_force(C, K, scale):
    z, truth, p, rep = problem(C, K, scale)
    assert (rep.n, rep.n_ignored, rep.n_nonfinite, rep.num_classes, rep.n_bins) == (N, 0, 0, C, K)
    assert rep.accuracy == 100.0 * (np.argmax(z, axis=1) == truth).sum() / N
    assert rep.thresholds[0] == np.inf and np.array_equal(rep.thresholds[1:], np.arange(K - 1, -1, -1) / K)
    tps, fps = [], []
    for c in range(C):
        tp, fp = brute_counts(p, truth, c, K)
        assert np.array_equal(rep.tp(c), tp) and np.array_equal(rep.fp(c), fp), c
        tps.append(tp)
        fps.append(fp)
    tps, fps = np.array(tps), np.array(fps)
    degenerate = [c for c in range(C) if tps[c, 0] == 0 or fps[c, 0] == 0]
    assert rep.degenerate_classes == degenerate
    if C == 1:
        assert degenerate == [0]
    # per class: (0, 0) first, (1, 1) last, rates = counts / totals
    curves = []
    for c in range(C):
        fpr, tpr, thr = rep.roc(c)
        assert len(fpr) == len(tpr) == len(thr) == K + 1
        if c in degenerate:
            assert not fpr.any() and not tpr.any()
            want = (np.zeros(K + 1), np.zeros(K + 1))
        else:
            want = (fps[c, ::-1] / fps[c, 0], tps[c, ::-1] / tps[c, 0])
            assert (fpr[0], tpr[0], fpr[-1], tpr[-1]) == (0.0, 0.0, 1.0, 1.0)
        assert np.array_equal(fpr, want[0]) and np.array_equal(tpr, want[1])
        curves.append(want)
    # micro: the ravelled one-hot problem (test.py:41)
    y = (np.arange(C)[None, :] == truth[:, None]).ravel()
    s = p.astype(np.float64).ravel()
    thr = np.arange(K, dtype=np.float64) / K
    at_least = lambda v: np.append(len(v) - np.searchsorted(np.sort(v), thr, side="left"), 0)  # how many of v are >= each threshold
    tp, fp = at_least(s[y]), at_least(s[~y])
    fpr, tpr, _ = rep.roc_micro()
    if C == 1:
        assert not fpr.any() and not tpr.any()
    else:
        assert np.array_equal(fpr, fp[::-1] / fp[0]) and np.array_equal(tpr, tp[::-1] / tp[0])
        j = K // 2
        far, frr = rep.far_frr_at(j / K)
        assert far == fp[j] / fp[0] and frr == 1.0 - tp[j] / tp[0]
        assert rep.far_frr_at(j / K - 0.25 / K) == (far, frr)  # rounded up to the next multiple of 1 / K
        assert rep.far_frr_at(2.0) == (0.0, 1.0) and rep.far_frr_at(0.0) == (1.0, 0.0)
        assert rep.far_micro_mean == np.average(fpr)
    # macro: test.py:44-55 restated on the brute-force curves
    all_fpr = np.unique(np.concatenate([f for f, _ in curves]))
    mean_tpr = np.zeros_like(all_fpr)
    for f, t in curves:
        mean_tpr += np.interp(all_fpr, f, t)
    mean_tpr /= C
    got_fpr, got_tpr, _ = rep.roc_macro()
    assert np.array_equal(got_fpr, all_fpr) and np.allclose(got_tpr, mean_tpr, rtol=0, atol=1e-15)
    assert abs(rep.frr_macro_mean - np.average(1 - mean_tpr)) <= 1e-15
    assert abs(rep.auc(rep.roc_macro()) - np.sum(np.diff(all_fpr) * (mean_tpr[1:] + mean_tpr[:-1]) / 2)) <= 1e-15


def test_precision_recall_f1_follow_the_definitions():
    """C = 12 with a class that is never predicted (5: its logit is far below the others) and a class with no support (3: its
    clips are relabelled): their 0 / 0 give 0, as sklearn's zero_division=0."""
    C, K = 12, 16
    z, truth = ref.logits_for(77, N, C, 5.0)
    z[:, 5] = -1000.0
    truth[truth == 3] = 4
    counts, confusion, pos, neg = ref.counts_from(ref.softmax32(z), z, truth, K)
    rep = EvalReport(counts, 123.5, confusion, pos, neg)
    pred = np.argmax(z, axis=1)
    assert not (pred == 5).any() and (truth == 5).any() and not (truth == 3).any() and (pred == 3).any()
    for c in range(C):
        tp = int(((pred == c) & (truth == c)).sum())
        n_pred, n_true = int((pred == c).sum()), int((truth == c).sum())
        prec = tp / n_pred if n_pred else 0.0
        rec = tp / n_true if n_true else 0.0
        f1 = 2 * prec * rec / (prec + rec) if prec + rec else 0.0
        assert rep.precision[c] == prec and rep.recall[c] == rec and abs(rep.f1[c] - f1) <= 1e-15 and rep.support[c] == n_true
    assert rep.precision[5] == 0.0 and rep.f1[5] == 0.0 and rep.recall[3] == 0.0 and rep.f1[3] == 0.0 and rep.support[3] == 0
    assert rep.loss == 123.5 / N and rep.n_correct == int((pred == truth).sum())
    assert 3 in rep.degenerate_classes and 5 not in rep.degenerate_classes
    assert not rep.roc(3)[0].any() and not rep.roc(3)[1].any()
    text = rep.format()
    lines = text.splitlines()
    assert lines[0].split() == ["precision", "recall", "f1-score", "support"]
    assert len([ln for ln in lines if ln.strip()]) == 1 + C + 3
    row7 = lines[2 + 7].split()
    assert row7 == ["7", f"{rep.precision[7]:.2f}", f"{rep.recall[7]:.2f}", f"{rep.f1[7]:.2f}", str(rep.support[7])]
    assert lines[-3].split() == ["accuracy", f"{rep.accuracy / 100:.2f}", str(N)]
    assert lines[-2].split()[:2] == ["macro", "avg"] and lines[-1].split()[:2] == ["weighted", "avg"]
    named = EvalReport(counts, 0.0, confusion, pos, neg, words=[f"w{c}" for c in range(C)]).format()
    assert named.splitlines()[2].split()[0] == "w0"


def test_auc_of_a_perfect_and_of_a_chance_classifier():
    K = 16
    # perfect: the true class's logit is 30 above the others
    _, truth = ref.logits_for(5, N, 12, 1.0)
    z = np.where(np.arange(12)[None, :] == truth[:, None], 30.0, 0.0).astype(np.float32)
    rep = EvalReport(*_with_loss(ref.counts_from(ref.softmax32(z), z, truth, K)))
    assert rep.accuracy == 100.0
    for curve in [rep.roc(c) for c in range(12)] + [rep.roc_micro(), rep.roc_macro()]:
        assert abs(rep.auc(curve) - 1.0) <= 1.0 / K
    assert rep.far_frr_at(0.5) == (0.0, 0.0)
    # chance: every score vector occurs once with each label, so positives and negatives of a class are distributed alike
    z2, _ = ref.logits_for(6, N, 2, 5.0)
    z2 = np.concatenate([z2, z2])
    t2 = np.concatenate([np.zeros(N, np.int32), np.ones(N, np.int32)])
    rep = EvalReport(*_with_loss(ref.counts_from(ref.softmax32(z2), z2, t2, K)))
    for curve in (rep.roc(0), rep.roc(1), rep.roc_micro(), rep.roc_macro()):
        assert abs(rep.auc(curve) - 0.5) <= 1.0 / K


def _with_loss(c):
    return c[0], 0.0, c[1], c[2], c[3]


def test_report_without_histograms_and_with_skipped_rows():
    z, truth = ref.logits_for(9, 300, 4, 5.0)
    truth[:7] = [-1, 4, -100, np.iinfo(np.int32).min, 0, 1, 2]
    z[10, 2] = np.nan
    z[11, 0] = np.inf
    z[0, 0] = np.nan  # an ignored row stays ignored
    counts, confusion, pos, neg = ref.counts_from(ref.softmax32(z), z, truth, 0)
    assert list(counts[[0, 2, 3]]) == [294, 4, 2] and confusion.sum() == 294
    from kws.common.errors import KWSError

    for rep in (EvalReport(counts, 1.0, confusion), EvalReport(counts, 1.0, confusion, pos, neg)):
        assert (rep.n, rep.n_ignored, rep.n_nonfinite, rep.n_bins) == (294, 4, 2, 0)
        with pytest.raises(KWSError, match="n_bins = 0"):
            rep.roc(0)
    empty = EvalReport(np.zeros(4), 0.0, np.zeros((3, 3)), np.zeros((3, 2)), np.zeros((3, 2)))
    assert (empty.loss, empty.accuracy) == (0.0, 0.0) and empty.degenerate_classes == [0, 1, 2] and not empty.f1.any()
    with pytest.raises(KWSError):
        EvalReport(counts, 1.0, confusion[:, :3])


def test_evaluator_without_a_gpu_fails_loudly():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from kws.common.errors import KWSError
    from kws.libs.evaluation import Evaluator

    with pytest.raises(KWSError, match="no CPU fallback"):
        Evaluator(12)


def test_the_bindings_follow_the_header():
    from kws import _native

    C = _native.C
    assert _native.SIGNATURES["kws_eval_update_f32"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p,
                                                                   C.c_void_p])
    assert _native.SIGNATURES["kws_eval_read"][1][2] == C.POINTER(C.c_double)
    for name in ("kws_eval_open", "kws_eval_reset", "kws_eval_close", "kws_eval_update_f32", "kws_eval_read"):
        assert hasattr(_native.lib(), name)
    for method in ("eval_open", "eval_reset", "eval_close", "eval_update_f32", "eval_read"):
        assert callable(getattr(_native.Context, method))


def test_evaluation_never_imports_the_oracle():
    src = open(os.path.join(PKG_ROOT, "kws", "libs", "evaluation.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M)
    assert "oracle" not in src
