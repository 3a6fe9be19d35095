"""Evaluation on the device: loss, accuracy, confusion matrix and ROC counts with one read-back.

The reference's loops leave the device twice per batch -- ``running_loss += loss.item()``, ``torch.max(outputs, 1)`` and
``(predicted == labels).sum().item()`` in ``train.py:51-54`` / ``kws/libs/training.py:300-303`` after every training step and
in ``Trainer.evaluate`` (``train.py:79-98``) / ``KWSTrainer.validate`` (``training.py:347-393``) per validation batch -- and
``test.py:27-58`` computes the per-class report, the one-vs-rest ROC curves, their micro and macro averages and the false-alarm /
false-reject figures with sklearn from posteriors copied to the host.

Here ``Evaluator.update(logits, labels)`` enqueues ``kws_eval_update_f32`` on torch's current stream: integer accumulators in
device memory take the batch (and the call optionally returns the cross-entropy gradient, so a training step has its loss and
accuracy without a synchronisation); ``Evaluator.report()`` synchronises once and returns an ``EvalReport``, plain NumPy, which
derives every figure from the counts.  ``evaluate(model, loader)`` is the validation pass around it.

Recordings are judged at the event level: ``KeywordSpotter.score`` scores a scan against annotations over a threshold sweep on the
device (``kws_scan_score_f32``) and returns a ``DetectionReport`` -- false alarms per hour against miss rate per threshold;
``truth_windows`` turns annotations in seconds into the window ranges it takes.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from kws.common.errors import ModelError

Curve = Tuple[np.ndarray, np.ndarray, np.ndarray]


def _ratio(num, den):
    """num / den elementwise in float64, 0 where den is 0 (sklearn's ``zero_division=0``)."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    return np.divide(num, den, out=np.zeros(np.broadcast(num, den).shape, dtype=np.float64), where=den != 0)


class EvalReport:
    """What ``kws_eval_read`` returns, and every metric derived from it.  Plain NumPy: it is built from the raw arrays.

    ``counts`` = (rows used, rows correct, rows ignored, rows non-finite), ``loss_sum`` = float64 sum of the used rows'
    cross-entropy, ``confusion`` [C, C] (row = truth, column = prediction), ``hist_pos`` / ``hist_neg`` [C, K]: how many clips
    whose truth is / is not class c had ``min(K - 1, int(p[c] * K))`` equal to the bin (``None`` or K = 0: no ROC).

    ``n``, ``n_correct``, ``n_ignored`` (label outside [0, C)), ``n_nonfinite`` (a NaN or infinite logit);
    ``loss``: the mean cross-entropy over the ``n`` clips used.  The reference averages the BATCH means
    (``running_loss / len(loader)``, ``train.py:96``, ``training.py:383``), which weights a short last batch's clips more; the
    two agree when every batch has the same size.
    ``accuracy``: in per cent, as the reference prints it (``100 * correct / total``).
    ``precision``, ``recall``, ``f1``, ``support``: per class from the confusion matrix, 0 where the denominator is 0.

    ROC.  At threshold index j = 0..K a clip is positive for class c when its bin is >= j: for j <= K - 1 that is
    ``p[c] >= j / K`` exactly, j = K is the (0, 0) end.  ``tp(c)[j]`` / ``fp(c)[j]`` are those counts.  The curves have K + 1
    points where sklearn's ``roc_curve`` has one per distinct score, so ``frr_macro_mean`` / ``far_micro_mean`` -- means over
    the points of a curve, as ``test.py:57-58`` prints them -- are the reference's figures on this grid, not its numbers.
    A class without positives or without negatives has no curve: its rates are zeros and it is listed in
    ``degenerate_classes``; like the reference's ``/ num_class`` the macro average divides by C all the same.
    """

    def __init__(self, counts, loss_sum: float, confusion, hist_pos=None, hist_neg=None, words: Optional[Sequence[str]] = None):
        counts = np.asarray(counts).astype(np.int64).reshape(4)
        self.confusion = np.asarray(confusion).astype(np.int64)
        if self.confusion.ndim != 2 or self.confusion.shape[0] != self.confusion.shape[1] or self.confusion.shape[0] < 1:
            raise ModelError("EvalReport: confusion must be a square matrix [C, C]")
        self.num_classes = int(self.confusion.shape[0])
        self.n, self.n_correct, self.n_ignored, self.n_nonfinite = (int(v) for v in counts)
        self.loss_sum = float(loss_sum)
        self.loss = self.loss_sum / self.n if self.n else 0.0
        self.accuracy = 100.0 * self.n_correct / self.n if self.n else 0.0
        if (hist_pos is None) != (hist_neg is None):
            raise ModelError("EvalReport: hist_pos and hist_neg come together")
        if hist_pos is not None and np.asarray(hist_pos).size:
            self.hist_pos = np.asarray(hist_pos).astype(np.int64)
            self.hist_neg = np.asarray(hist_neg).astype(np.int64)
            if self.hist_pos.shape != self.hist_neg.shape or self.hist_pos.ndim != 2 or self.hist_pos.shape[0] != self.num_classes:
                raise ModelError("EvalReport: hist_pos and hist_neg must both be [C, K]")
            self.n_bins = int(self.hist_pos.shape[1])
        else:
            self.hist_pos = self.hist_neg = None
            self.n_bins = 0
        self.words = list(words) if words is not None else [str(c) for c in range(self.num_classes)]
        if len(self.words) != self.num_classes:
            raise ModelError("EvalReport: one word per class is required")

    # -- the classification report --------------------------------------------------------------------------------------
    @property
    def support(self) -> np.ndarray:
        return self.confusion.sum(axis=1)

    @property
    def precision(self) -> np.ndarray:
        return _ratio(np.diag(self.confusion), self.confusion.sum(axis=0))

    @property
    def recall(self) -> np.ndarray:
        return _ratio(np.diag(self.confusion), self.confusion.sum(axis=1))

    @property
    def f1(self) -> np.ndarray:
        p, r = self.precision, self.recall
        return _ratio(2.0 * p * r, p + r)

    def format(self, digits: int = 2) -> str:
        """A text table in the manner of sklearn's ``classification_report`` (``test.py:27``): one row per class, then the
        accuracy and the macro and support-weighted averages."""
        p, r, f, s = self.precision, self.recall, self.f1, self.support
        width = max([len(w) for w in self.words] + [len("weighted avg")])
        head = f"{'':>{width}} " + " ".join(f"{h:>9}" for h in ("precision", "recall", "f1-score", "support"))
        row = lambda name, a, b, c, n: f"{name:>{width}} " + " ".join(f"{v:>9.{digits}f}" for v in (a, b, c)) + f" {n:>9d}"
        lines = [head, ""]
        lines += [row(self.words[c], p[c], r[c], f[c], int(s[c])) for c in range(self.num_classes)]
        total = int(s.sum())
        lines += ["", f"{'accuracy':>{width}} " + " " * 20 + f"{self.accuracy / 100.0:>9.{digits}f} {total:>9d}"]
        lines.append(row("macro avg", p.mean(), r.mean(), f.mean(), total))
        w = _ratio(s, total)
        lines.append(row("weighted avg", float((p * w).sum()), float((r * w).sum()), float((f * w).sum()), total))
        return "\n".join(lines) + "\n"

    # -- ROC from the histograms ----------------------------------------------------------------------------------------
    def _need_bins(self) -> None:
        if not self.n_bins:
            raise ModelError("EvalReport: no posterior histograms were collected (n_bins = 0)")

    @staticmethod
    def _at_least(hist: np.ndarray) -> np.ndarray:
        """[..., K] bin counts -> [..., K + 1]: entry j = the count in bins >= j."""
        tail = np.cumsum(hist[..., ::-1], axis=-1)[..., ::-1]
        return np.concatenate([tail, np.zeros(hist.shape[:-1] + (1,), dtype=hist.dtype)], axis=-1)

    def tp(self, c: int) -> np.ndarray:
        """``TP_c(j)`` for j = 0..K: clips of class c with ``p[c] >= j / K``."""
        self._need_bins()
        return self._at_least(self.hist_pos[c])

    def fp(self, c: int) -> np.ndarray:
        """``FP_c(j)`` for j = 0..K: clips of another class with ``p[c] >= j / K``."""
        self._need_bins()
        return self._at_least(self.hist_neg[c])

    @property
    def thresholds(self) -> np.ndarray:
        """The thresholds of every curve, from the (0, 0) end: inf (j = K), then (K - 1) / K down to 0."""
        self._need_bins()
        K = self.n_bins
        return np.concatenate([[np.inf], np.arange(K - 1, -1, -1, dtype=np.float64) / K])

    @property
    def degenerate_classes(self) -> List[int]:
        """Classes without positives or without negatives among the clips used: they have no ROC curve."""
        self._need_bins()
        return [c for c in range(self.num_classes) if self.hist_pos[c].sum() == 0 or self.hist_neg[c].sum() == 0]

    def _curve(self, tp: np.ndarray, fp: np.ndarray) -> Curve:
        P, N = int(tp[0]), int(fp[0])
        if P == 0 or N == 0:
            return np.zeros(len(tp)), np.zeros(len(tp)), self.thresholds
        return fp[::-1] / float(N), tp[::-1] / float(P), self.thresholds

    def roc(self, c: int) -> Curve:
        """(fpr, tpr, thresholds) of class c against the rest, K + 1 points from (0, 0) to (1, 1) as ``roc_curve`` orders
        them (``test.py:38``)."""
        return self._curve(self.tp(c), self.fp(c))

    def roc_micro(self) -> Curve:
        """The curve of the ravelled one-hot problem (``test.py:41``): TP, FP, P and N summed over the classes."""
        self._need_bins()
        return self._curve(self._at_least(self.hist_pos.sum(axis=0)), self._at_least(self.hist_neg.sum(axis=0)))

    def roc_macro(self) -> Curve:
        """``test.py:44-55``: the union of the classes' fpr values, every class's tpr interpolated there, their mean.  The
        third entry is ``None``: the points of the union belong to no single threshold."""
        curves = [self.roc(c) for c in range(self.num_classes)]
        all_fpr = np.unique(np.concatenate([f for f, _, _ in curves]))
        mean_tpr = np.zeros_like(all_fpr)
        for f, t, _ in curves:
            mean_tpr += np.interp(all_fpr, f, t)
        return all_fpr, mean_tpr / self.num_classes, None

    @staticmethod
    def auc(curve) -> float:
        """Area under (fpr, tpr) by trapezoids (sklearn's ``auc``, ``test.py:39``)."""
        x, y = np.asarray(curve[0], dtype=np.float64), np.asarray(curve[1], dtype=np.float64)
        return float(np.sum(np.diff(x) * (y[1:] + y[:-1]) * 0.5))

    def far_frr_at(self, threshold: float) -> Tuple[float, float]:
        """(false-alarm rate, false-reject rate), micro-averaged, when a class fires at ``p >= threshold``.  The histograms
        resolve multiples of 1 / K: the threshold is rounded up to the next one (above (K - 1) / K nothing fires)."""
        self._need_bins()
        K = self.n_bins
        j = int(min(K, max(0, np.ceil(float(threshold) * K))))
        tp, fp = self._at_least(self.hist_pos.sum(axis=0)), self._at_least(self.hist_neg.sum(axis=0))
        far = float(_ratio(fp[j], fp[0]))
        frr = 1.0 - float(_ratio(tp[j], tp[0])) if tp[0] else 0.0
        return far, frr

    @property
    def frr_macro_mean(self) -> float:
        """``np.average(1 - tpr["macro"])`` (``test.py:57``)."""
        return float(np.mean(1.0 - self.roc_macro()[1]))

    @property
    def far_micro_mean(self) -> float:
        """``np.average(fpr["micro"])`` (``test.py:58``)."""
        return float(np.mean(self.roc_micro()[0]))


def truth_windows(truth, end_s, tolerance_s: float = 1.0, words: Optional[Sequence[str]] = None, num_classes: Optional[int] = None,
                  recording: int = 0):
    """Annotations in seconds -> rows of the table ``kws_scan_score_f32`` takes, for ONE recording.

    ``truth``: a sequence of ``(word_or_index, t0, t1)``, a keyword spoken from ``t0`` to ``t1`` seconds; a word is looked up in
    ``words``.  ``end_s``: the end time of every window of the recording, ascending (``scan_window_times``) -- the time
    ``ScanResult.events`` reports for an event.  A truth maps to the windows whose end time lies in ``[t0, t1 + tolerance_s]``.
    The default ``tolerance_s = 1.0`` is one window length: a detector that fires once the whole word is inside its window fires
    up to a window after the word began, and an API choice, not a measured figure.

    Returns ``(rows int32 [N, 4], n_truth int64 [C], undetectable int64 [C])``, rows ``(recording, label, first_window,
    last_window)``.  A truth whose range holds no window (before the first window ends, after the last) is *undetectable*: it
    is counted in ``n_truth`` and in ``undetectable`` and left out of the rows.  Where two ranges of one label would overlap,
    the earlier one ends one window before the later one begins (and is undetectable if nothing is left of it)."""
    C = int(num_classes) if num_classes is not None else (len(words) if words is not None else None)
    if C is None:
        raise ModelError("truth_windows: give words or num_classes")
    end_s = np.asarray(end_s, dtype=np.float64).reshape(-1)
    n_truth, undetectable = np.zeros(C, np.int64), np.zeros(C, np.int64)
    ranges: dict = {}
    for item in truth:
        k, t0, t1 = item
        if isinstance(k, str):
            if words is None or k not in list(words):
                raise ModelError(f"truth_windows: {k!r} is not one of the model's words")
            k = list(words).index(k)
        k = int(k)
        if not 0 <= k < C or not float(t0) <= float(t1):
            raise ModelError(f"truth_windows: {item!r} needs a label in [0, {C}) and t0 <= t1")
        n_truth[k] += 1
        first = int(np.searchsorted(end_s, float(t0), "left"))
        last = int(np.searchsorted(end_s, float(t1) + float(tolerance_s), "right")) - 1
        if first > last:
            undetectable[k] += 1
        else:
            ranges.setdefault(k, []).append([first, last])
    rows = []
    for k in sorted(ranges):
        lst = sorted(ranges[k])
        for i, (first, last) in enumerate(lst):
            if i + 1 < len(lst):
                last = min(last, lst[i + 1][0] - 1)
            if first > last:
                undetectable[k] += 1
            else:
                rows.append((int(recording), k, first, last))
    return np.asarray(rows, np.int32).reshape(-1, 4), n_truth, undetectable


class DetectionReport:
    """Event-level detection figures over a threshold sweep, from the counters of ``kws_scan_score_f32``.  Plain NumPy.

    ``counts`` int64 [K, C, 4] = per threshold and class the hits, false alarms, duplicates and the hits' latency sum in windows;
    ``n_truth`` [C]: the annotations per class, the ``undetectable`` [C] among them included (they can only be missed);
    ``thresholds`` [K]; ``hours``: the audio scanned; ``hop_s``: seconds between two windows; ``words``: one per class.
    Reports of the same sweep over different audio add (``a + b``): the library does not accumulate across calls.

    With ``c=None`` a figure is over all classes together (sums, then the ratio), else of class ``c``; each is an array [K].
    A ratio with a zero denominator is 0."""

    def __init__(self, counts, n_truth, undetectable, thresholds, hours: float, hop_s: float, words: Optional[Sequence[str]] = None):
        self.counts = np.asarray(counts).astype(np.int64)
        if self.counts.ndim != 3 or self.counts.shape[2] != 4:
            raise ModelError("DetectionReport: counts must be [K, C, 4]")
        K, C = self.counts.shape[:2]
        self.n_truth = np.asarray(n_truth).astype(np.int64).reshape(-1)
        self.undetectable = np.asarray(undetectable).astype(np.int64).reshape(-1)
        self.thresholds = np.asarray(thresholds, dtype=np.float32).reshape(-1)
        if self.n_truth.shape != (C,) or self.undetectable.shape != (C,) or self.thresholds.shape != (K,):
            raise ModelError("DetectionReport: n_truth and undetectable must be [C], thresholds [K]")
        self.hours, self.hop_s = float(hours), float(hop_s)
        self.words = list(words) if words is not None else [str(c) for c in range(C)]
        if len(self.words) != C:
            raise ModelError("DetectionReport: one word per class is required")

    def __add__(self, other: "DetectionReport") -> "DetectionReport":
        if self.counts.shape != other.counts.shape or not np.array_equal(self.thresholds, other.thresholds, equal_nan=True) \
                or self.hop_s != other.hop_s:
            raise ModelError("DetectionReport: only reports of the same thresholds, classes and hop add")
        return DetectionReport(self.counts + other.counts, self.n_truth + other.n_truth, self.undetectable + other.undetectable,
                               self.thresholds, self.hours + other.hours, self.hop_s, self.words)

    @property
    def hits(self) -> np.ndarray:
        return self.counts[:, :, 0]

    @property
    def false_alarms(self) -> np.ndarray:
        return self.counts[:, :, 1]

    @property
    def duplicates(self) -> np.ndarray:
        return self.counts[:, :, 2]

    @property
    def misses(self) -> np.ndarray:
        """[K, C]: the annotations no event hit, the undetectable ones among them."""
        return self.n_truth[None, :] - self.hits

    def _of(self, a: np.ndarray, c) -> np.ndarray:
        return a.sum(axis=-1) if c is None else a[..., int(c)]

    def miss_rate(self, c=None) -> np.ndarray:
        return _ratio(self._of(self.misses, c), self._of(self.n_truth, c))

    def false_alarms_per_hour(self, c=None) -> np.ndarray:
        return _ratio(self._of(self.false_alarms, c), self.hours)

    def mean_latency_s(self, c=None) -> np.ndarray:
        """The mean, over the hits, of the time from the annotation's first window to the window that hit it."""
        return _ratio(self._of(self.counts[:, :, 3], c), self._of(self.hits, c)) * self.hop_s

    def det_curve(self, c=None) -> Curve:
        """(false alarms per hour, miss rate, thresholds), by ascending threshold (a NaN threshold last)."""
        order = np.argsort(self.thresholds, kind="stable")
        return self.false_alarms_per_hour(c)[order], self.miss_rate(c)[order], self.thresholds[order]

    def threshold_for(self, max_false_alarms_per_hour: float, c=None) -> Optional[float]:
        """The threshold with the lowest miss rate among those with at most ``max_false_alarms_per_hour``; of several, the one
        with the fewest false alarms, then the highest.  ``None`` when no threshold of the sweep meets the bound."""
        fa, mr = self.false_alarms_per_hour(c), self.miss_rate(c)
        ok = [i for i in range(len(self.thresholds)) if fa[i] <= float(max_false_alarms_per_hour) and not np.isnan(self.thresholds[i])]
        if not ok:
            return None
        return float(self.thresholds[min(ok, key=lambda i: (mr[i], fa[i], -self.thresholds[i]))])

    def format(self, digits: int = 3) -> str:
        """A text table, one row per threshold in ascending order, over all classes together."""
        head = " ".join(f"{h:>10}" for h in ("threshold", "hits", "misses", "false_al", "dupl", "miss_rate", "fa_per_h", "latency_s"))
        lines = [f"{int(self.n_truth.sum())} annotations ({int(self.undetectable.sum())} undetectable), {self.hours:.{digits}f} h", head]
        mr, fa, lat = self.miss_rate(), self.false_alarms_per_hour(), self.mean_latency_s()
        for i in np.argsort(self.thresholds, kind="stable"):
            lines.append(f"{self.thresholds[i]:>10.{digits}f} {int(self.hits[i].sum()):>10d} {int(self.misses[i].sum()):>10d} "
                         f"{int(self.false_alarms[i].sum()):>10d} {int(self.duplicates[i].sum()):>10d} {mr[i]:>10.{digits}f} "
                         f"{fa[i]:>10.{digits}f} {lat[i]:>10.{digits}f}")
        return "\n".join(lines) + "\n"


class Evaluator:
    """Accumulates the evaluation statistics of any number of batches on the device (``kws_eval_*``).

    Owns a native context bound to torch's current stream at every call.  ``update`` makes no host synchronisation;
    ``report`` makes the one.  Without a GPU the constructor raises (``KWSError`` tree): there is no CPU fallback."""

    def __init__(self, num_classes: int, n_bins: int = 256, device: int = 0, words: Optional[Sequence[str]] = None):
        from kws import _native

        self.num_classes, self.n_bins, self.words = int(num_classes), int(n_bins), words
        if words is not None and len(words) != self.num_classes:
            raise ModelError("Evaluator: one word per class is required")
        self._ctx = _native.Context(int(device), ModelError)
        self._ctx.use_torch_stream()
        self._ctx.eval_open(self.num_classes, self.n_bins)

    def update(self, logits, labels, grad_scale: Optional[float] = None):
        """One batch: ``logits`` float32 [B, C] and ``labels`` [B] (int64 as the loaders yield, cast to int32 on the device,
        or int32) on the GPU.  A label outside [0, C) makes its row ignored, a NaN or infinite logit makes it non-finite;
        both are counted and contribute nothing else.  With ``grad_scale`` set, returns ``dlogits`` float32 [B, C] =
        ``(softmax - onehot) * grad_scale`` (``1 / B``: the gradient of ``nn.CrossEntropyLoss()``), zeros for such rows."""
        import torch

        if not logits.is_cuda or not labels.is_cuda:
            raise ModelError("Evaluator.update needs CUDA/ROCm tensors: the statistics are HIP kernels and have no CPU fallback")
        if logits.dim() != 2 or logits.shape[1] != self.num_classes or labels.shape != (logits.shape[0],) or logits.shape[0] < 1:
            raise ModelError(f"Evaluator.update expects logits [B, {self.num_classes}] and labels [B], got {tuple(logits.shape)} and "
                             f"{tuple(labels.shape)}")
        if (logits.device.index or 0) != self._ctx.device:
            raise ModelError(f"Evaluator.update: the statistics live on cuda:{self._ctx.device}, the logits on {logits.device}")
        logits = logits.detach().to(torch.float32).contiguous()
        truth = labels.detach().to(logits.device, torch.int32).contiguous()
        self._ctx.use_torch_stream()
        dlogits = torch.empty_like(logits) if grad_scale is not None else None
        self._ctx.eval_update_f32(logits, truth, 0.0 if grad_scale is None else float(grad_scale), dlogits)
        return dlogits

    def reset(self) -> None:
        self._ctx.use_torch_stream()
        self._ctx.eval_reset()

    def report(self) -> EvalReport:
        """Wait for the stream, read the accumulators back -- the one synchronisation -- and wrap them."""
        self._ctx.use_torch_stream()
        counts, loss_sum, confusion, pos, neg = self._ctx.eval_read()
        return EvalReport(counts, loss_sum, confusion, pos if self.n_bins else None, neg if self.n_bins else None, self.words)

    def close(self) -> None:
        self._ctx.close()


def evaluate(model, loader, n_bins: int = 256, words: Optional[Sequence[str]] = None, evaluator: Optional[Evaluator] = None) -> EvalReport:
    """One validation pass (``Trainer.evaluate``, ``train.py:79-98``; ``KWSTrainer.validate``, ``training.py:347-393``):
    ``model.eval()``, no grad, every batch of ``loader`` through the model and into an ``Evaluator``, one ``report()`` at the
    end.  Serves any model that returns logits [B, C] on the GPU (``DepthwiseSeparableConv``, ``DepthwiseSeparableConvBN``,
    ``CnnTradFpool3``); batches on the host are moved to the GPU first.  ``evaluator``: one to reset and reuse, epoch after
    epoch, in place of a fresh one per call (``n_bins`` and ``words`` are then its own)."""
    import torch

    model.eval()
    ev = evaluator
    if ev is not None:
        ev.reset()
    try:
        with torch.no_grad():
            for x, y in loader:
                if not x.is_cuda:
                    x = x.cuda(non_blocking=True)
                logits = model(x)
                if ev is None:
                    ev = Evaluator(int(logits.shape[1]), n_bins, logits.device.index or 0, words)
                ev.update(logits, y.to(logits.device, non_blocking=True))
        if ev is None:
            raise ModelError("evaluate: the loader yielded no batch")
        return ev.report()
    finally:
        if ev is not None and ev is not evaluator:
            ev.close()
