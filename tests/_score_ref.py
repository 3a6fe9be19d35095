"""Expectations shared by tests/test_score_cpu.py and tests/test_score_gpu.py (not a test module): two NumPy matchers of an event
list against an annotation table, written independently of each other, and the random cases the CPU test feeds both.

Events: one list of ``(window, label)`` per recording, in window order.  Annotations: int rows ``(recording, label, first_window,
last_window)``.  Both matchers return int64 ``[C, 4]`` = hits, false alarms, duplicates, latency sum in windows."""
import numpy as np


def match_sorted(events, truth, C):
    """The rule of include/kws_hip.h over the sorted table: the rows by (recording, label, first_window), per event a binary
    search for the last interval of its recording and label that begins at or before it, and ONE integer of state per class --
    the interval that class hit last, which is all the kernel keeps as well."""
    truth = np.asarray(truth, np.int64).reshape(-1, 4)
    rows = truth[np.lexsort((truth[:, 2], truth[:, 1], truth[:, 0]))] if len(truth) else truth
    out = np.zeros((C, 4), np.int64)
    for r, ev in enumerate(events):
        last_hit = [-1] * C
        for w, k in ev:
            lo = int(np.searchsorted(rows[:, 0] * C + rows[:, 1], r * C + k, "left")) if len(rows) else 0
            hi = int(np.searchsorted(rows[:, 0] * C + rows[:, 1], r * C + k, "right")) if len(rows) else 0
            j = lo + int(np.searchsorted(rows[lo:hi, 2], w, "right")) - 1
            if j < lo or w > rows[j, 3]:
                out[k, 1] += 1
            elif j == last_hit[k]:
                out[k, 2] += 1
            else:
                out[k, 0] += 1
                out[k, 3] += w - rows[j, 2]
                last_hit[k] = j
    return out


def match_brute(events, truth, C):
    """Independent of any order: every event against every annotation of its recording and label, a matched flag per annotation."""
    truth = [tuple(int(v) for v in row) for row in np.asarray(truth, np.int64).reshape(-1, 4)]
    matched = [False] * len(truth)
    out = np.zeros((C, 4), np.int64)
    for r, ev in enumerate(events):
        for w, k in ev:
            inside = [i for i, (tr, tk, a, b) in enumerate(truth) if tr == r and tk == k and a <= w <= b]
            assert len(inside) <= 1, "two annotations of one recording and label overlap"
            if not inside:
                out[k, 1] += 1
            elif matched[inside[0]]:
                out[k, 2] += 1
            else:
                matched[inside[0]] = True
                out[k, 0] += 1
                out[k, 3] += w - truth[inside[0]][2]
    return out


def random_truth(rng, R, C, W, first_keyword, per_list=3, beyond=5):
    """Up to ``per_list`` disjoint intervals per (recording, keyword label), shuffled; rows of different labels may overlap, and
    a last window may lie up to ``beyond`` windows past the recording."""
    rows = []
    for r in range(R):
        for k in range(first_keyword, C):
            cuts = np.sort(rng.choice(W + beyond, size=min(2 * int(rng.integers(0, per_list + 1)), W + beyond), replace=False))
            rows += [(r, k, int(a), int(b)) for a, b in zip(cuts[0::2], cuts[1::2])]
    rows = np.asarray(rows, np.int32).reshape(-1, 4)
    return rows[rng.permutation(len(rows))]


def random_events(rng, R, C, W, first_keyword, refractory, density=0.3):
    """Per recording a window-ordered list of (window, label), at least ``refractory`` windows apart, labels keywords only."""
    out = []
    for _ in range(R):
        ev, nxt = [], 0
        for w in range(W):
            if w >= nxt and rng.random() < density:
                ev.append((w, int(rng.integers(first_keyword, C))))
                nxt = w + refractory
        out.append(ev)
    return out


def plan_ref(truth, R, C):
    """kws_host_score_plan by a NumPy sort: (rows by (recording, label, first_window), off [R * C + 1])."""
    truth = np.asarray(truth, np.int32).reshape(-1, 4)
    rows = truth[np.lexsort((truth[:, 2], truth[:, 1], truth[:, 0]))] if len(truth) else truth
    off = np.zeros(R * C + 1, np.int32)
    if len(rows):
        off[1:] = np.cumsum(np.bincount(rows[:, 0].astype(np.int64) * C + rows[:, 1], minlength=R * C))
    return rows, off
