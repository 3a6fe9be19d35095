"""CPU tests of scoring a scan against annotations (include/kws_hip.h: kws_host_score_plan; kws.libs.evaluation: truth_windows,
DetectionReport): the two matchers of tests/_score_ref.py against each other, the host plan against a NumPy sort and every one of
its refusals, the mapping of annotations in seconds to windows, and the report's arithmetic from hand-written counts."""
import ctypes as C

import numpy as np
import pytest

import _score_ref as ref

native = pytest.importorskip("kws._native")
from kws.common.errors import KWSError, ModelError  # noqa: E402
from kws.libs.evaluation import DetectionReport, truth_windows  # noqa: E402

EINVAL, EUNSUPPORTED = native.KWS_EINVAL, native.KWS_EUNSUPPORTED


# ---- the matchers ---------------------------------------------------------------------------------------------------
def test_the_two_matchers_agree_on_random_cases():
    """300 cases: refractory 1 (duplicates inside one interval), no annotations at all, labels overlapping in time (an event
    inside another label's interval is a false alarm).  Each situation must occur."""
    rng = np.random.default_rng(2024)
    seen = np.zeros(4, np.int64)
    foreign = 0
    for case in range(300):
        R, C, W = int(rng.integers(1, 4)), int(rng.integers(3, 8)), int(rng.integers(1, 90))
        fk = int(rng.integers(0, 3))
        refractory = 1 if case % 3 == 0 else int(rng.integers(2, 30))
        truth = np.zeros((0, 4), np.int32) if case % 10 == 0 else ref.random_truth(rng, R, C, W, fk)
        events = ref.random_events(rng, R, C, W, fk, refractory, density=0.5 if case % 3 == 0 else 0.2)
        a, b = ref.match_sorted(events, truth, C), ref.match_brute(events, truth, C)
        assert np.array_equal(a, b), (case, a, b)
        assert a[:, :3].sum() == sum(len(e) for e in events)
        seen += a.sum(axis=0)
        for r, ev in enumerate(events):
            for w, k in ev:
                own = any(t[0] == r and t[1] == k and t[2] <= w <= t[3] for t in truth)
                other = any(t[0] == r and t[1] != k and t[2] <= w <= t[3] for t in truth)
                foreign += (not own) and other
    assert all(seen > 0) and foreign > 0, (seen, foreign)


def test_matchers_by_hand():
    #            hit at 3 (latency 1), duplicate at 4, false alarm at 9; label 3 inside label 2's interval: a false alarm
    truth = [(0, 2, 2, 5), (0, 2, 6, 8)]
    events = [[(3, 2), (4, 2), (5, 3), (7, 2), (9, 2)]]
    want = np.zeros((4, 4), np.int64)
    want[2] = (2, 1, 1, 1 + 1)
    want[3] = (0, 1, 0, 0)
    assert np.array_equal(ref.match_sorted(events, truth, 4), want) and np.array_equal(ref.match_brute(events, truth, 4), want)


# ---- kws_host_score_plan --------------------------------------------------------------------------------------------
def plan_rc(truth, N, R, Cn, fk, with_sorted=True):
    t = np.ascontiguousarray(np.asarray(truth, np.int32).reshape(-1, 4))
    srt = np.full((max(len(t), 1), 4), -7, np.int32)
    off = np.full(max(R * Cn, 0) + 1, -7, np.int32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rc = native.lib().kws_host_score_plan(p(t) if len(t) else None, N, R, Cn, fk, p(srt) if with_sorted else None, p(off))
    return rc, srt, off


def test_plan_against_a_numpy_sort():
    rng = np.random.default_rng(5)
    for R, Cn, W, fk in ((1, 3, 40, 2), (4, 12, 200, 2), (3, 64, 100, 0), (7, 5, 30, 1)):
        truth = ref.random_truth(rng, R, Cn, W, fk)
        keep = truth.copy()
        srt, off = native.host_score_plan(truth, R, Cn, fk)
        want_rows, want_off = ref.plan_ref(truth, R, Cn)
        assert np.array_equal(truth, keep), "the caller's table was modified"
        assert srt.dtype == np.int32 and np.array_equal(srt, want_rows)
        assert np.array_equal(off, want_off) and off[-1] == len(truth)
        assert (np.diff(off) == 0).any(), "the case needs an empty (recording, label) list"
        for r in range(R):
            for k in range(Cn):
                rows = srt[off[r * Cn + k]:off[r * Cn + k + 1]]
                assert (rows[:, 0] == r).all() and (rows[:, 1] == k).all() and (np.diff(rows[:, 2]) > 0).all()


def test_plan_without_annotations():
    srt, off = native.host_score_plan(None, 3, 12, 2)
    assert srt.shape == (0, 4) and np.array_equal(off, np.zeros(37, np.int32))
    rc, _, off = plan_rc([], 0, 2, 5, 2, with_sorted=False)  # truth and sorted NULL
    assert rc == 0 and np.array_equal(off, np.zeros(11, np.int32))


def test_plan_adjacent_intervals_and_other_labels_are_fine():
    truth = [(0, 2, 5, 9), (0, 2, 10, 10), (0, 3, 0, 100), (1, 2, 5, 9), (0, 2, 0, 4)]
    srt, off = native.host_score_plan(truth, 2, 4, 2)
    assert srt.tolist() == [[0, 2, 0, 4], [0, 2, 5, 9], [0, 2, 10, 10], [0, 3, 0, 100], [1, 2, 5, 9]]
    assert off.tolist() == [0, 0, 0, 3, 4, 4, 4, 5, 5]


@pytest.mark.parametrize("name, truth, R, Cn, fk, code", [
    ("recording below 0", [(-1, 2, 0, 1)], 2, 4, 2, EINVAL),
    ("recording at R", [(2, 2, 0, 1)], 2, 4, 2, EINVAL),
    ("label at C", [(0, 4, 0, 1)], 2, 4, 2, EINVAL),
    ("label below 0", [(0, -1, 0, 1)], 2, 4, 0, EINVAL),
    ("label below first_keyword", [(0, 1, 0, 1)], 2, 4, 2, EINVAL),
    ("first after last", [(0, 2, 5, 4)], 2, 4, 2, EINVAL),
    ("negative first", [(0, 2, -1, 4)], 2, 4, 2, EINVAL),
    ("overlap", [(0, 2, 0, 10), (1, 2, 0, 10), (0, 2, 5, 20)], 2, 4, 2, EINVAL),
    ("touching at one window", [(0, 3, 11, 20), (0, 3, 0, 11)], 2, 4, 2, EINVAL),
    ("one inside another", [(0, 3, 0, 20), (0, 3, 5, 6)], 2, 4, 2, EINVAL),
    ("the same row twice", [(0, 3, 5, 6), (0, 3, 5, 6)], 2, 4, 2, EINVAL),
    ("R below 1", [(0, 2, 0, 1)], 0, 4, 2, EINVAL),
    ("C below 1", [], 2, 0, 0, EINVAL),
    ("C above 64", [(0, 2, 0, 1)], 2, 65, 2, EINVAL),
    ("negative first_keyword", [(0, 2, 0, 1)], 2, 4, -1, EINVAL),
    ("R above 2^20", [(0, 0, 0, 1)], (1 << 20) + 1, 1, 0, EUNSUPPORTED),
])
def test_plan_refusals(name, truth, R, Cn, fk, code):
    rc, srt, off = plan_rc(truth, len(truth), R, Cn, fk)
    assert rc == code, name
    assert (srt == -7).all() and (off == -7).all(), "a refused plan wrote something"
    if rc == EINVAL and R >= 1 and 1 <= Cn <= 64:
        with pytest.raises(KWSError):
            native.host_score_plan(truth, R, Cn, fk)


def test_plan_limits_and_null_pointers():
    lib = native.lib()
    off = np.zeros(9, np.int32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    one = np.array([[0, 2, 0, 1]], np.int32)
    assert lib.kws_host_score_plan(p(one), (1 << 24) + 1, 2, 4, 2, p(one), p(off)) == EUNSUPPORTED  # refused before a row is read
    assert lib.kws_host_score_plan(p(one), -1, 2, 4, 2, p(one), p(off)) == EINVAL
    assert lib.kws_host_score_plan(None, 1, 2, 4, 2, p(one), p(off)) == EINVAL
    assert lib.kws_host_score_plan(p(one), 1, 2, 4, 2, None, p(off)) == EINVAL
    assert lib.kws_host_score_plan(p(one), 1, 2, 4, 2, p(one), None) == EINVAL
    assert (off == 0).all()


# ---- truth_windows --------------------------------------------------------------------------------------------------
WORDS = ["_silence_", "_unknown_", "yes", "no"]
END_S = 1.0 + 0.5 * np.arange(10)  # windows end at 1.0, 1.5, ..., 5.5 s


def test_truth_windows_maps_end_times():
    rows, n, u = truth_windows([("yes", 2.0, 2.4), (3, 0.0, 0.2)], END_S, tolerance_s=1.0, words=WORDS, recording=4)
    # yes: ends in [2.0, 3.4] -> windows 2..4; no (index form): ends in [0.0, 1.2] -> window 0
    assert rows.dtype == np.int32 and rows.tolist() == [[4, 2, 2, 4], [4, 3, 0, 0]]
    assert n.tolist() == [0, 0, 1, 1] and u.tolist() == [0, 0, 0, 0]
    rows, _, _ = truth_windows([("yes", 2.0, 2.4)], END_S, tolerance_s=0.0, words=WORDS)
    assert rows.tolist() == [[0, 2, 2, 2]]  # only the window ending at 2.0: the bounds are inclusive
    rows, _, _ = truth_windows([(2, 2.0, 2.4)], END_S, num_classes=4)  # no words needed for the index form; the default is 1 s
    assert rows.tolist() == [[0, 2, 2, 4]]


def test_truth_windows_undetectable():
    truth = [("yes", 0.0, 0.5), ("yes", 6.0, 7.0), ("no", 5.4, 9.0), ("yes", 1.1, 1.2)]
    rows, n, u = truth_windows(truth, END_S, tolerance_s=0.25, words=WORDS)
    # before the first window ends (ends needed in [0, 0.75]); after the last (>= 6.0); "no" reaches the last window; ends in
    # [1.1, 1.45]: between two windows
    assert rows.tolist() == [[0, 3, 9, 9]]
    assert n.tolist() == [0, 0, 3, 1] and u.tolist() == [0, 0, 3, 0]
    rows, n, u = truth_windows([("yes", 1.0, 2.0)], np.zeros(0), words=WORDS)  # a recording without windows
    assert rows.shape == (0, 4) and n.tolist() == [0, 0, 1, 0] and u.tolist() == [0, 0, 1, 0]


def test_truth_windows_clips_overlapping_ranges_of_one_label():
    truth = [("yes", 3.0, 3.2), ("yes", 2.0, 2.2), ("no", 2.0, 2.2)]
    rows, n, u = truth_windows(truth, END_S, tolerance_s=1.0, words=WORDS)
    # yes: [2.0, 3.2] -> 2..4 and [3.0, 4.2] -> 4..6: the earlier one ends at 3; "no" overlaps both and stays as it is
    assert rows.tolist() == [[0, 2, 2, 3], [0, 2, 4, 6], [0, 3, 2, 4]]
    assert u.sum() == 0
    srt, _ = native.host_score_plan(rows, 1, 4, 2)  # what comes out is a valid table
    assert len(srt) == 3
    rows, n, u = truth_windows([("yes", 2.0, 2.2), ("yes", 2.0, 2.3)], END_S, words=WORDS)  # nothing is left of the earlier one
    assert rows.tolist() == [[0, 2, 2, 4]] and n[2] == 2 and u[2] == 1


def test_truth_windows_refuses_what_it_cannot_map():
    with pytest.raises(ModelError):
        truth_windows([("maybe", 1.0, 2.0)], END_S, words=WORDS)
    with pytest.raises(ModelError):
        truth_windows([(4, 1.0, 2.0)], END_S, words=WORDS)
    with pytest.raises(ModelError):
        truth_windows([("yes", 2.0, 1.0)], END_S, words=WORDS)
    with pytest.raises(ModelError):
        truth_windows([(2, 1.0, 2.0)], END_S)


# ---- DetectionReport ------------------------------------------------------------------------------------------------
def report():
    counts = np.zeros((3, 4, 4), np.int64)
    #               hits fa dup latency
    counts[0, 2] = (4, 6, 1, 8)   # threshold 0.2
    counts[0, 3] = (2, 2, 0, 2)
    counts[1, 2] = (3, 1, 0, 9)   # threshold 0.5
    counts[1, 3] = (1, 0, 0, 4)
    counts[2, 2] = (1, 0, 0, 5)   # threshold 0.9
    return DetectionReport(counts, n_truth=[0, 0, 5, 3], undetectable=[0, 0, 1, 0], thresholds=[0.2, 0.5, 0.9], hours=0.5, hop_s=0.01,
                           words=WORDS)


def test_report_arithmetic():
    rep = report()
    assert rep.hits.tolist() == [[0, 0, 4, 2], [0, 0, 3, 1], [0, 0, 1, 0]]
    assert rep.false_alarms[:, 2].tolist() == [6, 1, 0] and rep.duplicates[0].tolist() == [0, 0, 1, 0]
    assert rep.misses.tolist() == [[0, 0, 1, 1], [0, 0, 2, 2], [0, 0, 4, 3]]
    assert np.allclose(rep.miss_rate(), [2 / 8, 4 / 8, 7 / 8]) and np.allclose(rep.miss_rate(3), [1 / 3, 2 / 3, 1.0])
    assert np.allclose(rep.miss_rate(0), 0.0)  # no annotations of the class: 0, not a division by zero
    assert np.allclose(rep.false_alarms_per_hour(), [16.0, 2.0, 0.0]) and np.allclose(rep.false_alarms_per_hour(2), [12.0, 2.0, 0.0])
    assert np.allclose(rep.mean_latency_s(), [10 / 6 * 0.01, 13 / 4 * 0.01, 0.05]) and np.allclose(rep.mean_latency_s(3), [0.01, 0.04, 0.0])
    fa, mr, th = rep.det_curve()
    assert np.allclose(th, [0.2, 0.5, 0.9]) and np.allclose(fa, [16.0, 2.0, 0.0]) and np.allclose(mr, [0.25, 0.5, 0.875])
    text = rep.format()
    assert "8 annotations (1 undetectable)" in text and len(text.strip().split("\n")) == 5


def test_report_threshold_for():
    rep = report()
    assert rep.threshold_for(100.0) == pytest.approx(0.2)
    assert rep.threshold_for(16.0) == pytest.approx(0.2)  # the bound is inclusive
    assert rep.threshold_for(5.0) == pytest.approx(0.5)
    assert rep.threshold_for(0.0) == pytest.approx(0.9)
    assert rep.threshold_for(-1.0) is None  # no threshold meets the bound
    assert rep.threshold_for(5.0, c=3) == pytest.approx(0.2)  # class 3: 4 false alarms per hour at 0.2


def test_report_order_sum_and_shape_checks():
    rep = report()
    back = DetectionReport(rep.counts[::-1], rep.n_truth, rep.undetectable, rep.thresholds[::-1], rep.hours, rep.hop_s, WORDS)
    assert np.allclose(back.det_curve()[2], [0.2, 0.5, 0.9]) and np.allclose(back.det_curve()[1], rep.det_curve()[1])
    assert back.threshold_for(5.0) == pytest.approx(0.5)
    both = rep + rep
    assert np.array_equal(both.counts, 2 * rep.counts) and both.hours == 1.0 and both.n_truth.tolist() == [0, 0, 10, 6]
    assert np.allclose(both.miss_rate(), rep.miss_rate()) and np.allclose(both.false_alarms_per_hour(), rep.false_alarms_per_hour())
    with pytest.raises(ModelError):
        rep + back
    with pytest.raises(ModelError):
        DetectionReport(np.zeros((3, 4, 3)), [0] * 4, [0] * 4, [0.1, 0.2, 0.3], 1.0, 0.01)
    with pytest.raises(ModelError):
        DetectionReport(np.zeros((3, 4, 4)), [0] * 4, [0] * 4, [0.1, 0.2], 1.0, 0.01)
