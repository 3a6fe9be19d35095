"""CPU tests of the live utterance path (kws_stream_utt_*): the hop-by-hop restatement against the whole-signal definition over
the sweep the GPU test runs, what that sweep's reference answers cover, the history formula through the C ABI, the coverage of
the ring-cut cases and the energy margins of the push-driven audio.  tests/test_live_gpu.py runs the device against the same
expectations."""
import ctypes as C

import numpy as np
import pytest

import _live_ref as lr
from _segment_ref import WINDOW_PAIRS

native = pytest.importorskip("kws._native")


def test_hop_by_hop_equals_the_whole_signal_walk_and_the_sweep_covers_the_edges():
    """LiveRef stepped frame by frame and flushed == walk_ref (n_total beyond reach) for every case of the GPU sweep, and the
    REFERENCE's answers over that sweep hold every situation the device has to get right."""
    seen, n_sets = set(), 0
    cases = list(lr.sweep_cases()) + lr.EXTRA_CASES
    assert {F for F, _, _ in cases} == set(lr.SWEEP_FRAMES) and {p for _, p, _ in cases} == set(WINDOW_PAIRS)
    for F, (on, off), flags in cases:
        for pre_roll in lr.SWEEP_PRE_ROLLS:
            for max_frames in lr.sweep_max_frames(F):
                want = lr.whole_signal_records(flags, on, off, pre_roll, max_frames)
                got = lr.live_run(flags, on, off, pre_roll, max_frames)
                assert got == want, (F, on, off, pre_roll, max_frames)
                seen |= lr.coverage_of(want, flags.shape[0], F, pre_roll)
                n_sets += 1
    assert n_sets == (36 + len(lr.EXTRA_CASES)) * 9
    assert seen >= lr.COVERAGE, f"the sweep's reference answers never show: {sorted(lr.COVERAGE - seen)}"


def test_no_unprotected_hazard_in_the_live_unit():
    """The wait-state lint over the new unit's device listing, which also shows what the hand-off to the host rests on: the
    records and totals leave as write-through system-scope stores."""
    import os
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(repo, "tools"))
    import isa_hazard_lint as lint

    if not os.path.exists(lint.HIPCC):
        pytest.skip("hipcc not installed")
    findings, _, isa = lint.lint_file(os.path.join(repo, "keyword-spotting_amd", "csrc", "kws_live.hip"))
    flat = [(fn[:60], line, rule, msg) for fn, fs in findings.items() for line, rule, msg in fs]
    assert not flat, f"kws_live.hip ({isa}): {flat[:5]}"
    body = open(isa).read()
    assert "kws_live_step_kernel" in body and "kws_live_cut_kernel" in body
    assert body.count("global_store_dwordx2") >= 18 and "sc0 sc1" in body  # 6 record words + 3 totals, in step and flush


def _history(*args):
    n = C.c_int(-7)
    rc = native.lib().kws_host_stream_utt_history(*args, C.byref(n))
    return rc, n.value


def test_history_formula_and_its_refusals():
    # 400 / 160: K = 3
    assert _history(400, 160, 60, 1000, 8) == (native.KWS_OK, (60 + 1000 - 1 + 3 + 8) * 160)
    assert _history(400, 160, 0, 2, 0) == (native.KWS_OK, (0 + 2 - 1 + 3) * 160)
    # K = 1 (a frame of one hop) and K = 4
    assert _history(160, 160, 4, 12, 0) == (native.KWS_OK, (4 + 12 - 1 + 1) * 160)
    assert _history(512, 128, 7, 30, 2) == (native.KWS_OK, (7 + 30 - 1 + 4 + 2) * 128)
    assert _history(400, 100, 7, 30, 2) == (native.KWS_OK, (7 + 30 - 1 + 4 + 2) * 100)
    for f in ((400, 160, 60, 1000, 8), (400, 160, 0, 2, 0), (160, 160, 4, 12, 0), (512, 128, 7, 30, 2)):
        assert native.host_stream_utt_history(*f) == lr.history(f[2], f[3], f[4], f[0], f[1])
    # the longest span, in whole hops, plus the slack
    assert lr.history(60, 1000, 0) >= (60 + 1000 - 1) * 160 + 400 > lr.history(60, 1000, 0) - 160
    for bad in ((0, 160, 60, 1000, 8), (400, 0, 60, 1000, 8), (400, 160, -1, 1000, 8), (400, 160, 60, 1, 8), (400, 160, 60, 1000, -1),
                (400, 160, 2 ** 30, 2 ** 30, 0), (400, 160, 60, 2 ** 31 - 1, 8)):
        assert _history(*bad) == (native.KWS_EINVAL, -7), bad
    assert native.lib().kws_host_stream_utt_history(400, 160, 60, 1000, 8, None) == native.KWS_EINVAL
    with pytest.raises(Exception, match="kws_host_stream_utt_history"):
        native.host_stream_utt_history(400, 160, 60, 1, 8)


@pytest.mark.parametrize("name", list(lr.CUT_GEOMETRIES))
def test_ring_cut_cases_cover_the_seam(name):
    """The spans of the ring-cut test, from the reference's own records: the history is at the slack_hops = 0 minimum, wraps at
    least three times, and the spans cross the seam, start on it, (with a frame of whole hops) end on it, reach the longest
    length the formula allows, hold a -32768 and are all zeros."""
    frame_len, step, _ = lr.CUT_GEOMETRIES[name]
    flags, pcm, records, H, facts = lr.cut_case(name)
    assert H == native.host_stream_utt_history(frame_len, step, lr.CUT_PRE_ROLL, lr.CUT_MAX_FRAMES, 0)
    assert pcm.shape[1] >= 3 * H and len(records) >= 6
    assert facts >= lr.CUT_FACTS[name], f"{name}: never {sorted(lr.CUT_FACTS[name] - facts)}"
    assert all(0 <= a < b <= pcm.shape[1] and b - a <= H for _, a, b in lr.spans_of(records))
    assert min(b - a for _, a, b in lr.spans_of(records)) < min(lr.CUT_N_OUT) < max(b - a for _, a, b in lr.spans_of(records)) < max(lr.CUT_N_OUT) \
        or min(lr.CUT_N_OUT) < max(b - a for _, a, b in lr.spans_of(records)) < max(lr.CUT_N_OUT)
    # the walk the explicit steps drive is the whole-signal walk
    assert records == lr.whole_signal_records(flags, lr.CUT_ON, lr.CUT_OFF, lr.CUT_PRE_ROLL, lr.CUT_MAX_FRAMES, frame_len=frame_len,
                                              frame_step=step)


@pytest.mark.parametrize("on,off", lr.PUSH_PAIRS)
def test_push_audio_is_decided_by_a_wide_margin(on, off):
    """Every complete frame's float64 log energy is at least 3.0 away from the threshold (the margin of
    test_stream_decisions_gpu.py::_oracle_states), and the reference's answer has an endpoint close and a time-out."""
    pcm = lr.push_pcm(on, off)
    flags, worst = lr.oracle_flags(pcm)
    assert worst >= 3.0, worst
    assert flags.shape == (2, lr.push_hops(off) - (lr.LAG - 1))
    reasons = set()
    for pre_roll, max_frames in lr.push_runs(on, off):
        records = lr.live_run(flags, on, off, pre_roll, max_frames)
        assert records == lr.whole_signal_records(flags, on, off, pre_roll, max_frames)
        assert len(records) >= 4
        reasons |= {r[5] for r in records}
    assert {0, 1} <= reasons, (on, off, reasons)


def test_rate_audio_is_decided():
    """The 48 kHz case: every resampled sample's rounding is decided beyond the float64 error bound, and every complete frame of
    what the streams hear is at least 3.0 away from the threshold."""
    plan = native.host_stream_resample_plan(lr.RATE_IN, 16000)
    taps = native.host_resample_design(lr.RATE_IN, 16000)[4]
    heard, decided = lr.rate_heard(lr.rate_input(), plan, taps)
    assert decided > 1.0, decided
    assert heard.shape == (2, lr.RATE_HOPS * 160) and np.abs(heard.astype(np.int64)).max() < 32767
    flags, worst = lr.oracle_flags(heard)
    assert worst >= 3.0, worst
    records = lr.live_run(flags, *lr.RATE_PAIR, lr.RATE_PRE_ROLL, lr.RATE_MAX_FRAMES)
    assert len(records) >= 4 and {0, 1} <= {r[5] for r in records}
