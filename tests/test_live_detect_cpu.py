"""CPU tests of the live keyword events (kws_stream_detect_*): the hop-by-hop restatement against the whole-recording decision
layer (tests/_scan_ref.py) over the cases the GPU test runs, what that sweep's reference answers cover, the queue's overwrite
arithmetic, the first_hop mapping between decisions and scan windows, the wait-state lint over the new unit and the ABI surface.
tests/test_live_detect_gpu.py runs the device against the same expectations."""
import itertools
import os
import sys

import numpy as np
import pytest

import _live_detect_ref as ld
import _scan_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLD = 0.5


def test_hop_by_hop_equals_the_whole_recording_walk_and_the_sweep_covers_the_edges():
    """LiveDetectRef stepped decision by decision == events_ref(smooth_ref(...)) on detect_logits for every (W, C) of
    DETECT_SEEDS, and the REFERENCE's answers over that sweep hold every situation the device has to get right."""
    seen = set()
    for (W, C), seeds in ref.DETECT_SEEDS.items():
        z = ref.detect_logits(W, C, seeds)
        for S, refractory, first_keyword in itertools.product([1, 7, 256], [1, 3, 50], [0, 2]):
            s = ref.smooth_ref(z, S)
            want = ref.events_ref(s, first_keyword, THRESHOLD, refractory)
            got, smoothed, live = ld.run(z, S, first_keyword, THRESHOLD, refractory)
            what = (W, C, S, refractory, first_keyword)
            assert np.abs(smoothed - s).max() < 1e-12, what  # a direct sum against a difference of running sums, both float64
            assert [[e[:2] for e in ev] for ev in got] == [[e[:2] for e in ev] for ev in want], what
            for a, b in zip(got, want):
                assert all(abs(x[2] - y[2]) < 1e-12 for x, y in zip(a, b)), what
            assert live.total == sum(len(e) for e in want) and live.d == W
            # what these answers show
            k, top = ld.first_argmax(s)
            cand = (k >= first_keyword) & (top >= THRESHOLD)  # [streams, W]
            for r, ev in enumerate(want):
                fired = [e[0] for e in ev]
                if not fired:
                    seen.add("a stream with no event")
                if fired[:1] == [0]:
                    seen.add("an event at decision 0")
                nxt = 0
                for w in range(W):
                    if cand[r, w] and w < nxt:
                        seen.add("two candidates closer than the refractory")
                    if cand[r, w] and w == nxt and w > 0:
                        seen.add("a candidate exactly at next")
                    if cand[r, w] and w >= nxt:
                        nxt = w + refractory
            per_step = np.zeros(W, np.int64)
            for ev in want:
                per_step[np.array([e[0] for e in ev], np.int64)] += 1
            if (per_step == len(seeds)).any():
                seen.add("all streams firing at one step")
            if live.wrapped:
                seen.add("a ring that has wrapped")
    want_seen = {"a stream with no event", "an event at decision 0", "two candidates closer than the refractory", "a candidate exactly at next",
                 "all streams firing at one step", "a ring that has wrapped"}
    assert seen == want_seen, f"the sweep's reference answers never show: {sorted(want_seen - seen)}"


def test_queue_overwrite_arithmetic():
    """max_events = S and every stream firing at every step: the queue holds the newest S records at seq mod S, the total keeps
    counting, and exactly the sequence numbers [total - S, total) can be read."""
    S, C, steps = 5, 3, 7
    z = np.zeros((S, C), np.float32)
    z[:, 2] = 12.0
    live = ld.LiveDetectRef(S, C, 1, 0, THRESHOLD, 1, max_events=S)
    records = []
    for _ in range(steps):
        records += live.step(z)
    assert live.total == S * steps == len(records)
    assert [r[:2] for r in records] == [(s, d) for d in range(steps) for s in range(S)]  # ascending stream within a step
    for seq in range(live.total - S, live.total):
        s, d, h, k, score = records[seq]
        assert tuple(live.queue[seq % S]) == (s, d, h, k, ld.score_bits(score))
    total = live.total
    assert ld.readable(total - S, S, total, S) and ld.readable(total - 1, 1, total, S)
    assert not ld.readable(total - S - 1, 1, total, S)      # overwritten
    assert not ld.readable(total - S - 1, S + 1, total, S)
    assert not ld.readable(total - 1, 2, total, S)          # not landed yet
    assert not ld.readable(total, 1, total, S) and not ld.readable(0, 0, total, S)
    # the score travels as the float's bits in the low word
    assert np.array([ld.score_bits(0.75)], np.int64)[0] == 0x3F400000


@pytest.mark.parametrize("frame_len,frame_step,K", [(160, 160, 1), (400, 160, 3), (512, 128, 4), (400, 100, 4)])
def test_first_hop_maps_decisions_to_scan_windows(frame_len, frame_step, K):
    """Push h (from 1) has delivered h * frame_step samples.  The newest COMPLETE frame and the newest window of 99 complete
    frames follow from sample counts alone; decision d = h - first_hop must be that window, and its time the window's end."""
    T = ref.T_WIN
    assert ld.lag(frame_len, frame_step) == K
    fh = ld.first_hop(T, frame_len, frame_step)
    assert fh == T + K - 1
    live = ld.LiveDetectRef(1, 2, 1, 0, THRESHOLD, 1, first_hop=fh)
    z = np.array([[0.0, 12.0]], np.float32)
    for h in range(1, fh + 40):
        have = h * frame_step
        complete = 0 if have < frame_len else (have - frame_len) // frame_step + 1  # frames wholly inside the samples so far
        windows = max(0, complete - T + 1)                                            # scan windows at hop_frames = 1
        rec = live.step(z, hop=h)
        assert (len(rec) == 1) == (windows >= 1), h
        if rec:
            _, d, hop, _, _ = rec[0]
            w = windows - 1  # the newest
            assert (d, hop) == (w, h)
            end = w * frame_step + (T - 1) * frame_step + frame_len  # scan_window_times' end of window w
            assert ld.event_time(h, frame_len, frame_step) == end / 16000.0
            assert end <= have < end + frame_step
    # with first_hop 0 the partial windows decide too
    assert len(ld.LiveDetectRef(1, 2, 1, 0, THRESHOLD, 1, first_hop=0).step(z, hop=1)) == 1


def test_no_unprotected_hazard_in_the_live_detect_unit():
    """The wait-state lint over the new unit's device listing, which also shows what the hand-off to the host rests on: the
    records and totals leave as write-through system-scope stores."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import isa_hazard_lint as lint

    if not os.path.exists(lint.HIPCC):
        pytest.skip("hipcc not installed")
    findings, _, isa = lint.lint_file(os.path.join(REPO, "keyword-spotting_amd", "csrc", "kws_live_detect.hip"))
    flat = [(fn[:60], line, rule, msg) for fn, fs in findings.items() for line, rule, msg in fs]
    assert not flat, f"kws_live_detect.hip ({isa}): {flat[:5]}"
    body = open(isa).read()
    assert "kws_live_detect_step_kernel" in body
    assert body.count("global_store_dwordx2") >= 8 and "sc0 sc1" in body  # 5 record words + 3 totals to the host
    assert ".amdhsa_private_segment_fixed_size 0" in body  # no scratch


def test_the_abi_surface():
    """The six entries are in the header and in SIGNATURES with matching arity (tests/test_abi_cpu.py compares every symbol);
    the record layout and the Python surface are what the documents say."""
    native = pytest.importorskip("kws._native")
    header = open(os.path.join(REPO, "include", "kws_hip.h")).read()
    names = ["kws_stream_detect_open", "kws_stream_detect_close", "kws_stream_detect_step_f32", "kws_stream_detect_poll",
             "kws_stream_detect_read", "kws_stream_detect_smoothed"]
    arity = [8, 1, 2, 3, 4, 3]
    for name, n in zip(names, arity):
        assert f"int {name}(kws_ctx* ctx" in header, name
        assert name in native.SIGNATURES and len(native.SIGNATURES[name][1]) == n, name
        assert hasattr(native.Context, name[len("kws_"):]), name
    from dataclasses import fields

    from kws.inference import DetectConfig, KeywordEvent

    cfg = DetectConfig(0.7)
    assert (cfg.threshold, cfg.smooth_window, cfg.refractory, cfg.first_keyword, cfg.max_events, cfg.skip_partial_windows) == \
        (0.7, 1, 50, 2, None, True)
    assert [f.name for f in fields(KeywordEvent)] == ["stream", "time_s", "index", "word", "score", "decision", "hop"]
