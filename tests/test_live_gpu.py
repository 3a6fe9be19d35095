"""GPU tests of the live utterance path (include/kws_hip.h, kws_stream_utt_*): the step kernel's walk against the whole-signal
walk (tests/_segment_ref.walk_ref) over the sweep tests/test_live_cpu.py shows to be covering, sequence numbers across stream
counts, the event queue, the ring cut against cut_ref on the linear signal, the armed pushes with the real front end (records,
clips, utterance logits, and the pushes' own outputs against an unarmed context), the rate pushes, StreamingSpotter(utterances=)
and every refusal.  Every expectation is computed on the host; nothing here tolerates a difference."""
import ctypes as C

import numpy as np
import pytest
import torch

import _live_ref as lr
import _scan_ref
from _segment_ref import cut_ref
from kws import _native

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
STEP = lr.FRAME_STEP
N_CLASSES = 12
OK, EINVAL, ESTATE, EUNSUPPORTED = _native.KWS_OK, _native.KWS_EINVAL, _native.KWS_ESTATE, _native.KWS_EUNSUPPORTED


def _context(e2e_golden=None, frame=None):
    c = _native.Context(0)
    c.use_torch_stream()
    if frame is not None:
        c.set_frontend(16000, 16000, frame[0], frame[1], 512, 26, 10)
    if e2e_golden is not None:
        c.load_dscnn(e2e_golden["he.blob"], N_CLASSES)
    return c


@pytest.fixture()
def bare():
    """A context without a model: the explicit steps need none."""
    c = _context()
    yield c
    c.close()


def _arm(c, on, off, pre_roll, max_frames, slack_hops=0, max_events=4096, threshold=0.0, frame=(lr.FRAME_LEN, STEP)):
    H = _native.host_stream_utt_history(frame[0], frame[1], pre_roll, max_frames, slack_hops)
    c.stream_utt_open(threshold, on, off, pre_roll, max_frames, H, max_events)
    return H


def _energies(flags, threshold=0.0):
    """flags [S, F] -> float32 [F, S] on the device at threshold +- 1: one contiguous [S] row per step."""
    return torch.from_numpy(lr.energies(flags, threshold)).to(DEV)


_rows = lr.rows


def _all_records(c):
    total, steps = c.stream_utt_poll()
    return (_rows(c.stream_utt_read(0, total)) if total else []), total, steps


def _walk(c, flags, on, off, pre_roll, max_frames, max_events=4096):
    """Energy-only explicit steps over flags [S, F], then a flush: (records, total, steps)."""
    S, F = flags.shape
    c.stream_open(S)
    _arm(c, on, off, pre_roll, max_frames, max_events=max_events)
    e = _energies(flags)
    torch.cuda.synchronize()
    base = e.data_ptr()
    for f in range(F):
        c.stream_utt_step_i16(None, base + 4 * S * f)
    c.stream_utt_flush()
    return _all_records(c)


# ---- 5. the walk ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", lr.SWEEP_FRAMES)
def test_walk_sweep_equals_the_whole_signal_walk(bare, F):
    cases = [k for k in list(lr.sweep_cases()) + lr.EXTRA_CASES if k[0] == F]
    assert len(cases) >= 6
    for _, (on, off), flags in cases:
        for pre_roll in lr.SWEEP_PRE_ROLLS:
            for max_frames in lr.sweep_max_frames(F):
                want = lr.whole_signal_records(flags, on, off, pre_roll, max_frames)
                got, total, steps = _walk(bare, flags, on, off, pre_roll, max_frames)
                assert (total, steps) == (len(want), F), (F, on, off, pre_roll, max_frames)
                assert got == want, (F, on, off, pre_roll, max_frames)


def test_walk_at_the_longest_windows_past_one_turn_of_the_flag_ring(bare):
    """(1024, 1024) over 1100 frames: from frame 1024 on the flag that leaves both windows sits in the slot the new flag takes.
    Stream 0 (the flag track of test_stream_decisions_gpu.test_endpointer_longest_off_window's second case) has a voiced run, a
    pause and is voiced from then on: it opens past frame 1024, when frames of the run have left the windows, and the flush
    closes it.  Stream 1 never opens."""
    S, F, on, off = 2, 1100, 1024, 1024
    flags = np.zeros((S, F), np.int64)
    flags[0, 2:34] = 1
    flags[0, 250:] = 1
    flags[1, 2:30] = 1
    flags[1, 598:601] = 1
    want = lr.whole_signal_records(flags, on, off, 0, 2000)
    assert len(want) == 1 and want[0][0] == 0 and want[0][5] == 2 and want[0][3] >= 1024 and flags[0, :want[0][3] - 1023].any()
    assert want == lr.live_run(flags, on, off, 0, 2000)
    got, total, steps = _walk(bare, flags, on, off, 0, 2000)
    assert (total, steps) == (1, F) and got == want


def test_threshold_is_strict_and_a_nan_is_unvoiced(bare):
    S, F = 3, 12
    e = np.full((F, S), 5.0, np.float32)
    e[:, 1] = 0.25          # == threshold: unvoiced
    e[:, 2] = np.nan
    bare.stream_open(S)
    _arm(bare, 1, 1, 0, 1000, threshold=0.25)
    d = torch.from_numpy(e).to(DEV)
    torch.cuda.synchronize()
    for f in range(F):
        bare.stream_utt_step_i16(None, d[f])
    bare.stream_utt_flush()
    got, total, steps = _all_records(bare)
    assert got == [(0, 0, (F - 1) * STEP + lr.FRAME_LEN, 0, F - 1, 2)] and (total, steps) == (1, F)
    # no hop was appended: the span ends beyond the appended samples and its cut is refused
    clips = torch.full((1, 500), 77, dtype=torch.int16, device=DEV)
    peaks = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    bare.stream_utt_cut_i16(0, clips, 0, peaks)
    bare.sync()
    assert int(peaks.cpu()[0]) == -1 and not clips.cpu().numpy().any()


# ---- 6. stream counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 63, 64, 65, 130, 1024])
def test_sequence_numbers_across_stream_counts(bare, S):
    flags = lr.count_flags(S)
    want = lr.whole_signal_records(flags, 3, 5, 2, 1000)
    assert len(want) == 2 * S and [r[0] for r in want[S:]] == list(range(S)) and {r[4] for r in want[S:]} == {44}
    runs = []
    for _ in range(2):
        got, total, steps = _walk(bare, flags, 3, 5, 2, 1000, max_events=2 * S)
        assert (total, steps) == (2 * S, 46)
        assert got == want  # consecutive sequence numbers, ascending by stream within a step
        runs.append(bare.stream_utt_read(0, total).tobytes())
    assert runs[0] == runs[1]


def test_more_than_1024_streams_are_refused(bare):
    bare.stream_open(1025)
    H = _native.host_stream_utt_history(lr.FRAME_LEN, STEP, 2, 10, 0)
    assert bare._lib.kws_stream_utt_open(bare._h, 0.0, 3, 5, 2, 10, H, 1025) == EUNSUPPORTED
    assert "1024" in bare._lib.kws_last_error(bare._h).decode()
    assert bare._lib.kws_stream_utt_poll(bare._h, None, None) == ESTATE  # not armed


# ---- 8. (and 7.) the ring cut -----------------------------------------------------------------------------------------------
def _hops_dev(pcm, step=STEP, skew=0):
    """int16 [S, hops * step] on the host -> [hops, S, step] on the device, one contiguous [S, step] block per push.  skew: the
    block starts that many int16 past a 16-byte boundary (an allocation starts on one)."""
    S = pcm.shape[0]
    hops = torch.from_numpy(np.ascontiguousarray(pcm.reshape(S, -1, step).transpose(1, 0, 2)))
    buf = torch.empty(hops.numel() + skew, dtype=torch.int16, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = buf[skew:].view(hops.shape)
    out.copy_(hops)
    return out


def _cut_step(c, t, hops_dev, e_base, S, K):
    """Explicit step t: the hop, and from hop K - 1 on the energies of frame t - (K - 1) (every walked frame is complete)."""
    c.stream_utt_step_i16(hops_dev[t], e_base + 4 * S * (t - (K - 1)) if t >= K - 1 else None)


@pytest.mark.parametrize("name, skew", [pytest.param(n, 0, id=n) for n in lr.CUT_GEOMETRIES] + [pytest.param("400/160", 1, id="400/160-skewed")])
def test_ring_cut_equals_the_linear_cut(name, skew):
    """History at the slack_hops = 0 minimum, wrapping many times; every record is cut at once after its close, under every
    normalize_to and n_out; clips and peaks are the bits of cut_ref on the linear signal.  skewed: every hop is handed over from
    an address one int16 past a 16-byte boundary, so the step appends it sample by sample and not 16 bytes at a time."""
    frame_len, step, _ = lr.CUT_GEOMETRIES[name]
    K = -(-frame_len // step)
    flags, pcm, records, H, facts = lr.cut_case(name)
    assert facts >= lr.CUT_FACTS[name]
    S, N = flags.shape[0], len(records)
    combos = [(nz, n_out) for nz in lr.CUT_NORMALIZE for n_out in lr.CUT_N_OUT]
    c = _context(frame=None if name == "400/160" else (frame_len, step))
    try:
        c.stream_open(S)
        assert _arm(c, lr.CUT_ON, lr.CUT_OFF, lr.CUT_PRE_ROLL, lr.CUT_MAX_FRAMES, frame=(frame_len, step)) == H
        assert pcm.shape[1] >= 3 * H
        hops_dev, e = _hops_dev(pcm, step, skew), _energies(flags)
        assert all(hops_dev[t].data_ptr() % 16 == 2 * skew for t in (0, 1, lr.CUT_HOPS - 1))
        clips = [torch.full((N + 1, n_out), 77, dtype=torch.int16, device=DEV) for _, n_out in combos]
        peaks = torch.full((len(combos), N + 1), -7, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        done = 0

        def cut_new():
            nonlocal done
            total, _ = c.stream_utt_poll()
            assert total <= N
            if total > done:
                for k, (nz, _) in enumerate(combos):
                    c.stream_utt_cut_i16(done, clips[k][done:total], nz, peaks[k, done:total])
                done = total

        for t in range(lr.CUT_HOPS):
            _cut_step(c, t, hops_dev, e.data_ptr(), S, K)
            cut_new()
        c.stream_utt_flush()
        cut_new()
        got, total, steps = _all_records(c)
        assert total == N and steps == flags.shape[1] and got == records
        c.sync()
        peaks = peaks.cpu().numpy()
        for k, (nz, n_out) in enumerate(combos):
            want_clips, want_peaks = cut_ref(pcm, lr.spans_of(records), nz, n_out)
            have = clips[k].cpu().numpy()
            assert np.array_equal(peaks[k, :N], want_peaks) and peaks[k, N] == -7, (name, nz, n_out)
            assert np.array_equal(have[:N], want_clips) and (have[N] == 77).all(), (name, nz, n_out)
    finally:
        c.close()


def test_a_cut_one_hop_too_late_is_refused_and_the_same_cut_in_time_is_right(bare):
    """slack_hops = 0 and a span of the longest possible length: right when cut behind its close, refused (zero clip, peak -1)
    when one more hop (slack_hops + 1) has been appended."""
    flags, pcm, records, H, _ = lr.cut_case("400/160")
    longest = (lr.CUT_PRE_ROLL + lr.CUT_MAX_FRAMES - 1) * STEP + lr.FRAME_LEN
    seq = next(i for i, r in enumerate(records) if r[2] - r[1] == longest)
    close_hop = records[seq][4] + lr.LAG - 1
    S = flags.shape[0]
    bare.stream_open(S)
    _arm(bare, lr.CUT_ON, lr.CUT_OFF, lr.CUT_PRE_ROLL, lr.CUT_MAX_FRAMES)
    hops_dev, e = _hops_dev(pcm), _energies(flags)
    clips = torch.full((2, 3001), 77, dtype=torch.int16, device=DEV)
    peaks = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    for t in range(close_hop + 1):
        _cut_step(bare, t, hops_dev, e.data_ptr(), S, lr.LAG)
    bare.stream_utt_cut_i16(seq, clips[0:1], 16384, peaks[0:1])
    bare.stream_utt_step_i16(hops_dev[close_hop + 1], None)
    bare.stream_utt_cut_i16(seq, clips[1:2], 16384, peaks[1:2])
    total, _ = bare.stream_utt_poll()
    assert total > seq and _rows(bare.stream_utt_read(seq, 1)) == [records[seq]]
    bare.sync()
    want_clips, want_peaks = cut_ref(pcm, lr.spans_of(records[seq:seq + 1]), 16384, 3001)
    clips, peaks = clips.cpu().numpy(), peaks.cpu().numpy()
    assert peaks[0] == want_peaks[0] and np.array_equal(clips[0], want_clips[0])
    assert peaks[1] == -1 and not clips[1].any()


def test_queue_keeps_the_newest_max_events(bare):
    """max_events = S: after more than S events the oldest are gone, the total keeps counting, a lost sequence number cannot be
    read, and a cut of it (and of one not emitted yet) is refused while its neighbours in the same call are right."""
    flags, pcm, records, _, _ = lr.cut_case("400/160")
    S, N, slack = flags.shape[0], len(records), 60
    assert N > S + 2
    bare.stream_open(S)
    H = _arm(bare, lr.CUT_ON, lr.CUT_OFF, lr.CUT_PRE_ROLL, lr.CUT_MAX_FRAMES, slack_hops=slack, max_events=S)
    assert all(r[1] >= lr.CUT_HOPS * STEP - H for r in records[N - S:]), "the newest records must still be in the history"
    hops_dev, e = _hops_dev(pcm), _energies(flags)
    torch.cuda.synchronize()
    for t in range(lr.CUT_HOPS):
        _cut_step(bare, t, hops_dev, e.data_ptr(), S, lr.LAG)
    bare.stream_utt_flush()
    total, steps = bare.stream_utt_poll()
    assert (total, steps) == (N, flags.shape[1])
    assert _rows(bare.stream_utt_read(N - S, S)) == records[N - S:]
    out = (C.c_int64 * (6 * (S + 1)))()
    assert bare._lib.kws_stream_utt_read(bare._h, N - S - 1, 1, out) == EINVAL
    assert bare._lib.kws_stream_utt_read(bare._h, N - S - 1, S + 1, out) == EINVAL
    assert bare._lib.kws_stream_utt_read(bare._h, N - 1, 2, out) == EINVAL  # beyond what has landed
    assert bare._lib.kws_stream_utt_read(bare._h, 0, 1, out) == EINVAL
    clips = torch.full((S + 2, 3001), 77, dtype=torch.int16, device=DEV)
    peaks = torch.full((S + 2,), -7, dtype=torch.int32, device=DEV)
    bare.stream_utt_cut_i16(N - S - 1, clips, 16384, peaks)
    bare.sync()
    clips, peaks = clips.cpu().numpy(), peaks.cpu().numpy()
    want_clips, want_peaks = cut_ref(pcm, lr.spans_of(records[N - S:]), 16384, 3001)
    assert peaks[0] == -1 and not clips[0].any() and peaks[S + 1] == -1 and not clips[S + 1].any()
    assert np.array_equal(peaks[1:S + 1], want_peaks) and np.array_equal(clips[1:S + 1], want_clips)


# ---- 9. armed pushes, real front end ---------------------------------------------------------------------------------------------
def _push_all(c, entry, pcm, hops_dev, lg, lb, classify_at=None, scratch=None):
    """Every hop back to back, never waiting for a step.  entry 'device': kws_stream_push_i16 into lg / lb [hops, S, .];
    'host': kws_stream_push_host_i16, the host views copied out per hop.  classify_at: behind that hop, one cut + kws_infer_i16
    on this context (no wait), so that the later pushes run behind a classification."""
    S, hops = pcm.shape[0], pcm.shape[1] // STEP
    host_lg, host_lb = np.zeros((hops, S, N_CLASSES), np.float32), np.zeros((hops, S), np.int32)
    for t in range(hops):
        if entry == "device":
            c.stream_push_i16(hops_dev[t], lg[t], lb[t])
        else:
            h_lg, h_lb = c.stream_push_host_i16(np.ascontiguousarray(pcm[:, t * STEP:(t + 1) * STEP]), S)
            host_lg[t], host_lb[t] = h_lg, h_lb
        if t == classify_at:
            clip, plg, plb = scratch
            c.stream_utt_cut_i16(0, clip, 16384, None)
            c.infer_i16(clip, plg, plb)
    c.sync()
    if entry == "device":
        return lg.cpu().numpy(), lb.cpu().numpy()
    return host_lg, host_lb


@pytest.mark.parametrize("on,off", lr.PUSH_PAIRS)
def test_armed_pushes_with_the_real_front_end(e2e_golden, on, off):
    pcm = lr.push_pcm(on, off)
    S, hops = pcm.shape[0], lr.push_hops(off)
    flags, worst = lr.oracle_flags(pcm)
    assert worst >= 3.0, worst  # no float32 energy decides a case
    hops_dev = _hops_dev(pcm)
    armed, plain, other = _context(e2e_golden), _context(e2e_golden), _context(e2e_golden)
    try:
        lg = torch.zeros((hops, S, N_CLASSES), dtype=torch.float32, device=DEV)
        lb = torch.full((hops, S), -1, dtype=torch.int32, device=DEV)
        scratch = (torch.zeros((1, 16000), dtype=torch.int16, device=DEV), torch.zeros((1, N_CLASSES), dtype=torch.float32, device=DEV),
                   torch.zeros((1,), dtype=torch.int32, device=DEV))
        plain.stream_open(S)
        want_lg, want_lb = _push_all(plain, "device", pcm, hops_dev, lg, lb)
        want_lg, want_lb = want_lg.copy(), want_lb.copy()
        assert np.abs(want_lg).max() > 0
        reasons = set()
        for pre_roll, max_frames in lr.push_runs(on, off):
            want = lr.whole_signal_records(flags, on, off, pre_roll, max_frames)
            reasons |= {r[5] for r in want}
            for entry in ("device", "host"):
                armed.stream_open(S)
                _arm(armed, on, off, pre_roll, max_frames, slack_hops=hops, max_events=64, threshold=lr.THR)
                lg.zero_()
                lb.fill_(-1)
                got_lg, got_lb = _push_all(armed, entry, pcm, hops_dev, lg, lb, classify_at=(2 * hops) // 3, scratch=scratch)
                armed.stream_utt_flush()
                got, total, steps = _all_records(armed)
                assert steps == hops - (lr.LAG - 1) and total == len(want), (entry, pre_roll)
                assert got == want, (entry, pre_roll)
                # the pushes' own outputs: the bits of an unarmed context, before and after the classification
                assert np.array_equal(got_lg.view(np.uint32), want_lg.view(np.uint32)) and np.array_equal(got_lb, want_lb), (entry, pre_roll)
                U = len(want)
                clips = torch.full((U, 16000), 77, dtype=torch.int16, device=DEV)
                peaks = torch.full((U,), -7, dtype=torch.int32, device=DEV)
                ulg = torch.zeros((2, U, N_CLASSES), dtype=torch.float32, device=DEV)
                ulb = torch.full((2, U), -1, dtype=torch.int32, device=DEV)
                armed.stream_utt_cut_i16(0, clips, 16384, peaks)
                armed.infer_i16(clips, ulg[0], ulb[0])
                armed.sync()
                other.infer_i16(clips, ulg[1], ulb[1])
                other.sync()
                want_clips, want_peaks = cut_ref(pcm, lr.spans_of(want), 16384, 16000)
                assert np.array_equal(peaks.cpu().numpy(), want_peaks) and np.array_equal(clips.cpu().numpy(), want_clips), (entry, pre_roll)
                ulg, ulb = ulg.cpu().numpy(), ulb.cpu().numpy()
                assert np.abs(ulg[1]).max() > 0 and np.array_equal(ulg[0].view(np.uint32), ulg[1].view(np.uint32)) and np.array_equal(ulb[0], ulb[1])
        assert {0, 1} <= reasons  # a time-out fired
    finally:
        for c in (armed, plain, other):
            c.close()


def test_the_first_pushes_walk_nothing(e2e_golden):
    c = _context(e2e_golden)
    try:
        S = 2
        c.stream_open(S)
        _arm(c, 3, 5, 4, 12, threshold=lr.THR)
        hop = torch.zeros((S, STEP), dtype=torch.int16, device=DEV)
        lg = torch.zeros((S, N_CLASSES), dtype=torch.float32, device=DEV)
        for _ in range(lr.LAG - 1):
            c.stream_push_i16(hop, lg, None)
        assert c.stream_utt_poll() == (0, 0)
        c.stream_push_i16(hop, lg, None)
        assert c.stream_utt_poll() == (0, 1)
        c.stream_push_i16(hop, None, None)  # a features-only push steps too
        assert c.stream_utt_poll() == (0, 2)
    finally:
        c.close()


# ---- 10. rate pushes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["device", "host"])
def test_rate_pushes_cut_what_the_streams_heard(e2e_golden, entry):
    x48 = lr.rate_input()
    plan = _native.host_stream_resample_plan(lr.RATE_IN, 16000)
    heard, decided = lr.rate_heard(x48, plan, _native.host_resample_design(lr.RATE_IN, 16000)[4])
    assert decided > 1.0
    flags, worst = lr.oracle_flags(heard)
    assert worst >= 3.0, worst
    (on, off), S, hops = lr.RATE_PAIR, x48.shape[0], lr.RATE_HOPS
    want = lr.whole_signal_records(flags, on, off, lr.RATE_PRE_ROLL, lr.RATE_MAX_FRAMES)
    c = _context(e2e_golden)
    try:
        c.stream_open(S)
        c.stream_resample_open(S, lr.RATE_IN, 16000, 480)
        _arm(c, on, off, lr.RATE_PRE_ROLL, lr.RATE_MAX_FRAMES, slack_hops=hops, max_events=64, threshold=lr.THR)
        d_x = _hops_dev(x48, 480)
        lg = torch.zeros((S, N_CLASSES), dtype=torch.float32, device=DEV)
        lb = torch.zeros((S,), dtype=torch.int32, device=DEV)
        for t in range(hops):
            if entry == "device":
                c.stream_push_rate_i16(d_x[t], lg, lb)
            else:
                c.stream_push_host_rate_i16(np.ascontiguousarray(x48[:, t * 480:(t + 1) * 480]), S)
        c.stream_utt_flush()
        got, total, steps = _all_records(c)
        assert steps == hops - (lr.LAG - 1) and got == want
        clips = torch.full((total, 16000), 77, dtype=torch.int16, device=DEV)
        peaks = torch.full((total,), -7, dtype=torch.int32, device=DEV)
        c.stream_utt_cut_i16(0, clips, 16384, peaks)
        c.sync()
        want_clips, want_peaks = cut_ref(heard, lr.spans_of(want), 16384, 16000)
        assert np.array_equal(peaks.cpu().numpy(), want_peaks) and np.array_equal(clips.cpu().numpy(), want_clips)
    finally:
        c.close()


# ---- 11. Python ---------------------------------------------------------------------------------------------------------------------
def test_streaming_spotter_utterances(e2e_golden):
    from kws.common.errors import ModelError
    from kws.inference import KeywordSpotter, StreamingSpotter, Utterance, UtteranceConfig
    from kws.libs.models import DepthwiseSeparableConv

    model = DepthwiseSeparableConv(num_classes=N_CLASSES)
    model.load_state_dict(_scan_ref.state_from_blob(e2e_golden["he.blob"]))
    on, off, pre_roll, hops = 3, 5, 4, 66
    pattern = lr.delayed(lr.cycles(on, off, hops), [0, 3])
    pattern[0, hops - 12:] = False   # stream 0 ends in silence: all its utterances close by endpoint
    pattern[1, hops - 6:] = True     # stream 1 ends inside an utterance
    pcm = lr.pcm_of(pattern, 11)
    flags, worst = lr.oracle_flags(pcm)
    assert worst >= 3.0
    want = lr.whole_signal_records(flags, on, off, pre_roll, 1000)
    assert {r[5] for r in want if r[0] == 0} == {0} and [r[5] for r in want if r[0] == 1][-1] == 2
    cfg = UtteranceConfig(threshold=lr.THR, on_window=on, off_window=off, pre_roll=pre_roll)
    assert (cfg.max_seconds, cfg.normalize, cfg.max_events, cfg.slack_hops) == (10.0, 16384, None, 8)
    assert (UtteranceConfig(1.0).on_window, UtteranceConfig(1.0).off_window, UtteranceConfig(1.0).pre_roll) == (40, 80, 60)
    live, plain = StreamingSpotter(2, model, utterances=cfg), StreamingSpotter(2, model)
    try:
        assert live._host, "arming must not turn the zero-copy path off"
        with pytest.raises(ModelError, match="utterances"):
            plain.pop_utterances()
        got, closes_at = [], {}
        for r in want:
            if r[5] != 2:
                closes_at.setdefault(r[4] + lr.LAG - 1, []).append(r)
        for t in range(hops):
            hop = pcm[:, t * STEP:(t + 1) * STEP]
            lb, lg = live.push(hop)
            want_lb, want_lg = plain.push(hop)
            assert np.array_equal(lb, want_lb) and np.array_equal(lg.view(np.uint32), want_lg.view(np.uint32)), t
            new = live.pop_utterances()
            assert len(new) == len(closes_at.get(t, [])), t  # nothing between closes
            got += new
        assert live.pop_utterances() == []
        flushed = live.flush()
        assert [u.reason for u in flushed] == ["end_of_recording"] and flushed[0].recording == 1
        got += flushed
        assert len(got) == len(want)
        for u, (s, start, end, opened, closed, reason) in zip(got, want):
            assert isinstance(u, Utterance)
            assert (u.recording, u.start_s, u.end_s, u.open_s, u.close_s) == (s, start / 16000, end / 16000, opened * STEP / 16000, closed * STEP / 16000)
            assert u.reason == ("endpoint", "max_length", "end_of_recording")[reason]
            assert u.word == live.words[u.label] and u.logits.shape == (N_CLASSES,)
        _, want_peaks = cut_ref(pcm, lr.spans_of(want), 16384, 16000)
        assert [u.peak for u in got] == [int(p) for p in want_peaks]
        # stream 0, whose utterances all close by endpoint, against the recording path over the same audio
        seg = KeywordSpotter(model).segment(pcm[0], lr.THR, on_window=on, off_window=off, pre_roll=pre_roll)[0]
        mine = [u for u in got if u.recording == 0]
        assert len(seg) == len(mine) >= 2
        for a, b in zip(mine, seg):
            assert (a.start_s, a.end_s, a.open_s, a.close_s, a.reason, a.label, a.peak) == (b.start_s, b.end_s, b.open_s, b.close_s, b.reason, b.label, b.peak)
    finally:
        live.close()
        plain.close()
    again = StreamingSpotter(2, model, utterances=cfg)
    try:
        again.push(pcm[:, :STEP])
        assert again.pop_utterances() == [] and again.flush() == []
    finally:
        again.close()


# ---- 12. refusals -------------------------------------------------------------------------------------------------------------------
def test_argument_and_state_errors(e2e_golden):
    c = _context(e2e_golden)
    try:
        lib, h = c._lib, c._h
        S = 3
        H = _native.host_stream_utt_history(lr.FRAME_LEN, STEP, 4, 12, 0)
        hop = torch.zeros((S, STEP), dtype=torch.int16, device=DEV)
        energy = torch.zeros((S,), dtype=torch.float32, device=DEV)
        lg = torch.zeros((S, N_CLASSES), dtype=torch.float32, device=DEV)
        clips = torch.zeros((1, 100), dtype=torch.int16, device=DEV)
        rec = (C.c_int64 * 6)()
        u64 = C.c_uint64(0)

        def utt_open(thr=0.0, on=3, off=5, pre=4, mf=12, hist=H, ev=S):
            return lib.kws_stream_utt_open(h, thr, on, off, pre, mf, hist, ev)

        def unarmed():
            assert lib.kws_stream_utt_step_i16(h, hop.data_ptr(), energy.data_ptr()) == ESTATE
            assert lib.kws_stream_utt_flush(h) == ESTATE
            assert lib.kws_stream_utt_poll(h, C.byref(u64), C.byref(u64)) == ESTATE
            assert lib.kws_stream_utt_read(h, 0, 1, rec) == ESTATE
            assert lib.kws_stream_utt_cut_i16(h, 0, 1, 0, clips.data_ptr(), 100, None) == ESTATE
            assert lib.kws_stream_utt_close(h) == OK

        assert utt_open() == ESTATE  # no stream set
        unarmed()
        c.stream_open(S)
        unarmed()
        for bad in (dict(on=0), dict(on=6), dict(off=1025), dict(pre=-1), dict(mf=1), dict(mf=0), dict(hist=H - STEP), dict(hist=H + 1),
                    dict(ev=S - 1), dict(pre=2 ** 30, mf=2 ** 30)):
            assert utt_open(**bad) == EINVAL, bad
        assert utt_open(on=1024, off=1024, hist=H + STEP) == OK and utt_open() == OK  # a second open replaces the first
        assert lib.kws_stream_utt_step_i16(h, None, None) == EINVAL
        assert lib.kws_stream_utt_read(h, 0, 0, rec) == EINVAL and lib.kws_stream_utt_read(h, 0, 1, None) == EINVAL
        assert lib.kws_stream_utt_read(h, 0, 1, rec) == EINVAL  # nothing has landed
        for bad in (dict(U=0), dict(n_out=0), dict(nz=-1), dict(nz=32768), dict(p=None)):
            a = dict(U=1, n_out=100, nz=0, p=clips.data_ptr())
            a.update(bad)
            assert lib.kws_stream_utt_cut_i16(h, 0, a["U"], a["nz"], a["p"], a["n_out"], None) == EINVAL, bad
        assert lib.kws_stream_utt_cut_i16(h, 0, 1, 0, clips.data_ptr(), 100, None) == OK  # nothing emitted: a zero clip
        # the two drivers exclude each other
        assert lib.kws_stream_utt_step_i16(h, hop.data_ptr(), None) == OK
        assert lib.kws_stream_push_i16(h, hop.data_ptr(), lg.data_ptr(), None, 0) == ESTATE
        pl, py = C.c_void_p(), C.c_void_p()
        h_hop = np.zeros((S, STEP), np.int16)
        assert lib.kws_stream_push_host_i16(h, h_hop.ctypes.data, C.byref(pl), C.byref(py)) == ESTATE
        assert c.stream_state()[1] == 0, "a refused push reached the streams"
        assert utt_open() == OK
        assert lib.kws_stream_push_i16(h, hop.data_ptr(), lg.data_ptr(), None, 0) == OK
        assert lib.kws_stream_utt_step_i16(h, hop.data_ptr(), energy.data_ptr()) == ESTATE
        assert lib.kws_stream_utt_poll(h, None, None) == OK
        c.stream_open(S)  # drops the utterance set with the streams
        unarmed()
        assert lib.kws_stream_push_i16(h, hop.data_ptr(), lg.data_ptr(), None, 0) == OK
        c.sync()
    finally:
        c.close()
