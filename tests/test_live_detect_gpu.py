"""GPU tests of the live keyword events (include/kws_hip.h, kws_stream_detect_*): the step kernel against kws_scan_detect_f32 on
the same logits, bit for bit (smoothed posteriors after every step, labels, events), against the float64 restatement
(tests/_scan_ref.py) on the cases tests/test_live_detect_cpu.py shows to be covering, determinism, the queue, the armed pushes
with the real front end (the pushes' own outputs against an unarmed context, the records against kws_scan_detect_f32 over the
logits those pushes returned), StreamingSpotter(detect=) against KeywordSpotter.scan, and every refusal."""
import ctypes as C
import itertools
import time

import numpy as np
import pytest
import torch

import _live_detect_ref as ld
import _live_ref as lr
import _scan_ref as ref
from kws import _native

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
STEP = ref.FRAME_STEP
N_CLASSES = 12
FIRST_HOP = ld.first_hop(ref.T_WIN, ref.FRAME_LEN, STEP)  # 101
OK, EINVAL, ESTATE, EUNSUPPORTED = _native.KWS_OK, _native.KWS_EINVAL, _native.KWS_ESTATE, _native.KWS_EUNSUPPORTED


def _context(e2e_golden=None):
    c = _native.Context(0)
    c.use_torch_stream()
    if e2e_golden is not None:
        c.load_dscnn(e2e_golden["he.blob"], N_CLASSES)
    return c


@pytest.fixture(scope="module")
def bare():
    """A context without a model: the explicit steps and kws_scan_detect_f32 need none."""
    c = _context()
    yield c
    c.close()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _scan_decisions(c, z, smooth_window, first_keyword, threshold, refractory):
    """kws_scan_detect_f32 on z [S, W, C] (host): (smoothed float32 [S, W, C], per stream [(window, label, score bits)])."""
    S, W, _ = z.shape
    zd = torch.from_numpy(np.ascontiguousarray(z)).to(DEV)
    smoothed = torch.full(z.shape, float("nan"), device=DEV)
    count = torch.full((S,), -7, dtype=torch.int32, device=DEV)
    ev_w = torch.full((S, W), -1, dtype=torch.int32, device=DEV)
    ev_k = torch.full((S, W), -1, dtype=torch.int32, device=DEV)
    ev_s = torch.full((S, W), float("nan"), device=DEV)
    c.scan_detect_f32(zd, smooth_window, first_keyword, threshold, refractory, count, ev_w, ev_k, ev_s, W, smoothed)
    c.sync()
    count, ev_w, ev_k, ev_s = count.cpu().numpy(), ev_w.cpu().numpy(), ev_k.cpu().numpy(), _bits(ev_s.cpu().numpy())
    assert (count >= 0).all() and (count <= W).all()
    events = [[(int(ev_w[r, i]), int(ev_k[r, i]), int(ev_s[r, i])) for i in range(count[r])] for r in range(S)]
    return smoothed.cpu().numpy(), events


def _all_records(c):
    total, decisions = c.stream_detect_poll()
    return (c.stream_detect_read(0, total) if total else np.zeros((0, 5), np.int64)), total, decisions


def _live_steps(c, z, smooth_window, first_keyword, threshold, refractory, max_events=None, watch=True):
    """z [S, W, C] (host) through W explicit steps on a fresh stream set: (smoothed [W, S, C], labels [W, S] -- the newest after
    every step --, records int64 [n, 5], total, decisions)."""
    S, W, Cn = z.shape
    c.stream_open(S)
    c.stream_detect_open(Cn, smooth_window, first_keyword, threshold, refractory, 0, max_events if max_events is not None else S * W)
    zt = torch.from_numpy(np.ascontiguousarray(z.transpose(1, 0, 2))).to(DEV)  # one contiguous [S, C] block per step
    sm = torch.full((W, S, Cn), float("nan"), device=DEV)
    lb = torch.full((W, S), -1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    base = zt.data_ptr()
    for d in range(W):
        c.stream_detect_step_f32(base + 4 * S * Cn * d)
        if watch:
            c.stream_detect_smoothed(sm[d], lb[d])
    if max_events is None:
        rec, total, decisions = _all_records(c)
    else:  # the queue may have wrapped: the caller reads what is left
        rec, (total, decisions) = None, c.stream_detect_poll()
    c.sync()
    return sm.cpu().numpy(), lb.cpu().numpy(), rec, total, decisions


def _check_against_scan(c, z, smooth_window, first_keyword, threshold, refractory, what, nan_rows=False):
    """W explicit steps == kws_scan_detect_f32 over the same logits: smoothed bits and labels after EVERY step, records, counts."""
    S, W, _ = z.shape
    want_sm, want_ev = _scan_decisions(c, z, smooth_window, first_keyword, threshold, refractory)
    sm, lb, rec, total, decisions = _live_steps(c, z, smooth_window, first_keyword, threshold, refractory)
    assert decisions == W, what
    got_sm = sm.transpose(1, 0, 2)
    if nan_rows:
        assert np.array_equal(got_sm, want_sm, equal_nan=True), what
    else:
        assert np.array_equal(_bits(got_sm), _bits(want_sm)), what
    assert np.array_equal(lb.T, ld.first_argmax(want_sm)[0]), what
    assert total == sum(len(e) for e in want_ev) == len(rec), what
    assert ld.group_records(rec, S) == want_ev, what
    if len(rec):
        assert np.array_equal(rec[:, 2], rec[:, 1]), what                    # explicit steps: h is d
        order = rec[:, 1] * (S + 1) + rec[:, 0]
        assert (np.diff(order) > 0).all(), what                              # by decision, ascending stream within one
        assert (rec[:, 4] >> 32 == 0).all(), what                            # the score's bits in the low word
    return want_sm, want_ev


# ---- 1. bit identity with the scan's decision layer -------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 63, 64, 65, 130])
def test_steps_are_the_bits_of_kws_scan_detect_f32(bare, S):
    """Around one wavefront and across three; one class, the largest class count; no smoothing, a window of two, a window that
    wraps five times in 40 steps."""
    W, fired = 40, 0
    for Cn in (1, 2, 12, 64):
        z = ref.detect_logits(W, Cn, range(100 * Cn, 100 * Cn + S))
        for smooth_window, refractory in itertools.product((1, 2, 7), (1, 3)):
            first_keyword = 0 if Cn < 3 else 2
            _, ev = _check_against_scan(bare, z, smooth_window, first_keyword, 0.5, refractory, (S, Cn, smooth_window, refractory))
            fired += sum(len(e) for e in ev)
    assert fired > 40 * S


@pytest.mark.parametrize("S,Cn,smooth_window,W", [(2, 12, 256, 300), (1024, 12, 7, 20), (1024, 64, 256, 4)],
                         ids=["ring-wraps-at-256", "1024-streams", "largest-ring"])
def test_steps_at_the_largest_shapes(bare, S, Cn, smooth_window, W):
    z = ref.detect_logits(W, Cn, range(7, 7 + S))
    _, ev = _check_against_scan(bare, z, smooth_window, 2, 0.5, 3, (S, Cn, smooth_window, W))
    assert sum(len(e) for e in ev) >= S // 2
    if S == 1024:
        per_step = np.bincount([e[0] for evs in ev for e in evs], minlength=W)
        assert per_step.max() > 64  # more than one wavefront emits at one step


def test_ties_and_a_nan_row(bare):
    # two equal logits: the lower index wins, in the smoothed argmax as in the events
    z = np.zeros((3, 9, 6), np.float32)
    z[:, :, 4] = 3.0
    z[:, :, 2] = 3.0
    z[2, :, 0] = 3.0  # stream 2: a three-way tie that class 0 wins, below first_keyword
    _, ev = _check_against_scan(bare, z, 3, 2, 0.3, 1, "ties")
    assert [len(e) for e in ev] == [9, 9, 0] and {e[1] for e in ev[0]} == {2}
    # a NaN logit: the row's posteriors are NaN, and so is every mean that holds it; such a decision never fires, and the
    # stream fires again once the row has left the window -- whatever kws_scan_detect_f32 does, bit for bit
    z = ref.detect_logits(12, 4, [1, 2]) * 0
    z[:, :, 3] = 12.0
    z[1, 4, 1] = np.nan
    want_sm, ev = _check_against_scan(bare, z, 3, 0, 0.5, 1, "nan", nan_rows=True)
    assert np.isnan(want_sm[1, 4:7]).all() and not np.isnan(want_sm[1, 7:]).any() and not np.isnan(want_sm[0]).any()
    assert [e[0] for e in ev[1]] == [0, 1, 2, 3, 7, 8, 9, 10, 11] and len(ev[0]) == 12


# ---- 2. against the float64 restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smooth_window", [1, 7, 256])
def test_steps_match_the_float64_restatement(bare, smooth_window):
    threshold, tol = 0.5, ref.tol_smooth(smooth_window)
    worst = 0.0
    for (W, Cn), seeds in ref.DETECT_SEEDS.items():
        z = ref.detect_logits(W, Cn, seeds)
        s = ref.smooth_ref(z, smooth_window)
        m2, mt = ref.margins(s, threshold)
        assert m2 > 2 * tol and mt > 2 * tol, f"the restatement's own decisions are within 2 tol of a boundary: {m2:.2e}, {mt:.2e}"
        for refractory, first_keyword in ((1, 0), (3, 2), (50, 2)):
            what = (W, Cn, smooth_window, refractory, first_keyword)
            want = ref.events_ref(s, first_keyword, threshold, refractory)
            sm, _, rec, total, _ = _live_steps(bare, z, smooth_window, first_keyword, threshold, refractory)
            err = np.abs(sm.transpose(1, 0, 2).astype(np.float64) - s).max()
            worst = max(worst, err)
            assert err <= tol, f"{what}: smoothed posteriors {err:.2e} from the restatement (tol {tol:.2e})"
            got = ld.group_records(rec, len(seeds))
            assert [[e[:2] for e in ev] for ev in got] == [[e[:2] for e in ev] for ev in want], what
            for a, b in zip(got, want):
                for (_, _, bits), (_, _, score) in zip(a, b):
                    assert abs(float(np.uint32(bits).view(np.float32)) - score) <= tol, what
    print(f"[live-detect] smooth_window {smooth_window}: smoothed worst err / tol {worst / tol:.4f}")


# ---- 3. determinism and the queue ----------------------------------------------------------------------------------------------------
def test_queue_bytes_are_the_same_run_to_run(bare):
    z = ref.detect_logits(40, 12, range(130))
    runs = [_live_steps(bare, z, 7, 0, 0.5, 2, watch=False) for _ in range(2)]
    assert runs[0][3] == runs[1][3] > 130 and runs[0][2].tobytes() == runs[1][2].tobytes()


def test_queue_keeps_the_newest_max_events(bare):
    """max_events = S with every stream firing at every step: the oldest records are gone, the total keeps counting, and a
    lost or future sequence number cannot be read."""
    S, Cn, steps = 5, 3, 7
    z = np.zeros((S, steps, Cn), np.float32)
    z[:, :, 2] = 12.0
    live = ld.LiveDetectRef(S, Cn, 1, 0, 0.5, 1, max_events=S)
    for d in range(steps):
        live.step(z[:, d])
    _, _, _, total, decisions = _live_steps(bare, z, 1, 0, 0.5, 1, max_events=S, watch=False)
    N = S * steps
    assert (total, decisions) == (N, steps) == (live.total, live.d)
    got = bare.stream_detect_read(N - S, S)
    want = np.stack([live.queue[seq % S] for seq in range(N - S, N)])
    assert np.array_equal(got[:, :4], want[:, :4])
    assert np.abs(got[:, 4].astype(np.uint32).view(np.float32) - want[:, 4].astype(np.uint32).view(np.float32)).max() <= ref.tol_smooth(1)
    out = (C.c_int64 * (5 * (S + 1)))()
    lib, h = bare._lib, bare._h
    assert lib.kws_stream_detect_read(h, N - S - 1, 1, out) == EINVAL      # overwritten
    assert lib.kws_stream_detect_read(h, N - S - 1, S + 1, out) == EINVAL
    assert lib.kws_stream_detect_read(h, 0, 1, out) == EINVAL
    assert lib.kws_stream_detect_read(h, N - 1, 2, out) == EINVAL          # beyond what has landed
    assert lib.kws_stream_detect_read(h, N, 1, out) == EINVAL
    assert lib.kws_stream_detect_read(h, N - 1, 1, out) == OK
    # an idle set: nothing enqueued, poll returns at once (no 2 ms fallback, no synchronise)
    bare.stream_detect_open(Cn, 1, 0, 0.5, 1, 0, S)
    bare.sync()
    t0 = time.perf_counter()
    assert bare.stream_detect_poll() == (0, 0)
    assert time.perf_counter() - t0 < 1e-3


def test_both_sets_on_one_context_keep_their_own_queues(bare):
    """Utterances and detection armed on ONE context and stepped alternately, never waiting: both queues go through the same
    code (kws_event_queue.h), each with its own counters, slots and kernel count.  The utterance queue (max_events = S) wraps --
    2 S records, the last S closing in one step, the rules and flags of test_live_gpu.test_sequence_numbers_across_stream_counts
    --, the detection queue (46 S slots) never does and holds the bytes of the same steps with detection armed alone.  On the
    CPU (_live_detect_ref.LiveDetectRef, float64) these logits fire 834 events, every one of the 65 streams among them."""
    S, W, Cn = 65, 46, N_CLASSES
    flags = lr.count_flags(S)
    want_utt = lr.whole_signal_records(flags, 3, 5, 2, 1000)
    assert len(want_utt) == 2 * S and {r[4] for r in want_utt[S:]} == {44}
    z = ref.detect_logits(W, Cn, range(1200, 1200 + S))
    _, _, alone, n_alone, _ = _live_steps(bare, z, 2, 2, 0.5, 3, watch=False)
    assert n_alone > S
    bare.stream_open(S)
    bare.stream_utt_open(0.0, 3, 5, 2, 1000, _native.host_stream_utt_history(ref.FRAME_LEN, STEP, 2, 1000, 0), S)
    bare.stream_detect_open(Cn, 2, 2, 0.5, 3, 0, W * S)
    e = torch.from_numpy(lr.energies(flags)).to(DEV)                           # one contiguous [S] row per step
    zt = torch.from_numpy(np.ascontiguousarray(z.transpose(1, 0, 2))).to(DEV)  # one contiguous [S, C] block per step
    torch.cuda.synchronize()
    for t in range(W):
        bare.stream_utt_step_i16(None, e.data_ptr() + 4 * S * t)
        bare.stream_detect_step_f32(zt.data_ptr() + 4 * S * Cn * t)
    bare.stream_utt_flush()
    assert bare.stream_utt_poll() == (2 * S, W)
    assert lr.rows(bare.stream_utt_read(S, S)) == want_utt[S:]
    out = (C.c_int64 * 6)()
    assert bare._lib.kws_stream_utt_read(bare._h, S - 1, 1, out) == EINVAL  # overwritten
    total, decisions = bare.stream_detect_poll()
    assert (total, decisions) == (n_alone, W)
    assert bare.stream_detect_read(0, total).tobytes() == alone.tobytes()
    bare.sync()


# ---- 4. armed pushes, real front end -------------------------------------------------------------------------------------------------
PUSH_S, PUSH_HOPS = 5, 130
# Chosen on the CPU with oracle_scan + smooth_ref over mixed_recordings(5, 130 hops): at a window of 5 the complete windows' top
# posteriors lie in 0.15 .. 0.36; at 0.16 streams 0, 1 and 3 fire from the first complete window, stream 2 from the ninth or so,
# stream 4 (top <= 0.158) mostly not.  The expectation itself is kws_scan_detect_f32 over the logits the pushes returned: no
# margin is needed, only that events occur.
PUSH_RULES = dict(smooth_window=5, first_keyword=2, threshold=0.16, refractory=7)


def _hops_dev(pcm, step=STEP):
    S, n = pcm.shape
    return torch.from_numpy(np.ascontiguousarray(pcm.reshape(S, n // step, step).transpose(1, 0, 2))).to(DEV)


def _push_all(c, entry, pcm, hops_dev, lg, lb, extra=None):
    """Every hop back to back, never waiting for a step.  'device': kws_stream_push_i16 into lg / lb [hops, S, .]; 'host':
    kws_stream_push_host_i16, the host views copied out per hop."""
    S, hops = pcm.shape[0], pcm.shape[1] // STEP
    host_lg, host_lb = np.zeros((hops, S, N_CLASSES), np.float32), np.zeros((hops, S), np.int32)
    for t in range(hops):
        if entry == "device":
            c.stream_push_i16(hops_dev[t], lg[t], lb[t])
        else:
            host_lg[t], host_lb[t] = c.stream_push_host_i16(np.ascontiguousarray(pcm[:, t * STEP:(t + 1) * STEP]), S)
        if extra is not None:
            extra(t)
    c.sync()
    if entry == "device":
        return lg.cpu().numpy(), lb.cpu().numpy()
    return host_lg, host_lb


def _want_push_records(c, logits, first_hop, rules):
    """kws_scan_detect_f32 over the pushes' logits [hops, S, C] from push first_hop on -> rows (stream, d, h, label, bits) in
    queue order."""
    h0 = max(first_hop, 1)
    z = np.ascontiguousarray(logits[h0 - 1:].transpose(1, 0, 2))
    _, ev = _scan_decisions(c, z, rules["smooth_window"], rules["first_keyword"], rules["threshold"], rules["refractory"])
    rows = sorted((d, s, k, bits) for s, evs in enumerate(ev) for d, k, bits in evs)
    return np.array([(s, d, d + h0, k, bits) for d, s, k, bits in rows], np.int64).reshape(-1, 5), z.shape[1]


def _arm(c, first_hop, rules=PUSH_RULES, num_classes=N_CLASSES, max_events=256):
    c.stream_detect_open(num_classes, rules["smooth_window"], rules["first_keyword"], rules["threshold"], rules["refractory"], first_hop,
                         max_events)


def test_armed_pushes_with_the_real_front_end(e2e_golden):
    S, hops = PUSH_S, PUSH_HOPS
    pcm = ref.mixed_recordings(S, hops * STEP, e2e_golden["clips"])
    hops_dev = _hops_dev(pcm)
    armed, plain = _context(e2e_golden), _context(e2e_golden)
    try:
        lg = torch.zeros((hops, S, N_CLASSES), dtype=torch.float32, device=DEV)
        lb = torch.full((hops, S), -1, dtype=torch.int32, device=DEV)
        plain.stream_open(S)
        want_lg, want_lb = (a.copy() for a in _push_all(plain, "device", pcm, hops_dev, lg, lb))
        assert np.abs(want_lg).max() > 0
        alone = None
        for first_hop, entry in itertools.product((FIRST_HOP, 0), ("device", "host")):
            what = (first_hop, entry)
            want, n_dec = _want_push_records(plain, want_lg, first_hop, PUSH_RULES)
            assert n_dec == hops - max(first_hop, 1) + 1 and len(want) >= 4, what
            armed.stream_open(S)
            _arm(armed, first_hop)
            lg.zero_()
            lb.fill_(-1)
            got_lg, got_lb = _push_all(armed, entry, pcm, hops_dev, lg, lb)
            rec, total, decisions = _all_records(armed)
            # the pushes' own outputs: the bits of an unarmed context
            assert np.array_equal(_bits(got_lg), _bits(want_lg)) and np.array_equal(got_lb, want_lb), what
            assert (total, decisions) == (len(want), n_dec), what
            assert np.array_equal(rec, want), what
            if first_hop == 0:
                assert rec[:, 2].min() < FIRST_HOP, "the partial windows decide too"
            elif entry == "device":
                alone = rec
                assert len({int(s) for s in rec[:, 0]}) >= 3 and rec[0, 1] == 0 and rec[0, 2] == FIRST_HOP
        # armed together with live utterances (and with kws_stream_smooth_f32 / kws_stream_vad_f32 called behind every push): both
        # queues hold what each holds alone
        on, off, pre_roll, max_frames = 3, 5, 4, 12
        H = _native.host_stream_utt_history(ref.FRAME_LEN, STEP, pre_roll, max_frames, hops)
        utt = []
        for together in (False, True):
            armed.stream_open(S)
            armed.stream_utt_open(lr.THR, on, off, pre_roll, max_frames, H, 256)
            extra = None
            if together:
                _arm(armed, FIRST_HOP)
                sm = torch.zeros((S, N_CLASSES), dtype=torch.float32, device=DEV)
                aux = torch.zeros((2, S), dtype=torch.int32, device=DEV)

                def extra(t):
                    armed.stream_smooth_f32(lg[t], 4, sm, aux[0])
                    armed.stream_vad_f32(lr.THR, on, off, aux[1])
            _push_all(armed, "device", pcm, hops_dev, lg, lb, extra)
            n_utt, steps = armed.stream_utt_poll()
            assert n_utt >= 4 and steps == hops - (lr.LAG - 1)
            utt.append(armed.stream_utt_read(0, n_utt))
        rec, total, decisions = _all_records(armed)
        assert np.array_equal(utt[0], utt[1]) and np.array_equal(rec, alone) and decisions == hops - FIRST_HOP + 1
    finally:
        armed.close()
        plain.close()


def test_armed_rate_pushes(e2e_golden):
    """48 kHz in: the decisions are taken on the logits of what the streams heard, and h counts the 16 kHz hops."""
    x48 = lr.rate_input()
    S, hops = x48.shape[0], lr.RATE_HOPS
    rules = dict(smooth_window=3, first_keyword=0, threshold=0.1, refractory=4)  # every decision is a candidate: 12 classes
    c = _context(e2e_golden)
    try:
        c.stream_open(S)
        c.stream_resample_open(S, lr.RATE_IN, 16000, 480)
        _arm(c, 0, rules)
        d_x = _hops_dev(x48, 480)
        lg = torch.zeros((hops, S, N_CLASSES), dtype=torch.float32, device=DEV)
        lb = torch.zeros((hops, S), dtype=torch.int32, device=DEV)
        for t in range(hops):
            c.stream_push_rate_i16(d_x[t], lg[t], lb[t])
        rec, total, decisions = _all_records(c)
        c.sync()
        want, n_dec = _want_push_records(c, lg.cpu().numpy(), 0, rules)
        assert (total, decisions) == (len(want), n_dec) == (len(want), hops) and total >= S * (hops // 4)
        assert np.array_equal(rec, want)
    finally:
        c.close()


# ---- 5. Python -------------------------------------------------------------------------------------------------------------------------
# Chosen on the CPU: oracle_scan (psf's float64 MFCC + the reference forward, he weights) at hop_frames = 1 over clip a followed
# by the first half second of clip b, for 24 pairs (a, b); smooth_ref at a window of 5.  Kept: the three pairs whose smallest
# top-2 margin over all 51 windows is largest among those that change or hold a keyword -- (10, 27): 5.3e-3, (4, 33): 4.4e-3,
# (16, 21): 3.7e-3 -- and the threshold in the middle of the widest gap of their top scores, 0.1863 .. 0.1976.  The oracle thus
# keeps 3.7e-3 from a runner-up and 5.6e-3 from the threshold; the test asserts the 1e-3 it needs on the scan's own output.
SPOT_PAIRS, SPOT_SAMPLES = ((10, 27), (4, 33), (16, 21)), 24000
SPOT_RULES = dict(smooth_window=5, threshold=0.192, refractory=10, first_keyword=2)


def test_streaming_spotter_detect_against_scan(bare, e2e_golden):
    from kws.common.errors import ModelError
    from kws.inference import DetectConfig, KeywordEvent, KeywordSpotter, StreamingSpotter
    from kws.libs.models import DepthwiseSeparableConv

    clips = e2e_golden["clips"]
    pcm = np.stack([np.concatenate([clips[a], clips[b][:SPOT_SAMPLES - 16000]]) for a, b in SPOT_PAIRS])
    S, hops = pcm.shape[0], SPOT_SAMPLES // STEP
    model = DepthwiseSeparableConv(num_classes=N_CLASSES)
    model.load_state_dict(ref.state_from_blob(e2e_golden["he.blob"]))
    res = KeywordSpotter(model).scan(pcm, hop_frames=1, max_events=64, **SPOT_RULES)
    n_dec = hops - FIRST_HOP + 1  # 50 complete windows; the scan's 51st holds a zero-padded frame no push completes
    assert res.logits.shape == (S, n_dec + 1, N_CLASSES)
    # the condition, on the scan's own output
    smoothed, _ = _scan_decisions(bare, res.logits, SPOT_RULES["smooth_window"], SPOT_RULES["first_keyword"], SPOT_RULES["threshold"],
                                  SPOT_RULES["refractory"])
    m2, mt = ref.margins(smoothed[:, :n_dec], SPOT_RULES["threshold"])
    assert m2 >= 1e-3 and mt >= 1e-3, f"the scan's decisions are within 1e-3 of a boundary: {m2:.2e}, {mt:.2e}"
    end_of = lambda w: (w * STEP + (ref.T_WIN - 1) * STEP + ref.FRAME_LEN) / 16000.0
    want = sorted((t, r, k, score) for r, evs in enumerate(res.events) for t, k, _, score in evs if t <= end_of(n_dec - 1))
    assert len(want) >= 5 and len({r for _, r, _, _ in want}) == 2  # one stream never fires

    live = StreamingSpotter(S, model, detect=DetectConfig(**SPOT_RULES))
    plain = StreamingSpotter(S, model)
    try:
        assert live._host, "arming must not turn the zero-copy path off"
        with pytest.raises(ModelError, match="detect"):
            plain.pop_events()
        with pytest.raises(ModelError, match="detect"):
            plain.smoothed()
        got = []
        for t in range(hops):
            hop = pcm[:, t * STEP:(t + 1) * STEP]
            lb, lg = live.push(hop)
            want_lb, want_lg = plain.push(hop)
            assert np.array_equal(lb, want_lb) and np.array_equal(_bits(lg), _bits(want_lg)), t
            new = live.pop_events()
            assert all(e.hop == t + 1 for e in new), t
            got += new
            if t + 1 < FIRST_HOP:
                assert new == []
        assert live.pop_events() == []
        labels, post = live.smoothed()
        assert labels.shape == (S,) and post.shape == (S, N_CLASSES) and np.array_equal(labels, ld.first_argmax(post)[0])
        assert np.abs(post.astype(np.float64) - smoothed[:, n_dec - 1]).max() <= 1e-4
        assert len(got) == len(want)
        for e, (time_s, r, k, score) in zip(got, want):
            assert isinstance(e, KeywordEvent)
            assert (e.stream, e.index, e.word, e.time_s) == (r, k, live.words[k], time_s)
            assert e.decision == e.hop - FIRST_HOP and e.time_s == end_of(e.decision)
            assert abs(e.score - score) <= 1e-4
    finally:
        live.close()
        plain.close()
    # every push decides without skip_partial_windows; close() disarms
    early = StreamingSpotter(1, model, detect=DetectConfig(0.0, first_keyword=0, refractory=1, skip_partial_windows=False))
    try:
        early.push(pcm[:1, :STEP])
        (e,) = early.pop_events()
        assert (e.stream, e.decision, e.hop) == (0, 0, 1) and e.time_s == (STEP * (1 - lr.LAG) + ref.FRAME_LEN) / 16000.0
    finally:
        early.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_argument_and_state_errors(e2e_golden):
    c = _context(e2e_golden)
    try:
        lib, h = c._lib, c._h
        S = 3
        hop = torch.zeros((S, STEP), dtype=torch.int16, device=DEV)
        lg = torch.zeros((S, N_CLASSES), dtype=torch.float32, device=DEV)
        sm = torch.zeros((S, N_CLASSES), dtype=torch.float32, device=DEV)
        lb = torch.zeros((S,), dtype=torch.int32, device=DEV)
        rec = (C.c_int64 * 10)()
        u64 = C.c_uint64(0)

        def open_(Cn=N_CLASSES, smooth_window=3, first_keyword=2, threshold=0.5, refractory=2, first_hop=0, max_events=8):
            return lib.kws_stream_detect_open(h, Cn, smooth_window, first_keyword, threshold, refractory, first_hop, max_events)

        def unarmed():
            assert lib.kws_stream_detect_step_f32(h, lg.data_ptr()) == ESTATE
            assert lib.kws_stream_detect_poll(h, C.byref(u64), C.byref(u64)) == ESTATE
            assert lib.kws_stream_detect_read(h, 0, 1, rec) == ESTATE
            assert lib.kws_stream_detect_smoothed(h, sm.data_ptr(), lb.data_ptr()) == ESTATE
            assert lib.kws_stream_detect_close(h) == OK

        assert open_() == ESTATE  # no open stream set
        unarmed()
        c.stream_open(S)
        unarmed()
        assert open_() == OK
        for bad in (dict(Cn=0), dict(Cn=65), dict(smooth_window=0), dict(smooth_window=257), dict(refractory=0), dict(first_keyword=-1),
                    dict(first_hop=-1), dict(max_events=S - 1)):
            assert open_(**bad) == EINVAL, bad
        assert lib.kws_stream_detect_poll(h, None, None) == OK  # a refused open leaves the armed set alone
        assert lib.kws_stream_detect_step_f32(h, None) == EINVAL
        assert lib.kws_stream_detect_read(h, 0, 0, rec) == EINVAL and lib.kws_stream_detect_read(h, 0, 1, None) == EINVAL
        assert lib.kws_stream_detect_read(h, 0, 1, rec) == EINVAL  # nothing has landed
        assert lib.kws_stream_detect_smoothed(h, None, lb.data_ptr()) == EINVAL
        assert lib.kws_stream_detect_smoothed(h, sm.data_ptr(), None) == EINVAL
        # the two drivers exclude each other per armed set
        assert lib.kws_stream_detect_step_f32(h, lg.data_ptr()) == OK
        assert lib.kws_stream_push_i16(h, hop.data_ptr(), lg.data_ptr(), None, 0) == ESTATE
        assert c.stream_detect_poll()[1] == 1
        assert open_() == OK  # a second open replaces the first
        assert c.stream_detect_poll() == (0, 0)
        assert lib.kws_stream_push_i16(h, hop.data_ptr(), lg.data_ptr(), None, 0) == OK
        assert lib.kws_stream_detect_step_f32(h, lg.data_ptr()) == ESTATE
        # a push without logits on an armed context; another class count than the model's
        assert lib.kws_stream_push_i16(h, hop.data_ptr(), None, None, 0) == ESTATE
        assert c.stream_detect_poll()[1] == 1
        assert open_(Cn=5) == OK
        assert lib.kws_stream_push_i16(h, hop.data_ptr(), lg.data_ptr(), None, 0) == EINVAL
        assert c.stream_detect_poll() == (0, 0)
        # dropped with the streams
        assert lib.kws_stream_detect_close(h) == OK
        unarmed()
        assert lib.kws_stream_push_i16(h, hop.data_ptr(), None, None, 0) == OK  # disarmed: a features-only push is fine again
        for drop in (lambda: c.stream_open(S), lambda: c.stream_close(), lambda: c.set_frontend()):
            c.stream_open(S)
            assert open_() == OK
            drop()
            assert lib.kws_stream_detect_poll(h, None, None) == ESTATE
    finally:
        c.close()


def test_more_than_1024_streams_are_refused(bare):
    bare.stream_open(1025)
    assert bare._lib.kws_stream_detect_open(bare._h, 12, 1, 2, 0.5, 1, 0, 1025) == EUNSUPPORTED
    assert bare._lib.kws_stream_detect_poll(bare._h, None, None) == ESTATE
    bare.stream_close()
