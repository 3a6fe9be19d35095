"""Batches of recordings of unequal length on the GPU (kws_frames_ragged_i16, kws_scan_ragged_i16, kws_scan_detect_ragged_f32,
kws_segment_ragged_f32, KeywordSpotter.scan_batch / segment_batch / scan_files / segment_files).

Every comparison is np.array_equal on the words, against the EXISTING equal-length entry run on each recording alone in the same
process: no tolerance anywhere.  Output buffers are prefilled with NaN / -1 and over-allocated by one row.  The PCM buffer is
filled with +-32767 sentinels before the recordings are placed, so the samples directly before and after every span would show
in the frames if anything outside a span were read as part of it.

kws_create configures a front end, so KWS_ESTATE for "no front end" cannot be reached on a live context (as in
test_segment_gpu.py); "no model" can and is checked."""
import wave

import numpy as np
import pytest
import torch

import _scan_ref as sref
import _segment_ref as gref
from kws import _native

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
C = 12
T_WIN, N_CEP, FRAME_LEN, FRAME_STEP = sref.T_WIN, sref.N_CEP, sref.FRAME_LEN, sref.FRAME_STEP
u32 = lambda a: np.ascontiguousarray(a).view(np.uint32)


def n_for_frames(F, extra=0):
    """A length with exactly F frames: the last frame ends `extra` samples short of being full (0: no padded last frame)."""
    return FRAME_LEN + FRAME_STEP * (F - 1) - extra


@pytest.fixture(scope="module")
def clips(e2e_golden):
    return e2e_golden["clips"]


@pytest.fixture(scope="module")
def ctx(e2e_golden):
    c = _native.Context(0)
    c.use_torch_stream()
    c.load_dscnn(e2e_golden["he.blob"], C)
    yield c
    c.close()


def place(recs, layout):
    """Recordings -> (device buffer int16 [n_pcm], start int64 [R], length int32 [R]) in a buffer of +-32767 sentinels.  'packed':
    one after another, every start the next multiple of 8 that leaves at least one sentinel sample in between; 'rect': rows of
    equal pitch (the output of a ragged resample), eight sentinels ahead of the first."""
    length = np.array([len(x) for x in recs], np.int32)
    up8 = lambda n: (n + 7) & ~7
    if layout == "packed":
        start, at = [], 8
        for n in length:
            start.append(at)
            at = up8(at + int(n) + 1)
        n_pcm = at + 8
    else:
        pitch = up8(int(length.max()) + 1)
        start = [8 + r * pitch for r in range(len(recs))]
        n_pcm = 8 + len(recs) * pitch
    buf = np.where(np.arange(n_pcm) % 2 == 0, 32767, -32767).astype(np.int16)
    for s, x in zip(start, recs):
        buf[s:s + len(x)] = x
    for s, n in zip(start, length):
        assert abs(int(buf[s - 1])) == 32767 and abs(int(buf[s + n])) == 32767  # sentinels directly before and after each span
    return torch.from_numpy(buf).to(DEV), np.array(start, np.int64), length


# ---- 1. frames -------------------------------------------------------------------------------------------------------
def frame_recordings():
    """The edge lengths of the front end: 1 sample, around one frame, no padded last frame (560), around one second (a length
    that is a multiple of 8 takes the vector route alone, one that is not the tile kernel's scalar loads), a straddling vector of
    1 and 7 samples (16001, 16007), every F mod 4 (the last chunk holds 1..4 frames; 19 / 20 / 21 frames sit around the five
    chunks a wavefront owns in a large batch -- in a batch this small mfcc_wr_chunks_per_wave gives every wavefront ONE chunk,
    so every chunk boundary is a share boundary; test_frames_with_two_chunks_per_wavefront covers longer shares), a full-scale 1
    kHz tone (every frame is flagged for the float64 refinement), zeros and full-scale noise."""
    rng = np.random.default_rng(5)
    lengths = [1, 399, 400, 401, 560, 16000, 16001, 16007, 16008, n_for_frames(19), n_for_frames(20, 3), n_for_frames(21), n_for_frames(22, 150)]
    assert sorted(sref.scan_shape(n, 1)[0] % 4 for n in lengths[-4:]) == [0, 1, 2, 3]
    assert [sref.scan_shape(n, 1)[0] for n in lengths[-4:-1]] == [19, 20, 21]
    recs = [np.round(rng.normal(0.0, 2500.0, n)).clip(-32768, 32767).astype(np.int16) for n in lengths]
    t = np.arange(16003)
    recs.insert(3, np.round(32767.0 * np.sin(2.0 * np.pi * 1000.0 * t / 16000.0)).astype(np.int16))  # the tone, at index 3
    recs.append(np.zeros(8000, np.int16))
    recs.append(rng.integers(-32768, 32768, 24000, dtype=np.int64).astype(np.int16))
    return recs


def frames_alone(ctx, rec):
    """(frames [F, 10] on the host, (frames counted, frames refined)) of kws_frames_i16 on one recording."""
    F, _ = sref.scan_shape(len(rec), 1)
    before = ctx.frontend_stats()
    feat = torch.full((2, F, N_CEP), float("nan"), device=DEV)
    ctx.frames_i16(torch.from_numpy(np.ascontiguousarray(rec)).to(DEV)[None], feat[:1])
    torch.cuda.synchronize()
    after = ctx.frontend_stats()
    assert torch.isnan(feat[1]).all()
    return feat[0].cpu().numpy(), (after[0] - before[0], after[1] - before[1])


def frames_ragged(ctx, buf, start, length, row_multiple):
    frames, frame_off, _, _, _ = _native.host_ragged_plan(length, FRAME_LEN, FRAME_STEP, T_WIN, row_multiple)
    F_pack = int(frame_off[-1])
    before = ctx.frontend_stats()
    feat = torch.full((F_pack + 1, N_CEP), float("nan"), device=DEV)
    ctx.frames_ragged_i16(buf, start, length, row_multiple, feat[:F_pack])
    torch.cuda.synchronize()
    after = ctx.frontend_stats()
    assert torch.isnan(feat[F_pack]).all(), "frames were written beyond [F_pack, numcep]"
    return feat[:F_pack].cpu().numpy(), frames, frame_off, (after[0] - before[0], after[1] - before[1])


def check_frames(got, frames, frame_off, alone):
    for r, want in enumerate(alone):
        o, F = int(frame_off[r]), int(frames[r])
        assert want.shape[0] == F
        rows = got[o:o + F]
        bad = (u32(rows) != u32(want)).any(axis=1)
        assert not bad.any(), f"recording {r} ({F} frames): frames {np.flatnonzero(bad)[:8]} differ from kws_frames_i16 alone"
        pad = got[o + F:int(frame_off[r + 1])]
        assert (u32(pad) == 0).all(), f"recording {r}: the rounding rows are not zero"


@pytest.mark.parametrize("refine", [True, False])
def test_frames_equal_each_recording_alone(ctx, refine):
    recs = frame_recordings()
    ctx.set_frontend_refine(_native.FE_REFINE_SPAN_DEFAULT if refine else 0.0)
    try:
        singles = [frames_alone(ctx, x) for x in recs]
        alone = [s[0] for s in singles]
        counted, refined = sum(s[1][0] for s in singles), sum(s[1][1] for s in singles)
        assert (refined > 0) == refine, "the refinement leg is vacuous"
        for layout, row_multiple in (("packed", 1), ("rect", 1), ("packed", 3), ("rect", 7)):
            buf, start, length = place(recs, layout)
            got, frames, frame_off, delta = frames_ragged(ctx, buf, start, length, row_multiple)
            check_frames(got, frames, frame_off, alone)
            assert delta == (counted, refined), "kws_frontend_stats differs from the per-recording calls' sum"
    finally:
        ctx.set_frontend_refine(_native.FE_REFINE_SPAN_DEFAULT)


def test_frames_with_two_chunks_per_wavefront(ctx):
    """More than 4096 chunks in the batch: mfcc_wr_chunks_per_wave hands every wavefront two chunks, so recordings with an odd and
    an even number of chunks and a last share of one chunk are all there (one long recording carries the count)."""
    rng = np.random.default_rng(6)
    lengths = [n_for_frames(4 * 4097), n_for_frames(19), n_for_frames(20), n_for_frames(21, 5), n_for_frames(28), n_for_frames(33, 1), 16001]
    recs = [np.round(rng.normal(0.0, 2500.0, n)).clip(-32768, 32767).astype(np.int16) for n in lengths]
    alone = [frames_alone(ctx, x)[0] for x in recs]
    buf, start, length = place(recs, "packed")
    got, frames, frame_off, _ = frames_ragged(ctx, buf, start, length, 1)
    check_frames(got, frames, frame_off, alone)


# ---- 2. scan -----------------------------------------------------------------------------------------------------------
def scan_recordings(clips):
    """Exactly one window, one frame more, shorter than a window between two longer ones, longer ones of odd length."""
    lengths = [n_for_frames(T_WIN), 40000, 8000, 33333, n_for_frames(T_WIN + 1, 7), 399]
    return [sref.mixed_recordings(1, n, clips, seed=20 + i)[0] for i, n in enumerate(lengths)]


def scan_alone(ctx, rec, hop):
    F, W = sref.scan_shape(len(rec), hop)
    logits = torch.full((1, W + 1, C), float("nan"), device=DEV)
    labels = torch.full((1, W + 1), -1, dtype=torch.int32, device=DEV)
    ctx.scan_i16(torch.from_numpy(np.ascontiguousarray(rec)).to(DEV)[None], hop, logits[:, :W], labels[:, :W])
    torch.cuda.synchronize()
    return logits[0, :W].cpu().numpy(), labels[0, :W].cpu().numpy()


def scan_ragged(ctx, recs, hop, layout, keep_frames):
    buf, start, length = place(recs, layout)
    _, frame_off, windows, win_off, W_pack = _native.host_ragged_plan(length, FRAME_LEN, FRAME_STEP, T_WIN, hop)
    logits = torch.full((W_pack + 1, C), float("nan"), device=DEV)
    labels = torch.full((W_pack + 1,), -1, dtype=torch.int32, device=DEV)
    feat = torch.full((int(frame_off[-1]), N_CEP), float("nan"), device=DEV) if keep_frames else None
    ctx.scan_ragged_i16(buf, start, length, hop, logits[:W_pack], labels[:W_pack], feat)
    torch.cuda.synchronize()
    assert torch.isnan(logits[W_pack]).all() and int(labels[W_pack]) == -1, "written beyond the packed windows"
    return logits.cpu().numpy(), labels.cpu().numpy(), windows, win_off


@pytest.mark.parametrize("hop", [1, 3, 7])
def test_scan_equals_each_recording_alone(ctx, clips, hop):
    recs = scan_recordings(clips)
    logits, labels, windows, win_off = scan_ragged(ctx, recs, hop, "packed" if hop != 3 else "rect", keep_frames=hop == 1)
    assert [int(w) for w in windows] == [sref.scan_shape(len(x), hop)[1] for x in recs]
    assert windows[0] == 1 and windows[2] == 0 and windows[5] == 0 and windows[4] == (2 if hop == 1 else 1)
    for r, rec in enumerate(recs):
        W, o = int(windows[r]), int(win_off[r])
        if W == 0:
            continue  # kws_scan_i16 refuses a recording shorter than a window
        want_logits, want_labels = scan_alone(ctx, rec, hop)
        assert np.array_equal(u32(logits[o:o + W]), u32(want_logits)), f"recording {r}: logits differ from kws_scan_i16 alone"
        assert np.array_equal(labels[o:o + W], want_labels)
    # R = 1
    one_logits, one_labels, windows, win_off = scan_ragged(ctx, recs[3:4], hop, "packed", keep_frames=False)
    want_logits, want_labels = scan_alone(ctx, recs[3], hop)
    assert win_off[0] == 0 and np.array_equal(u32(one_logits[:int(windows[0])]), u32(want_logits))
    assert np.array_equal(one_labels[:int(windows[0])], want_labels)


def test_a_batch_without_a_window_launches_no_model(ctx):
    rng = np.random.default_rng(9)
    recs = [rng.integers(-3000, 3000, n).astype(np.int16) for n in (8000, 100, 15000)]
    buf, start, length = place(recs, "packed")
    _, _, windows, _, W_pack = _native.host_ragged_plan(length, FRAME_LEN, FRAME_STEP, T_WIN, 1)
    assert windows.sum() == 0 and W_pack > 0, "the packed array has windows, all of them straddling"
    logits = torch.full((W_pack, C), float("nan"), device=DEV)
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        ctx.scan_ragged_i16(buf, start, length, 1, logits)
        assert ctx.prof_read(_native.KWS_K_MFCC)[1] == 1 and ctx.prof_read(_native.KWS_K_DSCNN)[1] == 0
    finally:
        ctx.prof_enable(False)
    torch.cuda.synchronize()
    assert torch.isnan(logits).all()


# ---- 3. decisions --------------------------------------------------------------------------------------------------------
def detect_alone(ctx, z, S, first_keyword, threshold, refractory, max_events):
    W = z.shape[0]
    count = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    ev_w = torch.full((1, max_events), -1, dtype=torch.int32, device=DEV)
    ev_k = torch.full((1, max_events), -1, dtype=torch.int32, device=DEV)
    ev_s = torch.zeros((1, max_events), device=DEV)
    sm = torch.full((1, W, C), float("nan"), device=DEV)
    ctx.scan_detect_f32(torch.from_numpy(z[None]).to(DEV), S, first_keyword, threshold, refractory, count, ev_w, ev_k, ev_s, max_events, sm)
    torch.cuda.synchronize()
    return int(count[0]), ev_w[0].cpu().numpy(), ev_k[0].cpu().numpy(), ev_s[0].cpu().numpy(), sm[0].cpu().numpy()


def run_detect_case(ctx, per_rec, gaps, S, refractory, max_events):
    """per_rec: logits [W_r, C] per recording (W_r may be 0); gaps[r]: packed rows of no recording ahead of recording r, filled
    with a strong keyword posterior -- a leak across a recording's first window would fire."""
    R = len(per_rec)
    win_off, at = [], 0
    for z, g in zip(per_rec, gaps):
        at += g
        win_off.append(at)
        at += z.shape[0]
    packed = np.zeros((at + 5, C), np.float32)
    packed[:, 5] = 30.0
    for o, z in zip(win_off, per_rec):
        packed[o:o + z.shape[0]] = z
    windows = [z.shape[0] for z in per_rec]
    count = torch.full((R + 1,), -1, dtype=torch.int32, device=DEV)
    ev_w = torch.full((R + 1, max_events), -1, dtype=torch.int32, device=DEV)
    ev_k = torch.full((R + 1, max_events), -1, dtype=torch.int32, device=DEV)
    ev_s = torch.zeros((R + 1, max_events), device=DEV)
    sm = torch.full((packed.shape[0], C), float("nan"), device=DEV)
    ctx.scan_detect_ragged_f32(torch.from_numpy(packed).to(DEV), win_off, windows, S, 2, 0.5, refractory, count[:R], ev_w[:R], ev_k[:R],
                               ev_s[:R], max_events, sm)
    torch.cuda.synchronize()
    assert int(count[R]) == -1 and (ev_w[R] == -1).all()
    count, ev_w, ev_k, ev_s, sm = count.cpu().numpy(), ev_w.cpu().numpy(), ev_k.cpu().numpy(), ev_s.cpu().numpy(), sm.cpu().numpy()
    owned = np.zeros(packed.shape[0], bool)
    fired_late = False
    for r, z in enumerate(per_rec):
        W, o = z.shape[0], win_off[r]
        owned[o:o + W] = True
        if W == 0:
            assert count[r] == 0 and (ev_w[r] == -1).all()
            continue
        want = detect_alone(ctx, z, S, 2, 0.5, refractory, max_events)
        assert count[r] == want[0], f"recording {r}: {count[r]} events, {want[0]} alone"
        assert np.array_equal(ev_w[r], want[1]) and np.array_equal(ev_k[r], want[2]) and np.array_equal(u32(ev_s[r]), u32(want[3]))
        assert np.array_equal(u32(sm[o:o + W]), u32(want[4])), f"recording {r}: smoothed posteriors differ"
        fired_late |= r > 0 and want[0] > 0
    assert np.isnan(sm[~owned]).all(), "a row of no recording was written"
    return count, fired_late


@pytest.mark.parametrize("S", [1, 8, 256])
@pytest.mark.parametrize("refractory", [1, 50])
def test_detect_equals_each_recording_alone(ctx, S, refractory):
    z = sref.detect_logits(200, C, sref.DETECT_SEEDS[(200, C)])
    per_rec = [z[0], z[1][:65], np.zeros((0, C), np.float32), z[2][:1], z[2][:64], z[1]]
    count, fired_late = run_detect_case(ctx, per_rec, [3, 98, 98, 0, 98, 14], S, refractory, max_events=4)
    assert fired_late, "no event in a recording of index > 0"
    if refractory == 1:
        assert count.max() > 4, "no recording has more events than max_events"


def test_detect_sixty_five_recordings(ctx):
    z = sref.detect_logits(200, C, sref.DETECT_SEEDS[(200, C)])
    per_rec = [z[r % 3][(5 * r) % 90:(5 * r) % 90 + (7 * r) % 41] for r in range(65)]
    assert sum(x.shape[0] == 0 for x in per_rec) >= 2
    _, fired_late = run_detect_case(ctx, per_rec, [(3 * r) % 5 for r in range(65)], 8, 5, max_events=8)
    assert fired_late


# ---- 4. segment ------------------------------------------------------------------------------------------------------------
SEG_THRESHOLD = -6.0  # log frame energy: the floor of +-3 LSB lies near -13, a burst of sigma 3000 near +1
# (seed, bursts, length): two utterances; ends inside an utterance (reason 2); a burst longer than the time-out (reason 1);
# 22 frames, fewer than on_window = 40; 2 frames, fewer than on_window = 3; an odd length with one utterance
SEG_RECIPES = [(7, [(9000, 21000), (30000, 52000)], 64000), (8, [(4000, 15000), (30000, 40001)], 40001), (9, [(5000, 45000)], 50003),
               (10, [(500, 3000)], n_for_frames(22)), (11, [], 500), (12, [(8000, 20000)], 31111)]
SEG_MAX_FRAMES = 120


def seg_recordings():
    return [gref.recipe_recording(seed, bursts, n) for seed, bursts, n in SEG_RECIPES]


def test_the_segment_recipes_hold_utterances_on_the_cpu():
    """Without a GPU's help: walk_ref over the oracle's frames says what the recipes were chosen for."""
    for pair in gref.E2E_PAIRS:
        reasons = []
        for i, rec in enumerate(seg_recordings()):
            c0 = gref.oracle_frames(rec[None])[0, :, 0]
            utts = gref.walk_ref(gref.voiced_flags(c0, SEG_THRESHOLD), pair[0], pair[1], 60, SEG_MAX_FRAMES, len(rec))
            reasons.append([u[4] for u in utts])
        assert len(reasons[0]) >= 2 and reasons[1][-1] == 2 and 1 in reasons[2] and reasons[4] == [] and len(reasons[5]) >= 1, (pair, reasons)
        if pair[0] == 40:
            assert reasons[3] == []  # fewer frames than on_window


@pytest.mark.parametrize("pair", gref.E2E_PAIRS)
@pytest.mark.parametrize("max_utts", [1, 8])
def test_segment_equals_each_recording_alone(ctx, pair, max_utts):
    recs = seg_recordings()
    buf, start, length = place(recs, "packed")
    feat, frames, frame_off, _ = frames_ragged(ctx, buf, start, length, 3)
    R = len(recs)
    d_feat = torch.from_numpy(feat).to(DEV)
    count = torch.full((R + 1,), -1, dtype=torch.int32, device=DEV)
    utt = torch.full((R + 1, max_utts, 5), -1, dtype=torch.int32, device=DEV)
    ctx.segment_ragged_f32(d_feat, frame_off, frames, length, SEG_THRESHOLD, count[:R], utt[:R], max_utts, pair[0], pair[1], 60, SEG_MAX_FRAMES)
    torch.cuda.synchronize()
    assert int(count[R]) == -1 and (utt[R] == -1).all()
    count, utt = count.cpu().numpy(), utt.cpu().numpy()
    seen = set()
    for r, rec in enumerate(recs):
        o, F = int(frame_off[r]), int(frames[r])
        own = np.ascontiguousarray(feat[o:o + F])
        c1 = torch.full((1,), -1, dtype=torch.int32, device=DEV)
        u1 = torch.full((1, max_utts, 5), -1, dtype=torch.int32, device=DEV)
        ctx.segment_f32(torch.from_numpy(own[None]).to(DEV), len(rec), SEG_THRESHOLD, c1, u1, max_utts, pair[0], pair[1], 60, SEG_MAX_FRAMES)
        torch.cuda.synchronize()
        assert count[r] == int(c1[0]) and np.array_equal(utt[r], u1[0].cpu().numpy()), f"recording {r} differs from kws_segment_f32 alone"
        want = gref.walk_ref(gref.voiced_flags(own[:, 0], SEG_THRESHOLD), pair[0], pair[1], 60, SEG_MAX_FRAMES, len(rec))
        assert count[r] == len(want) and [tuple(int(v) for v in row) for row in utt[r, :min(len(want), max_utts)]] == want[:max_utts]
        assert all(0 <= s < e <= len(rec) for s, e, _, _, _ in want), "spans are relative to the recording's own start"
        seen |= {u[4] for u in want}
        if r == 0:
            assert len(want) >= 2  # more utterances than max_utts = 1
    assert seen == {0, 1, 2}


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spotter(e2e_golden):
    from kws.inference import KeywordSpotter
    from kws.libs.models import DepthwiseSeparableConv

    model = DepthwiseSeparableConv(num_classes=C)
    model.load_state_dict(sref.state_from_blob(e2e_golden["he.blob"]))
    return KeywordSpotter(model)


def _wav(path, x, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.asarray(x, "<i2").tobytes())
    return str(path)


def e2e_recordings(clips):
    """(samples, rate): the configured rate, two files at 8 kHz of different length (one resample launch with d_len), one at 48
    kHz, and one at the configured rate that is shorter than a window."""
    return [(gref.recipe_recording(7, [(9000, 21000), (25000, 36000)], 40000), 16000),
            (np.concatenate([clips[8], clips[20]])[::2].copy(), 8000),
            (gref.recipe_recording(8, [(12000, 40000)], 60001), 48000),
            (gref.recipe_recording(9, [(1000, 4000)], 5000), 16000),
            (gref.recipe_recording(10, [(2000, 7000)], 11111), 8000)]


def same_scan(a, b):
    return (np.array_equal(a.labels, b.labels) and np.array_equal(u32(a.logits), u32(b.logits)) and a.logits.shape == b.logits.shape
            and np.array_equal(a.window_start_s, b.window_start_s) and a.events == b.events)


def same_utts(a, b, recording):
    return len(a) == len(b) and all(
        (x.recording, x.start_s, x.end_s, x.open_s, x.close_s, x.reason, x.label, x.word, x.peak) ==
        (recording, y.start_s, y.end_s, y.open_s, y.close_s, y.reason, y.label, y.word, y.peak) and np.array_equal(u32(x.logits), u32(y.logits))
        for x, y in zip(a, b))


def test_scan_batch_and_files_equal_the_single_recording_methods(spotter, clips, tmp_path):
    from kws.common.errors import ModelError

    recs = e2e_recordings(clips)
    kw = dict(hop_frames=3, smooth_window=3, threshold=0.15, refractory=4, first_keyword=2, max_events=16)
    got = spotter.scan_batch([torch.from_numpy(x).to(DEV) if i == 2 else x for i, (x, _) in enumerate(recs)],
                             sample_rate=[r for _, r in recs], **kw)
    paths = [_wav(tmp_path / f"r{i}.wav", x, rate) for i, (x, rate) in enumerate(recs)]
    from_files = spotter.scan_files(paths, resample=True, **kw)
    assert len(got) == len(from_files) == len(recs)
    n_events = 0
    for i, (x, rate) in enumerate(recs):
        if i == 3:  # shorter than a window: zero windows instead of the single method's refusal
            with pytest.raises(ModelError, match="shorter than one window"):
                spotter.scan(x, sample_rate=rate, **kw)
            for res in (got[i], from_files[i]):
                assert res.labels.shape == (1, 0) and res.logits.shape == (1, 0, C) and res.window_start_s.shape == (0,) and res.events == [[]]
            continue
        want = spotter.scan(x, sample_rate=rate, **kw)
        assert same_scan(got[i], want), f"scan_batch: recording {i} differs from scan"
        assert same_scan(from_files[i], spotter.scan_file(paths[i], resample=True, **kw)), f"scan_files: file {i} differs from scan_file"
        n_events += len(want.events[0])
    assert n_events > 0
    no_events = spotter.scan_batch([recs[0][0], recs[3][0]], hop_frames=7)
    assert no_events[0].events is None and same_scan(no_events[0], spotter.scan(recs[0][0], hop_frames=7))


def test_segment_batch_and_files_equal_the_single_recording_methods(spotter, clips, tmp_path):
    recs = e2e_recordings(clips)
    kw = dict(threshold=SEG_THRESHOLD, on_window=3, off_window=5, pre_roll=20, max_seconds=1.5)
    got = spotter.segment_batch([x for x, _ in recs], sample_rate=[r for _, r in recs], **kw)
    paths = [_wav(tmp_path / f"s{i}.wav", x, rate) for i, (x, rate) in enumerate(recs)]
    from_files = spotter.segment_files(paths, resample=True, **kw)
    total = 0
    for i, (x, rate) in enumerate(recs):
        want = spotter.segment(x, sample_rate=rate, **kw)[0]
        assert same_utts(got[i], want, i), f"segment_batch: recording {i} differs from segment"
        assert same_utts(from_files[i], spotter.segment_file(paths[i], resample=True, **kw), i)
        total += len(want)
    assert total >= 4 and sum(len(g) > 0 for g in got) >= 3
    dropped = spotter.segment_batch([recs[0][0]], keep_unfinished=False, max_utterances=1, **kw)
    assert same_utts(dropped[0], spotter.segment(recs[0][0], keep_unfinished=False, max_utterances=1, **kw)[0], 0)


def test_cut_over_the_shared_buffer_equals_the_cut_per_recording(ctx):
    rng = np.random.default_rng(13)
    recs = [rng.integers(-20000, 20000, n).astype(np.int16) for n in (40000, 5001, 23456)]
    spans = [(0, 100, 30000), (0, 0, 40000), (1, 4000, 5001), (1, 17, 400), (2, 23000, 23456), (2, 1, 23455)]
    buf, start, _ = place(recs, "packed")
    shifted = torch.tensor([(0, int(start[r]) + a, int(start[r]) + b) for r, a, b in spans], dtype=torch.int32, device=DEV)
    clips = torch.full((len(spans) + 1, 16000), -1, dtype=torch.int16, device=DEV)
    peaks = torch.full((len(spans) + 1,), -7, dtype=torch.int32, device=DEV)
    ctx.cut_i16(buf[None], shifted, clips[:-1], 16384, peaks[:-1])
    torch.cuda.synchronize()
    assert (clips[-1] == -1).all() and int(peaks[-1]) == -7
    for u, (r, a, b) in enumerate(spans):
        c1 = torch.full((1, 16000), -1, dtype=torch.int16, device=DEV)
        p1 = torch.full((1,), -7, dtype=torch.int32, device=DEV)
        ctx.cut_i16(torch.from_numpy(recs[r]).to(DEV)[None], torch.tensor([(0, a, b)], dtype=torch.int32, device=DEV), c1, 16384, p1)
        torch.cuda.synchronize()
        assert torch.equal(clips[u], c1[0]) and int(peaks[u]) == int(p1[0]), f"span {u}"


# ---- 6. one host path, two layouts ---------------------------------------------------------------------------------------------
LAY_R, LAY_W, LAY_F = 3, 130, 300            # 130 windows: two chunks of 64 of the walk and two more; 300 frames: past one 256-frame workgroup
LAY_SEG = dict(on=3, off=5, pre_roll=2, max_frames=40, max_utts=8)


def layout_flags():
    """Voiced flags [3, 300]: a short utterance and one longer than the time-out; one that runs to the end; one of each."""
    v = np.zeros((LAY_R, LAY_F), np.int64)
    v[0, 20:50] = v[0, 100:200] = 1
    v[1, 250:] = 1
    v[2, 60:70] = v[2, 280:] = 1
    return v


def test_the_layout_flags_close_for_every_reason_on_the_cpu():
    n = n_for_frames(LAY_F)
    reasons = [{u[4] for u in gref.walk_ref(v, LAY_SEG["on"], LAY_SEG["off"], LAY_SEG["pre_roll"], LAY_SEG["max_frames"], n)} for v in layout_flags()]
    assert reasons[0] >= {0, 1} and 2 in reasons[1] and reasons[2] == {0, 2}, reasons


def packed_rows(per_rec, first, gap, tail=4):
    """[R, n, ...] -> (packed [rows, ...] with NaN rows ahead of, between and behind the recordings, the first row of each)."""
    R, n = per_rec.shape[:2]
    off = [first + r * (n + gap) for r in range(R)]
    packed = torch.full((off[-1] + n + tail,) + tuple(per_rec.shape[2:]), float("nan"), device=DEV)
    for r, o in enumerate(off):
        packed[o:o + n] = per_rec[r]
    return packed, off


@pytest.mark.parametrize("S", [1, 7])
@pytest.mark.parametrize("Cn", [12, 64])
def test_equal_and_ragged_layouts_agree(ctx, Cn, S):
    """The same values through the equal-length entry and, packed with first != 0 and NaN rows between the recordings, through
    its ragged twin: every output equal bit for bit, no row of no recording written."""
    R, W, M = LAY_R, LAY_W, 8
    gen = torch.Generator().manual_seed(100 * Cn + S)
    z = (3.0 * torch.randn((R, W, Cn), generator=gen)).to(DEV)
    packed, off = packed_rows(z, 5, 9)
    assert off == [5, 5 + 130 + 9, 5 + 2 * (130 + 9)]
    windows = [W] * R
    ints = lambda *shape: torch.full(shape, -1, dtype=torch.int32, device=DEV)
    # decisions
    a = dict(count=ints(R), w=ints(R, M), k=ints(R, M), s=torch.zeros((R, M), device=DEV), sm=torch.full((R, W, Cn), float("nan"), device=DEV))
    b = dict(count=ints(R), w=ints(R, M), k=ints(R, M), s=torch.zeros((R, M), device=DEV), sm=torch.full_like(packed, float("nan")))
    ctx.scan_detect_f32(z, S, 2, 1.5 / Cn, 4, a["count"], a["w"], a["k"], a["s"], M, a["sm"])
    ctx.scan_detect_ragged_f32(packed, off, windows, S, 2, 1.5 / Cn, 4, b["count"], b["w"], b["k"], b["s"], M, b["sm"])
    torch.cuda.synchronize()
    assert int(a["count"].min()) > M, "every recording fires more often than max_events"
    for key in ("count", "w", "k"):
        assert torch.equal(a[key], b[key]), key
    assert torch.equal(a["s"].view(torch.int32), b["s"].view(torch.int32))
    owned = torch.zeros(packed.shape[0], dtype=torch.bool, device=DEV)
    for r, o in enumerate(off):
        owned[o:o + W] = True
        assert torch.equal(a["sm"][r].view(torch.int32), b["sm"][o:o + W].view(torch.int32)), f"recording {r}: smoothed posteriors differ"
    assert torch.isnan(b["sm"][~owned]).all(), "a row of no recording was written"
    # scores: five thresholds, the one above among them, and a dozen annotations around the first four events of each recording
    # (events lie 4 windows apart, so no two rows overlap): hits at the third threshold, false alarms everywhere
    th = (np.array([0.5, 1.0, 1.5, 2.0, 3.0]) / Cn).astype(np.float32)
    ev_w, ev_k = a["w"].cpu().numpy(), a["k"].cpu().numpy()
    truth = np.array([(r, ev_k[r, i], max(ev_w[r, i] - 1, 0), ev_w[r, i] + 1) for r in range(R) for i in range(4)], np.int32)
    ca = torch.full((5, Cn, 4), -7, dtype=torch.int64, device=DEV)
    cb = torch.full((5, Cn, 4), -7, dtype=torch.int64, device=DEV)
    ctx.scan_score_f32(z, S, 2, 4, th, truth, ca)
    ctx.scan_score_ragged_f32(packed, off, windows, S, 2, 4, th, truth, cb)
    torch.cuda.synchronize()
    assert torch.equal(ca, cb) and int(ca[..., 0].sum()) > 0 and int(ca[..., 1].sum()) > 0, "hits and false alarms, the same"
    # utterances
    p = LAY_SEG
    n = n_for_frames(LAY_F)
    feat = torch.from_numpy(gref.frames_from_flags(layout_flags(), N_CEP, seed=Cn + S)).to(DEV)
    assert feat.shape == (R, LAY_F, N_CEP)
    fpacked, foff = packed_rows(feat, 4, 7)
    ua, ub = (ints(R), ints(R, p["max_utts"], 5)), (ints(R), ints(R, p["max_utts"], 5))
    ctx.segment_f32(feat, n, 0.0, ua[0], ua[1], p["max_utts"], p["on"], p["off"], p["pre_roll"], p["max_frames"])
    ctx.segment_ragged_f32(fpacked, foff, [LAY_F] * R, [n] * R, 0.0, ub[0], ub[1], p["max_utts"], p["on"], p["off"], p["pre_roll"], p["max_frames"])
    torch.cuda.synchronize()
    assert torch.equal(ua[0], ub[0]) and torch.equal(ua[1], ub[1])
    counts, slots = ua[0].cpu().numpy(), ua[1].cpu().numpy()
    assert {int(slots[r, i, 4]) for r in range(R) for i in range(min(int(counts[r]), p["max_utts"]))} == {0, 1, 2}


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx, e2e_golden):
    import ctypes as Ct

    lib = ctx._lib
    buf = torch.zeros(4096, dtype=torch.int16, device=DEV)
    feat = torch.full((64, N_CEP), float("nan"), device=DEV)
    logits = torch.full((64, C), float("nan"), device=DEV)
    i64 = lambda *v: (Ct.c_int64 * len(v))(*v)
    i32 = lambda *v: (Ct.c_int32 * len(v))(*v)
    last = lambda c=ctx: lib.kws_last_error(c._h).decode()
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        frames = lambda pcm, n_pcm, start, length, R, mult=1, out=feat.data_ptr(): lib.kws_frames_ragged_i16(
            ctx._h, pcm, n_pcm, start, length, R, mult, out)
        scan = lambda pcm, n_pcm, start, length, R, hop=1, out=logits.data_ptr(): lib.kws_scan_ragged_i16(
            ctx._h, pcm, n_pcm, start, length, R, hop, out, None, None)
        for entry, name in ((frames, "kws_frames_ragged_i16"), (scan, "kws_scan_ragged_i16")):
            cases = [(lambda: entry(buf.data_ptr(), 4096, i64(0, 1004), i32(1000, 1000), 2), "multiple of 8"),   # a misaligned start
                     (lambda: entry(buf.data_ptr(), 4096, i64(0, 3200), i32(1000, 897), 2), "runs past"),         # a span past n_pcm
                     (lambda: entry(buf.data_ptr(), 4096, i64(0, -8), i32(1000, 8), 2), "multiple of 8"),
                     (lambda: entry(buf.data_ptr(), 4096, i64(0, 1000), i32(1000, 0), 2), "no samples"),
                     (lambda: entry(None, 4096, i64(0), i32(1000), 1), "NULL"),
                     (lambda: entry(buf.data_ptr(), 4096, None, i32(1000), 1), "NULL"),
                     (lambda: entry(buf.data_ptr(), 4096, i64(0), i32(1000), 1, 1, None), "NULL"),
                     (lambda: entry(buf.data_ptr() + 2, 4094, i64(0), i32(1000), 1), "16-byte"),
                     (lambda: entry(buf.data_ptr(), 4096, i64(0), i32(1000), 0), "positive"),
                     (lambda: entry(buf.data_ptr(), 4096, i64(0), i32(1000), 1, 0), "positive")]
            for k, (call, word) in enumerate(cases):
                assert call() == _native.KWS_EINVAL, (name, k)
                assert name in last() and word in last(), (name, k, last())  # each refusal leaves its text behind
        assert frames(buf.data_ptr(), 4096, i64(0, 1004), i32(1000, 1000), 2) == _native.KWS_EINVAL
        assert "kws_frames_ragged_i16" in last() and "recording 1" in last() and "multiple of 8" in last()
        assert scan(buf.data_ptr(), 4096, i64(0, 3200), i32(1000, 897), 2) == _native.KWS_EINVAL
        assert "kws_scan_ragged_i16" in last() and "recording 1 runs past" in last()
        assert frames(buf.data_ptr(), (1 << 30) + 8, i64(0), i32(1000), 1) == _native.KWS_EUNSUPPORTED and "2^30" in last()
        # the float64 front end is a refused route
        ctx.set_frontend_math(_native.FE_F64)
        try:
            assert frames(buf.data_ptr(), 4096, i64(0), i32(1000), 1) == _native.KWS_EUNSUPPORTED and "KWS_FE_F32" in last()
        finally:
            ctx.set_frontend_math(_native.FE_F32)
        # no model: KWS_ESTATE from the scan, while the frames need none
        bare = _native.Context(0)
        try:
            bare.use_torch_stream()
            rc = lib.kws_scan_ragged_i16(bare._h, buf.data_ptr(), 4096, i64(0), i32(1000), 1, 1, logits.data_ptr(), None, None)
            assert rc == _native.KWS_ESTATE and "model not configured" in last(bare)
        finally:
            bare.close()
        # the decisions' and the endpointer's own table checks
        count = torch.full((2,), -1, dtype=torch.int32, device=DEV)
        rc = lib.kws_scan_detect_ragged_f32(ctx._h, logits.data_ptr(), i32(0, 5), i32(10, 3), 2, C, 1, 2, 0.5, 1, None, None, None, None, 0,
                                            count.data_ptr())
        assert rc == _native.KWS_EINVAL and "overlap" in last()
        rc = lib.kws_segment_ragged_f32(ctx._h, feat.data_ptr(), i32(0, 5), i32(10, 3), i32(1000, 1000), 2, 0.0, 3, 5, 0, 0, None, 0,
                                        count.data_ptr())
        assert rc == _native.KWS_EINVAL and "overlap" in last()
        rc = lib.kws_segment_ragged_f32(ctx._h, feat.data_ptr(), None, i32(10, 3), i32(1000, 1000), 2, 0.0, 3, 5, 0, 0, None, 0, count.data_ptr())
        assert rc == _native.KWS_EINVAL and "NULL" in last()
        for k in (_native.KWS_K_MFCC, _native.KWS_K_MFCC_REFINE, _native.KWS_K_MFCC_F64, _native.KWS_K_DSCNN):
            assert ctx.prof_read(k)[1] == 0, "a refused call launched a kernel"
    finally:
        ctx.prof_enable(False)
    torch.cuda.synchronize()
    assert torch.isnan(feat).all() and torch.isnan(logits).all() and (count == -1).all()
