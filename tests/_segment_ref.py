"""Expectations shared by tests/test_segment_cpu.py and tests/test_segment_gpu.py (not a test module): the NumPy restatement of
``kws_segment_f32``'s walk and of ``kws_cut_i16``, the flag tracks and cases the walk is tested on, the recordings of the
end-to-end test and their float64 oracle expectation."""
import numpy as np

from _scan_ref import FRAME_LEN, FRAME_STEP, N_CEP, scan_shape, state_from_blob  # noqa: F401  (re-exported)

WINDOW_PAIRS = [(1, 1), (3, 5), (40, 80), (64, 64), (65, 130), (5, 1024)]
REASONS = ("endpoint", "max_length", "end_of_recording")


# ---- the walk -------------------------------------------------------------------------------------------------------
def voiced_flags(c0, threshold):
    """float32 compare, strict; a NaN is unvoiced."""
    with np.errstate(invalid="ignore"):
        return (np.asarray(c0, np.float32) > np.float32(threshold)).astype(np.int64)


def window_counts(v, window):
    """c[f] = voiced frames among the last `window` frames ending at f (frames before 0 are unvoiced): cumulative sums."""
    c = np.concatenate([[0], np.cumsum(v)])
    f = np.arange(len(v))
    return c[f + 1] - c[np.maximum(0, f + 1 - window)]


def walk_ref(v, on_window, off_window, pre_roll, max_frames, n_total, frame_len=FRAME_LEN, frame_step=FRAME_STEP):
    """The definition of include/kws_hip.h, frame by frame: every utterance (start_sample, end_sample, open, close, reason) of
    one recording's voiced flags v, however many there are."""
    F = len(v)
    c_on, c_off = window_counts(v, on_window), window_counts(v, off_window)
    out, triggered, opened, prev_close = [], False, 0, -1

    def close(f, reason):
        nonlocal triggered, prev_close
        start_frame = max(opened - pre_roll, prev_close + 1, 0)
        out.append((start_frame * frame_step, min(n_total, f * frame_step + frame_len), opened, f, reason))
        prev_close, triggered = f, False

    for f in range(F):
        if not triggered:
            if 10 * c_on[f] > 8 * on_window:
                triggered, opened = True, f
                if f == F - 1:
                    close(f, 2)
            continue
        if 10 * (off_window - c_off[f]) > 9 * off_window:
            close(f, 0)
        elif max_frames > 0 and f - opened + 1 >= max_frames:
            close(f, 1)
        elif f == F - 1:
            close(f, 2)
    return out


def endpointer_events(c0, threshold, on_window, off_window):
    """(opens, closes) of oracle.endpointer.EnergyEndpointer fed the column hop by hop."""
    from oracle.endpointer import EnergyEndpointer

    ep = EnergyEndpointer(threshold, on_window, off_window)
    opens, closes = [], []
    for f, e in enumerate(c0):
        _, event = ep.update(float(e))
        if event == 1:
            opens.append(f)
        elif event == 2:
            closes.append(f)
    return opens, closes


def flag_track(F, seed, mean_run=None):
    """Random run-length flags with 5 % flips: alternating runs of 1 .. 2 * mean_run frames, then every twentieth frame or so
    inverted, so that counts hover around both hysteresis thresholds."""
    rng = np.random.default_rng(seed)
    mean_run = mean_run or max(2, F // 6)
    v = np.empty(F, np.int64)
    f, state = 0, int(rng.integers(0, 2))
    while f < F:
        n = int(rng.integers(1, 2 * mean_run + 1))
        v[f:f + n] = state
        state ^= 1
        f += n
    flip = rng.random(F) < 0.05
    return np.where(flip, 1 - v, v)


def frames_from_flags(v, numcep, seed, threshold=0.0):
    """float32 [R, F, numcep]: column 0 at threshold +- 1 by the flags, the other columns random (they must not be read)."""
    rng = np.random.default_rng(seed)
    v = np.asarray(v)
    feat = rng.normal(0.0, 5.0, size=v.shape + (numcep,)).astype(np.float32)
    feat[..., 0] = np.where(v > 0, threshold + 1.0, threshold - 1.0)
    return feat


# The walk cases of the GPU test: (F, window pair, (seed per recording, R = 3)), chosen on the CPU so that, over the parameter
# sweep of the test, the reference's own answer covers what test_walk_matches_the_reference asserts (test_segment_cpu.py checks
# the same conditions without a GPU).  A seed of -1 is an all-unvoiced recording, -2 an all-voiced one.
WALK_FRAMES = [1, 63, 64, 65, 129, 700]
WALK_PRE_ROLLS = [0, 60, 10000]
WALK_MAX_FRAMES = [0, 2, 50]
WALK_MAX_UTTS = [0, 1, 3, 1024]


def walk_n_total(F):
    """A recording of F frames whose last frame is zero-padded by 77 samples: the last frame's end is clipped to n_total."""
    return (F - 1) * FRAME_STEP + FRAME_LEN - 77


def walk_flags(F, seeds, pair):
    rows = []
    for s in seeds:
        if s == -1:
            rows.append(np.zeros(F, np.int64))
        elif s == -2:
            rows.append(np.ones(F, np.int64))
        else:
            rows.append(flag_track(F, s, mean_run=max(2, min(F // 6, 2 * pair[1]))))
    return np.stack(rows)


def walk_seeds(F, pair):
    """Three recordings per case: two random tracks and one edge track."""
    base = 1000 * WALK_FRAMES.index(F) + 10 * WINDOW_PAIRS.index(pair)
    return (base + 1, base + 2, -2 if (WALK_FRAMES.index(F) + WINDOW_PAIRS.index(pair)) % 2 else -1)


def coverage_of(utts, F, max_utts, pre_roll):
    """The coverage facts one recording's reference answer contributes (a set of names)."""
    got = set()
    if not utts:
        got.add("no_utterance")
    if len(utts) > max_utts > 0:
        got.add("count_above_max_utts")
    prev_close = -1
    for (_, _, o, c, reason) in utts:
        if o % 64 == 0:
            got.add("open_at_0_mod_64")
        if o % 64 == 63:
            got.add("open_at_63_mod_64")
        if c % 64 == 0:
            got.add("close_at_0_mod_64")
        if c % 64 == 63:
            got.add("close_at_63_mod_64")
        got.add(f"reason_{reason}")
        if o == F - 1:
            got.add("open_at_last_frame")
        if prev_close + 1 > max(o - pre_roll, 0):
            got.add("start_limited_by_prev_close")
        prev_close = c
    return got


COVERAGE = {"no_utterance", "count_above_max_utts", "open_at_0_mod_64", "open_at_63_mod_64", "close_at_0_mod_64", "close_at_63_mod_64",
            "reason_0", "reason_1", "reason_2", "open_at_last_frame", "start_limited_by_prev_close"}


# ---- the cut --------------------------------------------------------------------------------------------------------
def cut_ref(pcm, spans, normalize_to, n_out):
    """(clips int16 [U, n_out], peak int32 [U]) of kws_cut_i16 in NumPy: float64 divide, float64 multiply, np.trunc."""
    R, n_total = pcm.shape
    clips = np.zeros((len(spans), n_out), np.int16)
    peaks = np.zeros(len(spans), np.int32)
    for u, (r, start, end) in enumerate(spans):
        if not 0 <= r < R:
            peaks[u] = -1
            continue
        start, end = min(max(int(start), 0), n_total), min(max(int(end), 0), n_total)
        x = pcm[r, start:max(start, end)].astype(np.int64)
        peak = int(np.abs(x).max()) if len(x) else 0
        peaks[u] = peak
        if normalize_to > 0:
            y = np.trunc(x.astype(np.float64) * (float(normalize_to) / float(peak))) if peak > 0 else np.zeros(len(x))
        else:
            y = x
        n = min(len(x), n_out)
        clips[u, :n] = y[:n].astype(np.int16)
    return clips, peaks


def normalize_literal(snd_data, maximum=16384):
    """The reference's normalize (kws/inference/inference_local.py:102-109), sample by sample in Python numbers."""
    samples = [int(i) for i in snd_data]
    times = float(maximum) / max(abs(i) for i in samples)
    return np.array([int(i * times) for i in samples], np.int64)


# ---- recordings -----------------------------------------------------------------------------------------------------
RECIPE_N = 64000
# (seed, bursts): the recordings of the end-to-end test
RECIPES = [(7, [(9000, 21000), (30000, 52000)]), (8, [(4000, 15000), (24000, 31000), (40000, 60000)])]
E2E_PAIRS = [(3, 5), (40, 80)]


def recipe_recording(seed, bursts, n=RECIPE_N):
    """int16 [n]: a floor of integers in [-3, 3], bursts of round(N(0, 3000)) over the given sample ranges."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, n).astype(np.int64)
    for a, b in bursts:
        x[a:b] = np.round(rng.normal(0.0, 3000.0, b - a)).astype(np.int64)
    return np.clip(x, -32768, 32767).astype(np.int16)


def recipe_recordings():
    return np.stack([recipe_recording(s, b) for s, b in RECIPES])


def frame_kinds(bursts, F, n=RECIPE_N):
    """Per frame: 1 all burst, 0 all floor, -1 straddling (by the samples [f * step, f * step + len) inside the recording)."""
    inside = np.zeros(n + FRAME_LEN + FRAME_STEP, bool)
    for a, b in bursts:
        inside[a:b] = True
    kind = np.empty(F, np.int64)
    for f in range(F):
        s = inside[f * FRAME_STEP:min(n, f * FRAME_STEP + FRAME_LEN)]
        kind[f] = 1 if s.all() else (0 if not s.any() else -1)
    return kind


def oracle_frames(recs):
    """float64 [R, F, 10]: psf's MFCC of each recording as one clip."""
    from oracle import psf_mfcc as o_mfcc

    spec = o_mfcc.FrontendSpec(n_samples=recs.shape[1])
    return np.stack([o_mfcc.extract_features_pcm16(rec, spec) for rec in recs])


def recipe_threshold(c0, kinds):
    """Midway between the quietest all-burst frame and the loudest all-floor frame, over all recordings."""
    return 0.5 * (min(c[k == 1].min() for c, k in zip(c0, kinds)) + max(c[k == 0].max() for c, k in zip(c0, kinds)))


def oracle_clip_logits(clips, blob):
    """float64 [U, C]: oracle.psf_mfcc -> oracle.dscnn on int16 clips of one second."""
    import torch
    from oracle import dscnn as o_dscnn
    from oracle import psf_mfcc as o_mfcc

    feats = torch.from_numpy(o_mfcc.collate_pcm16(np.ascontiguousarray(clips)))
    return o_dscnn.forward(state_from_blob(blob), feats.double()).numpy()
