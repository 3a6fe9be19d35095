"""Expectations shared by tests/test_live_cpu.py and tests/test_live_gpu.py (not a test module): the live utterance walk of
``kws_stream_utt_*`` restated hop by hop in Python (``LiveRef``), the cases the device is tested on, and copies of the small PCM
pattern builders of the streaming decision tests.  The whole-signal definitions stay where they are: ``walk_ref`` / ``cut_ref``
in _segment_ref.py, the resampled signal in _resample_stream_ref.py."""
import numpy as np

from _segment_ref import FRAME_LEN, FRAME_STEP, WINDOW_PAIRS, cut_ref, flag_track, walk_flags, walk_ref, walk_seeds  # noqa: F401

FAR = 1 << 62            # an n_total beyond reach: a live span is never clipped
LAG = -(-FRAME_LEN // FRAME_STEP)
THR = -10.0              # silence sits at log(eps) = -36, a frame that holds any noise far above 0 (test_stream_decisions_gpu.py)


def history(pre_roll, max_frames, slack_hops=0, frame_len=FRAME_LEN, frame_step=FRAME_STEP):
    """kws_host_stream_utt_history's formula."""
    return (pre_roll + max_frames - 1 + -(-frame_len // frame_step) + slack_hops) * frame_step


class LiveRef:
    """The step kernel's walk for S streams in lockstep, one frame per ``step``: O(1) window counts over a flag history, the
    rules of kws_segment_f32, records (stream, start_sample, end_sample, open, close, reason) in ascending stream order."""

    def __init__(self, n_streams, on_window, off_window, pre_roll, max_frames, frame_len=FRAME_LEN, frame_step=FRAME_STEP):
        self.S, self.on, self.off, self.pre_roll, self.max_frames = n_streams, on_window, off_window, pre_roll, max_frames
        self.frame_len, self.frame_step = frame_len, frame_step
        self.flags = [[] for _ in range(n_streams)]
        self.c_on, self.c_off = [0] * n_streams, [0] * n_streams
        self.trig, self.open, self.prev_close = [False] * n_streams, [-1] * n_streams, [-1] * n_streams
        self.frames = 0

    def _close(self, s, f, reason):
        start_frame = max(self.open[s] - self.pre_roll, self.prev_close[s] + 1, 0)
        rec = (s, start_frame * self.frame_step, f * self.frame_step + self.frame_len, self.open[s], f, reason)
        self.prev_close[s], self.trig[s] = f, False
        return rec

    def step(self, voiced):
        f, out = self.frames, []
        for s in range(self.S):
            v, fl = int(voiced[s]), self.flags[s]
            self.c_on[s] += v - (fl[f - self.on] if f >= self.on else 0)
            self.c_off[s] += v - (fl[f - self.off] if f >= self.off else 0)
            fl.append(v)
            if not self.trig[s]:
                if 10 * self.c_on[s] > 8 * self.on:
                    self.trig[s], self.open[s] = True, f
            elif 10 * (self.off - self.c_off[s]) > 9 * self.off:
                out.append(self._close(s, f, 0))
            elif f - self.open[s] + 1 >= self.max_frames:
                out.append(self._close(s, f, 1))
        self.frames += 1
        return out

    def flush(self):
        return [self._close(s, self.frames - 1, 2) for s in range(self.S) if self.trig[s]]


def live_run(flags, on_window, off_window, pre_roll, max_frames, **geometry):
    """All records of ``flags`` [S, F] stepped frame by frame and flushed, in emission order."""
    flags = np.asarray(flags)
    ref = LiveRef(flags.shape[0], on_window, off_window, pre_roll, max_frames, **geometry)
    out = []
    for f in range(flags.shape[1]):
        out += ref.step(flags[:, f])
    return out + ref.flush()


def whole_signal_records(flags, on_window, off_window, pre_roll, max_frames, **geometry):
    """The same from the whole-signal definition: walk_ref per stream, merged by close frame, then stream (a flush's closes
    share the last frame with that frame's own closes but belong to other streams, and come after them)."""
    rows = []
    for s, v in enumerate(np.asarray(flags)):
        rows += [(s,) + u for u in walk_ref(v, on_window, off_window, pre_roll, max_frames, FAR, **geometry)]
    return sorted(rows, key=lambda r: (r[4], r[5] == 2, r[0]))


def rows(rec):
    """Records as the queue returns them (int64 [n, 6]) -> the tuples of the two functions above."""
    return [tuple(int(v) for v in r) for r in rec]


def energies(flags, threshold=0.0):
    """flags [S, F] -> float32 [F, S] at threshold +- 1: one contiguous [S] row of energies per explicit step."""
    return np.ascontiguousarray(np.where(np.asarray(flags).T > 0, threshold + 1.0, threshold - 1.0).astype(np.float32))


def count_flags(S):
    """Stream s: a first run [2 + d, 8 + d), d = s mod 7, that closes by endpoint at 12 + d, then a run from 16 + d up to frame 40
    for everyone: all streams close at step 44."""
    v = np.zeros((S, 46), np.int64)
    for s in range(S):
        d = s % 7
        v[s, 2 + d:8 + d] = 1
        v[s, 16 + d:40] = 1
    return v


# ---- the walk sweep -----------------------------------------------------------------------------------------------------
SWEEP_FRAMES = [1, 63, 64, 65, 129, 700]
SWEEP_PRE_ROLLS = [0, 60, 10000]


def sweep_max_frames(F):
    return [2, 50, F + 1]  # F + 1: the time-out never fires


def sweep_cases():
    """(F, (on, off), flags [3, F]) for every frame count and window pair; pre-rolls and time-outs are swept inside a case."""
    for F in SWEEP_FRAMES:
        for pair in WINDOW_PAIRS:
            yield F, pair, walk_flags(F, walk_seeds(F, pair), pair)


# two extra sets of three streams: the same track three times (every close is a step in which all streams close) and a track
# beside itself one frame late
EXTRA_CASES = [(129, (3, 5), np.stack([flag_track(129, 4242, mean_run=10)] * 3)),
               (129, (3, 5), np.stack([flag_track(129, 4242, mean_run=10), flag_track(129, 4242, mean_run=10),
                                       np.concatenate([[0], flag_track(129, 4242, mean_run=10)[:-1]])]))]

COVERAGE = {"no_utterance", "reason_0", "reason_1", "reason_2", "open_at_last_frame", "start_limited_by_prev_close", "start_clamped_at_0",
            "open_at_0_mod_64", "open_at_63_mod_64", "close_at_0_mod_64", "close_at_63_mod_64", "two_close_at_one_step",
            "all_close_at_one_step"}


def coverage_of(records, S, F, pre_roll):
    """The coverage facts the reference's answer for one stream set contributes."""
    got = set()
    per_stream = {s: [r for r in records if r[0] == s] for s in range(S)}
    for s, rows in per_stream.items():
        if not rows:
            got.add("no_utterance")
        prev_close = -1
        for (_, _, _, o, c, reason) in rows:
            got.add(f"reason_{reason}")
            for name, x in (("open", o), ("close", c)):
                if x % 64 == 0:
                    got.add(f"{name}_at_0_mod_64")
                if x % 64 == 63:
                    got.add(f"{name}_at_63_mod_64")
            if o == F - 1:
                got.add("open_at_last_frame")
            if prev_close + 1 > max(o - pre_roll, 0):
                got.add("start_limited_by_prev_close")
            if o - pre_roll < 0 and prev_close == -1:
                got.add("start_clamped_at_0")
            prev_close = c
    steps = {}
    for r in records:
        if r[5] != 2:  # a step's own closes; the flush is not a step
            steps[r[4]] = steps.get(r[4], 0) + 1
    if any(n >= 2 for n in steps.values()):
        got.add("two_close_at_one_step")
    if S > 1 and any(n == S for n in steps.values()):
        got.add("all_close_at_one_step")
    return got


# ---- the ring cut ---------------------------------------------------------------------------------------------------------
# Small windows, pre-roll and time-out, so that the history of kws_host_stream_utt_history(slack_hops = 0) is a few thousand
# samples and wraps many times.  Two frame geometries: with 400 / 160 a span's end is never a multiple of the hop, so "ends
# exactly on the seam" needs a frame that is a whole number of hops (320 / 160).
CUT_ON, CUT_OFF, CUT_PRE_ROLL, CUT_MAX_FRAMES = 3, 5, 4, 12
CUT_NORMALIZE = [0, 16384, 32767]
CUT_N_OUT = [700, 3001]  # shorter and longer than the spans
CUT_GEOMETRIES = {"400/160": (400, 160, 2024), "320/160": (320, 160, 2024)}  # frame_len, frame_step, seed
CUT_HOPS = 260
CUT_STREAMS = 3


def cut_case(name):
    """(flags [S, F], pcm int16 [S, hops * step], records, H, facts) of one geometry.  F = hops - (K - 1) frames are walked:
    the first K - 1 hops are appended without a walk, so every walked frame is complete.  The PCM is random with one span set to
    zeros and one given a -32768 (spans chosen from the reference's own records)."""
    frame_len, step, seed = CUT_GEOMETRIES[name]
    K = -(-frame_len // step)
    F = CUT_HOPS - (K - 1)
    geometry = dict(frame_len=frame_len, frame_step=step)
    flags = np.stack([flag_track(F, seed + s, mean_run=7) for s in range(CUT_STREAMS)])
    records = live_run(flags, CUT_ON, CUT_OFF, CUT_PRE_ROLL, CUT_MAX_FRAMES, **geometry)
    H = history(CUT_PRE_ROLL, CUT_MAX_FRAMES, 0, frame_len, step)
    rng = np.random.default_rng(seed)
    pcm = rng.integers(-32767, 32768, (CUT_STREAMS, CUT_HOPS * step)).astype(np.int16)
    by_len = sorted(range(len(records)), key=lambda i: (records[i][2] - records[i][1], i))
    zero, loud = records[by_len[len(by_len) // 2]], records[by_len[len(by_len) // 3]]
    pcm[loud[0], (loud[1] + loud[2]) // 2] = -32768
    pcm[zero[0], zero[1]:zero[2]] = 0
    longest = (CUT_PRE_ROLL + CUT_MAX_FRAMES - 1) * step + frame_len
    facts = set()
    for (s, a, b, _, _, _) in records:
        if a // H != (b - 1) // H and b % H:
            facts.add("crosses_the_seam")
        if b % H == 0:
            facts.add("ends_on_the_seam")
        if a % H == 0:
            facts.add("starts_on_the_seam")
        if b - a == longest:
            facts.add("longest_span")
        x = pcm[s, a:b].astype(np.int64)
        if np.abs(x).max() == 32768:
            facts.add("peak_32768")
        if not x.any():
            facts.add("all_zero")
    return flags, pcm, records, H, facts


CUT_FACTS = {"400/160": {"crosses_the_seam", "starts_on_the_seam", "longest_span", "peak_32768", "all_zero"},
             "320/160": {"crosses_the_seam", "ends_on_the_seam", "starts_on_the_seam", "longest_span", "peak_32768", "all_zero"}}


def spans_of(records):
    return [(r[0], r[1], r[2]) for r in records]


# ---- PCM patterns (copies of tests/test_stream_decisions_gpu.py's builders) ---------------------------------------------------
def pcm_of(pattern, seed, step=FRAME_STEP):
    """Voiced / unvoiced pattern bool [S, H] -> int16 [S, H * step]: a voiced hop is uniform noise in +-20000 whose last sample
    is 0 (pre-emphasis then leaks nothing into the next frame), an unvoiced hop is zeros."""
    pattern = np.asarray(pattern, bool)
    S, H = pattern.shape
    x = np.random.default_rng(seed).integers(-20000, 20001, size=(S, H, step)).astype(np.int16)
    x[:, :, step - 1] = 0
    x[~pattern] = 0
    return x.reshape(S, H * step)


def delayed(base, delays):
    """One stream per entry of ``delays``: the base pattern, that many hops late."""
    base = np.asarray(base, bool)
    out = np.zeros((len(delays), len(base)), bool)
    for s, d in enumerate(delays):
        out[s, d:] = base[:len(base) - d]
    return out


def cycles(on, off, hops):
    """Silence, then voiced runs long enough to open and pauses long enough to close, repeated; from on = 10 up every run has a
    dropout of three hops (one unvoiced frame) near its start."""
    run = [True] * (on + 8)
    if on >= 10:
        run[3:6] = [False] * 3
    cycle = run + [False] * (off + 6)
    return ([False] * 4 + cycle * (hops // len(cycle) + 1))[:hops]


# ---- the push-driven cases ------------------------------------------------------------------------------------------------
PUSH_PAIRS = [(3, 5), (10, 20), (40, 80)]
def push_runs(on, off):
    """(pre_roll, max_frames) of the two runs per window pair.  The first time-out is shorter than a run's utterance (a run of
    on + 8 voiced hops opens after about 0.8 on of them and closes about 0.9 off frames after it ends), so it fires; under the
    second every utterance closes by endpoint."""
    return [(60, off + 2), (0, 1000)]


def push_hops(off):
    return 3 * off + 20


def push_pcm(on, off):
    """int16 [2, hops * 160]: the cycles pattern, the second stream three hops late."""
    return pcm_of(delayed(cycles(on, off, push_hops(off)), [0, 3]), 100 * on + off)


def oracle_flags(pcm, threshold=THR, margin=3.0):
    """(flags int [S, F], worst margin): voiced flags of the COMPLETE frames of pcm [S, hops * 160] from the float64 oracle's log
    energy; every energy must be at least ``margin`` away from the threshold, so that no float32 energy decides a case."""
    from oracle import psf_mfcc as o_mfcc

    F = pcm.shape[1] // FRAME_STEP - (LAG - 1)
    rows, worst = [], np.inf
    for x in pcm:
        c0 = o_mfcc.mfcc(o_mfcc.pcm16_to_float(x), o_mfcc.FrontendSpec(n_samples=len(x)))[:F, 0]
        worst = min(worst, float(np.abs(c0 - threshold).min()))
        rows.append((c0 > threshold).astype(np.int64))
    return np.stack(rows), worst


# ---- the rate case --------------------------------------------------------------------------------------------------------
RATE_IN, RATE_HOPS, RATE_PAIR, RATE_PRE_ROLL, RATE_MAX_FRAMES = 48000, 70, (3, 5), 4, 10


def rate_input():
    """int16 [2, hops * 480] at 48 kHz: the (3, 5) cycles as bursts of half-scale noise (nothing clips in the resampler) over a
    floor of exact zeros, the second stream three hops late."""
    pattern = delayed(cycles(RATE_PAIR[0], RATE_PAIR[1], RATE_HOPS), [0, 3])
    S, H = pattern.shape
    x = np.random.default_rng(48).integers(-12000, 12001, size=(S, H, 480)).astype(np.int16)
    x[~pattern] = 0
    return x.reshape(S, H * 480)


def rate_heard(x48, plan, taps):
    """int16 [S, hops * 160]: what the streams hear -- _resample_stream_ref.batch_window's float64 signal rounded as the device
    stores it -- and the smallest distance of any value from a rounding boundary relative to its float64 error bound (> 1: the
    rounding of every sample is decided)."""
    import _resample_ref as ref
    import _resample_stream_ref as sref

    up, down, delay, _ = plan
    n_total = x48.shape[1] * up // down
    y, sabs = sref.batch_window(x48, up, down, taps, delay, -(-delay // up), n_total)
    frac = np.abs(y - np.floor(y) - 0.5)
    decided = float((frac / np.maximum(ref.dot_bound(up, down) * sabs, 1e-300)).min())
    return ref.to_int16(y), decided
