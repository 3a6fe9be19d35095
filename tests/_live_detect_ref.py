"""Expectations shared by tests/test_live_detect_cpu.py and tests/test_live_detect_gpu.py (not a test module): the rules of
``kws_stream_detect_*`` restated hop by hop in NumPy (``LiveDetectRef``: a posterior ring, a direct sum and ``next`` per stream),
the queue's arithmetic, the ``first_hop`` mapping between decisions and scan windows, and the first argmax as the kernels take it."""
import numpy as np

REC = 5  # int64 words per record: stream, decision, hop, label, score bits


def lag(frame_len, frame_step):
    """K: hops a frame spans; push h (from 1) completes frame h - K."""
    return -(-frame_len // frame_step)


def first_hop(num_frames, frame_len, frame_step):
    """The first push whose window holds num_frames complete frames."""
    return num_frames + lag(frame_len, frame_step) - 1


def event_time(hop, frame_len, frame_step, sample_rate=16000):
    """End of the window that push ``hop`` decided on = end of frame hop - K, in seconds."""
    return ((hop - lag(frame_len, frame_step)) * frame_step + frame_len) / float(sample_rate)


def first_argmax(s):
    """The kernels' argmax of rows [..., C]: best = -1, arg = 0, a later class wins only when strictly greater (a NaN never is)."""
    s = np.asarray(s)
    best = np.full(s.shape[:-1], -1.0, s.dtype)
    arg = np.zeros(s.shape[:-1], np.int64)
    for c in range(s.shape[-1]):
        v = s[..., c]
        with np.errstate(invalid="ignore"):
            m = v > best
        best = np.where(m, v, best)
        arg = np.where(m, c, arg)
    return arg, best


def score_bits(x):
    return int(np.float32(x).view(np.uint32))


def readable(first_seq, n, total, max_events):
    """kws_stream_detect_read's two checks: landed, and still in the queue."""
    return n >= 1 and first_seq + n <= total and first_seq + max_events >= total


class LiveDetectRef:
    """One decision per step for S streams, in float64 (the definition; the device's float32 is held to it within tol_smooth)."""

    def __init__(self, S, C, smooth_window, first_keyword, threshold, refractory, first_hop=0, max_events=None, dtype=np.float64):
        self.S, self.C, self.W = S, C, smooth_window
        self.first_keyword, self.threshold, self.refractory, self.first_hop = first_keyword, threshold, refractory, first_hop
        self.max_events = max_events if max_events is not None else max(S, 64)
        self.dtype = dtype
        self.ring = np.zeros((S, smooth_window, C), dtype)
        self.next = np.zeros(S, np.int64)
        self.d = 0
        self.total = 0
        self.queue = np.zeros((self.max_events, REC), np.int64)
        self.smoothed = np.zeros((S, C), dtype)
        self.label = np.zeros(S, np.int64)
        self.wrapped = False

    def step(self, logits, hop=None):
        """logits [S, C]; hop: the context's hop count of a push (None: an explicit step).  Returns the records of this step,
        (stream, d, h, label, score) with the score as a float."""
        if hop is not None and hop < self.first_hop:
            return []
        d, W = self.d, self.W
        z = np.asarray(logits).astype(self.dtype)
        with np.errstate(invalid="ignore"):
            e = np.exp(z - np.fmax.reduce(z, axis=1, keepdims=True))
            self.ring[:, d % W] = e / e.sum(axis=1, keepdims=True)
        self.wrapped |= d >= W
        terms = min(W, d + 1)
        acc = np.zeros((self.S, self.C), self.dtype)
        for v in range(terms):  # oldest first
            acc = acc + self.ring[:, (d - terms + 1 + v) % W]
        self.smoothed = acc / self.dtype(terms)
        self.label, best = first_argmax(self.smoothed)
        out = []
        for s in range(self.S):
            k = int(self.label[s])
            if k >= self.first_keyword and best[s] >= self.threshold and d >= self.next[s]:
                self.next[s] = d + self.refractory
                rec = (s, d, d if hop is None else hop, k, float(best[s]))
                self.queue[self.total % self.max_events] = rec[:4] + (score_bits(best[s]),)
                self.total += 1
                out.append(rec)
        self.d += 1
        return out


def run(logits, smooth_window, first_keyword, threshold, refractory, **kw):
    """logits [S, W, C] through W explicit steps: (per-stream events [(d, label, score)], smoothed [S, W, C], ref)."""
    S, W, C = logits.shape
    ref = LiveDetectRef(S, C, smooth_window, first_keyword, threshold, refractory, **kw)
    events, smoothed = [[] for _ in range(S)], np.zeros((S, W, C), ref.dtype)
    for d in range(W):
        for s, dd, _, k, score in ref.step(logits[:, d]):
            events[s].append((dd, k, score))
        smoothed[:, d] = ref.smoothed
    return events, smoothed, ref


def group_records(rec, S):
    """Queue records int64 [n, 5] -> per stream [(d, label, score bits)], in queue order."""
    out = [[] for _ in range(S)]
    for s, d, _, k, bits in np.asarray(rec).reshape(-1, REC):
        out[int(s)].append((int(d), int(k), int(bits)))
    return out
