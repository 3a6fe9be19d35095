"""Expectations shared by tests/test_stream_reset_cpu.py and tests/test_stream_reset_gpu.py (not a test module): what
``kws_stream_reset`` does to the two decision layers, restated on top of ``_live_ref.LiveRef`` and
``_live_detect_ref.LiveDetectRef``, and the cases the device is tested on.  The rings need no restatement: a reset stream must
equal, bit for bit, the same stream of a second set that was fed zeros up to the reset."""
import numpy as np

from _live_detect_ref import LiveDetectRef, first_argmax, score_bits
from _live_ref import FRAME_LEN, FRAME_STEP, LiveRef

T = 99                                   # frames of a window
K = -(-FRAME_LEN // FRAME_STEP)          # hops a frame spans
POST = T + K + 5                         # pushes after a reset: the window turns over once, the ring's seam is crossed
H0S = [0, 1, K - 1, K, 50, T + K - 1, 150]   # no frame yet, the first frame, a part window, the first full window, a wrapped ring
RESET_SETS = [(0,), (4,), (1, 2), (0, 1, 2, 3, 4)]   # S = 5: stream 4 has no pair partner in the frame wavefront
DETECT_WINDOWS = [1, 4, 30]


def silent_rows(h0, num_frames=T, lag=K):
    """Rows of a stream's feature ring that hold a frame after h0 pushes: frames 0 .. h0 - lag, frame f in row f mod num_frames."""
    return min(max(h0 - lag + 1, 0), num_frames)


class ResetLiveRef(LiveRef):
    """LiveRef with the reset's rule.  ``appended``: hops appended so far -- the walk lags them by K - 1 behind pushes."""

    def reset(self, s, appended):
        out = [self._close(s, self.frames - 1, 2)] if self.trig[s] else []
        self.flags[s] = [0] * len(self.flags[s])
        self.c_on[s] = self.c_off[s] = 0
        self.trig[s], self.open[s], self.prev_close[s] = False, -1, appended - 1
        return out


class ResetDetectRef(LiveDetectRef):
    """LiveDetectRef with an epoch per stream: the mean of stream s runs over the last min(W, d - epoch[s] + 1) decisions."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.epoch = np.zeros(self.S, np.int64)

    def reset(self, s):
        self.epoch[s] = self.d
        self.next[s] = 0

    def step(self, logits, hop=None):
        if hop is not None and hop < self.first_hop:
            return []
        d, W = self.d, self.W
        z = np.asarray(logits).astype(self.dtype)
        with np.errstate(invalid="ignore"):
            e = np.exp(z - np.fmax.reduce(z, axis=1, keepdims=True))
            self.ring[:, d % W] = e / e.sum(axis=1, keepdims=True)
        for s in range(self.S):
            terms = int(min(W, d - self.epoch[s] + 1))
            acc = np.zeros(self.C, self.dtype)
            for v in range(terms):  # oldest first
                acc = acc + self.ring[s, (d - terms + 1 + v) % W]
            self.smoothed[s] = acc / self.dtype(terms)
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


# ---- the live utterance scenario: S = 3, on / off = 3 / 5 ---------------------------------------------------------------------
UTT_ON, UTT_OFF, UTT_PRE_ROLL, UTT_MAX_FRAMES = 3, 5, 4, 1000
UTT_STREAM, UTT_H0, UTT_HOPS = 1, 45, 110


def utt_pattern(at_once):
    """Voiced hops bool [3, UTT_HOPS].  Stream 1 is the one reset after UTT_H0 pushes: a run that closes long before the reset, a
    run that is open at it, and after it either a run that starts more than pre_roll + on_window frames later (the records then
    equal a silent past's) or one that goes straight on (the span start is then held at the reset).  Streams 0 and 2 are
    neighbours with runs of their own, one of them open across the reset."""
    v = np.zeros((3, UTT_HOPS), bool)
    v[0, 8:24] = v[0, 40:58] = v[0, 80:92] = True
    v[2, 3:15] = v[2, 30:44] = v[2, 62:75] = True
    s = UTT_STREAM
    v[s, 6:20] = True
    v[s, 34:UTT_H0] = True
    if at_once:
        v[s, UTT_H0:UTT_H0 + 14] = True
    else:
        late = UTT_H0 + UTT_PRE_ROLL + UTT_ON + K + 3
        v[s, late:late + 14] = True
    return v
