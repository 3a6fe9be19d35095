"""The streaming resampler's definition in NumPy float64 (include/kws_hip.h, "streaming sample-rate conversion"), shared by
test_stream_resample_cpu.py and test_stream_resample_gpu.py.

A stream's signal x[m] is zero before ``first_sample`` and grows by one chunk per push.  With P samples received the absolute
outputs j < floor(P up / down) have been emitted, and output j is

    y[j - d],   y[k] = sum over m of x[m] * h[half + k * down - m * up]   for every integer k,   d = ceil(half / down).

``StreamRef`` keeps what the library keeps -- the last ``history`` samples and a position -- and builds each output's row of
samples and taps exactly as _resample_ref.resample_ref does (newest sample first, ``rows`` terms, zeros for the table's padding).
A sample index outside history || chunk raises: the history would be too short, or the delay too small."""
import numpy as np

import _resample_ref as ref


def delay_of(up, down):
    """d = ceil(half / down) output samples; 0 for equal rates (a copy)."""
    if up == down == 1:
        return 0
    return -(-10 * max(up, down) // down)


def count(P0, n_in, up, down):
    """Samples a push of n_in emits after P0 samples: floor((P0 + n_in) up / down) - floor(P0 up / down), in Python integers."""
    return (int(P0) + int(n_in)) * up // down - int(P0) * up // down


class StreamRef:
    """One set of S streams in lockstep.  ``push(chunk [S, n_in])`` -> (y, Sabs) float64 [S, n_out]: the exact sums in NumPy's
    order and the sums of |x| |h| that scale the float64 error bound."""

    def __init__(self, n_streams, up, down, taps, history, first_sample=0):
        assert first_sample % down == 0
        self.up, self.down = int(up), int(down)
        self.taps = np.asarray(taps, np.float64)
        self.half = (len(self.taps) - 1) // 2
        self.rows = (2 * self.half + up) // up
        self.d = delay_of(up, down)
        self.H = int(history)
        self.pos = int(first_sample)                       # Python integers: no 64-bit limit in the reference
        self.hist = np.zeros((int(n_streams), self.H))     # samples pos - H .. pos - 1
        self.lowest_index = None                           # the deepest reach into the history so far (0 = its oldest sample)

    def push(self, chunk):
        chunk = np.atleast_2d(np.asarray(chunk)).astype(np.float64)
        S, n_in = chunk.shape
        up, down, half, rows = self.up, self.down, self.half, self.rows
        buf = np.concatenate([self.hist, chunk], axis=1)   # index i holds sample pos - H + i
        j0 = self.pos * up // down
        n_out = count(self.pos, n_in, up, down)
        if up == down == 1:
            y = chunk.copy()
            sabs = np.abs(chunk)
        else:
            c = [half + (j0 + t - self.d) * down for t in range(n_out)]              # Python integers, floor semantics
            q = np.array([ci // up - (self.pos - self.H) for ci in c], np.int64)      # newest sample, as an index into buf
            ph = np.array([ci % up for ci in c], np.int64)
            idx = q[:, None] - np.arange(rows)[None, :]
            t = ph[:, None] + np.arange(rows)[None, :] * up
            if n_out:
                if idx.min() < 0 or idx.max() >= buf.shape[1]:
                    raise IndexError(f"an output reads index {idx.min()}..{idx.max()} of history || chunk [0, {buf.shape[1]})")
                self.lowest_index = int(idx.min()) if self.lowest_index is None else min(self.lowest_index, int(idx.min()))
            h = np.where(t <= 2 * half, self.taps[np.minimum(t, 2 * half)], 0.0)
            y, sabs = np.zeros((S, n_out)), np.zeros((S, n_out))
            for r in range(S if n_out else 0):  # row by row, the arrays and the sum of resample_ref
                v = np.ascontiguousarray(buf[r][idx])
                y[r] = (v * h).sum(axis=1)
                sabs[r] = (np.abs(v) * np.abs(h)).sum(axis=1)
        self.hist = buf[:, buf.shape[1] - self.H:]
        self.pos += n_in
        return y, sabs

    def history_used(self):
        """Samples of the history the outputs so far reached back to (H - lowest index), 0 before any output."""
        return 0 if self.lowest_index is None else max(0, self.H - self.lowest_index)


def batch_window(x, up, down, taps, d, z, n_total):
    """What the stream must equal: resample_ref of ``x`` [S, N] front-padded by down * z zeros, read at [up z - d, up z - d +
    n_total) -- (y, Sabs).  z is chosen by the caller so that up z >= d."""
    x = np.atleast_2d(np.asarray(x))
    padded = np.concatenate([np.zeros((x.shape[0], down * z), x.dtype), x], axis=1)
    lo = up * z - d
    assert lo >= 0
    y, s = ref.resample_ref(padded, up, down, taps, n_out=lo + n_total)
    return y[:, lo:], s[:, lo:]
