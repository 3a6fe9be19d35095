"""Helpers of the float32 recording tests (test_scan_f32_gpu.py, test_ragged_f32_gpu.py, test_scan_f32_cpu.py): lengths,
the exact int16 -> float32 scaling of the grid property, and kws_cut_f32 restated in NumPy."""
import numpy as np

from _scan_ref import FRAME_LEN, FRAME_STEP


def n_for_frames(F, extra=0):
    """A length with exactly F frames: the last frame ends `extra` samples short of being full (0: no padded last frame)."""
    return FRAME_LEN + FRAME_STEP * (F - 1) - extra


def unit(pcm):
    """int16 -> the float32 samples the int16 entries see: pcm / 32768, an exact division."""
    return np.asarray(pcm).astype(np.float32) / np.float32(32768.0)


def cut_f32_ref(x, spans, normalize_to, n_out):
    """kws_cut_f32 restated in NumPy: a float32 peak that a NaN never raises, a float64 divide and multiply, one rounding."""
    R, n = x.shape
    clips = np.zeros((len(spans), n_out), np.float32)
    peaks = np.zeros(len(spans), np.float32)
    for u, (r, s, e) in enumerate(spans):
        if not 0 <= r < R:
            peaks[u] = -1.0
            continue
        s, e = min(max(s, 0), n), min(max(e, 0), n)
        seg = x[r, s:e] if e > s else x[r, :0]
        mags = np.abs(seg)
        mags = mags[~np.isnan(mags)]
        peak = np.float32(mags.max()) if mags.size else np.float32(0.0)
        peaks[u] = peak
        body = seg[:n_out]
        if normalize_to > 0:
            if peak > 0:
                times = np.float64(np.float32(normalize_to)) / np.float64(peak)
                with np.errstate(over="ignore"):
                    clips[u, :len(body)] = (body.astype(np.float64) * times).astype(np.float32)
        else:
            clips[u, :len(body)] = body
    return clips, peaks
