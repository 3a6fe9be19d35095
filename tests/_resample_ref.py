"""The resampler's definition in NumPy float64 (include/kws_hip.h, "sample-rate conversion on the device"), shared by
test_resample_cpu.py and test_resample_gpu.py:

    y[k] = sum over m of x[m] * h[half + k * down - m * up],   0 <= m < len, tap index in [0, 2 * half],   k < ceil(len * up / down)

and zero for k at or beyond the natural length.  Beside y it returns S[k] = sum of |x[m]| * |h[...]|, the scale of the float64
rounding error of any evaluation order: |fl(y) - y| <= 2 * terms * 2^-53 * S, with or without fused multiply-adds."""
from math import gcd

import numpy as np

# The first four run the staged kernel with 256 threads per workgroup.  192 -> 16 kHz runs it with 64 (its span fits LDS only for a
# tile of 256 outputs) and 96 -> 16 kHz with 128; 48 -> 2 kHz fits no tile and runs the instantiation that reads global memory.
PAIRS = {"1/3": (48000, 16000), "2/1": (8000, 16000), "160/441": (44100, 16000), "640/441": (44100, 64000),
         "1/6": (96000, 16000), "1/12": (192000, 16000), "1/24": (48000, 2000)}
F64_DOT = 2.0 ** -44  # 2 * 256 * 2^-53: a float64 dot product of at most 256 terms, in any order


def dot_bound(up, down):
    """The same forward bound for a pair: 2 * terms * 2^-53 with terms = max(256, ceil((20 max(up, down) + 1) / up)); 2^-44 for
    every pair of at most 256 terms per output, more only where an output has more terms (481 for 1/24)."""
    terms = (20 * max(up, down) + up) // up
    return 2.0 * max(256, terms) * 2.0 ** -53


def ratio(rate_in, rate_out):
    g = gcd(int(rate_in), int(rate_out))
    return int(rate_out) // g, int(rate_in) // g


def natural_len(n, up, down):
    return -((-int(n) * up) // down)


def firwin_taps(up, down):
    """scipy's own design: what resample_poly(x, up, down, window=("kaiser", 14.0)) filters with."""
    from scipy.signal import firwin

    M = max(up, down)
    return firwin(2 * 10 * M + 1, 1.0 / M, window=("kaiser", 14.0)) * up


def resample_ref(x, up, down, taps, d_len=None, n_out=None):
    """x [R, n_in] (or [n_in]) of any real dtype -> (y, S) float64 [R, n_out]; ``taps`` float64 [2 * half + 1]; ``d_len`` the valid
    samples per row (clamped to [0, n_in]; None: n_in); ``n_out`` defaults to the natural length of n_in samples."""
    x = np.atleast_2d(np.asarray(x)).astype(np.float64)
    R, n_in = x.shape
    taps = np.asarray(taps, np.float64)
    half = (len(taps) - 1) // 2
    rows = (2 * half + up) // up
    lens = np.full(R, n_in) if d_len is None else np.clip(np.asarray(d_len, np.int64), 0, n_in)
    n_out = natural_len(n_in, up, down) if n_out is None else int(n_out)
    y, S = np.zeros((R, n_out)), np.zeros((R, n_out))
    k = np.arange(n_out, dtype=np.int64)
    c = half + k * down
    m = (c // up)[:, None] - np.arange(rows)[None, :]            # [n_out, rows]: newest sample first
    t = (c % up)[:, None] + np.arange(rows)[None, :] * up
    h = np.where(t <= 2 * half, taps[np.minimum(t, 2 * half)], 0.0)
    for r in range(R):
        L = int(lens[r])
        live = (m >= 0) & (m < L) & (k < natural_len(L, up, down))[:, None]
        v = np.where(live, x[r][np.clip(m, 0, n_in - 1)], 0.0)
        y[r] = (v * h).sum(axis=1)
        S[r] = (np.abs(v) * np.abs(h)).sum(axis=1)
    return y, S


def to_int16(y):
    """clamp to [-32768, 32767], round to nearest even: what kws_resample_i16 stores."""
    return np.rint(np.clip(y, -32768.0, 32767.0)).astype(np.int16)


def n_in_for(n_nat, up, down):
    """The shortest input whose natural length is at least ``n_nat`` (exactly n_nat when down >= up)."""
    return max(1, ((int(n_nat) - 1) * down) // up + 1)
