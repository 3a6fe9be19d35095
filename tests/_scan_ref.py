"""Expectations shared by tests/test_scan_cpu.py and tests/test_scan_gpu.py (not a test module): the float64 NumPy restatement of
``kws_scan_detect_f32``, the synthetic logits its test feeds, the recordings of the scan tests and their oracle expectation."""
import numpy as np

T_WIN = 99       # frames per window
N_CEP = 10
FRAME_LEN, FRAME_STEP = 400, 160


def tol_smooth(S):
    """The gate tests/test_stream_decisions_gpu.py derives for a mean of S float32 posteriors: 2e-6 + (S + 1) 2^-24."""
    return 2e-6 + (S + 1) * 2.0 ** -24


def scan_shape(n_total, hop, frame_len=FRAME_LEN, frame_step=FRAME_STEP, window=T_WIN):
    """(frames, windows) by the formulas of include/kws_hip.h, restated."""
    frames = 1 if n_total <= frame_len else 1 + -(-(n_total - frame_len) // frame_step)
    return frames, (0 if frames < window else (frames - window) // hop + 1)


# ---- decisions ------------------------------------------------------------------------------------------------------
def detect_logits(W, C, seeds):
    """One recording per seed.  A piecewise-constant label track (segments of 1..40 windows): logit 12 on the track's class, 0
    elsewhere, plus uniform noise of +-0.5."""
    z = np.zeros((len(seeds), W, C), np.float64)
    for r, seed in enumerate(seeds):
        rng = np.random.default_rng(seed)
        track = np.empty(W, np.int64)
        w = 0
        while w < W:
            n = int(rng.integers(1, 41))
            track[w:w + n] = int(rng.integers(0, C))
            w += n
        z[r, np.arange(W), track] = 12.0
        z[r] += rng.uniform(-0.5, 0.5, size=(W, C))
    return z.astype(np.float32)


# Seeds per (W, C), one per recording, chosen on the CPU so that for S in {1, 7, 256} and a threshold of 0.5 no top-2 margin and
# no threshold comparison of the float64 restatement lies within 3 tol(S) of its boundary (equal class counts inside a smoothing
# window are ties to within the noise; most seeds have one somewhere).  The GPU test asserts the 2 tol(S) it needs.
DETECT_SEEDS = {(1, 2): (0, 1, 2), (1, 12): (0, 1, 2), (1, 64): (0, 1, 2), (63, 2): (0, 2, 3), (63, 12): (0, 2, 3), (63, 64): (0, 2, 3),
                (64, 2): (0, 2, 3), (64, 12): (0, 2, 3), (64, 64): (0, 2, 3), (65, 2): (0, 2, 3), (65, 12): (0, 2, 3), (65, 64): (0, 2, 3),
                (200, 2): (1, 4, 7), (200, 12): (249, 599, 756), (200, 64): (8, 11, 32)}


def smooth_ref(logits, S):
    """float64: softmax per window, then the mean over the last min(S, w + 1) windows."""
    z = logits.astype(np.float64)
    e = np.exp(z - z.max(axis=2, keepdims=True))
    p = e / e.sum(axis=2, keepdims=True)
    c = np.concatenate([np.zeros_like(p[:, :1]), np.cumsum(p, axis=1)], axis=1)
    w = np.arange(p.shape[1])
    lo = np.maximum(0, w - S + 1)
    return (c[:, w + 1] - c[:, lo]) / (w + 1 - lo)[None, :, None]


def margins(s, threshold):
    """(smallest top-2 margin, smallest |top - threshold|) over all windows of the smoothed posteriors s."""
    top = np.sort(s, axis=2)
    m2 = (top[..., -1] - top[..., -2]).min() if s.shape[2] > 1 else np.inf
    return m2, np.abs(top[..., -1] - threshold).min()


def events_ref(s, first_keyword, threshold, refractory):
    """Per recording the list of (window, label, score) the causal walk fires."""
    out = []
    k = s.argmax(axis=2)  # first maximum
    top = np.take_along_axis(s, k[..., None], axis=2)[..., 0]
    for r in range(s.shape[0]):
        ev, nxt = [], 0
        for w in range(s.shape[1]):
            if k[r, w] >= first_keyword and top[r, w] >= threshold and w >= nxt:
                ev.append((w, int(k[r, w]), float(top[r, w])))
                nxt = w + refractory
        out.append(ev)
    return out


# ---- recordings -----------------------------------------------------------------------------------------------------
def mixed_recordings(R, n_total, clips, seed=11):
    """Recordings that put full-scale noise, a second of zeros, a second of +-1 LSB noise and golden clips next to each other, in
    another order for every recording: neighbouring windows then have very different per-clip scales."""
    rng = np.random.default_rng(seed)
    out = np.empty((R, n_total), np.int16)
    for r in range(R):
        parts = [rng.integers(-32768, 32768, 16000, dtype=np.int64).astype(np.int16), np.zeros(16000, np.int16),
                 rng.integers(-1, 2, 16000, dtype=np.int64).astype(np.int16)]
        parts += [clips[(5 * r + 7 * i + 3) % len(clips)] for i in range(3)]
        parts = parts[r % len(parts):] + parts[:r % len(parts)]
        rec = np.concatenate(parts)
        out[r] = np.resize(rec, n_total)
    return out


def oracle_recordings(clips):
    """The two recordings of the oracle test: 48 053 samples each, 299 frames, 41 windows at a hop of 5."""
    a = np.concatenate([clips[8], clips[20], clips[33], np.zeros(53, np.int16)])
    b = np.concatenate([clips[18], clips[33], clips[22], clips[4][:53]])
    return np.stack([a, b])


def state_from_blob(blob, num_classes=12):
    import torch
    from oracle import dscnn as o_dscnn

    st, off = {}, 0
    for k, shp in o_dscnn.state_shapes(num_classes).items():
        n = int(np.prod(shp))
        st[k] = torch.from_numpy(np.asarray(blob[off:off + n]).reshape(shp).copy())
        off += n
    return st


def oracle_scan(recs, blob, hop):
    """(frames float64 [R, F, 10], logits float64 [R, W, C]): psf's MFCC of each recording as one clip, then the reference
    forward on the float32 windows."""
    import torch
    from oracle import dscnn as o_dscnn
    from oracle import psf_mfcc as o_mfcc

    spec = o_mfcc.FrontendSpec(n_samples=recs.shape[1])
    frames = np.stack([o_mfcc.extract_features_pcm16(rec, spec) for rec in recs])
    F, W = scan_shape(recs.shape[1], hop)
    assert frames.shape[1] == F
    f32 = frames.astype(np.float32)
    win = np.stack([[f32[r, w * hop:w * hop + T_WIN] for w in range(W)] for r in range(recs.shape[0])])  # [R, W, 99, 10]
    x = torch.from_numpy(win.reshape(-1, 1, T_WIN, N_CEP))
    logits = o_dscnn.forward(state_from_blob(blob), x.double()).numpy().reshape(recs.shape[0], W, -1)
    return frames, logits
