"""Streaming-push helpers shared by tests/test_stream_push_edges_gpu.py: one seeded PCM set, the window unroller of
StreamingSpotter.features() written against kws_stream_copy_features / kws_stream_state, and the two float64 references --
oracle.psf_mfcc.mfcc of the continuous signal for the feature ring, oracle.dscnn.forward on the window THE DEVICE HOLDS for the
network (so the network check carries no front-end rounding).  Both references are computed once and cached: the psf frames per
stream of the PCM set, the float64 logits per (model, window bits)."""
import hashlib

import numpy as np
import torch

from _dscnn_forward import DEV, TOL, he_scale
from oracle import dscnn as o_dscnn
from oracle import psf_mfcc as o_mfcc

HOP, T, F = 160, 99, 10
LAG = 3                     # hops a 400-sample frame spans: after h pushes the newest complete frame is h - LAG
MAX_STREAMS, MAX_HOPS = 257, 302
TILE_RTOL = 2e-5            # tile shapes against one workgroup per stream, as test_streaming_time_tile_clusters_agree
ZERO, TONE, FADE, LATE = 1, 2, 3, 4   # the special streams (present where the stream count reaches them); every other one is noise

_pcm = None
_frames = {}
_logits = {}


def stream_pcm(S, hops):
    """int16 [S, hops * 160]: the first S streams and hops of ONE seeded set (a stream's samples do not depend on S or hops, so the
    psf frames of a stream are computed once for all tests).  Noise streams each at its own level (uniform ** 3: some are down at a
    few LSBs); stream 1 exact zeros; 2 a 700 Hz tone; 3 noise fading in over the first 104 hops; 4 zero for the first 40 hops."""
    global _pcm
    if _pcm is None:
        rng = np.random.default_rng(20240607)
        n = MAX_HOPS * HOP
        pcm = rng.integers(-20000, 20000, size=(MAX_STREAMS, n), dtype=np.int16)
        level = rng.uniform(0.0, 1.0, MAX_STREAMS) ** 3
        level[[0, FADE, LATE]] = (0.8, 1.0, 0.6)
        pcm = np.round(pcm * level[:, None]).astype(np.int16)
        pcm[ZERO] = 0
        pcm[TONE] = np.round(9000 * np.sin(2 * np.pi * 700 * np.arange(n) / 16000.0)).astype(np.int16)
        pcm[FADE, : 104 * HOP] = (pcm[FADE, : 104 * HOP] * np.linspace(0.001, 1.0, 104 * HOP)).astype(np.int16)
        pcm[LATE, : 40 * HOP] = 0
        pcm.setflags(write=False)
        _pcm = pcm
    assert S <= MAX_STREAMS and hops <= MAX_HOPS
    return _pcm[:S, : hops * HOP]


def pcm_hops(S, hops):
    """The set as the pushes take it: int16 [hops, S, 160], C-contiguous per hop (host), and the same on the device."""
    host = np.ascontiguousarray(stream_pcm(S, hops).reshape(S, hops, HOP).transpose(1, 0, 2))
    dev = torch.from_numpy(host).to(DEV)
    torch.cuda.synchronize()
    return host, dev


def psf_frames(s):
    """float64 [MAX_HOPS - 2, 10]: the psf MFCC of every complete frame of stream s of the set.  Pre-emphasis and framing are
    causal, so frame f is what a push sees once hop f + LAG - 1 is in, however many hops follow."""
    if s not in _frames:
        sig = o_mfcc.pcm16_to_float(stream_pcm(MAX_STREAMS, MAX_HOPS)[s])
        _frames[s] = np.asarray(o_mfcc.mfcc(sig, o_mfcc.FrontendSpec(n_samples=len(sig))), np.float64)[: MAX_HOPS - LAG + 1]
    return _frames[s]


def psf_window(s, pushed):
    """float64 [99, 10]: stream s's window after ``pushed`` hops, oldest frame first, zeros where no frame exists yet."""
    want = np.zeros((T, F))
    newest = pushed - LAG
    lo = max(0, newest - (T - 1))
    if newest >= 0:
        want[T - 1 - (newest - lo):] = psf_frames(s)[lo:newest + 1]
    return want


def unroll(ring, pushed):
    """The ring [S, 99, 10] as the kernel reads it: frame f lives in row f mod 99, the window starts one row past the newest."""
    return np.roll(ring, -((pushed - LAG + 1) % T), axis=1)


def device_window(ctx, S):
    """(window float32 [S, 99, 10] oldest frame first, raw ring, pushes) of a context, through kws_stream_copy_features and
    kws_stream_state -- the logic of StreamingSpotter.features()."""
    ring = torch.empty((S, T, F), dtype=torch.float32, device=DEV)
    ctx.stream_copy_features(ring)
    _, pushed = ctx.stream_state()          # synchronises the context's stream
    raw = ring.cpu().numpy()
    return unroll(raw, pushed), raw, pushed


def blob_state(blob, C):
    """A flat weight blob (the layout kws_load_dscnn takes) as a state dict."""
    state, off = {}, 0
    for k, shp in o_dscnn.state_shapes(C).items():
        n = int(np.prod(shp))
        state[k] = torch.from_numpy(np.asarray(blob[off:off + n], np.float32).reshape(shp).copy())
        off += n
    return state


def random_model(C, seed=None):
    """He-scaled body, small biases, fc.weight ~ N(0, 1): float64 top-2 margins far above TOL."""
    return he_scale(o_dscnn.random_state(900 + C if seed is None else seed, num_classes=C, std=1.0))


def f64_logits(key, state, window):
    """oracle.dscnn.forward in float64 on float32 windows [n, 99, 10]; cached per (key, window bits) -- tile shapes, arithmetics
    and delivery routes hold the same ring bits, so they share one reference.  ``key`` names the model."""
    out = np.empty((len(window), int(state["fc.weight"].shape[0])))
    todo = []
    for i, w in enumerate(window):
        k = (key, hashlib.sha1(np.ascontiguousarray(w).tobytes()).digest())
        if k in _logits:
            out[i] = _logits[k]
        else:
            todo.append((i, k))
    if todo:
        x = torch.from_numpy(np.stack([window[i] for i, _ in todo]))[:, None].double()
        got = o_dscnn.forward(state, x).numpy()
        for (i, k), row in zip(todo, got):
            _logits[k] = row
            out[i] = row
    return out


def sure_rows(want):
    """Rows whose float64 top-2 margin exceeds TOL (every row at C == 1, where the label is 0)."""
    if want.shape[1] == 1:
        return np.ones(len(want), bool)
    top = np.sort(want, axis=1)
    return top[:, -1] - top[:, -2] > TOL


def logit_gate(want):
    return TOL * max(1.0, float(np.abs(want).max()) / 100)


class Sink:
    """Device outputs of a push with one guard row beyond S: NaN logits, label -1.  ``read`` returns host copies of the S rows
    after asserting that the guard row is untouched."""

    def __init__(self, S, C):
        self.S, self.C = S, C
        self.logits = torch.full((S + 1, C), float("nan"), dtype=torch.float32, device=DEV)
        self.labels = torch.full((S + 1,), -1, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()

    def read(self, ctx, what=""):
        ctx.sync()
        lg, lb = self.logits.cpu().numpy(), self.labels.cpu().numpy()
        assert np.isnan(lg[self.S]).all() and lb[self.S] == -1, f"guard row written {what}"
        return lg[: self.S].copy(), lb[: self.S].copy()


def check_network(key, state, window, logits, labels, what, stats=None, rows=None):
    """Logits within the gate of the float64 reference on ``window`` and labels equal on every sure row; returns the sure mask.
    ``rows`` restricts the check to some streams; ``stats`` (a dict) collects the worst error-to-gate ratio under "logits"."""
    rows = np.arange(len(window)) if rows is None else np.asarray(rows)
    want = f64_logits(key, state, window[rows])
    err, gate = float(np.abs(logits[rows].astype(np.float64) - want).max()), logit_gate(want)
    if stats is not None:
        stats["logits"] = max(stats.get("logits", 0.0), err / gate)
    assert err <= gate, f"{what}: max |logit - f64| = {err:.3e} > {gate:.3e}"
    sure = sure_rows(want)
    ref = want.argmax(axis=1)
    assert np.array_equal(labels[rows][sure], ref[sure]), f"{what}: labels {labels[rows][sure]} vs {ref[sure]}"
    return sure


def check_ring(window, pushed, what, stats=None, rows=None):
    """The device's window within TOL of the psf oracle of the continuous signal."""
    rows = range(len(window)) if rows is None else rows
    err = max(float(np.abs(window[s] - psf_window(s, pushed)).max()) for s in rows)
    if stats is not None:
        stats["ring"] = max(stats.get("ring", 0.0), err / TOL)
    assert err <= TOL, f"{what}: max |ring - psf| = {err:.3e}"
