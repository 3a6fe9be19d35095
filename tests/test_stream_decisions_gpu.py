"""The streaming decision layer -- kws_softmax_f32, kws_stream_smooth_f32 (posterior ring, running sum, first-maximum label) and
kws_stream_vad_f32 (the energy endpointer) -- at stream-count, window and class edges, driven through kws._native.Context with
no model loaded: smoothing needs only an open stream set, the endpointer only features-only pushes.

References: a float64 NumPy softmax; for smoothing the float64 mean of that softmax over the last min(count + 1, W) hops; for
the endpointer oracle.endpointer.EnergyEndpointer fed cepstrum 0 of oracle.psf_mfcc over the whole continuous signal.

Gates: softmax 1e-6 absolute; smoothing tol(W) = 2e-6 + (W + 1) 2^-24 -- 2e-6 is the gate of
test_softmax_and_streaming_posterior_smoothing, the second term bounds the running sum's rounding between two rebuilds (at most W
incremental updates, each rounding a sum <= W (<= W 2^-24) and a difference <= 1 (<= 2^-25), the total divided by W).  A float32
NumPy restatement of the kernel's recurrence stays below 2.2e-7 against float64 (randn x 5 and randn x 30 logits, S = 3, C = 12,
W = 1, 2, 7, 50, 64, up to 5000 hops), so the reference sits far inside the gate.  Every smoothing case prints its worst err / tol
and the share of label rows the margin rule excludes.

All logits and PCM of a case are placed on the device for all hops before the first call and every hop writes into its own row of one result tensor,
so a case reads back once."""
import re

import numpy as np
import pytest
import torch

from kws import _native
from kws.common.errors import KWSError
from oracle import psf_mfcc as o_mfcc
from oracle.endpointer import EnergyEndpointer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
STEP, FRAME_LEN = 160, 400
LAG = -(-FRAME_LEN // STEP)  # hops a frame spans: the first complete frame exists after LAG pushes
THR = -10.0                  # silence sits at log(eps) = -36, a frame that holds any noise above 0


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    c.use_torch_stream()
    yield c
    c.close()


@pytest.fixture()
def sctx():
    """A context of its own per streaming test: no history from another test."""
    c = _native.Context(0)
    c.use_torch_stream()
    yield c
    c.close()


def _rc(c, name, *args):
    """Return code of the raw C entry (the Context methods cannot pass NULL for a required pointer)."""
    return getattr(c._lib, name)(c._h, *args)


def _code(excinfo):
    return int(re.search(r"\(code (-?\d+)\)", str(excinfo.value)).group(1))


def softmax64(z):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------------------------- softmax
def _softmax_rows(kind, B, C, rng):
    z = (rng.standard_normal((B, C)) * 5).astype(np.float32)
    if kind == "randn5":
        return z
    if kind == "equal":
        return np.repeat((rng.standard_normal((B, 1)) * 5).astype(np.float32), C, axis=1)
    if kind == "offset+1e4":
        return (z + np.float32(1e4)).astype(np.float32)
    if kind == "offset-1e4":
        return (z - np.float32(1e4)).astype(np.float32)
    if kind == "spread200":  # skewed towards the bottom: about three quarters of a row lie more than 104 below its maximum
        z = (-200.0 * np.sqrt(rng.uniform(0, 1, (B, C)))).astype(np.float32)
        if C >= 2:  # the spread is exactly 200 in every row
            j = np.arange(B) % C
            z[np.arange(B), j] = 0.0
            z[np.arange(B), (j + 1) % C] = -200.0
        return z
    if kind == "max_first":
        z[:, 0] = z.max(axis=1) + 3
        return z
    if kind == "max_last":
        z[:, C - 1] = z.max(axis=1) + 3
        return z
    if kind == "max_twice":  # C >= 2
        top = z.max(axis=1) + 1
        j = np.arange(B) % C
        z[np.arange(B), j] = top
        z[np.arange(B), (j + 1 + np.arange(B) % (C - 1)) % C] = top
        return z
    if kind == "neg_inf":    # C >= 2
        z[np.arange(B), np.arange(B) % C] = -np.inf
        return z
    raise ValueError(kind)


SOFTMAX_KINDS = ("randn5", "equal", "offset+1e4", "offset-1e4", "spread200", "max_first", "max_last", "max_twice", "neg_inf")


@pytest.mark.parametrize("C", [1, 2, 12, 35, 64])
@pytest.mark.parametrize("B", [1, 255, 256, 257, 513])
def test_softmax_against_float64_at_grid_and_class_edges(ctx, B, C):
    """kws_softmax_f32 (one thread per row, 256-thread workgroups) at B around the workgroup edges and C from 1 to the maximum,
    for every row content that can go wrong: plain, all-equal (bit-equal outputs, sum 1 within C 2^-24), a common offset of
    +-1e4, a spread of 200 (underflow; the row still sums to 1 within 1e-6), the maximum first / last / duplicated, one -inf
    entry (exactly 0).  The output is allocated 7 rows too long and prefilled with NaN: the rows past B stay NaN."""
    rng = np.random.default_rng(1000 * B + C)
    for kind in SOFTMAX_KINDS:
        if C == 1 and kind in ("max_twice", "neg_inf"):
            continue
        z = _softmax_rows(kind, B, C, rng)
        zd = torch.from_numpy(z).to(DEV)
        out = torch.full((B + 7, C), float("nan"), device=DEV)
        ctx.softmax_f32(zd, out)
        ctx.sync()
        got = out.cpu().numpy()
        assert np.isnan(got[B:]).all(), (kind, "rows past B were written")
        p = got[:B]
        assert not np.isnan(p).any(), kind
        want = softmax64(z)
        err = np.abs(p - want).max()
        assert err <= 1e-6, (kind, err)
        rowsum = p.astype(np.float64).sum(axis=1)
        if kind == "equal":
            assert (_bits(p) == _bits(p)[:, :1]).all()
            assert np.abs(rowsum - 1.0).max() <= C * 2.0 ** -24
        if kind == "spread200":
            assert np.abs(rowsum - 1.0).max() <= 1e-6
            if C >= 12:
                assert (want < 1e-45).mean() > 0.5  # most exponentials do underflow
        if kind == "max_first":
            assert (p.argmax(axis=1) == 0).all()
        if kind == "max_last":
            assert (p.argmax(axis=1) == C - 1).all()
        if kind == "max_twice":
            top = z == z.max(axis=1, keepdims=True)
            assert (top.sum(axis=1) == 2).all()
            pair = _bits(p)[top].reshape(B, 2)
            assert (pair[:, 0] == pair[:, 1]).all() and (p.max(axis=1) == p[top].reshape(B, 2)[:, 0]).all()
        if kind == "neg_inf":
            assert (p[np.isneginf(z)] == 0.0).all() and np.isneginf(z).sum() == B
        if C == 1:
            assert (p == 1.0).all()


def test_softmax_rejects_bad_arguments(ctx):
    z = torch.zeros((4, 64), device=DEV)
    out = torch.full((4, 64), float("nan"), device=DEV)
    zp, op = z.data_ptr(), out.data_ptr()
    assert _rc(ctx, "kws_softmax_f32", zp, 4, 0, op) == _native.KWS_EUNSUPPORTED
    assert _rc(ctx, "kws_softmax_f32", zp, 4, 65, op) == _native.KWS_EUNSUPPORTED
    assert _rc(ctx, "kws_softmax_f32", zp, 4, 12, None) == _native.KWS_EINVAL
    assert _rc(ctx, "kws_softmax_f32", zp, 0, 12, op) == _native.KWS_EINVAL
    assert _rc(ctx, "kws_softmax_f32", zp, -3, 12, op) == _native.KWS_EINVAL
    assert _rc(ctx, "kws_softmax_f32", None, 4, 12, op) == _native.KWS_EINVAL
    ctx.sync()
    assert torch.isnan(out).all()  # a refused call writes nothing
    assert _rc(ctx, "kws_softmax_f32", zp, 4, 64, op) == _native.KWS_OK
    ctx.sync()
    assert bool((out == 1.0 / 64).all())


# ----------------------------------------------------------------------------------------------------------------- smoothing
def tol_smooth(W):
    return 2e-6 + (W + 1) * 2.0 ** -24


def _logits(H, S, C, seed, gain=5.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn((H, S, C), generator=g) * gain).to(DEV)


def _smooth(c, z, W, want_label=True):
    """kws_stream_smooth_f32 hop after hop on device logits [H, S, C]: (smoothed float32 [H, S, C], labels int32 [H, S]) on the host."""
    H, S, C = z.shape
    sm = torch.full((H, S, C), float("nan"), device=DEV)
    lb = torch.full((H, S), -1, dtype=torch.int32, device=DEV)
    for h in range(H):
        c.stream_smooth_f32(z[h], W, sm[h], lb[h] if want_label else None)
    c.sync()
    return sm.cpu().numpy(), lb.cpu().numpy()


def _mean_last(P, W):
    """float64 [H, ...] -> the mean over the last min(h + 1, W) hops, for every hop h."""
    out = np.empty_like(P)
    for h in range(P.shape[0]):
        out[h] = P[max(0, h - W + 1):h + 1].mean(axis=0)
    return out


def _check_smooth(name, z, W, sm, lb, hops=None, margin_rule=True):
    """Smoothed posteriors of a run that began with an empty history against float64 at `hops` (default: all), its labels at
    every hop."""
    H, S, C = z.shape
    ref = _mean_last(softmax64(z.cpu().numpy()), W)
    hops = np.arange(H) if hops is None else np.asarray(sorted(set(hops)))
    tol = tol_smooth(W)
    assert not np.isnan(sm).any(), name
    ratio = np.abs(sm[hops] - ref[hops]).max() / tol
    got, want, labels = sm, ref, lb
    excluded = 0.0
    if margin_rule:
        if C >= 2:
            top2 = np.sort(want, axis=-1)[..., -2:]
            clear = (top2[..., 1] - top2[..., 0]) > 2 * tol
        else:
            clear = np.ones(labels.shape, bool)
        excluded = 1.0 - clear.mean()
    print(f"[stream-decisions] smooth {name}: worst err/tol {ratio:.4f}, label rows excluded by the margin rule {100 * excluded:.2f} %")
    assert ratio <= 1.0, (name, ratio)
    assert np.array_equal(labels, got.argmax(axis=-1)), (name, "the label is not the first maximum of the smoothed row")
    if margin_rule:
        assert np.array_equal(labels[clear], want.argmax(axis=-1)[clear]), name
        assert excluded <= 0.05, (name, excluded)
    return ratio


@pytest.mark.parametrize("S", [1, 63, 64, 65, 130])
def test_smoothing_hop_counter_across_workgroups(sctx, S):
    """One thread per stream in 64-thread workgroups: beyond 64 streams every workgroup reads the hop count and the last one to
    finish advances it.  Every hop is compared -- a count that advanced twice, or not at all, shows in hop 1's divisor and hop 3's
    ring slot (W = 3), in every stream."""
    z = _logits(10, S, 12, seed=S)
    sctx.stream_open(S)
    sm, lb = _smooth(sctx, z, 3)
    _check_smooth(f"S={S} W=3 C=12", z, 3, sm, lb)


def test_smoothing_window_of_one_is_the_softmax(sctx):
    z = _logits(9, 3, 12, seed=11)
    sctx.stream_open(3)
    sm, lb = _smooth(sctx, z, 1)
    p = torch.full((9, 3, 12), float("nan"), device=DEV)
    for h in range(9):
        sctx.softmax_f32(z[h], p[h])
    sctx.sync()
    assert np.array_equal(_bits(sm), _bits(p.cpu().numpy()))
    _check_smooth("S=3 W=1 C=12", z, 1, sm, lb)


@pytest.mark.parametrize("W,hops", [(2, 8), (7, 23), (64, 200)])
def test_smoothing_windows_and_rebuilds(sctx, W, hops):
    """W = 2 and 7 over 3 W + 2 hops (three rebuilds of the running sum); W = 64 over 200 hops: longer than the first 63 hops of
    history, so the divisor is count + 1 there."""
    z = _logits(hops, 3, 12, seed=100 + W)
    sctx.stream_open(3)
    sm, lb = _smooth(sctx, z, W)
    _check_smooth(f"S=3 W={W} C=12 hops={hops}", z, W, sm, lb)


def test_smoothing_largest_window_and_window_errors(sctx):
    """W = 4096 is accepted (S = 2, C = 12: a 393 KB ring) and its first 5 hops divide by count + 1; 0 and 4097 are refused."""
    z = _logits(5, 2, 12, seed=4096)
    sctx.stream_open(2)
    sm, lb = _smooth(sctx, z, 4096)
    _check_smooth("S=2 W=4096 C=12 hops=5", z, 4096, sm, lb)
    zp, op = z[0].data_ptr(), torch.empty((2, 12), device=DEV).data_ptr()
    assert _rc(sctx, "kws_stream_smooth_f32", zp, 12, 0, op, None) == _native.KWS_EINVAL
    assert _rc(sctx, "kws_stream_smooth_f32", zp, 12, 4097, op, None) == _native.KWS_EINVAL
    assert _rc(sctx, "kws_stream_smooth_f32", zp, 12, -1, op, None) == _native.KWS_EINVAL
    assert _rc(sctx, "kws_stream_smooth_f32", None, 12, 4, op, None) == _native.KWS_EINVAL
    assert _rc(sctx, "kws_stream_smooth_f32", zp, 12, 4, None, None) == _native.KWS_EINVAL


@pytest.mark.parametrize("C", [1, 2, 35, 64])
def test_smoothing_class_counts(sctx, C):
    z = _logits(12, 5, C, seed=200 + C)
    sctx.stream_open(5)
    sm, lb = _smooth(sctx, z, 4)
    _check_smooth(f"S=5 W=4 C={C}", z, 4, sm, lb)
    if C == 1:
        assert (sm == 1.0).all() and (lb == 0).all()


def test_smoothing_refuses_too_many_classes_and_a_closed_stream_set(sctx):
    z = torch.zeros((5, 65), device=DEV)
    out = torch.empty((5, 65), device=DEV)
    assert _rc(sctx, "kws_stream_smooth_f32", z.data_ptr(), 12, 4, out.data_ptr(), None) == _native.KWS_ESTATE  # never opened
    sctx.stream_open(5)
    assert _rc(sctx, "kws_stream_smooth_f32", z.data_ptr(), 65, 4, out.data_ptr(), None) == _native.KWS_EUNSUPPORTED
    assert _rc(sctx, "kws_stream_smooth_f32", z.data_ptr(), 0, 4, out.data_ptr(), None) == _native.KWS_EUNSUPPORTED
    assert _rc(sctx, "kws_stream_smooth_f32", z.data_ptr(), 64, 4, out.data_ptr(), None) == _native.KWS_OK
    sctx.stream_close()
    with pytest.raises(KWSError) as e:
        sctx.stream_smooth_f32(z[:, :12].contiguous(), 4, out)
    assert _code(e) == _native.KWS_ESTATE


def test_smoothing_drift_over_5000_hops(sctx):
    """The running sum is rebuilt from the ring every W hops so that its float32 error does not grow over a stream's life:
    5000 hops at W = 7 (714 rebuilds) with logits randn x 30, whose posteriors swing between about 0 and about 1; hops 0-20, every
    499th hop and the last 8 stay within tol(7).  The labels are judged at all 5000 hops: posteriors this close to one-hot make the
    smoothed top two an exact tie (k / 7 each) in about 4 % of the rows, which 78 rows would not measure against the 5 % bound."""
    H = 5000
    z = _logits(H, 2, 12, seed=5000, gain=30.0)
    sctx.stream_open(2)
    sm, lb = _smooth(sctx, z, 7)
    hops = list(range(21)) + list(range(0, H, 499)) + list(range(H - 8, H))
    _check_smooth("drift S=2 W=7 C=12 hops=5000 randn x 30", z, 7, sm, lb, hops=hops)
    p = softmax64(z.cpu().numpy())
    assert (p.max(axis=-1) > 0.99).mean() > 0.5 and (p < 1e-6).mean() > 0.5  # the posteriors do swing


def test_smoothing_ties_go_to_the_lower_index(sctx):
    """Classes 2 and 7 carry identical logits at every hop: their smoothed values are bit-equal at every hop, rebuild hops
    (every 4th) included, and when the pair leads the label is 2.  Against float64 the pair counts as one class: the label is the
    float64 argmax (NumPy's first maximum) wherever the margin to the best other class exceeds 2 tol."""
    H, S, C, W, lo, hi = 30, 3, 12, 4, 2, 7
    z = _logits(H, S, C, seed=77)
    z[:, :, lo] += 14.0 * (torch.arange(H, device=DEV) % 3 != 0).float()[:, None]  # the pair leads in most hops
    z[:, :, hi] = z[:, :, lo]
    sctx.stream_open(S)
    sm, lb = _smooth(sctx, z, W)
    _check_smooth(f"ties S={S} W={W} C={C}", z, W, sm, lb, margin_rule=False)
    assert np.array_equal(_bits(sm[..., lo]), _bits(sm[..., hi]))
    leads = sm[..., lo] == sm.max(axis=-1)
    assert 0.5 < leads.mean() < 1.0
    assert (lb[leads] == lo).all() and (lb[~leads] != hi).all()
    ref = _mean_last(softmax64(z.cpu().numpy()), W)
    others = np.delete(ref, hi, axis=-1)
    top2 = np.sort(others, axis=-1)[..., -2:]
    clear = (top2[..., 1] - top2[..., 0]) > 2 * tol_smooth(W)
    assert np.array_equal(lb[clear], ref.argmax(axis=-1)[clear]) and clear.mean() >= 0.95


def test_smoothing_history_restarts(sctx):
    """A change of window, a change of C, and kws_stream_open each restart the history: the next output is the softmax of that
    hop alone (1e-6), the one after it the mean of two -- after reopening with more streams (70: two workgroups) for all of them."""
    def first_two(z, W, name):
        sm, lb = _smooth(sctx, z, W)
        p = softmax64(z.cpu().numpy())
        assert np.abs(sm[0] - p[0]).max() <= 1e-6, name
        _check_smooth(name, z, W, sm, lb)

    sctx.stream_open(3)
    z = _logits(9, 3, 12, seed=31, gain=8.0)
    sm, lb = _smooth(sctx, z, 4)
    _check_smooth("restart: 9 hops at W=4", z, 4, sm, lb)
    first_two(_logits(2, 3, 12, seed=32, gain=8.0), 5, "restart: W 4 -> 5")
    first_two(_logits(2, 3, 7, seed=33, gain=8.0), 5, "restart: C 12 -> 7")
    sctx.stream_close()
    sctx.stream_open(70)
    first_two(_logits(2, 70, 7, seed=34, gain=8.0), 5, "restart: reopened with S 3 -> 70")
    # and the same window and C again after a window in between start from nothing as well
    first_two(_logits(2, 70, 7, seed=35, gain=8.0), 6, "restart: W 5 -> 6")
    first_two(_logits(2, 70, 7, seed=36, gain=8.0), 5, "restart: W 6 -> 5")


def test_smoothing_without_a_label_buffer(sctx):
    z = _logits(11, 5, 12, seed=41)
    sctx.stream_open(5)
    with_label, lb = _smooth(sctx, z, 4)
    sctx.stream_close()
    sctx.stream_open(5)
    without, untouched = _smooth(sctx, z, 4, want_label=False)
    assert np.array_equal(_bits(with_label), _bits(without)) and (untouched == -1).all() and (lb >= 0).all()


# ---------------------------------------------------------------------------------------------------------------- endpointer
def _pcm(pattern, seed):
    """Voiced / unvoiced pattern bool [S, H] -> int16 [S, H * 160]: a voiced hop is uniform noise in +-20000 whose last sample is
    0 (pre-emphasis then leaks nothing into the next frame), an unvoiced hop is zeros."""
    pattern = np.asarray(pattern, bool)
    S, H = pattern.shape
    x = np.random.default_rng(seed).integers(-20000, 20001, size=(S, H, STEP)).astype(np.int16)
    x[:, :, STEP - 1] = 0
    x[~pattern] = 0
    return x.reshape(S, H * STEP)


def _delayed(base, delays):
    """One stream per entry of `delays`: the base pattern, that many hops late."""
    base = np.asarray(base, bool)
    out = np.zeros((len(delays), len(base)), bool)
    for s, d in enumerate(delays):
        out[s, d:] = base[:len(base) - d]
    return out


def _cycles(on, off, hops):
    """Silence, then voiced runs long enough to open and pauses long enough to close, repeated; from on = 10 up every run has a
    dropout of three hops (one unvoiced frame) near its start."""
    run = [True] * (on + 8)
    if on >= 10:
        run[3:6] = [False] * 3
    cycle = run + [False] * (off + 6)
    return ([False] * 4 + cycle * (hops // len(cycle) + 1))[:hops]


def _oracle_states(pcm, on, off, first_hop=0, last_hop=None):
    """What kws_stream_vad_f32 reports after each of the pushes first_hop .. last_hop - 1 of `pcm` when its history starts empty at
    first_hop: int [hops, S], and per stream and hop (voiced of the last `on` flags, voiced of all `off` flags, event, newest
    flag) as the oracle's flag deque shows them (None while no frame is complete)."""
    S, H = pcm.shape[0], pcm.shape[1] // STEP
    last_hop = H if last_hop is None else last_hop
    want = np.zeros((last_hop - first_hop, S), np.int32)
    stats = [[None] * (last_hop - first_hop) for _ in range(S)]
    for s in range(S):
        c0 = o_mfcc.mfcc(o_mfcc.pcm16_to_float(pcm[s]), o_mfcc.FrontendSpec(n_samples=pcm.shape[1]))[:, 0]
        ref = EnergyEndpointer(THR, on, off)
        for t in range(first_hop, last_hop):
            if t < LAG - 1:
                continue
            v = float(c0[t - (LAG - 1)])
            assert abs(v - THR) > 3.0, (s, t, v)  # a float32 log energy never decides a case
            trig, ev = ref.update(v)
            flags = list(ref.flags)
            want[t - first_hop, s] = int(trig) | (ev << 1)
            stats[s][t - first_hop] = (sum(flags[-on:]), sum(flags), ev, flags[-1])
    return want, stats


def _to_hops(pcm):
    """int16 [S, H * 160] on the host -> [H, S, 160] on the device, one contiguous [S, 160] block per push."""
    S = pcm.shape[0]
    return torch.from_numpy(np.ascontiguousarray(pcm.reshape(S, -1, STEP).transpose(1, 0, 2))).to(DEV)


def _vad(c, hops_dev, on, off, first_hop=0, last_hop=None):
    last_hop = hops_dev.shape[0] if last_hop is None else last_hop
    st = torch.full((last_hop - first_hop, hops_dev.shape[1]), -1, dtype=torch.int32, device=DEV)
    for t in range(first_hop, last_hop):
        c.stream_push_i16(hops_dev[t])
        c.stream_vad_f32(THR, on, off, st[t - first_hop])
    c.sync()
    return st.cpu().numpy()


def _events(want):
    return [[(t, int(v) >> 1) for t, v in enumerate(want[:, s]) if v >> 1] for s in range(want.shape[1])]


@pytest.mark.parametrize("on,off", [(1, 1), (1, 5), (3, 3), (5, 10), (10, 20), (40, 80)])
def test_endpointer_windows(sctx, on, off):
    """Two streams (the second three hops late) over at least 3 off + 20 hops, so the cursor wraps the flag ring at least three
    times; every utterance opens and closes at least twice.  State bit 0 and the event bits equal the oracle's at every hop,
    and the first two hops (no complete frame) report 0."""
    run_and_pause = (on + 8) + (off + 6)
    hops = max(3 * off + 20, 4 + 2 * run_and_pause + 3 + 2)
    pcm = _pcm(_delayed(_cycles(on, off, hops), [0, 3]), seed=on * 100 + off)
    want, _ = _oracle_states(pcm, on, off)
    for ev in _events(want):
        assert [k for _, k in ev].count(1) >= 2 and [k for _, k in ev].count(2) >= 2, ev
    sctx.stream_open(2)
    got = _vad(sctx, _to_hops(pcm), on, off)
    assert (got[:LAG - 1] == 0).all()
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def test_endpointer_inequality_edges_at_10_20(sctx):
    """Open: 10 n_on > 8 on.  Close: 10 (off - n_all) > 9 off.  The oracle's flag deque, asserted here, passes through
    8 of the last 10 voiced while closed (no event, twice: once with the run still growing, once with an unvoiced frame inside),
    then 9 of 10 (opens); while open through 3 voiced of the last 20 that all come from ONE voiced hop (a frame spans three hops;
    the utterance stays open) and exactly 2 of 20 (18 unvoiced: 180 > 180 is false, no event); then exactly 1 of 20 -- 19 unvoiced,
    190 > 180 -- which closes, as oracle.endpointer and the rule it restates (more than 90 % unvoiced) have it; 0 of 20 is then
    reached while closed, with no event."""
    on, off, a = 10, 20, 5
    p = np.zeros(120, bool)
    p[a + 2:a + 8] = True     # frames a .. a+7 voiced: 8 of 10
    p[a + 11:a + 31] = True   # frame a+8 unvoiced (still 8 of 10), frame a+9 voiced: 9 of 10
    p[a + 43] = True          # one voiced hop 12 hops after the run: alone in the last 20 frames for a while
    p[a + 75:a + 90] = True   # and a second utterance
    pcm = _pcm(p[None], seed=1020)
    want, stats = _oracle_states(pcm, on, off)
    st = stats[0]
    seq = [(t, x) for t, x in enumerate(st) if x is not None]
    opened = [t for t, x in seq if x[2] == 1]
    closed = [t for t, x in seq if x[2] == 2]
    assert len(opened) == 2 and len(closed) == 2 and opened[0] < closed[0] < opened[1] < closed[1]
    before = [x for t, x in seq if t < opened[0]]
    assert [x[0] for x in before][-2:] == [8, 8] and all(x[2] == 0 for x in before) and st[opened[0]][0] == 9
    held = [x for t, x in seq if opened[0] < t < closed[0]]
    assert any(x[1] == 3 for x in held[-14:]) and held[-1][1] == 2 and all(x[2] == 0 for x in held)
    assert st[closed[0]][1] == 1 and st[closed[0] + 1][1] == 0 and st[closed[0] + 1][2] == 0
    sctx.stream_open(1)
    got = _vad(sctx, _to_hops(pcm), on, off)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert got[opened[0] - 1, 0] == 0 and got[opened[0], 0] == 3 and got[closed[0] - 1, 0] == 1 and got[closed[0], 0] == 4


def test_endpointer_longest_off_window(sctx):
    """(10, 1024) is accepted and followed for 1100 hops, so the cursor wraps the 1024-flag ring.  Stream 0 is voiced
    throughout: it opens at once and -- the history before the stream counting as unvoiced -- closes and reopens until more than
    a tenth of the last 1024 flags are voiced (103), then stays open to the end.  Stream 1 has a voiced run and afterwards a single
    voiced hop inside every 1024: by the closing rule (more than 90 % of the last 1024 unvoiced) it cannot stay open, and the
    device closes it where the oracle does.

    Then (1024, 1024) over the same 1100 hops: a flag leaves BOTH windows through the slot the new one takes.  Stream 0 has a
    short voiced run, a pause and is voiced from then on, so that it opens only at a frame of 1024 or later, when voiced frames
    of the run have left the window: a count that never subtracts a leaving flag would open it earlier.  Stream 1 never opens."""
    on, off, H = 10, 1024, 1100
    p = np.zeros((2, H), bool)
    p[0, 4:] = True
    p[1, 4:30] = True
    p[1, 600] = True
    pcm = _pcm(p, seed=1024)
    want, stats = _oracle_states(pcm, on, off)
    ev0 = _events(want)[0]
    assert want[-1, 0] == 1 and ev0[-1][1] == 1 and stats[0][ev0[-1][0]][1] == 103 and len(ev0) > 3
    assert want[-1, 1] == 0 and len(_events(want)[1]) >= 2
    sctx.stream_open(2)
    got = _vad(sctx, _to_hops(pcm), on, off)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]

    on = off = 1024
    p = np.zeros((2, H), bool)
    p[0, 4:34] = True
    p[0, 252:] = True
    p[1, 4:30] = True
    p[1, 600] = True
    pcm = _pcm(p, seed=2048)
    want, stats = _oracle_states(pcm, on, off)
    ev0, ev1 = _events(want)
    voiced = [x[3] for x in stats[0] if x is not None]  # the oracle's flag of every frame
    first_open = ev0[0][0] - (LAG - 1)                  # as a frame index
    assert ev0[0][1] == 1 and first_open >= 1024 and sum(voiced[:first_open - 1023]) > 0  # voiced frames have left the window
    never_leaving = next(f for f in range(len(voiced)) if 10 * sum(voiced[:f + 1]) > 8 * on)
    assert never_leaving != first_open and not ev1
    sctx.stream_close()
    sctx.stream_open(2)
    got = _vad(sctx, _to_hops(pcm), on, off)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


_COUNTS = {}


def _counts_case():
    """130 streams at (5, 10), shared by the stream-count cases: PCM, the oracle's states and the device copy of the hops."""
    if not _COUNTS:
        pcm = _pcm(_delayed(_cycles(5, 10, 70), [s % 7 for s in range(130)]), seed=510)
        want, _ = _oracle_states(pcm, 5, 10)
        _COUNTS.update(pcm=pcm, want=want)
    return _COUNTS["pcm"], _COUNTS["want"]


@pytest.mark.parametrize("S", [1, 63, 64, 65, 130])
def test_endpointer_stream_counts(sctx, S):
    """One thread per stream, 64 per workgroup: 130 streams make three.  Stream s carries the base pattern delayed by s mod 7
    hops, so neighbouring lanes and workgroups differ; every stream at every hop."""
    pcm, want = _counts_case()
    assert len({tuple(want[:, s]) for s in range(7)}) == 7
    sctx.stream_open(S)
    got = _vad(sctx, _to_hops(pcm[:S]), 5, 10)
    assert np.array_equal(got, want[:, :S]), np.argwhere(got != want[:, :S])[:5]


def test_endpointer_history_restarts(sctx):
    """A change of (on, off) mid-stream restarts the flags (the oracle restarts at that hop): changed inside an utterance, the
    stream is closed again and reopens under the new windows.  kws_stream_open restarts them too: a second signal that begins
    silent after a first one that ended inside an utterance."""
    base = np.zeros(64, bool)
    base[4:40] = True
    pcm = _pcm(_delayed(base, [0, 1, 2]), seed=77)
    r = 25
    first, _ = _oracle_states(pcm, 5, 10, 0, r)
    second, _ = _oracle_states(pcm, 3, 3, r, 64)
    assert (first[-1] & 1).all() and (second[0] == 0).all() and all(e and e[0][1] == 1 for e in _events(second))
    sctx.stream_open(3)
    hops = _to_hops(pcm)
    got = np.concatenate([_vad(sctx, hops, 5, 10, 0, r), _vad(sctx, hops, 3, 3, r, 64)])
    assert np.array_equal(got, np.concatenate([first, second]))

    a = np.zeros(30, bool)
    a[4:] = True
    b = np.zeros(48, bool)
    b[15:30] = True
    pcm_a, pcm_b = _pcm(_delayed(a, [0, 1, 2]), seed=78), _pcm(_delayed(b, [s % 7 for s in range(66)]), seed=79)
    want_a, _ = _oracle_states(pcm_a, 3, 3)
    want_b, _ = _oracle_states(pcm_b, 3, 3)
    assert (want_a[-1] & 1).all() and (want_b[:12] == 0).all() and all(len(e) == 2 for e in _events(want_b))
    sctx.stream_open(3)
    got_a = _vad(sctx, _to_hops(pcm_a), 3, 3)
    sctx.stream_open(66)                        # the same (3, 3): only kws_stream_open lies between the two histories
    got_b = _vad(sctx, _to_hops(pcm_b), 3, 3)
    assert np.array_equal(got_a, want_a) and np.array_equal(got_b, want_b)


def test_endpointer_rejects_bad_arguments(sctx):
    st = torch.full((3,), -1, dtype=torch.int32, device=DEV)
    sp = st.data_ptr()
    thr = THR
    assert _rc(sctx, "kws_stream_vad_f32", thr, 5, 10, sp) == _native.KWS_ESTATE  # no open streams
    sctx.stream_open(3)
    assert _rc(sctx, "kws_stream_vad_f32", thr, 0, 10, sp) == _native.KWS_EINVAL
    assert _rc(sctx, "kws_stream_vad_f32", thr, 6, 5, sp) == _native.KWS_EINVAL
    assert _rc(sctx, "kws_stream_vad_f32", thr, 10, 1025, sp) == _native.KWS_EINVAL
    assert _rc(sctx, "kws_stream_vad_f32", thr, 5, 10, None) == _native.KWS_EINVAL
    sctx.sync()
    assert bool((st == -1).all())
    assert _rc(sctx, "kws_stream_vad_f32", thr, 1024, 1024, sp) == _native.KWS_OK
    sctx.sync()
    assert bool((st == 0).all())  # no push yet: no complete frame
    sctx.stream_close()
    with pytest.raises(KWSError) as e:
        sctx.stream_vad_f32(THR, 5, 10, st)
    assert _code(e) == _native.KWS_ESTATE
