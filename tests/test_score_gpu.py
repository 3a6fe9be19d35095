"""Scoring a scan against annotations over a threshold sweep on the GPU (kws_scan_score_f32, kws_scan_score_ragged_f32,
KeywordSpotter.score).

The contract is equality with kws_scan_detect_f32: for every threshold of a sweep the counts must be those of the brute-force
matcher of tests/_score_ref.py over the events kws_scan_detect_f32 fires at that threshold on the same logits.  Every comparison is
exact integer equality.  The counters are prefilled with a sentinel and over-allocated by one threshold's rows: all of [K, C, 4]
must be written and nothing beyond."""
import ctypes

import numpy as np
import pytest
import torch

import _scan_ref as sref
import _score_ref as ref
from kws import _native

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = -0x0123456789ABCDEF
NAN = float("nan")


@pytest.fixture(scope="module")
def ctx():
    """A context without a model: the decisions and their scoring need none."""
    c = _native.Context(0)
    c.use_torch_stream()
    yield c
    c.close()


def detect(ctx, zd, S, fk, threshold, refractory, want_scores=False):
    """kws_scan_detect_f32 with max_events = W -> per recording the list of (window, label) [and the scores]."""
    R, W, _ = zd.shape
    count = torch.zeros((R,), dtype=torch.int32, device=DEV)
    ev_w, ev_k = (torch.zeros((R, W), dtype=torch.int32, device=DEV) for _ in range(2))
    ev_s = torch.zeros((R, W), device=DEV)
    ctx.scan_detect_f32(zd, S, fk, threshold, refractory, count, ev_w, ev_k, ev_s, W)
    torch.cuda.synchronize()
    count, ev_w, ev_k, ev_s = count.cpu().numpy(), ev_w.cpu().numpy(), ev_k.cpu().numpy(), ev_s.cpu().numpy()
    assert (count <= W).all()
    events = [[(int(ev_w[r, i]), int(ev_k[r, i])) for i in range(count[r])] for r in range(R)]
    return (events, [ev_s[r, :count[r]] for r in range(R)]) if want_scores else events


def counters(K, Cn):
    return torch.full((K + 1, Cn, 4), SENTINEL, dtype=torch.int64, device=DEV)


def read(counts):
    torch.cuda.synchronize()
    host = counts.cpu().numpy()
    assert (host[-1] == SENTINEL).all(), "counters were written beyond [K, C, 4]"
    assert (host[:-1] >= 0).all(), "a counter was not written"
    return host[:-1]


def score(ctx, zd, S, fk, refractory, thresholds, truth):
    counts = counters(len(thresholds), zd.shape[2])
    ctx.scan_score_f32(zd, S, fk, refractory, thresholds, truth, counts[:-1])
    return read(counts)


def score_ragged(ctx, zd, win_off, windows, S, fk, refractory, thresholds, truth):
    counts = counters(len(thresholds), zd.shape[1])
    ctx.scan_score_ragged_f32(zd, win_off, windows, S, fk, refractory, thresholds, truth, counts[:-1])
    return read(counts)


def edge_threshold(ctx, zd, S, fk):
    """A window's own smoothed score, bit for bit, from kws_scan_detect_f32's d_smoothed: the median top score of the windows whose
    argmax is a keyword (of all windows if there is none).  Returns (threshold, whether a keyword window has exactly that score)."""
    R, W, Cn = zd.shape
    count = torch.zeros((R,), dtype=torch.int32, device=DEV)
    smoothed = torch.zeros((R, W, Cn), device=DEV)
    ctx.scan_detect_f32(zd, S, fk, 0.0, 1, count, smoothed=smoothed)
    torch.cuda.synchronize()
    top, arg = smoothed.reshape(-1, Cn).max(dim=1)
    keyword = top[arg >= fk]
    pool = np.sort((keyword if len(keyword) else top).cpu().numpy())
    return float(pool[len(pool) // 2]), bool(len(keyword))


# ---- 1. equality with kws_scan_detect_f32 ------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 7, 256])
@pytest.mark.parametrize("Cn", [2, 12, 64])
@pytest.mark.parametrize("W", [1, 63, 64, 65, 200])
def test_counts_are_the_matched_events_of_detect(ctx, W, Cn, S):
    R = 3
    fk = 0 if Cn == 2 else 2  # with two classes and first_keyword 2 nothing could fire
    zd = torch.from_numpy(sref.detect_logits(W, Cn, sref.DETECT_SEEDS[(W, Cn)])).to(DEV)
    edge, edge_fires = edge_threshold(ctx, zd, S, fk)
    thresholds = np.array([0.0, 0.5, 1.0, 1.5, NAN, edge], np.float32)
    assert thresholds[5] == np.float32(edge)
    truth = ref.random_truth(np.random.default_rng(1000 * W + 10 * Cn + S), R, Cn, W, fk)
    fired = 0
    for refractory in (1, 50, W + 1):
        got = score(ctx, zd, S, fk, refractory, thresholds, truth)
        for i, t in enumerate(thresholds):
            events = detect(ctx, zd, S, fk, float(t), refractory)
            what = f"refractory {refractory}, threshold {t!r}"
            np.testing.assert_array_equal(got[i], ref.match_brute(events, truth, Cn), err_msg=what)
            assert got[i, :, :3].sum() == sum(len(e) for e in events), what
            fired += sum(len(e) for e in events)
            if i == 5 and refractory == 1 and edge_fires:  # the >= edge: the window whose score the threshold is fires
                _, scores = detect(ctx, zd, S, fk, float(t), 1, want_scores=True)
                assert np.float32(edge) in np.concatenate(scores)
        assert got[4].sum() == 0 and got[3].sum() == 0, "NaN and 1.5 fire nothing"
    assert fired > 0 or not edge_fires  # one window per recording may be no keyword at all


# ---- 2. annotation edges ---------------------------------------------------------------------------------------------
def edge_truth(events, W):
    """Annotations built from the events of three recordings (refractory 5) so that every situation of the matching rule occurs;
    each block asserts, with the brute-force matcher on its own rows, that it does.  Returns the table."""
    C = 12
    alone = lambda rows, r: ref.match_brute([e if i == r else [] for i, e in enumerate(events)], rows, C)
    rows = []
    # recording 0: one window exactly at the first event; the last event inside an interval that ends beyond W
    (w0, k0), (wl, kl) = events[0][0], events[0][-1]
    assert wl > w0
    block = [(0, k0, w0, w0), (0, kl, wl, W + 50)]
    got = alone(block, 0)
    assert got[:, 0].sum() == 2 and got[:, 3].sum() == 0, "both are hits at latency 0"
    rows += block
    # recording 1: one window before and one after an event: the event is a false alarm; later, overlapping intervals of two labels
    w, k = next(e for e in events[1] if e[0] >= 1)
    block = [(1, k, w - 1, w - 1), (1, k, w + 1, w + 1)]
    assert alone(block, 1)[k, 0] == 0 and alone(block, 1)[:, 1].sum() == len(events[1])
    rows += block
    wd, kd = next(e for e in events[1] if e[0] >= w + 10)
    other = 2 if kd != 2 else 3
    block = [(1, kd, wd - 2, wd + 2), (1, other, wd - 3, wd + 3)]
    got = alone(block, 1)
    assert got[kd, 0] == 1 and got[kd, 3] == 2 and got[other, 0] == sum(1 for e in events[1] if e[1] == other and wd - 3 <= e[0] <= wd + 3)
    rows += block
    # recording 0 again: an interval straddling windows 63 | 64 with an event of its label on either side: a hit, then a duplicate
    ws, ks = next(e for e in events[0] if 60 <= e[0] <= 63)
    assert any(e[1] == ks and 64 <= e[0] <= 67 for e in events[0]) and (ks != k0 or w0 < 60) and (ks != kl or wl > 67)
    block = [(0, ks, 60, 67)]
    got = alone(block, 0)
    assert got[ks, 0] == 1 and got[ks, 2] >= 1 and got[ks, 3] == ws - 60
    rows += block
    # recording 2: two adjacent intervals [a, b], [b + 1, c], each hit once
    pair = next((a, b) for a, b in zip(events[2], events[2][1:]) if a[1] == b[1])
    (w1, kp), (w2, _) = pair
    block = [(2, kp, w1, w1 + 2), (2, kp, w1 + 3, w2)]
    got = alone(block, 2)
    assert got[kp, 0] == 2 and got[kp, 3] == w2 - (w1 + 3)
    rows += block
    return np.asarray(rows, np.int32), ks


def test_annotation_edges(ctx):
    W, Cn, S, fk = 200, 12, 7, 2
    zd = torch.from_numpy(sref.detect_logits(W, Cn, sref.DETECT_SEEDS[(W, Cn)])).to(DEV)
    truth, ks = edge_truth(detect(ctx, zd, S, fk, 0.5, 5), W)
    thresholds = np.array([0.5, 0.9], np.float32)
    dups = 0
    for refractory in (1, 5):  # 1: every window of a label's run fires, so intervals collect duplicates, across 63 | 64 too
        got = score(ctx, zd, S, fk, refractory, thresholds, truth[::-1])
        for i, t in enumerate(thresholds):
            events = detect(ctx, zd, S, fk, float(t), refractory)
            np.testing.assert_array_equal(got[i], ref.match_brute(events, truth, Cn))
            if refractory == 1 and i == 0:
                assert sum(1 for w, k in events[0] if 60 <= w <= 63 and k == ks) > 1 and \
                    sum(1 for w, k in events[0] if 64 <= w <= 67 and k == ks) > 1, "events on both sides of 63 | 64"
        dups += got[:, :, 2].sum()
    assert dups > 0
    # no annotations: every event is a false alarm (a NULL table and an empty one)
    events = detect(ctx, zd, S, fk, 0.5, 5)
    for none in (None, np.zeros((0, 4), np.int32)):
        got = score(ctx, zd, S, fk, 5, [0.5], none)  # K = 1
        assert got.shape == (1, Cn, 4) and got[0, :, 1].sum() == sum(len(e) for e in events) and got[0, :, [0, 2, 3]].sum() == 0
        np.testing.assert_array_equal(got[0], ref.match_brute(events, [], Cn))


def test_one_threshold_and_1024(ctx):
    W, Cn, S, fk, refractory = 200, 12, 7, 2, 5
    zd = torch.from_numpy(sref.detect_logits(W, Cn, sref.DETECT_SEEDS[(W, Cn)])).to(DEV)
    truth = ref.random_truth(np.random.default_rng(3), 3, Cn, W, fk)
    thresholds = np.linspace(1.2, 0.0, 1024).astype(np.float32)  # descending: any order is fine
    sweep = score(ctx, zd, S, fk, refractory, thresholds, truth)
    assert (sweep[0] == 0).all() and sweep[-1].sum() > 0
    assert len({sweep[i].tobytes() for i in range(1024)}) > 3, "the sweep distinguishes thresholds"
    for i in list(range(0, 1024, 73)) + [1020, 1021, 1022, 1023]:
        one = score(ctx, zd, S, fk, refractory, thresholds[i:i + 1], truth)
        np.testing.assert_array_equal(one[0], sweep[i])
        np.testing.assert_array_equal(sweep[i], ref.match_brute(detect(ctx, zd, S, fk, float(thresholds[i]), refractory), truth, Cn))


# ---- 3. ragged -------------------------------------------------------------------------------------------------------
def ragged_case():
    """Recordings of 0, 1, 64, 65 and 130 windows packed with gaps: (per-recording logits, win_off, windows, packed rows)."""
    Cn = 12
    windows = [0, 1, 64, 65, 130]
    win_off = [3, 3, 6, 71, 136]  # 3 rows before the first, 2 between recordings 1 and 2, 1 before 3, none before 4, 4 at the end
    recs = [sref.detect_logits(max(w, 1), Cn, [40 + r])[0][:w] for r, w in enumerate(windows)]
    return recs, win_off, windows, 136 + 130 + 4


def pack(recs, win_off, rows, fill):
    z = np.full((rows, recs[1].shape[1]), fill, np.float32)
    for rec, o in zip(recs, win_off):
        z[o:o + len(rec)] = rec
    return torch.from_numpy(z).to(DEV)


@pytest.mark.parametrize("refractory", [1, 50])
def test_ragged_is_the_sum_of_the_recordings_alone(ctx, refractory):
    Cn, S, fk = 12, 7, 2
    recs, win_off, windows, rows = ragged_case()
    thresholds = np.array([0.0, 0.5, 0.9, NAN], np.float32)
    truth = ref.random_truth(np.random.default_rng(8), len(recs), Cn, 130, fk)  # intervals beyond a short recording's end included
    got = score_ragged(ctx, pack(recs, win_off, rows, NAN), win_off, windows, S, fk, refractory, thresholds, truth)
    want = np.zeros_like(got)
    for r, rec in enumerate(recs):
        if len(rec):
            own = truth[truth[:, 0] == r].copy()
            own[:, 0] = 0
            want += score(ctx, torch.from_numpy(rec[None]).to(DEV), S, fk, refractory, thresholds, own)
    np.testing.assert_array_equal(got, want)
    assert got[0, :, 0].sum() > 0 and got[0, :, 1].sum() > 0
    # what the rows of no recording hold changes nothing
    again = score_ragged(ctx, pack(recs, win_off, rows, 50.0), win_off, windows, S, fk, refractory, thresholds, truth)
    np.testing.assert_array_equal(again, got)


def test_ragged_without_any_window_gives_zeros(ctx):
    z = torch.full((8, 12), NAN, device=DEV)
    truth = np.array([[0, 2, 0, 5], [1, 3, 1, 1]], np.int32)
    got = score_ragged(ctx, z, [0, 4], [0, 0], 7, 2, 5, [0.0, 0.5], truth)
    assert got.shape == (2, 12, 4) and (got == 0).all()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_counters_and_the_context_alone(ctx):
    lib, h = ctx._lib, ctx._h
    INV, UNS = _native.KWS_EINVAL, _native.KWS_EUNSUPPORTED
    R, W, Cn, K = 3, 65, 12, 3
    zd = torch.from_numpy(sref.detect_logits(W, Cn, sref.DETECT_SEEDS[(W, Cn)])).to(DEV)
    th = np.array([0.2, 0.5, 0.8], np.float32)
    truth = ref.random_truth(np.random.default_rng(4), R, Cn, W, 2)
    before = score(ctx, zd, 7, 2, 5, th, truth)
    rag_off, rag_win = np.array([0, 65, 130], np.int32), np.array([65, 65, 65], np.int32)
    before_ragged = score_ragged(ctx, zd.reshape(R * W, Cn), rag_off, rag_win, 7, 2, 5, th, truth)
    np.testing.assert_array_equal(before_ragged, before)
    counts = counters(K, Cn)
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    ip = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    row = lambda *v: np.array([v], np.int32)
    two = lambda a, b: np.array([a, b], np.int32)

    def call(logits=zd.data_ptr(), R=R, W=W, Cn=Cn, S=7, fk=2, refractory=5, th=fp(th), K=K, truth=truth, N=None, counts=counts.data_ptr()):
        n = len(truth) if N is None else N
        return lib.kws_scan_score_f32(h, logits, R, W, Cn, S, fk, refractory, th, K, ip(truth), n, counts)

    def call_ragged(logits=zd.data_ptr(), off=rag_off, win=rag_win, R=R, Cn=Cn, S=7, fk=2, refractory=5, th=fp(th), K=K, truth=truth,
                    N=None, counts=counts.data_ptr()):
        n = len(truth) if N is None else N
        return lib.kws_scan_score_ragged_f32(h, logits, ip(off), ip(win), R, Cn, S, fk, refractory, th, K, ip(truth), n, counts)

    shared = [(dict(logits=None), INV), (dict(th=None), INV), (dict(counts=None), INV), (dict(K=0), INV), (dict(K=1025), INV),
              (dict(N=-1), INV), (dict(R=0), INV), (dict(Cn=0), INV), (dict(Cn=65), INV), (dict(S=0), INV), (dict(S=257), INV),
              (dict(refractory=0), INV), (dict(fk=-1), INV), (dict(truth=None, N=1), INV),
              (dict(N=(1 << 24) + 1), UNS), (dict(R=(1 << 20) + 1), UNS),
              (dict(truth=row(3, 2, 0, 1)), INV), (dict(truth=row(-1, 2, 0, 1)), INV), (dict(truth=row(0, 1, 0, 1)), INV),
              (dict(truth=row(0, 12, 0, 1)), INV), (dict(truth=row(0, 2, 5, 4)), INV), (dict(truth=row(0, 2, -1, 4)), INV),
              (dict(truth=two((0, 2, 0, 10), (0, 2, 5, 20))), INV), (dict(truth=two((0, 2, 11, 20), (0, 2, 0, 11))), INV)]
    cases = [(call, kw, code) for kw, code in shared + [(dict(W=0), INV), (dict(R=1 << 20, W=1 << 11), UNS)]]
    cases += [(call_ragged, kw, code) for kw, code in shared if "R" not in kw or kw["R"] == 0]
    cases += [(call_ragged, kw, code) for kw, code in [
        (dict(off=None), INV), (dict(win=None), INV), (dict(win=np.array([65, -1, 65], np.int32)), INV),
        (dict(off=np.array([0, 64, 130], np.int32)), INV), (dict(off=np.array([0, 65, 1 << 30], np.int32)), UNS),
        (dict(R=(1 << 20) + 1), UNS)]]
    for fn, kw, code in cases:
        assert fn(**kw) == code, (fn.__name__, kw)
        assert ctx._lib.kws_last_error(h), "a refusal names its reason"
        torch.cuda.synchronize()
        assert (counts == SENTINEL).all(), f"{fn.__name__} {kw}: a refused call wrote counters"
        # the next valid call on the same context gives what it gave before
        after = score(ctx, zd, 7, 2, 5, th, truth) if fn is call else \
            score_ragged(ctx, zd.reshape(R * W, Cn), rag_off, rag_win, 7, 2, 5, th, truth)
        np.testing.assert_array_equal(after, before, err_msg=f"after {fn.__name__} {kw}")
    assert call() == _native.KWS_OK and call_ragged() == _native.KWS_OK
    np.testing.assert_array_equal(read(counts), before)


# ---- 5. the Python surface -------------------------------------------------------------------------------------------
RULES = dict(hop_frames=5, smooth_window=3, refractory=4, first_keyword=2)
THRESHOLDS = [0.1, 0.15, 0.3, 0.6, 2.0]


def spotter_truths(sp, recordings):
    """Annotations in seconds from what a scan at a low threshold fires, so that hits, misses and false alarms all occur: the first
    two events of each recording, spoken just before the window that fired ends; one word form, one index form; an annotation
    before any window ends (undetectable) and one more."""
    truths = []
    for rec in recordings:
        ev = sp.scan(rec, threshold=0.1, max_events=64, **RULES).events[0]
        assert len(ev) >= 2
        truths.append([(ev[0][2], ev[0][0] - 1.2, ev[0][0] - 0.9), (ev[1][1], ev[1][0] - 0.5, ev[1][0] - 0.2), ("yes", 0.0, 0.0),
                       ("no", 1.9, 2.0)])
    return truths


def counts_by_scan(sp, scan, recordings, truths, tolerance_s=1.0):
    """The expectation: per threshold scan(...).events, each event's window found by its end time, matched by brute force against
    truth_windows of the recording."""
    from kws.inference import scan_window_times
    from kws.libs.evaluation import truth_windows

    Cn = len(sp.words)
    out = np.zeros((len(THRESHOLDS), Cn, 4), np.int64)
    for rec, truth in zip(recordings, truths):
        n = len(rec)
        _, W = sref.scan_shape(n, RULES["hop_frames"])
        if W < 1:
            continue
        _, end_s = scan_window_times(W, RULES["hop_frames"], n_total=n)
        table, _, _ = truth_windows(truth, end_s, tolerance_s, sp.words)
        for i, t in enumerate(THRESHOLDS):
            ev = scan(rec, threshold=t, max_events=W, **RULES).events[0]
            windows = [int(np.flatnonzero(end_s == e[0])[0]) for e in ev]
            out[i] += ref.match_brute([[(w, e[1]) for w, e in zip(windows, ev)]], table, Cn)
    return out


def test_keyword_spotter_score(e2e_golden):
    from kws.inference import KeywordSpotter
    from kws.libs.evaluation import DetectionReport
    from kws.libs.models import DepthwiseSeparableConv

    model = DepthwiseSeparableConv(num_classes=12)
    model.load_state_dict(sref.state_from_blob(e2e_golden["he.blob"]))
    sp = KeywordSpotter(model)
    pcm = sref.oracle_recordings(e2e_golden["clips"])  # [2, 48053]
    truths = spotter_truths(sp, pcm)
    rep = sp.score(pcm, truths, THRESHOLDS, **RULES)
    assert isinstance(rep, DetectionReport) and rep.counts.shape == (5, 12, 4) and rep.counts.dtype == np.int64
    want = counts_by_scan(sp, sp.scan, pcm, truths)
    np.testing.assert_array_equal(rep.counts, want)
    assert want[0, :, 0].sum() > 0 and want[:, :, 1].sum() > 0 and (want[4] == 0).all(), "hits, false alarms and a silent threshold"
    # the two annotations before any window ends are undetectable (clipping may add to them); nothing fires at 2.0
    assert rep.n_truth.sum() == 8 and rep.undetectable[2] == 2 and rep.misses[4].sum() == 8
    assert rep.hours == pytest.approx(2 * 48053 / 16000 / 3600) and rep.hop_s == pytest.approx(0.05)
    assert np.array_equal(rep.thresholds, np.asarray(THRESHOLDS, np.float32)) and rep.words == sp.words
    # one recording [n] with its list given directly
    one = sp.score(pcm[0], truths[0], THRESHOLDS, **RULES)
    np.testing.assert_array_equal(one.counts, counts_by_scan(sp, sp.scan, pcm[:1], truths[:1]))
    # the float32 twin on pcm / 32768
    f32 = sp.score_f32(pcm.astype(np.float32) / np.float32(32768.0), truths, THRESHOLDS, **RULES)
    np.testing.assert_array_equal(f32.counts, rep.counts)
    # unequal lengths in one pass: the sum of the recordings alone; one too short for a window only adds undetectable truth
    recs = [pcm[0], pcm[1][:30000], np.zeros(8000, np.int16)]
    lists = [truths[0], truths[1], [("yes", 0.1, 0.2)]]
    batch = sp.score_batch(recs, lists, THRESHOLDS, **RULES)
    alone = [sp.score(recs[r], lists[r], THRESHOLDS, **RULES) for r in range(2)]
    np.testing.assert_array_equal(batch.counts, alone[0].counts + alone[1].counts)
    np.testing.assert_array_equal(batch.counts, counts_by_scan(sp, sp.scan, recs, lists))
    assert batch.n_truth.sum() == 9 and batch.undetectable.sum() == (alone[0] + alone[1]).undetectable.sum() + 1
    assert batch.hours == pytest.approx((48053 + 30000 + 8000) / 16000 / 3600)
    batch_f32 = sp.score_batch_f32([r.astype(np.float32) / np.float32(32768.0) for r in recs], lists, THRESHOLDS, **RULES)
    np.testing.assert_array_equal(batch_f32.counts, batch.counts)


def test_keyword_spotter_score_cnn_trad():
    from kws.inference import KeywordSpotter
    from kws.libs.models import CnnTradFpool3
    from oracle import cnn_trad as o_ct

    model = CnnTradFpool3(12)
    model.load_state_dict(o_ct.random_state(1, num_classes=12))
    sp = KeywordSpotter(model)
    rng = np.random.default_rng(31)
    pcm = rng.integers(-3000, 3000, size=(2, 40000), dtype=np.int16)
    # random weights favour few classes: annotate by index what a scan without a threshold labels most windows with
    labels = sp.scan(pcm, hop_frames=RULES["hop_frames"]).labels
    top = int(np.bincount(labels.reshape(-1), minlength=12)[2:].argmax()) + 2
    truths = [[(top, 0.5, 0.8), (2 if top != 2 else 3, 1.0, 1.2)], [(top, 1.0, 1.3)]]
    rep = sp.score(pcm, truths, THRESHOLDS, **RULES)
    np.testing.assert_array_equal(rep.counts, counts_by_scan(sp, sp.scan, pcm, truths))
    batch = sp.score_batch([pcm[0], pcm[1][:25000]], truths, THRESHOLDS, **RULES)
    np.testing.assert_array_equal(batch.counts, counts_by_scan(sp, sp.scan, [pcm[0], pcm[1][:25000]], truths))
