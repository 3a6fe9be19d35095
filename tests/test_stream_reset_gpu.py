"""GPU tests of kws_stream_reset through the C ABI.  The oracle is a second set: set A is reset after h0 pushes, set B is opened and
armed identically, fed zeros on the streams to be reset for pushes 1 .. h0 and A's samples otherwise; from push h0 + 1 on the two
must agree bit for bit -- logits, labels, feature rings, hop counts, records of the armed layers.  Where a reset stream is
allowed to differ from a silent past (a span start held at the reset, the posterior window and refractory wait starting over)
the expectation is a flush on a copy of the run, or a fresh detection set over the logits A's own pushes returned."""
import ctypes as C

import numpy as np
import pytest
import torch

import _live_detect_ref as ld
import _live_ref as lr
import _reset_ref as rr
import _scan_ref as ref
import _stream_ref as sr
from kws import _native

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
STEP, T, NF, K = sr.HOP, sr.T, sr.F, rr.K
N_CLASSES = 12
OK, EINVAL, ESTATE, EUNSUPPORTED = _native.KWS_OK, _native.KWS_EINVAL, _native.KWS_ESTATE, _native.KWS_EUNSUPPORTED


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _context(e2e_golden, cnn_trad=False, own_stream=False):
    """own_stream: the context keeps its own stream (a push is captured into a graph there, which the default stream refuses);
    _run reads nothing before kws_stream_state has drained it."""
    c = _native.Context(0)
    if not own_stream:
        c.use_torch_stream()
    if cnn_trad:
        from oracle import cnn_trad as o_ct

        c.load_cnn_trad(o_ct.flatten_state(o_ct.random_state(1, num_classes=N_CLASSES)), N_CLASSES)
    else:
        c.load_dscnn(e2e_golden["he.blob"], N_CLASSES)
    return c


def _hops_of(pcm, step=STEP):
    """int16 [S, n * step] -> [n, S, step] on the device, one contiguous block per push."""
    S = pcm.shape[0]
    d = torch.from_numpy(np.array(pcm.reshape(S, -1, step).transpose(1, 0, 2), order="C")).to(DEV)
    torch.cuda.synchronize()
    return d


def _silenced(pcm, streams, h0, step=STEP):
    out = np.array(pcm)
    out[list(streams), :h0 * step] = 0
    return out


def _ring(c, S):
    ring = torch.empty((S, T, NF), dtype=torch.float32, device=DEV)
    c.stream_copy_features(ring)
    _, hops = c.stream_state()
    return ring.cpu().numpy(), hops


def _run(c, hops_dev, resets=None, route="device", setup=None, behind=None):
    """A fresh set of S streams on c, every hop pushed back to back; resets: {pushes so far: streams}.  Returns (logits
    [n, S, C], labels [n, S], final ring, hop count); features-only: the ring after every push instead of the logits."""
    n, S = hops_dev.shape[0], hops_dev.shape[1]
    c.stream_open(S)
    if setup:
        setup(c)
    if route == "zero-copy":
        c.stream_host_results(True)
    lg = torch.zeros((n, S, N_CLASSES), dtype=torch.float32, device=DEV)
    lb = torch.full((n, S), -1, dtype=torch.int32, device=DEV)
    rings = torch.zeros((n, S, T, NF), dtype=torch.float32, device=DEV) if route == "features" else None
    host_lg, host_lb = np.zeros((n, S, N_CLASSES), np.float32), np.zeros((n, S), np.int32)
    torch.cuda.synchronize()
    for t in range(n + 1):
        if resets and t in resets:
            c.stream_reset(resets[t])
        if t == n:
            break
        if route == "cnn-trad":
            c.stream_push_cnn_trad_i16(hops_dev[t], lg[t], lb[t])
        elif route == "rate":
            c.stream_push_rate_i16(hops_dev[t], lg[t], lb[t])
        elif route == "features":
            c.stream_push_i16(hops_dev[t], None, None)
            c.stream_copy_features(rings[t])
        else:
            c.stream_push_i16(hops_dev[t], lg[t], lb[t], use_graph=route == "graph")
            if route == "zero-copy":
                h_lg, h_lb = c.stream_wait_host(S)
                host_lg[t], host_lb[t] = h_lg, h_lb
        if behind:
            behind(c, t)
    ring, hops = _ring(c, S)
    if route == "features":
        return rings.cpu().numpy(), None, ring, hops
    if route == "zero-copy":
        assert np.array_equal(_bits(host_lg), _bits(lg.cpu().numpy())) and np.array_equal(host_lb, lb.cpu().numpy())
    return lg.cpu().numpy(), lb.cpu().numpy(), ring, hops


def _check_pair(a, b, h0, what):
    """From push h0 + 1 on set A is set B, and at the end so are ring and hop count of ALL streams."""
    assert np.array_equal(_bits(a[0][h0:]), _bits(b[0][h0:])), what
    if a[1] is not None:
        assert np.array_equal(a[1][h0:], b[1][h0:]), what
    assert np.array_equal(_bits(a[2]), _bits(b[2])), what
    assert a[3] == b[3] == len(a[0]), what


def _pair(e2e_golden, S, streams, h0, route="device", setup=None, cnn_trad=False, pcm=None, step=STEP):
    pcm = sr.stream_pcm(S, h0 + rr.POST) if pcm is None else pcm
    ca, cb = (_context(e2e_golden, cnn_trad, own_stream=route == "graph") for _ in range(2))
    try:
        a = _run(ca, _hops_of(pcm, step), {h0: list(streams)}, route, setup)
        b = _run(cb, _hops_of(_silenced(pcm, streams, h0, step), step), None, route, setup)
    finally:
        ca.close()
        cb.close()
    _check_pair(a, b, h0, (S, streams, h0, route))
    return a, b


# ---- 1. rings and network -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h0", rr.H0S)
@pytest.mark.parametrize("streams", rr.RESET_SETS, ids=lambda s: "-".join(map(str, s)))
def test_reset_equals_a_silent_past(e2e_golden, streams, h0):
    a, b = _pair(e2e_golden, 5, streams, h0)
    assert np.abs(a[0][h0:]).max() > 0
    if h0 >= T + K - 1:  # the reset changed something: before it the two sets differ on the reset streams, and only there
        differs = [bool((_bits(a[0][h0 - 1, s]) != _bits(b[0][h0 - 1, s])).any()) for s in range(5)]
        assert differs == [s in streams and s != sr.ZERO for s in range(5)]


def test_the_ring_right_after_a_reset_is_a_silent_streams(e2e_golden):
    """Before any later push: the reset streams' rows are those of set B, which heard zeros throughout -- the silence row in the
    rows of the frames that exist, zeros elsewhere -- and the neighbours' rows are untouched."""
    S, streams = 5, (0, 4)
    for h0 in rr.H0S:
        pcm = sr.stream_pcm(S, max(h0, 1))[:, :h0 * STEP]
        ca, cb = _context(e2e_golden), _context(e2e_golden)
        try:
            ca.stream_open(S)
            cb.stream_open(S)
            lg = torch.zeros((S, N_CLASSES), dtype=torch.float32, device=DEV)
            for t, (x, y) in enumerate(zip(_hops_of(pcm), _hops_of(_silenced(pcm, streams, h0)))):
                ca.stream_push_i16(x, lg if t % 2 else None, None)
                cb.stream_push_i16(y, lg if t % 2 else None, None)
            ca.stream_reset(streams)
            (ra, ha), (rb, hb) = _ring(ca, S), _ring(cb, S)
        finally:
            ca.close()
            cb.close()
        assert ha == hb == h0 and np.array_equal(_bits(ra), _bits(rb)), h0
        rows = rr.silent_rows(h0)
        assert not ra[0, rows:].any() and (rows == 0 or (ra[0, :rows] == ra[0, 0]).all()), h0
        if rows:
            assert ra[0, 0, 0] < lr.THR  # log energy of an all-zero frame


@pytest.mark.parametrize("route,setup", [
    ("zero-copy", None),
    ("device", lambda c: c.stream_cluster(1)),
    ("device", lambda c: c.stream_cluster(2)),
    ("device", lambda c: c.stream_cluster(4)),
    ("features", None),
    ("graph", lambda c: c.set_pointwise_math(_native.PW_F32)),
    ("cnn-trad", None),
], ids=["zero-copy", "cluster1", "cluster2", "cluster4", "features-only", "graph-replay", "cnn-trad"])
@pytest.mark.parametrize("h0", [1, T + K - 1])
def test_reset_on_every_push_route(e2e_golden, route, setup, h0):
    _pair(e2e_golden, 5, (1, 2) if h0 == 1 else (0, 4), h0, route, setup, cnn_trad=route == "cnn-trad")


def test_reset_across_three_wavefronts_of_streams(e2e_golden):
    _pair(e2e_golden, 130, (0, 63, 64, 129), 120)


def test_reset_beyond_one_chunk_of_1024_streams(e2e_golden):
    """The selection travels as one 1024-bit mask per chunk of 1024 streams: a plain set of 1030 with one stream reset in the
    first chunk, two in the second (its first and its last stream) and one at the first chunk's end."""
    S, h0, post = 1030, 105, K + 9
    pcm = np.random.default_rng(1030).integers(-9000, 9001, size=(S, (h0 + post) * STEP)).astype(np.int16)
    a, b = _pair(e2e_golden, S, (7, 1023, 1024, 1029), h0, pcm=pcm)
    differs = np.flatnonzero((_bits(a[0][h0 - 1]) != _bits(b[0][h0 - 1])).any(axis=1))
    assert differs.tolist() == [7, 1023, 1024, 1029]


def test_two_identical_runs_give_identical_bits(e2e_golden):
    runs = [_pair(e2e_golden, 5, (1, 2), 50)[0] for _ in range(2)]
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][2].tobytes() == runs[1][2].tobytes()


# ---- 2. rate push ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [48000, 44100])
def test_reset_behind_the_streaming_resampler(e2e_golden, rate):
    S, h0, hop_in = 3, 120, rate // 100
    x = np.random.default_rng(rate).integers(-12000, 12001, size=(S, (h0 + rr.POST) * hop_in)).astype(np.int16)
    setup = lambda c: c.stream_resample_open(S, rate, 16000, hop_in)
    a, _ = _pair(e2e_golden, S, (1,), h0, "rate", setup, pcm=x, step=hop_in)
    assert np.abs(a[0][h0:]).max() > 0


# ---- 3. live utterances ---------------------------------------------------------------------------------------------------------------
def _arm_utt(c):
    H = _native.host_stream_utt_history(lr.FRAME_LEN, STEP, rr.UTT_PRE_ROLL, rr.UTT_MAX_FRAMES, rr.UTT_HOPS)
    c.stream_utt_open(lr.THR, rr.UTT_ON, rr.UTT_OFF, rr.UTT_PRE_ROLL, rr.UTT_MAX_FRAMES, H, 256)


def _utt_records(c):
    total, steps = c.stream_utt_poll()
    return (lr.rows(c.stream_utt_read(0, total)) if total else []), total, steps


def _cut(c, seq, n_out, normalize_to):
    clip = torch.full((1, n_out), 77, dtype=torch.int16, device=DEV)
    peak = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    c.stream_utt_cut_i16(seq, clip, normalize_to, peak)
    c.sync()
    return clip.cpu().numpy()[0], int(peak.cpu().numpy()[0])


@pytest.mark.parametrize("at_once", [False, True], ids=["speech-later", "speech-at-once"])
def test_reset_of_a_stream_inside_an_utterance(e2e_golden, at_once):
    s, h0, hops = rr.UTT_STREAM, rr.UTT_H0, rr.UTT_HOPS
    pcm = lr.pcm_of(rr.utt_pattern(at_once), 7)
    ca, cb, cc, cd = (_context(e2e_golden) for _ in range(4))
    try:
        a = _run(ca, _hops_of(pcm), {h0: [s]}, setup=_arm_utt)
        # the threshold lies above an all-zero frame's log energy: what set B's stream s holds at the reset is unvoiced
        quiet = _run(cb, _hops_of(_silenced(pcm, [s], h0)[:, :h0 * STEP]), None, setup=_arm_utt)[2][s]
        assert (quiet[:h0 - K + 1, 0] < lr.THR - 3.0).all() and not quiet[h0 - K + 1:].any()
        b = _run(cb, _hops_of(_silenced(pcm, [s], h0)), None, setup=_arm_utt)
        _check_pair(a, b, h0, "armed")
        rec_a, total_a, steps_a = _utt_records(ca)
        rec_b, _, steps_b = _utt_records(cb)
        assert steps_a == steps_b == hops - (K - 1)
        # (a) the open utterance closes at the newest walked frame with reason 2, as a flush on a copy of the run closes it
        _run(cc, _hops_of(pcm[:, :h0 * STEP]), None, setup=_arm_utt)
        cc.stream_utt_flush()
        flushed = [r for r in _utt_records(cc)[0] if r[0] == s and r[5] == 2]
        at_reset = [r for r in rec_a if r[0] == s and r[5] == 2]
        assert len(flushed) == 1 and at_reset == flushed and at_reset[0][4] == h0 - K
        mine = [r for r in rec_a if r[0] == s]
        before, after = mine[:mine.index(at_reset[0])], mine[mine.index(at_reset[0]) + 1:]
        assert len(before) == 1 and before[0][5] == 0 and len(after) == 1 and after[0][5] == 0
        # (b) later records: a silent past's, or -- speech straight on -- a span that starts at the reset's first sample
        theirs = [r for r in rec_b if r[0] == s]
        assert len(theirs) == 1 and after[0][2:] == theirs[0][2:]
        if at_once:
            assert after[0][1] == h0 * STEP and theirs[0][1] < h0 * STEP
            clip, peak = _cut(ca, rec_a.index(after[0]), after[0][2] - after[0][1], 0)
            assert peak > 0 and np.array_equal(clip, pcm[s, h0 * STEP:after[0][2]])
        else:
            assert after[0][3] - rr.UTT_PRE_ROLL > h0 and after == theirs
        # (c) the utterance that closed before the reset, cut after it: the bits of a run without the reset
        _run(cd, _hops_of(pcm), None, setup=_arm_utt)
        rec_d = _utt_records(cd)[0]
        assert before[0] in rec_d
        got, want = _cut(ca, rec_a.index(before[0]), 3001, 16384), _cut(cd, rec_d.index(before[0]), 3001, 16384)
        assert got[1] == want[1] > 0 and np.array_equal(got[0], want[0])
        # (d) every other stream: the same records in A, in B and in a run without the reset
        for k in (0, 2):
            assert [r for r in rec_a if r[0] == k] == [r for r in rec_b if r[0] == k] == [r for r in rec_d if r[0] == k] != []
        assert total_a == len(rec_a)
    finally:
        for c in (ca, cb, cc, cd):
            c.close()


# ---- 4. live events -------------------------------------------------------------------------------------------------------------------
REFRACTORY = 20


def _arm_detect(W, first_hop=0):
    return lambda c: c.stream_detect_open(N_CLASSES, W, 0, 0.0, REFRACTORY, first_hop, 4096)


def _watch(sm, lb):
    return lambda c, t: c.stream_detect_smoothed(sm[t], lb[t])


def _detect_records(c):
    total, decisions = c.stream_detect_poll()
    return (c.stream_detect_read(0, total) if total else np.zeros((0, 5), np.int64)), decisions


def _fresh_steps(c, z, W):
    """z [n, C] (host): a fresh one-stream detection set stepped explicitly: (smoothed [n, C], labels [n], events)."""
    n = len(z)
    c.stream_open(1)
    _arm_detect(W)(c)
    zd = torch.from_numpy(np.ascontiguousarray(z)).to(DEV)
    sm = torch.zeros((n, 1, N_CLASSES), dtype=torch.float32, device=DEV)
    lb = torch.zeros((n, 1), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    for d in range(n):
        c.stream_detect_step_f32(zd[d:d + 1])
        c.stream_detect_smoothed(sm[d], lb[d])
    rec, decisions = _detect_records(c)
    assert decisions == n
    return sm.cpu().numpy()[:, 0], lb.cpu().numpy()[:, 0], ld.group_records(rec, 1)[0]


@pytest.mark.parametrize("W", rr.DETECT_WINDOWS)
@pytest.mark.parametrize("h0,h1", [(41, None), (40, 47), (150, None)], ids=["just-fired", "with-its-neighbours-then-again", "wrapped-ring"])
def test_reset_of_a_detecting_stream(e2e_golden, W, h0, h1):
    """Threshold 0 and first_keyword 0: every stream fires whenever its refractory wait of 20 is over, i.e. at decisions 0, 20,
    40 ... (decision d is push d + 1).  h0 = 41: stream 1 fired at decision 40 and fires again at 41, its first after the reset.
    h0 = 40: it fires at decision 40 together with its neighbours; reset once more after 47 pushes it fires at 47."""
    S, s = 3, 1
    last = h1 if h1 is not None else h0
    n = last + W + 25
    pcm = sr.stream_pcm(S + 2, n)[[0, 3, 4]]
    resets = {h0: [s]} if h1 is None else {h0: [s], h1: [s, s]}
    ca, cb, cd, cf = (_context(e2e_golden) for _ in range(4))
    try:
        sm = torch.zeros((n, S, N_CLASSES), dtype=torch.float32, device=DEV)
        lb = torch.zeros((n, S), dtype=torch.int32, device=DEV)
        a = _run(ca, _hops_of(pcm), resets, setup=_arm_detect(W), behind=_watch(sm, lb))
        rec_a, decisions = _detect_records(ca)
        assert decisions == n
        sm, lb = sm.cpu().numpy(), lb.cpu().numpy()
        b = _run(cb, _hops_of(_silenced(pcm, [s], last)), None, setup=_arm_detect(W))
        _check_pair(a, b, last, "armed")
        rec_b = _detect_records(cb)[0]
        _run(cd, _hops_of(pcm), None, setup=_arm_detect(W))
        rec_d = _detect_records(cd)[0]
        ga, gb, gd = (ld.group_records(r, S) for r in (rec_a, rec_b, rec_d))
        # the neighbours: set B's records, bit for bit; queued events of the reset stream from before the reset are still there
        for k in (0, 2):
            assert ga[k] == gb[k] == gd[k] and len(ga[k]) == -(-n // REFRACTORY)
        assert [e for e in ga[s] if e[0] < h0] == [e for e in gd[s] if e[0] < h0] != []
        assert (rec_a[:, 2] - rec_a[:, 1] == 1).all()  # first_hop 0: decision d is push d + 1
        for lo, hi in ([(h0, n)] if h1 is None else [(h0, h1), (h1, n)]):
            # the reset stream from its epoch on: a fresh set, and the float64 restatement, over the logits A's pushes returned
            z = a[0][lo:hi, s]
            f_sm, f_lb, f_ev = _fresh_steps(cf, z, W)
            look = min(W + 2, hi - lo)
            assert np.array_equal(_bits(sm[lo:lo + look, s]), _bits(f_sm[:look]))
            assert np.array_equal(_bits(sm[lo:hi, s]), _bits(f_sm)) and np.array_equal(lb[lo:hi, s], f_lb)
            mine = [(d - lo, k, bits) for d, k, bits in ga[s] if lo <= d < hi]
            assert mine == f_ev and mine[0][0] == 0  # fires at its first decision, whatever its wait was
            want_ev, want_sm, _ = ld.run(z[None], W, 0, 0.0, REFRACTORY)
            tol = ref.tol_smooth(W)
            assert np.abs(sm[lo:hi, s] - want_sm[0]).max() <= tol
            top = np.sort(want_sm[0], axis=1)
            sure = top[:, -1] - top[:, -2] > 2 * tol
            assert sure.any() and np.array_equal(lb[lo:hi, s][sure], want_sm[0].argmax(axis=1)[sure])
            assert [e[0] for e in mine] == [e[0] for e in want_ev[0]]
            for (_, k, bits), (d, wk, score) in zip(mine, want_ev[0]):
                assert (k == wk or not sure[d]) and abs(float(np.uint32(bits).view(np.float32)) - score) <= tol
        if h0 == 40:  # the reset stream and its neighbours fire in one hop: ascending stream, consecutive sequence numbers
            at = [int(r[0]) for r in rec_a if r[1] == 40]
            assert at == [0, 1, 2]
    finally:
        for c in (ca, cb, cd, cf):
            c.close()


def test_reset_below_first_hop_and_behind_it(e2e_golden):
    """first_hop stays a gate of the set: a reset before the first decision has epoch 0 and changes no decision's term count; a
    reset behind it starts the reset stream's window over while its rows hold silence, not zeros."""
    S, s, W = 3, 1, 4
    first_hop = ld.first_hop(T, lr.FRAME_LEN, STEP)
    for h0 in (50, first_hop + 20):
        n = max(h0, first_hop) + 12
        pcm = sr.stream_pcm(S + 2, n)[[0, 3, 4]]
        ca, cb, cf = (_context(e2e_golden) for _ in range(3))
        try:
            sm = torch.zeros((n, S, N_CLASSES), dtype=torch.float32, device=DEV)
            lb = torch.zeros((n, S), dtype=torch.int32, device=DEV)
            a = _run(ca, _hops_of(pcm), {h0: [s]}, setup=_arm_detect(W, first_hop), behind=_watch(sm, lb))
            b = _run(cb, _hops_of(_silenced(pcm, [s], h0)), None, setup=_arm_detect(W, first_hop))
            _check_pair(a, b, h0, h0)
            rec_a, decisions = _detect_records(ca)
            assert decisions == n - first_hop + 1 and (rec_a[:, 2] - rec_a[:, 1] == first_hop).all()
            lo = max(h0, first_hop - 1)
            f_sm, _, f_ev = _fresh_steps(cf, a[0][lo:, s], W)
            assert np.array_equal(_bits(sm.cpu().numpy()[lo:, s]), _bits(f_sm))
            epoch = lo - (first_hop - 1)
            assert [(d - epoch, k, bits) for d, k, bits in ld.group_records(rec_a, S)[s] if d >= epoch] == f_ev
        finally:
            for c in (ca, cb, cf):
                c.close()


def test_reset_clears_the_vad_history(e2e_golden):
    """kws_stream_vad_f32 behind every push: from the reset on stream 1's state is that of a silent past."""
    S, s, h0 = 3, 1, 60
    pattern = np.stack([lr.cycles(3, 5, 100)] * 3)
    pattern[s, 50:70] = True  # inside an utterance at the reset
    pcm = lr.pcm_of(pattern, 3)
    out = []
    for x, resets in ((pcm, {h0: [s]}), (_silenced(pcm, [s], h0), None)):
        c = _context(e2e_golden)
        try:
            st = torch.full((100, S), -1, dtype=torch.int32, device=DEV)
            _run(c, _hops_of(x), resets, behind=lambda c, t: c.stream_vad_f32(lr.THR, 3, 5, st[t]))
            out.append(st.cpu().numpy())
        finally:
            c.close()
    assert out[0][h0 - 1, s] & 1 and not out[1][h0 - 1, s] & 1
    assert np.array_equal(out[0][h0:], out[1][h0:]) and np.array_equal(out[0][:, [0, 2]], out[1][:, [0, 2]])
    assert (out[0][h0:, s] & 1).any()


# ---- 5. neighbours and determinism ----------------------------------------------------------------------------------------------------
def test_resetting_twice_is_resetting_once_and_n_zero_is_nothing(e2e_golden):
    S, h0 = 5, 60
    pcm = sr.stream_pcm(S, h0 + 20)
    arm = lambda c: (_arm_utt(c), _arm_detect(4)(c))
    out = []
    for resets in ([[1, 2]], [[1, 2], [2, 1]], [[2, 2, 1, 1, 2]]):
        c = _context(e2e_golden)
        try:
            c.stream_open(S)
            arm(c)
            hops = _hops_of(pcm)
            lg = torch.zeros((len(hops), S, N_CLASSES), dtype=torch.float32, device=DEV)
            for t in range(h0):
                c.stream_push_i16(hops[t], lg[t], None)
            before = _ring(c, S)[0]
            c.stream_reset([])
            assert c._lib.kws_stream_reset(c._h, None, 0) == OK
            assert np.array_equal(_bits(_ring(c, S)[0]), _bits(before))
            for r in resets:
                c.stream_reset(r)
            for t in range(h0, len(hops)):
                c.stream_push_i16(hops[t], lg[t], None)
            out.append((lg.cpu().numpy().tobytes(), _ring(c, S)[0].tobytes(), _utt_records(c)[0], _detect_records(c)[0].tobytes()))
        finally:
            c.close()
    assert out[0] == out[1] == out[2]


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(e2e_golden):
    c = _context(e2e_golden)
    try:
        lib, h = c._lib, c._h
        err = lambda: lib.kws_last_error(h).decode()
        idx = lambda *v: (C.c_int32 * len(v))(*v)
        assert lib.kws_stream_reset(h, idx(0), 1) == ESTATE and "kws_stream_reset" in err() and "kws_stream_open" in err()
        S = 3
        c.stream_open(S)
        _arm_utt(c)
        _arm_detect(4)(c)
        hops = _hops_of(lr.pcm_of(np.ones((S, 30), bool), 5))
        lg = torch.zeros((S, N_CLASSES), dtype=torch.float32, device=DEV)
        sm = torch.zeros((S, N_CLASSES), dtype=torch.float32, device=DEV)
        for x in hops:
            c.stream_push_i16(x, lg, None)
        state = lambda: (_ring(c, S)[0].tobytes(), c.stream_utt_poll(), c.stream_detect_poll())
        before = state()
        assert before[1][1] == 28 and before[2][0] >= S
        for args in ((idx(-1), 1), (idx(S), 1), (idx(0, 1, S), 3), (idx(1, -7), 2), (None, 1), (idx(0), -1)):
            assert lib.kws_stream_reset(h, *args) == EINVAL and "kws_stream_reset" in err(), args
            assert state() == before
        assert lib.kws_stream_reset(None, idx(0), 1) == EINVAL
        # the running-sum smoother keeps one hop count for all streams: refused while its history is live, before anything changes
        c.stream_smooth_f32(lg, 8, sm)
        assert lib.kws_stream_reset(h, idx(1), 1) == EUNSUPPORTED
        assert "kws_stream_reset" in err() and "running sum" in err() and "kws_stream_detect_" in err()
        assert state() == before
        # a new set has no such history: the same call goes through
        c.stream_open(S)
        assert lib.kws_stream_reset(h, idx(1), 1) == OK
        c.sync()
    finally:
        c.close()


# ---- 7. Python ------------------------------------------------------------------------------------------------------------------------
def test_streaming_spotter_reset(e2e_golden):
    from kws.common.errors import ModelError
    from kws.inference import DetectConfig, StreamingSpotter, UtteranceConfig
    from kws.libs.models import DepthwiseSeparableConv

    model = DepthwiseSeparableConv(num_classes=N_CLASSES)
    model.load_state_dict(ref.state_from_blob(e2e_golden["he.blob"]))
    S, h0, hops = 4, 45, 70  # decision 40 (push 41) fires everywhere; stream 2 fires again at its first decision after the reset
    pattern = np.stack([lr.cycles(3, 5, hops)] * S)
    pattern[2, 30:55] = True  # stream 2 is inside an utterance at the reset
    pcm = lr.pcm_of(pattern, 21)
    kw = dict(utterances=UtteranceConfig(threshold=lr.THR, on_window=3, off_window=5, pre_roll=4, slack_hops=hops),
              detect=DetectConfig(threshold=0.0, smooth_window=4, refractory=REFRACTORY, first_keyword=0, skip_partial_windows=False))
    live, plain = StreamingSpotter(S, model, **kw), StreamingSpotter(S, model, **kw)
    try:
        assert live.stream_origin.dtype == np.int64 and not live.stream_origin.any()
        assert live.reset([]) == 0
        closed = []
        for t in range(hops):
            if t == h0:
                assert {u.reason for u in live.pop_utterances()} == {"endpoint"}  # what closed so far, stream 2's first among it
                assert live.reset([2]) == h0 and live.stream_origin.tolist() == [0, 0, h0, 0]
                closed = [u for u in live.pop_utterances() if u.recording == 2]
                assert [u.reason for u in closed] == ["end_of_recording"]
            if t == h0 + 5:
                assert live.reset(3) == h0 + 5 and live.reset(np.array([3, 3])) == h0 + 5
                assert live.stream_origin.tolist() == [0, 0, h0, h0 + 5]
            hop = pcm[:, t * STEP:(t + 1) * STEP]
            lb, lg = live.push(hop)
            want_lb, want_lg = plain.push(hop)
            keep = [0, 1] if t >= h0 + 5 else [0, 1, 3]
            assert np.array_equal(lb[keep], want_lb[keep]) and np.array_equal(_bits(lg[keep]), _bits(want_lg[keep])), t
        ev, want_ev = live.pop_events(), plain.pop_events()
        assert [e for e in ev if e.stream < 2] == [e for e in want_ev if e.stream < 2] != []
        mine = [e.hop for e in ev if e.stream == 2]
        assert h0 + 1 in mine and h0 + 1 not in [e.hop for e in want_ev if e.stream == 2]
        assert min(e.hop - live.stream_origin[2] for e in ev if e.stream == 2 and e.hop > h0) == 1
        for bad in ([-1], [S], 2.5, [[0, 1]]):
            with pytest.raises(ModelError, match="reset"):
                live.reset(bad)
    finally:
        live.close()
        plain.close()
    smooth = StreamingSpotter(S, model, smooth_window=8)
    try:
        with pytest.raises(ModelError, match="kws_stream_reset.*running sum"):  # before the first push too
            smooth.reset([1])
        smooth.push(pcm[:, :STEP])
        with pytest.raises(ModelError, match="kws_stream_reset.*running sum"):
            smooth.reset([1])
        assert not smooth.stream_origin.any()
    finally:
        smooth.close()
