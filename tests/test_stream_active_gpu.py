"""GPU tests of the sparse live sets (kws_stream_deactivate, kws_stream_activate, kws_stream_active) through the C ABI.  The oracle
is a DENSE second set on a second context (tests/_active_ref.py): the same audio on a stream while it is active in the sparse set
A, zeros while it is idle there, kws_stream_reset wherever A activates or deactivates it.  A's idle rows hold +-32767 noise, to
prove they are not read.  Everything is bit equality: each active stream runs the same code on the same data."""
import ctypes as C

import numpy as np
import pytest
import torch

import _active_ref as ar
import _live_ref as lr
import _reset_ref as rr
import _scan_ref as ref
import _stream_ref as sr
from kws import _native

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
STEP, T, NF, K = sr.HOP, sr.T, sr.F, rr.K
N_CLASSES = 12
SENTINEL, NO_LABEL = 12345.5, -9
OK, EINVAL, ESTATE, EUNSUPPORTED = _native.KWS_OK, _native.KWS_EINVAL, _native.KWS_ESTATE, _native.KWS_EUNSUPPORTED


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _context(e2e_golden, own_stream=False):
    c = _native.Context(0)
    if not own_stream:
        c.use_torch_stream()
    c.load_dscnn(e2e_golden["he.blob"], N_CLASSES)
    return c


def _hops_of(pcm, step=STEP):
    """int16 [S, n * step] -> [n, S, step] on the device, one contiguous block per push."""
    S = pcm.shape[0]
    d = torch.from_numpy(np.array(pcm.reshape(S, -1, step).transpose(1, 0, 2), order="C")).to(DEV)
    torch.cuda.synchronize()
    return d


def _ring(c, S):
    ring = torch.empty((S, T, NF), dtype=torch.float32, device=DEV)
    c.stream_copy_features(ring)
    _, hops = c.stream_state()
    return ring.cpu().numpy(), hops


def _apply(c, ops):
    for op, streams in ops:
        getattr(c, "stream_" + op)(list(streams))


def _run(c, hops_dev, plan=None, route="device", setup=None, behind=None):
    """A fresh set of S streams on c, every hop pushed back to back; plan: {pushes so far: [(op, streams)]}.  Every push writes a
    row block of its own, pre-filled with a sentinel.  Returns (logits [n, S, C], labels [n, S], final ring, hop count)."""
    n, S = hops_dev.shape[0], hops_dev.shape[1]
    plan = plan or {}
    c.stream_open(S)
    if setup:
        setup(c)
    lg = torch.full((n, S, N_CLASSES), SENTINEL, dtype=torch.float32, device=DEV)
    lb = torch.full((n, S), NO_LABEL, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    for t in range(n + 1):
        _apply(c, plan.get(t, []))
        if t == n:
            break
        if route == "rate":
            c.stream_push_rate_i16(hops_dev[t], lg[t], lb[t])
        else:
            c.stream_push_i16(hops_dev[t], lg[t], lb[t])
        if behind:
            behind(c, t)
    ring, hops = _ring(c, S)
    return lg.cpu().numpy(), lb.cpu().numpy(), ring, hops


def _pair(e2e_golden, pcm, plan, setup=None, route="device", step=STEP, behind_a=None, behind_b=None, keep=False):
    """Set A under `plan`, dense set B under its resets: (a, b, table) and, with keep, the two open contexts."""
    S, n = pcm.shape[0], pcm.shape[1] // step
    table = ar.active_table(S, n, plan)
    xa, xb = ar.two_inputs(pcm, table, step)
    ca, cb = _context(e2e_golden), _context(e2e_golden)
    try:
        a = _run(ca, _hops_of(xa, step), plan, route, setup, behind_a)
        b = _run(cb, _hops_of(xb, step), ar.dense_plan(plan), route, setup, behind_b)
    except BaseException:
        ca.close()
        cb.close()
        raise
    if keep:
        return a, b, table, ca, cb
    ca.close()
    cb.close()
    return a, b, table


def _check_active_rows(a, b, table, what=""):
    """Wherever a stream is active, A's row is B's; wherever it is idle, A's row still holds the sentinel."""
    on = table
    assert np.array_equal(_bits(a[0][on]), _bits(b[0][on])), what
    assert np.array_equal(a[1][on], b[1][on]), what
    assert (a[0][~on] == SENTINEL).all() and (a[1][~on] == NO_LABEL).all(), what
    assert a[3] == b[3] == len(a[0]), what
    assert np.abs(b[0][on]).max() > 0


MATHS = {"split-bf16": _native.PW_SPLIT_BF16, "f16-pair": _native.PW_PAIR_F16}


def _shape(math, cluster):
    def setup(c):
        c.set_pointwise_math(MATHS[math])
        c.stream_cluster(cluster)
    return setup


# ---- 1. sparse equals dense, from the open ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cluster", [1, 4])
@pytest.mark.parametrize("math", sorted(MATHS))
def test_sparse_equals_dense_from_the_open(e2e_golden, math, cluster):
    S, n, idle = 5, T + K - 1 + 20, [0, 2]
    a, b, table = _pair(e2e_golden, sr.stream_pcm(S, n), {0: [("deactivate", idle)]}, _shape(math, cluster))
    assert table[:, [1, 3, 4]].all() and not table[:, idle].any()
    _check_active_rows(a, b, table, (math, cluster))
    # the idle streams' feature rows are what kws_stream_open left; the active ones' are B's
    assert not a[2][idle].any() and np.array_equal(_bits(a[2][[1, 3, 4]]), _bits(b[2][[1, 3, 4]]))


def test_idle_feature_rows_do_not_move_across_pushes(e2e_golden):
    """A stream that was active, then idle: its ring holds what its last active push left, push after push."""
    S, n = 5, 30
    c = _context(e2e_golden)
    try:
        x = _hops_of(ar.two_inputs(sr.stream_pcm(S, n), ar.active_table(S, n, {10: [("deactivate", [0, 2])]}), STEP)[0])
        c.stream_open(S)
        lg = torch.zeros((S, N_CLASSES), dtype=torch.float32, device=DEV)
        seen = []
        for t in range(n):
            if t == 10:
                c.stream_deactivate([0, 2])
                seen.append(_ring(c, S)[0])
            c.stream_push_i16(x[t], lg, None)
            if t in (10, 20, n - 1):
                seen.append(_ring(c, S)[0])
        assert seen[0][[0, 2]].any()
        for r in seen[1:]:
            assert np.array_equal(_bits(r[[0, 2]]), _bits(seen[0][[0, 2]]))
            assert not np.array_equal(_bits(r[[1, 3, 4]]), _bits(seen[0][[1, 3, 4]]))
        assert c.stream_state()[1] == n
        mask, count = c.stream_active(S)
        assert mask.tolist() == [False, True, False, True, True] and count == 3
    finally:
        c.close()


# ---- 2. join and leave mid-run ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h0", rr.H0S)
def test_join_and_leave_mid_run(e2e_golden, h0):
    S, n = 5, h0 + 19 + rr.POST
    plan = {0: [("deactivate", [2])], h0 + 7: [("deactivate", [3])], h0 + 19: [("activate", [3])]}
    plan.setdefault(h0, []).append(("activate", [2]))   # (h0 == 0: right behind the deactivation)
    a, b, table = _pair(e2e_golden, sr.stream_pcm(S, n), plan)
    assert table[:, [0, 1, 4]].all() and table[h0:, 2].all() and not table[:h0, 2].any()
    assert not table[h0 + 7:h0 + 19, 3].any() and table[:h0 + 7, 3].all() and table[h0 + 19:, 3].all()
    _check_active_rows(a, b, table, h0)
    assert np.array_equal(_bits(a[2]), _bits(b[2]))   # every stream is active at the end: the whole ring


# ---- 3. index mapping at word and chunk edges ---------------------------------------------------------------------------------------------
EDGE_SLOTS = [0, 63, 64, 1023, 1024, 1029]


def _scattered(signals, S, slots, fill):
    """signals int16 [k, m] in rows `slots` of an [S, m] array; `fill`: "noise" (+-32767) or "zeros" elsewhere."""
    m = signals.shape[1]
    if fill == "noise":
        out = np.random.default_rng(S).choice(np.array([-32767, 32767], np.int16), size=(S, m))
    else:
        out = np.zeros((S, m), np.int16)
    out[slots] = signals
    return out


@pytest.fixture(scope="module")
def six_dense(e2e_golden):
    """The dense 6-stream set's logits and labels, cluster 1 and default (4): computed once."""
    n = T + K + 5
    sig = sr.stream_pcm(6, n)
    out = {}
    for name, cluster in (("one", 1), ("default", 0)):
        c = _context(e2e_golden)
        try:
            out[name] = _run(c, _hops_of(sig), setup=lambda c: c.stream_cluster(cluster))
        finally:
            c.close()
    return sig, out


def test_a_streams_result_does_not_depend_on_its_slot(e2e_golden, six_dense):
    """What the next test rests on, on DENSE sets: six signals in slots 0 .. 5 of a 6-stream set and in the edge slots of a
    1030-stream set give the same bits (cluster 1 on both)."""
    sig, dense = six_dense
    c = _context(e2e_golden)
    try:
        big = _run(c, _hops_of(_scattered(sig, 1030, EDGE_SLOTS, "zeros")), setup=lambda c: c.stream_cluster(1))
    finally:
        c.close()
    assert np.array_equal(_bits(big[0][:, EDGE_SLOTS]), _bits(dense["one"][0])) and np.array_equal(big[1][:, EDGE_SLOTS], dense["one"][1])


@pytest.mark.parametrize("pinned", [True, False], ids=["cluster1", "cluster-from-active-count"])
def test_six_active_of_1030_at_word_and_chunk_edges(e2e_golden, six_dense, pinned):
    """Unpinned, 6 active of 1030 take the default of a 6-stream set (4 workgroups per stream), not a 1030-stream set's (1)."""
    sig, dense = six_dense
    want = dense["one" if pinned else "default"]
    idle = [s for s in range(1030) if s not in EDGE_SLOTS]
    c = _context(e2e_golden)
    try:
        got = _run(c, _hops_of(_scattered(sig, 1030, EDGE_SLOTS, "noise")), {0: [("deactivate", idle)]},
                   setup=(lambda c: c.stream_cluster(1)) if pinned else None)
        mask, count = c.stream_active(1030)
    finally:
        c.close()
    assert count == 6 and np.flatnonzero(mask).tolist() == EDGE_SLOTS
    assert np.array_equal(_bits(got[0][:, EDGE_SLOTS]), _bits(want[0])) and np.array_equal(got[1][:, EDGE_SLOTS], want[1])
    assert (got[0][:, idle] == SENTINEL).all() and (got[1][:, idle] == NO_LABEL).all() and got[3] == len(want[0])
    if not pinned:  # the two defaults are different launches with different bits somewhere, or this test shows nothing
        assert not np.array_equal(_bits(dense["one"][0]), _bits(dense["default"][0]))


def test_65_active_of_70_take_the_cluster_of_65(e2e_golden):
    n, idle = T + K + 5, [3, 10, 33, 64, 69]
    on = [s for s in range(70) if s not in idle]
    sig = sr.stream_pcm(65, n)
    ca, cb = _context(e2e_golden), _context(e2e_golden)
    try:
        got = _run(ca, _hops_of(_scattered(sig, 70, on, "noise")), {0: [("deactivate", idle)]})
        want = _run(cb, _hops_of(sig))
    finally:
        ca.close()
        cb.close()
    assert ar.default_cluster(65) == 2 == ar.default_cluster(70)
    assert np.array_equal(_bits(got[0][:, on]), _bits(want[0])) and np.array_equal(got[1][:, on], want[1])
    assert (got[0][:, idle] == SENTINEL).all()


# ---- 4. degenerate counts ---------------------------------------------------------------------------------------------------------------
def test_one_active_stream_of_five(e2e_golden):
    S, n = 5, T + K + 5
    a, b, table = _pair(e2e_golden, sr.stream_pcm(S, n), {0: [("deactivate", [0, 1, 2, 4])]})
    assert table.sum(axis=1).tolist() == [1] * n
    _check_active_rows(a, b, table)


def test_no_active_stream_then_one_again(e2e_golden):
    """Pushes with zero active streams: the hop counter advances, the zero-copy flag reaches the push number, nothing else moves;
    a later activation equals the dense set."""
    S, h0, n = 5, 12, 12 + rr.POST
    pcm = sr.stream_pcm(S, n)
    plan = {0: [("deactivate", list(range(S)))], h0: [("activate", [3])]}
    table = ar.active_table(S, n, plan)
    xa, xb = ar.two_inputs(pcm, table, STEP)
    ca, cb = _context(e2e_golden), _context(e2e_golden)
    try:
        b = _run(cb, _hops_of(xb), ar.dense_plan(plan))
        ca.stream_open(S)
        ca.stream_host_results(True)
        ca.stream_deactivate(list(range(S)))
        assert ca.stream_active(S)[1] == 0
        x = _hops_of(xa)
        lg = torch.full((n, S, N_CLASSES), SENTINEL, dtype=torch.float32, device=DEV)
        lb = torch.full((n, S), NO_LABEL, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        for t in range(h0):
            ca.stream_push_i16(x[t], lg[t], lb[t])
            h_lg, h_lb = ca.stream_wait_host(S)          # returns once the flag holds this push's number
            assert not h_lg.any() and not h_lb.any()     # the host rows keep what kws_stream_host_results left
            ring, hops = _ring(ca, S)
            assert hops == t + 1 and not ring.any()
        ca.stream_activate([3])
        for t in range(h0, n):
            ca.stream_push_i16(x[t], lg[t], lb[t])
        h_lg, h_lb = ca.stream_wait_host(S)
        ring, hops = _ring(ca, S)
        a = (lg.cpu().numpy(), lb.cpu().numpy(), ring, hops)
        assert np.array_equal(_bits(h_lg[3]), _bits(a[0][-1, 3])) and h_lb[3] == a[1][-1, 3] and not h_lg[[0, 1, 2, 4]].any()
    finally:
        ca.close()
        cb.close()
    _check_active_rows(a, b, table)
    assert np.array_equal(_bits(a[2][3]), _bits(b[2][3])) and not a[2][[0, 1, 2, 4]].any()


def test_all_deactivated_and_activated_again_is_all_reset(e2e_golden):
    S, h0, n = 5, 40, 40 + rr.POST
    everyone = list(range(S))
    a, b, table = _pair(e2e_golden, sr.stream_pcm(S, n), {h0: [("deactivate", everyone), ("activate", everyone)]})
    assert table.all()
    _check_active_rows(a, b, table)
    assert np.array_equal(_bits(a[2]), _bits(b[2]))


# ---- 5. zero-copy and rate routes -------------------------------------------------------------------------------------------------------
def test_host_push_with_two_of_five_inactive(e2e_golden):
    S, n, idle, on = 5, T + K + 5, [1, 4], [0, 2, 3]
    pcm = sr.stream_pcm(S, n)
    plan = {0: [("deactivate", idle)]}
    table = ar.active_table(S, n, plan)
    xa, xb = ar.two_inputs(pcm, table, STEP)
    ca, cb = _context(e2e_golden), _context(e2e_golden)
    try:
        b = _run(cb, _hops_of(xb), ar.dense_plan(plan))
        ca.stream_open(S)
        ca.stream_host_results(True)
        ca.stream_deactivate(idle)
        host_hops = np.ascontiguousarray(xa.reshape(S, n, STEP).transpose(1, 0, 2))
        dev_hops = _hops_of(xa)
        lg = torch.full((S, N_CLASSES), SENTINEL, dtype=torch.float32, device=DEV)
        lb = torch.full((S,), NO_LABEL, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        for t in range(n):
            if t % 2:   # the hop from host memory, the results from the flag alone
                h_lg, h_lb = ca.stream_push_host_i16(host_hops[t], S)
            else:       # a device push that also delivers to host memory: host rows = device rows
                ca.stream_push_i16(dev_hops[t], lg, lb)
                h_lg, h_lb = ca.stream_wait_host(S)
                h_lg, h_lb = h_lg.copy(), h_lb.copy()
                ca.sync()
                d_lg, d_lb = lg.cpu().numpy(), lb.cpu().numpy()
                assert np.array_equal(_bits(h_lg[on]), _bits(d_lg[on])) and np.array_equal(h_lb[on], d_lb[on]), t
                assert (d_lg[idle] == SENTINEL).all() and (d_lb[idle] == NO_LABEL).all()
            assert np.array_equal(_bits(h_lg[on]), _bits(b[0][t, on])) and np.array_equal(h_lb[on], b[1][t, on]), t
            assert not h_lg[idle].any() and not h_lb[idle].any()   # what kws_stream_host_results left
        assert ca.stream_state()[1] == n
    finally:
        ca.close()
        cb.close()


def test_rate_push_with_a_stream_joining_mid_run(e2e_golden):
    S, h0, rate = 3, 60, 48000
    hop_in = rate // 100
    n = h0 + rr.POST
    x = np.random.default_rng(rate).integers(-12000, 12001, size=(S, n * hop_in)).astype(np.int16)
    setup = lambda c: c.stream_resample_open(S, rate, 16000, hop_in)
    a, b, table = _pair(e2e_golden, x, {0: [("deactivate", [1])], h0: [("activate", [1])]}, setup, "rate", hop_in)
    _check_active_rows(a, b, table)
    assert np.array_equal(_bits(a[2]), _bits(b[2]))


# ---- 6. live utterances -------------------------------------------------------------------------------------------------------------------
UTT_S, UTT_LEAVE, UTT_JOIN = 1, rr.UTT_H0, 70


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


def test_utterances_of_a_stream_that_leaves_mid_utterance_and_joins_again(e2e_golden):
    """Stream 1 leaves after 45 pushes, inside an utterance, and joins after 70.  The threshold (-10) lies far above an all-zero
    frame's log energy (-36), so the dense set's zero-fed stream opens nothing while it is idle -- asserted first, on B alone --
    while A's idle rows are full-scale noise."""
    v = np.zeros((3, rr.UTT_HOPS), bool)
    v[0, 8:24] = v[0, 40:58] = v[0, 80:92] = True
    v[2, 3:15] = v[2, 30:44] = v[2, 62:75] = True
    v[UTT_S, 6:20] = v[UTT_S, 34:60] = v[UTT_S, 85:99] = True
    pcm = lr.pcm_of(v, 7)
    plan = {UTT_LEAVE: [("deactivate", [UTT_S])], UTT_JOIN: [("activate", [UTT_S])]}
    a, b, table, ca, cb = _pair(e2e_golden, pcm, plan, _arm_utt, keep=True)
    try:
        rec_a, total_a, steps_a = _utt_records(ca)
        rec_b, total_b, steps_b = _utt_records(cb)
        mine_b = [r for r in rec_b if r[0] == UTT_S]
        assert [r[5] for r in mine_b] == [0, 2, 0]                               # B alone: nothing opens on zeros
        assert not any(UTT_LEAVE - K < r[3] < UTT_JOIN - K for r in mine_b)      # no open frame inside the idle time
        assert mine_b[1][4] == UTT_LEAVE - K and mine_b[2][3] > UTT_JOIN
        _check_active_rows(a, b, table)
        assert steps_a == steps_b == rr.UTT_HOPS - (K - 1)
        assert rec_a == rec_b and total_a == total_b == len(rec_a)              # all streams, in order
        assert all(len([r for r in rec_a if r[0] == k]) >= 3 for k in (0, 2))
        seq = rec_a.index(mine_b[1])                                            # the record the deactivation closed
        n_out = mine_b[1][2] - mine_b[1][1]
        got, want = _cut(ca, seq, n_out, 16384), _cut(cb, seq, n_out, 16384)
        assert got[1] == want[1] > 0 and np.array_equal(got[0], want[0])
    finally:
        ca.close()
        cb.close()


# ---- 7. live events -----------------------------------------------------------------------------------------------------------------------
REFRACTORY = 20


def test_events_of_a_stream_that_leaves_and_joins_again(e2e_golden):
    """Threshold 0, first_keyword 0: a stream fires whenever its refractory wait is over, and at its first decision after a
    reset.  B's records at (stream, hop) pairs at which the stream was idle in A are dropped; the rest is A's list, in order."""
    S, s, W, leave, join, n = 3, 1, 4, 30, 55, 90
    pcm = sr.stream_pcm(S + 2, n)[[0, 3, 4]]
    arm = lambda c: c.stream_detect_open(N_CLASSES, W, 0, 0.0, REFRACTORY, 0, 4096)
    sm = {k: torch.zeros((n, S, N_CLASSES), dtype=torch.float32, device=DEV) for k in "ab"}
    lb = {k: torch.zeros((n, S), dtype=torch.int32, device=DEV) for k in "ab"}
    watch = lambda k: (lambda c, t: c.stream_detect_smoothed(sm[k][t], lb[k][t]))
    plan = {leave: [("deactivate", [s])], join: [("activate", [s])]}
    a, b, table, ca, cb = _pair(e2e_golden, pcm, plan, arm, behind_a=watch("a"), behind_b=watch("b"), keep=True)
    try:
        _check_active_rows(a, b, table)
        (ta, da), (tb, db) = ca.stream_detect_poll(), cb.stream_detect_poll()
        assert da == db == n
        rec_a, rec_b = ca.stream_detect_read(0, ta), cb.stream_detect_read(0, tb)
        kept = [tuple(int(v) for v in r) for r in rec_b if table[int(r[2]) - 1, int(r[0])]]   # hop h is push h - 1 (0-based)
        assert [tuple(int(v) for v in r) for r in rec_a] == kept
        dropped = [tuple(int(v) for v in r) for r in rec_b if not table[int(r[2]) - 1, int(r[0])]]
        assert dropped and all(r[0] == s for r in dropped)
        assert (s, join, join + 1) in [(r[0], r[1], r[2]) for r in kept]     # its first decision after it joined
        sa, sb = sm["a"].cpu().numpy(), sm["b"].cpu().numpy()
        assert np.array_equal(_bits(sa[table]), _bits(sb[table])) and np.array_equal(lb["a"].cpu().numpy()[table], lb["b"].cpu().numpy()[table])
        assert np.array_equal(_bits(sa[leave:join, s]), _bits(np.broadcast_to(sa[leave - 1, s], (join - leave, N_CLASSES))))   # stale while idle
    finally:
        ca.close()
        cb.close()


# ---- 8. refusals and validation ---------------------------------------------------------------------------------------------------------
def _idx(*v):
    return (C.c_int32 * len(v))(*v)


def test_refused_routes_take_no_hop_and_work_again(e2e_golden):
    S = 3
    c = _context(e2e_golden, own_stream=True)
    try:
        lib, h = c._lib, c._h
        err = lambda: lib.kws_last_error(h).decode()
        hop = torch.zeros((S, STEP), dtype=torch.int16, device=DEV)
        lg = torch.zeros((S, N_CLASSES), dtype=torch.float32, device=DEV)
        st = torch.zeros((S,), dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        p = lambda t: C.c_void_p(t.data_ptr())
        calls = {
            "features-only": ("kws_stream_push_i16", lambda: lib.kws_stream_push_i16(h, p(hop), None, None, 0)),
            "use_graph": ("kws_stream_push_i16", lambda: lib.kws_stream_push_i16(h, p(hop), p(lg), None, 1)),
            "vad": ("kws_stream_vad_f32", lambda: lib.kws_stream_vad_f32(h, C.c_float(lr.THR), 3, 5, p(st))),
        }
        c.stream_open(S)
        c.stream_deactivate([1])
        for what, (name, call) in calls.items():
            assert call() == EUNSUPPORTED and name in err() and "inactive" in err(), what
        c.set_pointwise_math(_native.PW_F32)
        assert lib.kws_stream_push_i16(h, p(hop), p(lg), None, 0) == EUNSUPPORTED and "kws_stream_push_i16" in err() and "diagnostic" in err()
        c.set_pointwise_math(_native.PW_DEFAULT)
        assert c.stream_state()[1] == 0
        c.stream_activate([1])
        for what, (name, call) in calls.items():
            assert call() == OK, (what, err())
        assert c.stream_state()[1] == 2
        # the explicit steps of the armed units
        c.stream_open(S)
        _arm_utt(c)
        c.stream_detect_open(N_CLASSES, 4, 0, 0.0, REFRACTORY, 0, 64)
        energy = torch.zeros((S,), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        steps = {"kws_stream_utt_step_i16": lambda: lib.kws_stream_utt_step_i16(h, p(hop), p(energy)),
                 "kws_stream_detect_step_f32": lambda: lib.kws_stream_detect_step_f32(h, p(lg))}
        c.stream_deactivate([0, 2])
        for name, call in steps.items():
            assert call() == EUNSUPPORTED and name in err() and "inactive" in err()
        assert c.stream_utt_poll()[1] == 0 and c.stream_detect_poll()[1] == 0
        c.stream_activate([0, 2])
        for name, call in steps.items():
            assert call() == OK, (name, err())
        c.sync()
    finally:
        c.close()


def test_cnn_trad_push_is_refused_while_a_stream_is_inactive():
    from oracle import cnn_trad as o_ct

    S = 3
    c = _native.Context(0)
    try:
        c.use_torch_stream()
        c.load_cnn_trad(o_ct.flatten_state(o_ct.random_state(1, num_classes=N_CLASSES)), N_CLASSES)
        c.stream_open(S)
        hop = torch.zeros((S, STEP), dtype=torch.int16, device=DEV)
        lg = torch.zeros((S, N_CLASSES), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        c.stream_deactivate([2])
        rc = c._lib.kws_stream_push_cnn_trad_i16(c._h, C.c_void_p(hop.data_ptr()), C.c_void_p(lg.data_ptr()), None)
        msg = c._lib.kws_last_error(c._h).decode()
        assert rc == EUNSUPPORTED and "kws_stream_push_cnn_trad_i16" in msg and "inactive" in msg
        assert c.stream_state()[1] == 0
        c.stream_activate([2])
        c.stream_push_cnn_trad_i16(hop, lg, None)
        assert c.stream_state()[1] == 1
    finally:
        c.close()


@pytest.mark.parametrize("entry", ["kws_stream_deactivate", "kws_stream_activate"])
def test_validation_changes_nothing(e2e_golden, entry):
    c = _context(e2e_golden)
    try:
        lib, h = c._lib, c._h
        fn = getattr(lib, entry)
        err = lambda: lib.kws_last_error(h).decode()
        assert fn(h, _idx(0), 1) == ESTATE and entry in err() and "kws_stream_open" in err()
        n = C.c_int(-1)
        assert lib.kws_stream_active(h, None, C.byref(n)) == ESTATE and "kws_stream_active" in err()
        S = 3
        c.stream_open(S)
        c.stream_deactivate([2])
        lg = torch.zeros((S, N_CLASSES), dtype=torch.float32, device=DEV)
        sm = torch.zeros((S, N_CLASSES), dtype=torch.float32, device=DEV)
        hop = torch.from_numpy(np.array(sr.stream_pcm(S, 1))).to(DEV)
        torch.cuda.synchronize()
        c.stream_push_i16(hop, lg, None)
        state = lambda: (_ring(c, S)[0].tobytes(), c.stream_active(S)[0].tolist(), c.stream_active(S)[1])
        before = state()
        assert before[1:] == ([True, True, False], 2)
        for args in ((_idx(-1), 1), (_idx(S), 1), (_idx(0, 1, S), 3), (_idx(1, -7), 2), (None, 1), (_idx(0), -1)):
            assert fn(h, *args) == EINVAL and entry in err(), args
            assert state() == before
        assert fn(None, _idx(0), 1) == EINVAL
        assert fn(h, None, 0) == OK and state() == before
        assert lib.kws_stream_active(h, None, None) == OK
        # the running-sum smoother keeps one hop count for all streams: refused while its history is live, before anything changes
        c.stream_activate([2])
        before = state()
        c.stream_smooth_f32(lg, 8, sm)
        assert fn(h, _idx(1), 1) == EUNSUPPORTED and entry in err() and "running sum" in err()
        assert state() == before
        # a new set: every stream active, the list gone, the same call goes through
        c.stream_open(S)
        assert c.stream_active(S) [1] == S and fn(h, _idx(1, 1), 2) == OK
        assert c.stream_active(S)[0].tolist() == [True, entry == "kws_stream_activate", True]
        c.sync()
    finally:
        c.close()


def test_reset_of_an_inactive_stream_is_a_no_op(e2e_golden):
    S, n = 3, 20
    c = _context(e2e_golden)
    try:
        x = _hops_of(np.array(sr.stream_pcm(S, n)))
        c.stream_open(S)
        lg = torch.zeros((S, N_CLASSES), dtype=torch.float32, device=DEV)
        for t in range(n):
            c.stream_push_i16(x[t], lg, None)
        c.stream_deactivate([0])
        before = _ring(c, S)[0]
        c.stream_reset([0])
        assert np.array_equal(_bits(_ring(c, S)[0]), _bits(before)) and before[0].any()
        c.stream_reset([0, 2])
        after = _ring(c, S)[0]
        assert np.array_equal(_bits(after[:2]), _bits(before[:2])) and not np.array_equal(_bits(after[2]), _bits(before[2]))
    finally:
        c.close()


# ---- 9. Python ----------------------------------------------------------------------------------------------------------------------------
def test_streaming_spotter_activate_and_deactivate(e2e_golden):
    from kws.common.errors import ModelError
    from kws.inference import DetectConfig, StreamingSpotter, UtteranceConfig
    from kws.libs.models import CnnTradFpool3, DepthwiseSeparableConv

    model = DepthwiseSeparableConv(num_classes=N_CLASSES)
    model.load_state_dict(ref.state_from_blob(e2e_golden["he.blob"]))
    S, join, leave, hops = 4, 20, 45, 70
    pattern = np.stack([lr.cycles(3, 5, hops)] * S)
    pattern[2, 30:55] = True  # stream 2 is inside an utterance when it leaves
    pcm = lr.pcm_of(pattern, 21)
    plan = {0: [("deactivate", [1])], join: [("activate", [1])], leave: [("deactivate", [2])]}
    table = ar.active_table(S, hops, plan)
    xa, xb = ar.two_inputs(pcm, table, STEP)
    kw = dict(utterances=UtteranceConfig(threshold=lr.THR, on_window=3, off_window=5, pre_roll=4, slack_hops=hops),
              detect=DetectConfig(threshold=0.0, smooth_window=4, refractory=REFRACTORY, first_keyword=0, skip_partial_windows=False))
    sparse = StreamingSpotter(S, model, active=np.array([True, False, True, True]), **kw)
    dense = StreamingSpotter(S, model, **kw)
    try:
        assert sparse.active.dtype == np.bool_ and sparse.active.tolist() == [True, False, True, True] and dense.active.all()
        dense.reset([1])
        closed = None
        for t in range(hops):
            if t == join:
                assert sparse.activate([1]) == join == dense.reset([1]) and sparse.stream_origin.tolist() == [0, join, 0, 0]
                assert sparse.active.all()
            if t == leave:
                sparse.pop_utterances()
                sparse.deactivate(2)
                sparse.deactivate(np.array([2, 2]))
                dense.reset([2])
                closed = [u for u in sparse.pop_utterances() if u.recording == 2]
                assert [u.reason for u in closed] == ["end_of_recording"] and sparse.active.tolist() == [True, True, False, True]
            lb, lg = sparse.push(xa[:, t * STEP:(t + 1) * STEP])
            want_lb, want_lg = dense.push(xb[:, t * STEP:(t + 1) * STEP])
            on = table[t]
            assert np.array_equal(lb[on], want_lb[on]) and np.array_equal(_bits(lg[on]), _bits(want_lg[on])), t
        ev = [(e.stream, e.hop, e.index, e.decision, e.score) for e in sparse.pop_events()]
        want_ev = [(e.stream, e.hop, e.index, e.decision, e.score) for e in dense.pop_events() if table[e.hop - 1, e.stream]]
        assert ev == want_ev != [] and (1, join + 1) in [e[:2] for e in ev]
        for bad in ([-1], [S], 2.5, [[0, 1]]):
            with pytest.raises(ModelError, match="activate"):
                sparse.activate(bad)
            with pytest.raises(ModelError, match="deactivate"):
                sparse.deactivate(bad)
        with pytest.raises(ModelError, match="active expects"):
            StreamingSpotter(S, model, active=[1, 0, 1])
    finally:
        sparse.close()
        dense.close()
    for kwargs, match in ((dict(smooth_window=8), "running sum"), (dict(use_graph=True), "use_graph"), (dict(vad_log_energy=lr.THR), "vad_log_energy")):
        sp = StreamingSpotter(S, model, **kwargs)
        try:
            for call in (sp.deactivate, sp.activate):
                with pytest.raises(ModelError, match=match):
                    call([1])
            assert sp.active.all()
        finally:
            sp.close()
    ct = StreamingSpotter(S, CnnTradFpool3(num_classes=N_CLASSES))
    try:
        with pytest.raises(ModelError, match="CnnTradFpool3"):
            ct.deactivate([0])
        with pytest.raises(ModelError, match="CnnTradFpool3"):
            ct.activate([0])
    finally:
        ct.close()
