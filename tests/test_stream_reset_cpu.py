"""CPU tests of kws_stream_reset: the boundary carries the entry (header, exports, ctypes signature), and the two rules the device
applies to the decision layers mean what the entry promises -- a reset stream's endpointer equals a silent past wherever the
span start is not held at the reset, and the epoch-clipped causal mean equals a fresh run (tests/_reset_ref.py, built on
_live_ref.LiveRef and _live_detect_ref.LiveDetectRef)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _live_detect_ref as ld
import _live_ref as lr
import _reset_ref as rr
import _scan_ref as ref
from conftest import REPO

native = pytest.importorskip("kws._native")


def test_header_exports_and_signature_agree():
    text = open(os.path.join(REPO, "include", "kws_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.findall(r"\bint\s+kws_stream_reset\s*\(([^()]*)\)\s*;", text)
    assert len(m) == 1
    assert [" ".join(p.split()) for p in m[0].split(",")] == ["kws_ctx* ctx", "const int32_t* streams", "int n"]
    res, args = native.SIGNATURES["kws_stream_reset"]
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_int]
    assert hasattr(native.lib(), "kws_stream_reset")
    assert native.lib().kws_abi_version() == 1
    assert callable(native.Context.stream_reset)


def test_the_case_tables_reach_every_path():
    assert rr.K == 3 and rr.POST == 107
    assert [rr.silent_rows(h) for h in rr.H0S] == [0, 0, 0, 1, 48, 99, 99]
    assert set(s for sel in rr.RESET_SETS for s in sel) == set(range(5)) and (4,) in rr.RESET_SETS


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_cleared_endpointer_equals_a_silent_past(seed):
    """Stream 1 of three is reset at every frame of a random flag track.  Its later records equal those of a run whose stream 1 was
    unvoiced up to the reset, except that a span may not start before the reset: where the silent past's start lies at or
    behind the reset they are the same tuple, otherwise only the start differs and it is the reset's first sample.  An utterance
    open at the reset closes there with reason 2, as a flush would close it; the other streams never notice."""
    on, off, pre_roll, max_frames, F, s = 3, 5, 4, 40, 160, 1
    flags = np.stack([lr.flag_track(F, 100 * seed + k, mean_run=9) for k in range(3)])
    clipped = unclipped = closed_open = 0
    for f0 in range(0, F, 7):
        appended = f0 + rr.K - 1  # behind pushes the walk lags the hops by K - 1
        a = rr.ResetLiveRef(3, on, off, pre_roll, max_frames)
        b = lr.LiveRef(3, on, off, pre_roll, max_frames)
        plain = lr.LiveRef(3, on, off, pre_roll, max_frames)
        silent = flags.copy()
        silent[s, :f0] = 0
        got, want, at_reset = [], [], []
        for f in range(F):
            if f == f0:
                flushed = [r for r in plain.flush() if r[0] == s] if f0 else []
                at_reset = a.reset(s, appended)
                assert at_reset == flushed and all(r[4] == f0 - 1 and r[5] == 2 for r in at_reset)
                closed_open += len(at_reset)
                plain = None
            if plain is not None:
                plain.step(flags[:, f])
            got += a.step(flags[:, f])
            want += b.step(silent[:, f])
        assert [r for r in got if r[0] != s] == [r for r in lr.live_run(flags, on, off, pre_roll, max_frames) if r[0] != s and r[5] != 2]
        mine = [r for r in got if r[0] == s and r[4] >= f0]
        theirs = [r for r in want if r[0] == s]
        assert len(mine) == len(theirs)
        for x, y in zip(mine, theirs):
            assert x[2:] == y[2:]
            if y[1] >= appended * lr.FRAME_STEP:
                assert x == y
                unclipped += 1
            else:
                assert x[1] == appended * lr.FRAME_STEP
                clipped += 1
    assert clipped >= 1 and unclipped >= 10 and closed_open >= 3


@pytest.mark.parametrize("W", rr.DETECT_WINDOWS)
def test_epoch_clipped_mean_equals_a_fresh_run(W):
    """Stream 1 of three is reset at decision d0, once more later: from d0 on its smoothed posteriors are, to the bit of float64,
    those of a fresh run over the same logits, its events the fresh run's with d offset by d0 -- the first right at d0, whatever
    its refractory wait was --, and the other streams are those of a run without a reset."""
    S, Cn, steps, s = 3, 12, 90, 1
    z = ref.detect_logits(steps, Cn, [5, 6, 7])
    plain_ev, plain_sm, _ = ld.run(z, W, 2, 0.3, 9)
    for d0, d1 in ((0, 13), (1, 2), (W, W + 1), (41, 70)):
        a = rr.ResetDetectRef(S, Cn, W, 2, 0.3, 9)
        ev, sm = [[] for _ in range(S)], np.zeros((S, steps, Cn))
        for d in range(steps):
            if d in (d0, d1):
                a.reset(s)
            for k, dd, _, label, score in a.step(z[:, d]):
                ev[k].append((dd, label, score))
            sm[:, d] = a.smoothed
        for k in (0, 2):
            assert ev[k] == plain_ev[k] and np.array_equal(sm[k], plain_sm[k])
        for lo, hi in ((d0, d1), (d1, steps)):
            f_ev, f_sm, _ = ld.run(z[s:s + 1, lo:hi], W, 2, 0.3, 9)
            assert np.array_equal(sm[s, lo:hi], f_sm[0])
            assert [(d - lo, k, x) for d, k, x in ev[s] if lo <= d < hi] == f_ev[0]
        assert [e for e in ev[s] if e[0] < d0] == [e for e in plain_ev[s] if e[0] < d0]
    assert sum(len(e) for e in plain_ev) > 10
