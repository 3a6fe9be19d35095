"""The one-launch streaming push (kws_stream_push_i16 with logits on the product arithmetic: launch_dscnn_stream, the F_STREAM
and F_STREAM | F_CLUSTER instantiations of kws_dscnn_fwd_kernel in modes 4 and 5) away from the corner the other streaming
tests run it in: class counts off 12, stream counts at the automatic tile thresholds and beyond the CU count, more than one
ring wrap, route / arithmetic / tile-shape changes on ONE context, and a class-count change under zero-copy delivery.

Gates (the project's own, none new): logits within TOL * max(1, max|f64| / 100) of oracle.dscnn.forward in float64 on the window
the device holds; labels equal wherever the float64 top-2 margin exceeds TOL (at least half of the cases must be such); the
ring within TOL of oracle.psf_mfcc.mfcc of the continuous signal; tile shapes against one workgroup per stream: rings bit for
bit, logits within 2e-5 * max(1, max|logit|), labels identical.  Every device output carries a guard row beyond S."""
import numpy as np
import pytest

import _stream_ref as R
from _dscnn_forward import TOL, load_state
from _stream_ref import Sink

pytestmark = pytest.mark.gpu

CHECKS = (2, 98, 99, 100, 103)   # a partial window, the last partial one, the first full one, the first wrap, the end


@pytest.fixture(scope="module")
def native():
    from kws import _native

    return _native


@pytest.fixture(scope="module")
def he12(e2e_golden):
    """The golden 12-class signal-preserving weights as (cache key, state)."""
    return "he12", R.blob_state(e2e_golden["he.blob"], 12)


def open_push(native, S, state, math, tiles):
    """A context on its own stream with ``state`` loaded and S streams open.  The tests keep the order by hand: inputs are on
    the device before the first push, outputs are read after Context.sync()."""
    c = native.Context(0)
    try:
        load_state(c, state)
        c.set_pointwise_math(getattr(native, math))
        c.stream_open(S)
        c.stream_cluster(tiles)
    except Exception:
        c.close()
        raise
    return c


def report(name, stats):
    print(f"[stream-push-edges] {name}: " + ", ".join(f"{k} {v:.3f} of its gate" for k, v in sorted(stats.items())))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---------------------------------------------------------------------------------- 1. class counts
@pytest.mark.parametrize("tiles", [1, 2, 4])
@pytest.mark.parametrize("math", ["PW_SPLIT_BF16", "PW_PAIR_F16"])
@pytest.mark.parametrize("C", [1, 2, 35, 64])
def test_class_counts_through_the_push(native, C, math, tiles):
    """C = 1, 2, 35, 64 through the push's fc prologue (wv == 0 && lane < C), the logits[clip * C + lane] store, the pinned host
    copy at stride C and -- with 2 and 4 tiles -- fc run by the last tile to arrive.  Three contexts take the same 104 hops at 5
    streams: device outputs only; zero-copy delivery on, read with kws_stream_wait_host; kws_stream_push_host_i16.  At EVERY hop
    the host arrays of the second and third equal the first's device arrays bit for bit and the guard rows are intact; at the
    checked hops the hop counters equal the push count, the three rings are the same bits and within TOL of the psf oracle, and
    logits and labels meet the float64 reference on the device's own window."""
    S, hops = 5, 104
    state, key = R.random_model(C), f"random{C}"
    host, dev = R.pcm_hops(S, hops)
    ctxs = [open_push(native, S, state, math, tiles) for _ in range(3)]
    a, b, c = ctxs
    stats, sure, cases = {}, 0, 0
    try:
        b.stream_host_results(True)
        sa, sb = Sink(S, C), Sink(S, C)
        for t in range(hops):
            a.stream_push_i16(dev[t], sa.logits, sa.labels)
            b.stream_push_i16(dev[t], sb.logits, sb.labels)
            hb = [x.copy() for x in b.stream_wait_host(S)]
            hc = [x.copy() for x in c.stream_push_host_i16(host[t], S)]
            lg, lb = sa.read(a, f"hop {t}")
            lgb, lbb = sb.read(b, f"hop {t} (host results on)")
            assert hb[0].shape == hc[0].shape == (S, C)
            assert same_bits(lgb, lg) and np.array_equal(lbb, lb), f"hop {t}: device arrays with host results on"
            assert same_bits(hb[0], lg) and np.array_equal(hb[1], lb), f"hop {t}: kws_stream_wait_host"
            assert same_bits(hc[0], lg) and np.array_equal(hc[1], lb), f"hop {t}: kws_stream_push_host_i16"
            if C == 1:
                assert (lb == 0).all()
            if t not in CHECKS:
                continue
            wins = [R.device_window(x, S) for x in ctxs]
            assert [w[2] for w in wins] == [t + 1] * 3, f"hop counters after {t + 1} pushes"
            assert same_bits(wins[1][1], wins[0][1]) and same_bits(wins[2][1], wins[0][1]), f"hop {t}: rings"
            R.check_ring(wins[0][0], t + 1, f"hop {t}", stats)
            m = R.check_network(key, state, wins[0][0], lg, lb, f"C={C} {math} tiles={tiles} hop {t}", stats)
            sure, cases = sure + int(m.sum()), cases + len(m)
        assert 2 * sure >= cases, "at least half of the (stream, hop) cases must be sure"
    finally:
        for x in ctxs:
            x.close()
    report(f"class counts C={C} {math} tiles={tiles}", stats)


# ---------------------------------------------------------------------------------- 2. stream counts
def run_shape(native, S, state, shape, dev, hops, checks, math="PW_PAIR_F16"):
    """One context, ``shape`` workgroups per stream (0: automatic): {hop: (logits, labels, raw ring)} at the checked hops; the
    hop counter is asserted there."""
    c = open_push(native, S, state, math, shape)
    out = {}
    try:
        sink = Sink(S, 12)
        for t in range(hops):
            c.stream_push_i16(dev[t], sink.logits, sink.labels)
            if t in checks:
                lg, lb = sink.read(c, f"S={S} shape {shape} hop {t}")
                _, raw, pushed = R.device_window(c, S)
                assert pushed == t + 1, f"S={S} shape {shape}: hop counter {pushed} after {t + 1} pushes"
                out[t] = (lg, lb, raw)
    finally:
        c.close()
    return out


def assert_same_run(x, y, what):
    for t in x:
        assert same_bits(x[t][0], y[t][0]) and np.array_equal(x[t][1], y[t][1]) and same_bits(x[t][2], y[t][2]), f"{what}, hop {t}"


# S: (what the automatic choice must equal, or None; the forced tile shapes held to one workgroup per stream)
STREAM_COUNTS = {1: (None, (4,)), 2: (None, (4, 2)), 64: (4, ()), 65: (2, (4,)), 128: (2, ()), 129: (1, (2,)), 257: (None, (4, 2))}


@pytest.mark.parametrize("S", sorted(STREAM_COUNTS))
def test_stream_counts_at_the_tile_thresholds_and_beyond_the_cus(native, he12, S):
    """The automatic choice (4 tiles up to 64 streams, 2 up to 128, else 1) gives the bits of the forced shape on either side of
    both thresholds.  Forced shapes that no other test launches -- 4 tiles at 1, 2, 65 and 257 streams (1028 workgroups: several
    dispatch waves cross the arrival counters), 2 tiles at 2, 129 and 257 -- hold the ring of the one-workgroup run bit for bit,
    its logits within 2e-5 * max(1, max|logit|) and its labels, advance the hop counter once per push, and repeat their own bits
    on a rerun.  Six streams of the one-workgroup run (first, last, silent, tone, two in the middle) are held to the psf oracle and
    to the float64 logits; the rest are anchored through that run."""
    key, state = he12
    auto, forced = STREAM_COUNTS[S]
    hops = 104
    _, dev = R.pcm_hops(S, hops)
    stats = {}
    run = lambda shape: run_shape(native, S, state, shape, dev, hops, CHECKS)
    base = run(1)
    if auto is not None:
        assert_same_run(run(0), base if auto == 1 else run(auto), f"S={S}: automatic choice vs {auto} tiles")
    for shape in forced:
        first = run(shape)
        assert_same_run(run(shape), first, f"S={S}: {shape} tiles, rerun")
        for t in CHECKS:
            (lg, lb, raw), (lg1, lb1, raw1) = first[t], base[t]
            assert same_bits(raw, raw1), f"S={S} {shape} tiles hop {t}: ring"
            err, gate = float(np.abs(lg - lg1).max()), R.TILE_RTOL * max(1.0, float(np.abs(lg1).max()))
            stats["tile agreement"] = max(stats.get("tile agreement", 0.0), err / gate)
            assert err <= gate, f"S={S} {shape} tiles hop {t}: {err:.3e} > {gate:.3e}"
            assert np.array_equal(lb, lb1), f"S={S} {shape} tiles hop {t}: labels"
    rows = sorted({s for s in (0, S - 1, R.ZERO, R.TONE, S // 3, (2 * S) // 3) if s < S})
    sure = cases = 0
    for t in CHECKS:
        lg, lb, raw = base[t]
        win = R.unroll(raw, t + 1)
        R.check_ring(win, t + 1, f"S={S} hop {t}", stats, rows)
        m = R.check_network(key, state, win, lg, lb, f"S={S} hop {t}", stats, rows)
        sure, cases = sure + int(m.sum()), cases + len(m)
    assert 2 * sure >= cases
    report(f"stream counts S={S}", stats)


# ---------------------------------------------------------------------------------- 3. ring wraps
@pytest.mark.parametrize("tiles", [1, 2])
@pytest.mark.parametrize("math", ["PW_SPLIT_BF16", "PW_PAIR_F16"])
def test_more_than_one_ring_wrap(native, he12, math, tiles):
    """302 hops at 3 streams: the ring wraps at hops 99, 198 and 297.  Ring and logits against their oracles on both sides of
    the second and third wrap and at the end, for the push and for a features-only context (the frame kernel's ring) beside it."""
    key, state = he12
    S, hops = 3, 302
    checks = (197, 198, 199, 296, 297, 298, 301)
    _, dev = R.pcm_hops(S, hops)
    push, feat = open_push(native, S, state, math, tiles), open_push(native, S, state, math, tiles)
    stats, sure, cases = {}, 0, 0
    try:
        sink = Sink(S, 12)
        for t in range(hops):
            push.stream_push_i16(dev[t], sink.logits, sink.labels)
            feat.stream_push_i16(dev[t])
            if t not in checks:
                continue
            lg, lb = sink.read(push, f"hop {t}")
            win, _, pushed = R.device_window(push, S)
            fwin, _, fpushed = R.device_window(feat, S)
            assert pushed == fpushed == t + 1
            R.check_ring(win, t + 1, f"push, hop {t}", stats)
            R.check_ring(fwin, t + 1, f"features only, hop {t}", stats)
            m = R.check_network(key, state, win, lg, lb, f"{math} tiles={tiles} hop {t}", stats)
            sure, cases = sure + int(m.sum()), cases + len(m)
        assert 2 * sure >= cases
    finally:
        push.close()
        feat.close()
    report(f"ring wraps {math} tiles={tiles}", stats)


# ---------------------------------------------------------------------------------- 4. one context, many routes
# The route of hop t is ROUTES[t % 15]: every route is entered from every other kind at some position.  "pair" / "triple": the
# one-launch push on f16 pairs / the bf16 triple; "feat": features only (frame kernel); "f32" / "f32g": the two-launch push
# under KWS_PW_F32, eager / with use_graph.  The tile setting moves 0 -> 4 -> 1 -> 2 -> 0 every fourth hop (period 16 against 15).
ROUTES = ("pair", "triple", "feat", "pair", "f32", "triple", "f32g", "f32g", "pair", "feat", "f32g", "f32", "feat", "triple", "pair")
TILE_CYCLE = (0, 4, 1, 2)
# The checked hops, each right behind a change: 33 feat -> pair (automatic tiles), 34 pair -> f32, 35 f32 -> triple, 36 triple ->
# f32g (a capture), 37 a graph replay, 38 f32g -> pair (tiles 0 -> 4 since the last one-launch push), 39 pair -> feat, 40 feat ->
# f32g, 41 f32g -> f32, 42 f32 -> feat, 43 feat -> triple (tiles 4 -> 1), 44 triple -> pair (tiles 1 -> 2), 46 pair -> triple,
# 48 feat -> pair (tiles 2 -> 0); 98 .. 100: the last partial window, the first full one, the first wrap (pair, feat, f32g)
ROUTE_CHECKS = (33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 46, 48, 98, 99, 100, 134)


def test_one_context_through_every_route(native, he12):
    """One context changes route, arithmetic and tile shape from hop to hop over the shared PCM ring, feature ring and hop
    counter; a second one takes the same 135 hops on the plain one-launch push.  After each kind of change: both hop counters
    equal the push count, the two rings are within TOL of each other and of the psf oracle (one frame against two streams per
    packed transform: float32 rounding only), and the logits of whichever route ran meet the float64 reference on that context's
    own window."""
    key, state = he12
    S, hops = 7, 135
    _, dev = R.pcm_hops(S, hops)
    mixed, plain = open_push(native, S, state, "PW_PAIR_F16", 0), open_push(native, S, state, "PW_PAIR_F16", 0)
    math_of = {"pair": native.PW_PAIR_F16, "triple": native.PW_SPLIT_BF16, "f32": native.PW_F32, "f32g": native.PW_F32}
    stats, sure, cases = {}, 0, 0
    try:
        sm, sp = Sink(S, 12), Sink(S, 12)
        for t in range(hops):
            route = ROUTES[t % len(ROUTES)]
            mixed.stream_cluster(TILE_CYCLE[(t // 4) % 4])
            if route == "feat":
                mixed.stream_push_i16(dev[t])
            else:
                mixed.set_pointwise_math(math_of[route])
                mixed.stream_push_i16(dev[t], sm.logits, sm.labels, use_graph=route == "f32g")
            plain.stream_push_i16(dev[t], sp.logits, sp.labels)
            if t not in ROUTE_CHECKS:
                continue
            what = f"hop {t} ({ROUTES[(t - 1) % len(ROUTES)]} -> {route})"
            lgm, lbm = sm.read(mixed, what)
            lgp, lbp = sp.read(plain, what)
            wm, _, pm = R.device_window(mixed, S)
            wp, _, pp = R.device_window(plain, S)
            assert pm == pp == t + 1, f"{what}: hop counters {pm}, {pp}"
            err = float(np.abs(wm - wp).max())
            stats["ring"] = max(stats.get("ring", 0.0), err / TOL)
            assert err <= TOL, f"{what}: the two rings differ by {err:.3e}"
            R.check_ring(wm, t + 1, f"{what}, mixed routes", stats)
            R.check_ring(wp, t + 1, f"{what}, plain push", stats)
            m = R.check_network(key, state, wp, lgp, lbp, f"{what}, plain push", stats)
            sure, cases = sure + int(m.sum()), cases + len(m)
            if route != "feat":
                m = R.check_network(key, state, wm, lgm, lbm, f"{what}, mixed routes", stats)
                sure, cases = sure + int(m.sum()), cases + len(m)
        assert 2 * sure >= cases
    finally:
        mixed.close()
        plain.close()
    report("one context, many routes", stats)


# ---------------------------------------------------------------------------------- 5. class-count change, zero-copy delivery
def test_class_count_change_under_zero_copy_delivery(native, he12):
    """The zero-copy arrays are sized for the class count loaded when they were made and no loader retires them.  After a reload
    with another class count kws_stream_push_host_i16 makes them again and delivers the new model's results; a
    kws_stream_push_i16 under the stale arrays writes the caller's arrays only, and kws_stream_wait_host then refuses with a
    message that names the class-count change.  12 -> 35 -> 2 -> 12 classes on one context, against a second context that takes
    the same loads and hops through device pushes with host results off: logits and labels bit for bit at every hop, one
    continuous hop counter, guards intact, and the float64 reference after each load."""
    from kws.common.errors import ModelError

    S, first = 5, 101
    models = [he12, ("random35", R.random_model(35)), ("random2", R.random_model(2)), ("random12", R.random_model(12))]
    hops = first + 4 * (len(models) - 1)
    host, dev = R.pcm_hops(S, hops)
    zc, ref = open_push(native, S, he12[1], "PW_PAIR_F16", 0), open_push(native, S, he12[1], "PW_PAIR_F16", 0)
    stats = {}
    try:
        zc.stream_host_results(True)
        t = 0
        for i, (key, state) in enumerate(models):
            C = int(state["fc.weight"].shape[0])
            sink, stale = Sink(S, C), Sink(S, C)
            if i:
                load_state(zc, state)
                load_state(ref, state)
                # a device push under the arrays made for the previous class count: the hop is taken, the caller's arrays hold
                # the results, nothing is delivered to the host arrays and the wait says why
                zc.stream_push_i16(dev[t], stale.logits, stale.labels)
                with pytest.raises(ModelError, match="class count changed"):
                    zc.stream_wait_host(S)
                ref.stream_push_i16(dev[t], sink.logits, sink.labels)
                got, want = stale.read(zc, f"{C} classes, stale arrays"), sink.read(ref, f"{C} classes")
                assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]), f"{C} classes: push under stale arrays"
                t += 1
            for _ in range(first if i == 0 else 3):
                lg, lb = (x.copy() for x in zc.stream_push_host_i16(host[t], S))
                ref.stream_push_i16(dev[t], sink.logits, sink.labels)
                lgr, lbr = sink.read(ref, f"{C} classes, hop {t}")
                assert lg.shape == (S, C)
                assert same_bits(lg, lgr) and np.array_equal(lb, lbr), f"{C} classes, hop {t}"
                t += 1
            wz, _, pz = R.device_window(zc, S)
            wr, _, pr = R.device_window(ref, S)
            assert pz == pr == t, f"{C} classes: hop counters {pz}, {pr} after {t} pushes"
            assert same_bits(wz, wr)
            R.check_ring(wr, t, f"{C} classes, after {t} pushes", stats)
            R.check_network(key, state, wr, lgr, lbr, f"{C} classes, after {t} pushes", stats)
            stale.read(zc, f"{C} classes, after the host pushes")   # they own their outputs: the caller's guard row stays
        assert t == hops
    finally:
        zc.close()
        ref.close()
    report("class-count change", stats)
