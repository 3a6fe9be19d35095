"""CPU tests: pin the oracle.

1. against the golden vectors generated from the reference's importable modules
   (tests/golden/make_golden.py): pre-emphasis, framing, power spectrum, DS-CNN;
2. against the recipe of the reference's own unit test
   (tests/kws/libs/speech_features/test_sigproc.py:8-21, rtol 1e-5 / atol 1e-8);
3. analytic known answers for the psf-only tail, which no reference-held
   vector covers (PARITY UNPINNED for mel/log/DCT/lifter/energy).
"""
import math
import os

import numpy as np
import pytest
import torch
from scipy.fftpack import dct

from oracle import dscnn as o_dscnn
from oracle import psf_mfcc as o

SPEC = o.DEFAULT_SPEC


# ------------------------------------------------------------------ golden: sigproc
def test_spec_defaults_match_audio_config():
    assert (SPEC.frame_len, SPEC.frame_step, SPEC.nfft, SPEC.n_bins) == (400, 160, 512, 257)
    assert SPEC.num_frames == 99 and SPEC.nfilt == 26 and SPEC.numcep == 10


def test_preemphasis_bit_exact_float32(sigproc_golden):
    g = sigproc_golden
    for clip, head in zip(g["clips"], g["preemph_head_f32"]):
        y = o.preemphasis(o.pcm16_to_float(clip), 0.97)
        assert y.dtype == np.float32
        assert np.array_equal(y[:64], head)


def test_powspec_matches_reference(sigproc_golden):
    g = sigproc_golden
    keep = g["keep_frames"]
    for clip, ps_ref, en_ref in zip(g["clips"], g["powspec_f64"], g["frame_energy_f64"]):
        y = o.preemphasis(o.pcm16_to_float(clip), 0.97)
        frames = o.framesig(y, 400, 160)
        assert frames.shape == (99, 400) and frames.dtype == np.float64
        ps = o.powspec(frames, 512)
        scale = max(ps_ref.max(), 1e-300)
        np.testing.assert_allclose(ps[keep], ps_ref, rtol=1e-9, atol=1e-12 * scale)
        np.testing.assert_allclose(ps.sum(1), en_ref, rtol=1e-9, atol=1e-12 * scale)


def test_reference_unit_test_recipe(sigproc_golden):
    g = sigproc_golden
    np.random.seed(0)
    sig = np.random.rand(16000)
    mag = o.magspec(o.framesig(sig, 400, 160), 512)
    np.testing.assert_allclose(mag[g["keep_frames"]], g["reftest_magspec_f64"], rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(mag.sum(0), g["reftest_magspec_colsum_f64"], rtol=1e-9)


def test_framing_tail_is_zero_padded():
    sig = np.arange(1, 16001, dtype=np.float64)
    fr = o.framesig(sig, 400, 160)
    assert fr.shape == (99, 400)
    assert np.array_equal(fr[98, :320], sig[15680:]) and np.all(fr[98, 320:] == 0)  # 80 trailing zeros
    assert np.array_equal(fr[1], sig[160:560])
    assert o.framesig(sig[:300], 400, 160).shape == (1, 400)  # shorter than a frame -> 1 frame


def test_fix_length_and_pcm_scale():
    x = np.array([-32768, -1, 0, 1, 32767], np.int16)
    f = o.pcm16_to_float(x)
    assert f.dtype == np.float32 and f[0] == -1.0 and f[4] == np.float32(32767 / 32768)
    assert np.array_equal(o.fix_length(f, 3), f[:3])
    assert np.array_equal(o.fix_length(f, 7), np.concatenate([f, np.zeros(2, np.float32)]))


# ------------------------------------------------------------------ analytic KATs (psf tail, unpinned)
MEL_BINS = [0, 2, 4, 7, 10, 13, 16, 20, 24, 29, 34, 40, 46, 53, 60, 68, 77, 87, 97, 109, 122, 136, 152, 169, 188, 209, 231, 256]
LIFTER = [1, 2.565463, 4.099058, 5.569565, 6.947049, 8.203468, 9.313245, 10.253789, 11.005952, 11.554423]


def test_mel_bin_edges_and_filterbank_shape():
    b = o.mel_bin_edges(26, 512, 16000)
    assert b.astype(int).tolist() == MEL_BINS  # SURVEY.md section 8 a5 [probe]
    fb = o.get_filterbanks(26, 512, 16000)
    assert fb.shape == (26, 257)
    assert np.count_nonzero(fb) == 459
    assert np.all(fb[:, 0] == 0) and np.all(fb[:, 256] == 0)  # bins 0 and 256 feed no filter
    assert np.all(np.count_nonzero(fb, axis=0) <= 2)          # every bin feeds at most two filters
    for j in range(26):  # each triangle peaks at exactly 1.0 on its centre bin
        assert fb[j, MEL_BINS[j + 1]] == 1.0
        assert np.all(fb[j, : MEL_BINS[j]] == 0) and np.all(fb[j, MEL_BINS[j + 2]:] == 0)


def test_lifter_vector():
    np.testing.assert_allclose(o.lifter_vector(10, 22), LIFTER, atol=5e-7)
    assert np.array_equal(o.lifter_vector(10, 0), np.ones(10))


def test_dct_matrix_equals_scipy():
    x = np.random.RandomState(3).standard_normal((5, 26))
    m = o.dct2_ortho_matrix(26, 10)
    np.testing.assert_allclose(x @ m.T, dct(x, type=2, axis=1, norm="ortho")[:, :10], atol=1e-13)


def test_all_zero_clip_known_answer():
    feat = o.extract_features_pcm16(np.zeros(16000, np.int16))
    assert feat.shape == (99, 10) and feat.dtype == np.float64
    assert np.all(feat[:, 0] == math.log(o.EPS))                 # log(eps) = -36.04365338911715
    assert feat[0, 0] == pytest.approx(-36.04365338911715, abs=1e-13)
    np.testing.assert_allclose(feat[:, 1:], 0.0, atol=1e-12)     # constant log-mel vector -> DCT k>=1 vanishes


def test_mfcc_equals_explicit_matrix_form():
    """mfcc() == log-energy + (DCT x lifter) matrix applied to log mel energies."""
    clip = np.random.default_rng(5).integers(-32768, 32768, 16000, dtype=np.int16)
    x = o.pcm16_to_float(clip)
    feat, energy = o.fbank(x)
    m = o.dct2_ortho_matrix(26, 10) * o.lifter_vector(10, 22)[:, None]
    want = np.log(feat) @ m.T
    want[:, 0] = np.log(energy)
    np.testing.assert_allclose(o.mfcc(x), want, atol=1e-11)


def test_impulse_spectrum_is_flat():
    """A single impulse inside a frame gives |X[k]|^2 = a^2 for every bin."""
    clip = np.zeros(16000, np.int16)
    clip[8100] = 16384
    x = o.preemphasis(o.pcm16_to_float(clip), 0.0)  # no pre-emphasis: pure impulse
    ps = o.powspec(o.framesig(x, 400, 160), 512)
    f = 8100 // 160
    np.testing.assert_allclose(ps[f], (0.5 ** 2) / 512, rtol=1e-12)


def test_collate_contract():
    clips = np.random.default_rng(2).integers(-2000, 2000, (3, 16000), dtype=np.int16)
    batch = o.collate_pcm16(clips)
    assert batch.shape == (3, 1, 99, 10) and batch.dtype == np.float32
    np.testing.assert_array_equal(batch[1, 0], o.extract_features_pcm16(clips[1]).astype(np.float32))


# ------------------------------------------------------------------ golden: DS-CNN
@pytest.mark.parametrize("tag", ["n01", "default"])
def test_dscnn_matches_reference(dscnn_golden, tag):
    g = dscnn_golden
    blob = g[f"{tag}.blob"]
    assert blob.shape == (26444,)
    state, off = {}, 0
    for k, shp in o_dscnn.state_shapes(12).items():
        n = int(np.prod(shp))
        state[k] = torch.from_numpy(blob[off:off + n].reshape(shp).copy())
        off += n
    x = torch.from_numpy(g["x"])
    logits, layers = o_dscnn.forward(state, x, return_layers=True)
    np.testing.assert_allclose(logits.numpy(), g[f"{tag}.logits"], rtol=0, atol=1e-6)
    assert np.array_equal(o_dscnn.predict(logits).numpy(), g[f"{tag}.label"])
    probe = [0, 4]
    for name, t in layers.items():
        if t.ndim != 4:
            continue
        a = t.numpy()
        assert list(a.shape) == g[f"{tag}.{name}.shape"].tolist()
        tol = 2e-6 * max(1.0, float(np.abs(a).max()))
        np.testing.assert_allclose(a.mean(axis=(2, 3)), g[f"{tag}.{name}.chan_mean"], atol=tol)
        np.testing.assert_allclose(a[probe][:, :, :3, :3], g[f"{tag}.{name}.corner"], atol=tol)
        np.testing.assert_allclose(a[probe][:, :, a.shape[2] // 2, :], g[f"{tag}.{name}.row_mid"], atol=tol)
        np.testing.assert_allclose(a[probe][:, :, :, 1], g[f"{tag}.{name}.col1"], atol=tol)


def _state_of(blob, input_channels=1):
    state, off = {}, 0
    for k, shp in o_dscnn.state_shapes(12, input_channels).items():
        n = int(np.prod(shp))
        state[k] = torch.from_numpy(blob[off:off + n].reshape(shp).copy())
        off += n
    assert off == blob.size
    return state


def test_dscnn_matches_reference_on_signal_preserving_weights(e2e_golden):
    """The 'he' tag: weights that carry the input to the logits, 8 random maps + the oracle MFCC of 48 diverse clips.
    Expected values are the imported reference module's; gates are RELATIVE to each tensor's scale.  The fixture itself
    is checked for power: >= 6 classes, logits that move from clip to clip, silence far from noise."""
    g = e2e_golden
    x = torch.from_numpy(np.concatenate([g["x_rand"], o.collate_pcm16(g["clips"])]))
    logits, layers = o_dscnn.forward(_state_of(g["he.blob"]), x, return_layers=True)
    ref = g["he.logits"]
    assert np.abs(logits.numpy() - ref).max() <= 2e-6 * np.abs(ref).max()
    assert np.array_equal(o_dscnn.predict(logits).numpy(), g["he.label"])
    assert len(set(g["he.label"][8:].tolist())) >= 6 and ref[8:].std(axis=0).mean() >= 0.1
    assert np.abs(ref[8] - ref[12]).max() > 0.5           # zeros vs full-range uniform noise
    top2 = np.sort(ref, axis=1)[:, -2:]
    assert (top2[:, 1] - top2[:, 0]).min() > 1e-3          # no near-tie in the fixture: every label is decidable
    probe = [0, 4]
    for name, t in layers.items():
        a = t.numpy()
        if a.ndim != 4:
            continue
        tol = 2e-6 * float(np.abs(a).max())
        np.testing.assert_allclose(a.mean(axis=(2, 3)), g[f"he.{name}.chan_mean"], atol=tol)
        np.testing.assert_allclose(a[probe][:, :, :3, :3], g[f"he.{name}.corner"], atol=tol)
        np.testing.assert_allclose(a[probe][:, :, a.shape[2] // 2, :], g[f"he.{name}.row_mid"], atol=tol)
        np.testing.assert_allclose(a[probe][:, :, :, 1], g[f"he.{name}.col1"], atol=tol)
    d4 = layers["dsconv4"].numpy()
    np.testing.assert_allclose(d4[probe], g["he.dsconv4.full"], atol=2e-6 * float(np.abs(d4).max()))
    np.testing.assert_allclose(layers["pool"].numpy(), g["he.pool"], atol=2e-6 * float(np.abs(g["he.pool"]).max()))


def test_argmax_ties_follow_torch_max(e2e_golden):
    """First maximum wins (kws/libs/training.py:371): the oracle's predict() on the two tie fixtures gives the labels
    the reference module's torch.max gave."""
    g = e2e_golden
    x = torch.from_numpy(np.concatenate([g["x_rand"], o.collate_pcm16(g["clips"])]))
    lo, hi = (int(v) for v in g["tie_pair.lo_hi"])
    for tag in ("tie_all", "tie_pair"):
        logits = o_dscnn.forward(_state_of(g[f"{tag}.blob"]), x)
        assert np.abs(logits.numpy() - g[f"{tag}.logits"]).max() <= 2e-6 * np.abs(g[f"{tag}.logits"]).max()
        # decide on the reference's own logits, so the tie is exact whatever this host's summation order is
        assert np.array_equal(o_dscnn.predict(torch.from_numpy(g[f"{tag}.logits"])).numpy(), g[f"{tag}.label"])
    assert np.all(g["tie_all.label"] == 0)
    assert np.array_equal(g["tie_pair.logits"][:, lo], g["tie_pair.logits"][:, hi])
    assert (g["tie_pair.label"] == lo).sum() >= 3 and not (g["tie_pair.label"] == hi).any()


def test_standalone_block_matches_reference(dsblock_golden):
    g = dsblock_golden
    for i, (ci, co, k, st, pd, B, H, W) in enumerate(g["cases"].tolist()):
        params = {n: torch.from_numpy(g[f"c{i}.{n}"]) for n in ("depthwise.weight", "depthwise.bias", "pointwise.weight", "pointwise.bias")}
        y = o_dscnn.block_forward(params, torch.from_numpy(g[f"c{i}.x"]), k, st, pd).numpy()
        want = g[f"c{i}.y"]
        ho, wo = (H + 2 * pd - k) // st + 1, (W + 2 * pd - k) // st + 1
        assert y.shape == want.shape == (B, co, ho + 2 * pd, wo + 2 * pd)
        assert np.abs(y - want).max() <= 2e-6 * np.abs(want).max()
        if pd:  # the ring of the padded 1x1 convolution is relu(bias)
            ring = np.maximum(g[f"c{i}.pointwise.bias"], 0)
            assert np.array_equal(want[0, :, 0, :], np.broadcast_to(ring[:, None], want[0, :, 0, :].shape))


def test_multichannel_oracle_matches_reference():
    """oracle.dscnn.forward(input_channels=3) in float64 reproduces what the imported reference module recorded
    (make_golden.py multichannel): the logits of the ten maps and conv1's output on the first two, within 2e-6 of the output's
    scale -- the generator's own cross-check gate.  The GPU tests of the multi-channel model use this oracle as their truth."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "multichannel_golden.npz"))
    state = _state_of(g["blob"], 3)
    assert tuple(state["conv1.weight"].shape) == (64, 3, 10, 10)
    logits, layers = o_dscnn.forward(state, torch.from_numpy(g["x"]).double(), return_layers=True)
    assert logits.dtype == torch.float64 and logits.shape == g["logits"].shape
    assert np.abs(logits.numpy() - g["logits"]).max() <= 2e-6 * np.abs(g["logits"]).max()
    conv1 = layers["conv1"][:2].numpy()
    assert conv1.shape == g["conv1"].shape == (2, 64, 47, 3)
    assert not g["x"][1].any()  # the second map is all zero: conv1's recorded output there is relu(bias), exactly
    assert np.array_equal(g["conv1"][1], np.broadcast_to(np.maximum(state["conv1.bias"].numpy(), 0)[:, None, None], (64, 47, 3)))
    assert np.abs(conv1 - g["conv1"]).max() <= 2e-6 * np.abs(g["conv1"]).max()
    assert np.array_equal(o_dscnn.predict(torch.from_numpy(g["logits"])).numpy(), g["label"])


def test_dscnn_shapes_and_relu_bias_ring():
    st = o_dscnn.random_state(seed=3)
    x = torch.randn(2, 1, 99, 10)
    logits, layers = o_dscnn.forward(st, x, return_layers=True)
    assert logits.shape == (2, 12)
    assert [tuple(layers[f"dsconv{i}"].shape[2:]) for i in range(1, 5)] == [(49, 5), (51, 7), (53, 9), (55, 11)]
    assert tuple(layers["conv1"].shape[1:]) == (64, 47, 3)
    for i in range(1, 5):  # the ring a 1x1 conv with padding=1 adds is exactly relu(bias)
        z = layers[f"dsconv{i}"]
        ring = torch.relu(st[f"dsconv{i}.pointwise.bias"])
        assert torch.equal(z[0, :, 0, :], ring[:, None].expand(-1, z.shape[3]))
        assert torch.equal(z[1, :, :, -1], ring[:, None].expand(-1, z.shape[2]))


def test_dscnn_double_precision_agrees():
    st = o_dscnn.random_state(seed=4)
    x = torch.randn(4, 1, 99, 10)
    np.testing.assert_allclose(o_dscnn.forward(st, x).numpy(), o_dscnn.forward(st, x.double()).numpy(), atol=5e-6)


def test_endpointer_known_answer():
    """The endpointer's hysteresis (reference thresholds, inference_local.py:151,161): a 100-hop voiced stretch in
    silence opens after 33 voiced hops of the 40-hop window and closes after 73 unvoiced hops of the 80-hop window."""
    from oracle.endpointer import EnergyEndpointer

    e = EnergyEndpointer(-10.0)
    events = []
    for t in range(300):
        trig, ev = e.update(0.0 if 50 <= t < 150 else -36.0)
        if ev:
            events.append((t, ev))
    assert events == [(82, 1), (222, 2)]
    short = EnergyEndpointer(-10.0)
    assert not any(short.update(0.0 if 10 <= t < 40 else -36.0)[0] for t in range(200))  # 30 voiced hops never reach 80 % of 40


def test_audit_fixtures_hold_what_their_names_say():
    """tests/golden/audit_hard_clips.npz and audit_exception_clips.npz (make_audit_fixture.py): the named frames have log-mel
    spans of 11.5-12.0 and 10.8-11.5 -- under the span thresholds round 3 tried first -- and lie well over the threshold of the
    flag the kernel has now (largest spectral bin against the weakest mel band, default 10.2)."""
    here = os.path.join(os.path.dirname(__file__), "golden")
    for name, lo, hi in (("audit_hard_clips.npz", 11.5, 12.0), ("audit_exception_clips.npz", 10.8, 11.5)):
        d = np.load(os.path.join(here, name))
        assert d["clips"].shape == (4, 16000) and d["clips"].dtype == np.int16
        for c, fr in zip(d["clips"], d["frames"]):
            sig = o.fix_length(o.pcm16_to_float(c), 16000)
            feat, _ = o.fbank(sig)
            lm = np.log(feat)
            span = lm.max(1) - lm.min(1)
            ps = o.powspec(o.framesig(o.preemphasis(sig, 0.97), 400, 160), 512)
            with np.errstate(divide="ignore"):
                ratio = np.log(ps.max(1)) - lm.min(1)
            for f in np.atleast_1d(fr):
                if f >= 0:
                    assert lo < span[f] <= hi, (name, f, span[f])
                    assert ratio[f] > 10.7, (name, f, ratio[f])
