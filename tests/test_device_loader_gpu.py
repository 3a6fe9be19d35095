"""GPU tests of the resident training loader: kws_augment_draw against its NumPy restatement, kws_mfcc_augment_i16 against
the composed route (gather, kws_augment_i16, kws_mfcc_f32) bit for bit and against the psf oracle, and DeviceBatchLoader
under the reference's training loop."""
import os
import wave

import numpy as np
import pytest
import torch

from conftest import synth_clips
from oracle import psf_mfcc as o_mfcc
from test_device_loader_cpu import draws

pytestmark = pytest.mark.gpu

TOL = 1e-4  # the suite's MFCC tolerance (tests/test_gpu_parity.py)
N_SAMPLES = 16000
SPECIAL_SHIFTS = [-1600, -1599, -9, -8, -7, -1, 0, 1, 7, 8, 9, 1599]


@pytest.fixture(scope="module")
def native():
    from kws import _native

    return _native


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture()
def ctx(native):
    c = native.Context(0)
    c.use_torch_stream()
    yield c
    c.close()


def to_dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------- draws
@pytest.mark.parametrize("B", [1, 5, 1028, 4096])
def test_draws_equal_the_numpy_restatement(ctx, dev, B):
    N, seed = 5000, 0x1234_5678_9ABC_DEF1
    rng = np.random.default_rng(B)
    labels = rng.integers(0, 12, N).astype(np.int32)
    index = rng.integers(0, N, B).astype(np.int32)
    pools = {1: [40000], 6: [20000, 48000, 16001, 960000, 32000, 61234]}
    out = [torch.empty(B, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.float32, torch.uint8)]
    for with_labels in (True, False):
        for S in (0, 1600):
            for K, lens in pools.items():
                starts = np.cumsum([0] + lens[:-1]).astype(np.int32)
                for epoch in (0, 7):
                    for use_bg in (True, False):
                        ctx.augment_draw(seed, epoch, to_dev(index, dev), *out, labels=to_dev(labels, dev) if with_labels else None,
                                         time_shift=S, bg_start=to_dev(starts, dev), bg_len=to_dev(np.asarray(lens, np.int32), dev),
                                         bg_volume=0.1, bg_frequency=0.8, use_background=use_bg, n_samples=N_SAMPLES)
                        want = draws(seed, epoch, index, labels if with_labels else None, S, starts, lens, N_SAMPLES, 0.1, 0.8, use_bg)
                        for g, w in zip(out, want):
                            g = g.cpu().numpy()
                            assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)), (with_labels, S, K, epoch)
    # no pool at all
    ctx.augment_draw(seed, 0, to_dev(index, dev), *out, labels=to_dev(labels, dev), time_shift=1600, n_samples=N_SAMPLES)
    want = draws(seed, 0, index, labels, 1600, [], [], N_SAMPLES, 0.0, 0.0)
    for g, w in zip(out, want):
        assert np.array_equal(g.cpu().numpy(), w)


def test_draws_of_an_index_do_not_depend_on_the_batch(ctx, dev):
    N, seed, lens = 3000, 99, [20000, 48000, 16001]
    starts = np.cumsum([0] + lens[:-1]).astype(np.int32)
    labels = np.random.default_rng(1).integers(0, 12, N).astype(np.int32)

    def run(index):
        index = np.asarray(index, np.int32)
        out = [torch.empty(len(index), dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.float32, torch.uint8)]
        ctx.augment_draw(seed, 2, to_dev(index, dev), *out, labels=to_dev(labels, dev), time_shift=1600, bg_start=to_dev(starts, dev),
                         bg_len=to_dev(np.asarray(lens, np.int32), dev), bg_volume=0.1, bg_frequency=0.8, n_samples=N_SAMPLES)
        return [o.cpu().numpy() for o in out]

    alone = run([1234])
    other = run([5, 17, 1234, 2999, 0])
    twice = run([1234, 8, 1234])
    for a, o, t in zip(alone, other, twice):
        assert a[0] == o[2] == t[0] == t[2]
    assert any(a[0] != o[0] for a, o in zip(alone, other))  # another index, other draws


# ------------------------------------------------------------------------------------------- fused kernel
@pytest.fixture(scope="module")
def resident(e2e_golden):
    """The 48 diverse golden clips followed by 16 speech-like ones (dense precision flags)."""
    from speechlike import speechlike_set

    return np.ascontiguousarray(np.concatenate([e2e_golden["clips"], speechlike_set()[0]]).astype(np.int16))


def numpy_augment(clips, case):
    """kws_augment_i16's definition in NumPy (the restatement of tests/test_gpu_parity.py::test_augment_matches_numpy_bit_exact)
    on the gathered rows."""
    B, n = len(case["index"]), N_SAMPLES
    out = np.empty((B, n), np.float32)
    for b, row in enumerate(case["index"]):
        a = np.zeros(n, np.float32)
        if not (case["silence"] is not None and case["silence"][b]):
            x = o_mfcc.pcm16_to_float(clips[row])
            s = int(case["shift"][b]) if case["shift"] is not None else 0
            if s >= 0:
                a[s:] = x[: n - s]
            else:
                a[: n + s] = x[-s:]
        if case["bg"] is not None:
            off = int(case["off"][b])
            a = a + case["bg"][off: off + n] * case["vol"][b]
        out[b] = a
    return out


def make_cases(n_clips):
    rng = np.random.default_rng(77)
    bg = (rng.standard_normal(60001) * 0.1).astype(np.float32)
    room = len(bg) - N_SAMPLES

    def case(index, shift=True, pool=True, silence=(), zero_vol=()):
        B = len(index)
        c = dict(index=np.asarray(index, np.int32), shift=None, bg=None, off=None, vol=None, silence=None)
        if shift is True:
            c["shift"] = rng.integers(-1600, 1600, B).astype(np.int32)
            c["shift"][: min(B, 12)] = SPECIAL_SHIFTS[: min(B, 12)]
        elif shift is not None:
            c["shift"] = np.asarray(shift, np.int32)
        if pool:
            c["bg"], c["off"] = bg, rng.integers(0, room + 1, B).astype(np.int32)
            c["vol"] = rng.uniform(0, 1, B).astype(np.float32)
            c["vol"][list(zero_vol)] = 0.0
            c["off"][-1] = room  # the last sample of the pool is read
        if silence is not None:
            c["silence"] = np.zeros(B, np.uint8)
            c["silence"][list(silence)] = 1
        return c

    every = np.tile(np.arange(n_clips), len(SPECIAL_SHIFTS))
    return {
        "b1028_pool": case(rng.integers(0, n_clips, 1028), silence=(20, 21, 500), zero_vol=(21, 22, 23)),
        "b1028_no_pool": case(rng.integers(0, n_clips, 1028), pool=False, silence=(3, 700)),
        "every_clip_every_special_shift": case(every, shift=np.repeat(SPECIAL_SHIFTS, n_clips), silence=None),
        "every_clip_special_shifts_no_pool": case(every, shift=np.repeat(SPECIAL_SHIFTS, n_clips), pool=False, silence=None),
        "b5_no_shift_array": case([4, 9, 50, 63, 1], shift=None, silence=(2,)),
        "b5_descending_repeated": case([63, 40, 40, 7, 0], silence=()),
        "b1_shift_-1600": case([55], shift=[-1600], silence=None),
        "b1_shift_1599_silence": case([3], shift=[1599], silence=(0,)),
        "b1_plain": case([60], shift=None, pool=False, silence=None),
        "plain_all_in_order": case(np.arange(n_clips), shift=None, pool=False, silence=None),
    }


CASE_NAMES = list(make_cases(64))


def run_both(ctx, dev, pcm_dev, case):
    """(fused output, composed output, rows the fused call refined, rows the composed call refined)"""
    B = len(case["index"])
    nf, nc = ctx.frontend_shape()
    idx = to_dev(case["index"], dev)
    kw = dict(shift=to_dev(case["shift"], dev), bg=to_dev(case["bg"], dev), bg_off=to_dev(case["off"], dev),
              bg_vol=to_dev(case["vol"], dev), silence=to_dev(case["silence"], dev))
    fused = torch.full((B, 1, nf, nc), float("nan"), dtype=torch.float32, device=dev)
    rc = ctx.mfcc_augment_i16(pcm_dev, idx, fused, **kw)
    assert rc == 0
    ctx.sync()
    refined_f = ctx.frontend_stats()[2]
    rows = pcm_dev.index_select(0, idx.long())
    sig = torch.empty((B, N_SAMPLES), dtype=torch.float32, device=dev)
    composed = torch.full((B, 1, nf, nc), float("nan"), dtype=torch.float32, device=dev)
    ctx.augment_i16(rows, sig, **kw)
    ctx.mfcc_f32(sig, composed)
    ctx.sync()
    refined_c = ctx.frontend_stats()[2]
    return fused, composed, refined_f, refined_c, sig


@pytest.mark.parametrize("refine", [True, False], ids=["refine", "no_refine"])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_fused_is_bit_identical_to_the_composed_route(ctx, dev, resident, name, refine):
    case = make_cases(len(resident))[name]
    if not refine:
        ctx.set_frontend_refine(0.0)
    fused, composed, rf, rc, sig = run_both(ctx, dev, to_dev(resident, dev), case)
    assert not torch.isnan(fused).any()
    assert torch.equal(fused, composed), f"{name}: {(fused != composed).sum().item()} of {fused.numel()} values differ"
    assert rf == rc
    if not refine:
        assert rf == 0
    elif name in ("b1028_pool", "every_clip_every_special_shift"):
        assert rf > 0  # speech-like clips: the refinement has work, so the equality covers it
    # the composed route's signal is the NumPy restatement's, so both routes transform exactly these samples
    assert np.array_equal(sig.cpu().numpy(), numpy_augment(resident, case))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_fused_features_match_the_psf_oracle(ctx, dev, resident, name):
    """Every frame of every case within TOL of oracle.psf_mfcc on the NumPy-augmented signal: closes the chain from the fused
    kernel to the reference-pinned oracle without a new tolerance."""
    case = make_cases(len(resident))[name]
    B = len(case["index"])
    nf, nc = ctx.frontend_shape()
    kw = dict(shift=to_dev(case["shift"], dev), bg=to_dev(case["bg"], dev), bg_off=to_dev(case["off"], dev),
              bg_vol=to_dev(case["vol"], dev), silence=to_dev(case["silence"], dev))
    got = torch.empty((B, 1, nf, nc), dtype=torch.float32, device=dev)
    ctx.mfcc_augment_i16(to_dev(resident, dev), to_dev(case["index"], dev), got, **kw)
    ctx.sync()
    got = got.cpu().numpy()[:, 0]
    sig = numpy_augment(resident, case)
    worst, where = 0.0, None
    for b in range(B):
        err = np.abs(got[b] - o_mfcc.mfcc(sig[b])).max(axis=1)
        if err.max() > worst:
            worst, where = float(err.max()), (b, int(case["index"][b]), int(err.argmax()))
    print(f"{name}: max |mfcc - oracle| = {worst:.3e} at (row, clip, frame) {where}")
    assert worst <= TOL, (worst, where)


def test_unsupported_front_ends_are_refused_and_the_loader_composes(native, dev, resident):
    from kws.libs.audio_processor import AudioConfig, AudioProcessor
    from kws.libs.data_loader import DeviceBatchLoader

    pcm = to_dev(resident, dev)
    idx = torch.arange(4, dtype=torch.int32, device=dev)
    for setup in ("f64", "40ms"):
        c = native.Context(0)
        c.use_torch_stream()
        if setup == "f64":
            c.set_frontend_math(native.FE_F64)
        else:
            c.set_frontend(frame_len=640, nfft=640)
        nf, nc = c.frontend_shape()
        out = torch.empty((4, 1, nf, nc), dtype=torch.float32, device=dev)
        assert c.mfcc_augment_i16(pcm, idx, out) == native.KWS_EUNSUPPORTED
        c.close()
    # argument errors of the supported configuration
    c = native.Context(0)
    c.use_torch_stream()
    out = torch.empty((4, 1) + c.frontend_shape(), dtype=torch.float32, device=dev)
    with pytest.raises(Exception, match="B must be positive"):
        c.mfcc_augment_i16(pcm, idx[:0], out)
    with pytest.raises(Exception, match="background pool"):
        c.mfcc_augment_i16(pcm, idx, out, bg=torch.zeros(20000, device=dev))
    c.close()

    rng = np.random.default_rng(3)
    labels = rng.integers(0, 12, len(resident))
    noise = [(rng.standard_normal(9000) * 0.1).astype(np.float32), (rng.standard_normal(30000) * 0.1).astype(np.float32)]
    for ap in (AudioProcessor(None, precise=True), AudioProcessor(None, AudioConfig(frame_length=0.040))):
        ap.background_data = noise
        loader = DeviceBatchLoader.from_arrays(resident, labels, ap, 24, seed=11)
        assert loader.fused is False
        batches = list(loader)
        assert [len(y) for _, y in batches] == [24, 24, 16]
        # the composed route by hand, from the NumPy draws
        pool, starts, lens = ap.background_pool(N_SAMPLES)
        order = loader._order(0).cpu().numpy()
        cfg = ap.config
        ctx = loader._ctx
        for k, (x, y) in enumerate(batches):
            index = order[24 * k: 24 * k + 24]
            shift, off, vol, sil = draws(11, 0, index, labels, cfg.time_shift, starts, lens, N_SAMPLES, cfg.background_volume,
                                         cfg.background_frequency)
            sig = torch.empty((len(index), N_SAMPLES), dtype=torch.float32, device=dev)
            ctx.augment_i16(to_dev(resident[index], dev), sig, shift=to_dev(shift, dev), bg=to_dev(pool, dev), bg_off=to_dev(off, dev),
                            bg_vol=to_dev(vol, dev), silence=to_dev(sil, dev))
            want = torch.empty_like(x)
            ctx.mfcc_f32(sig, want)
            assert torch.equal(x, want)
            assert np.array_equal(y.cpu().numpy(), labels[index]) and y.dtype == torch.int64


# ------------------------------------------------------------------------------------------- the loader
@pytest.fixture(scope="module")
def synthetic():
    from kws.libs.audio_processor import AudioProcessor

    rng = np.random.default_rng(8)
    N = 2500
    pcm = synth_clips(N, 12, "gauss")
    labels = rng.integers(0, 12, N)
    ap = AudioProcessor(None)
    ap.background_data = [(rng.standard_normal(7000) * 0.1).astype(np.float32), (rng.standard_normal(50000) * 0.1).astype(np.float32)]
    return pcm, labels, ap


def test_loader_batches_epochs_and_determinism(synthetic, dev):
    from kws.libs.data_loader import DeviceBatchLoader

    pcm, labels, ap = synthetic
    N = len(pcm)
    plain = ap.extract_features_batch(to_dev(pcm, dev))

    loader = DeviceBatchLoader.from_arrays(pcm, labels, ap, 1028, seed=5)
    assert loader.fused and len(loader) == 3 and loader.batch_size == 1028 and len(loader.dataset) == N
    assert loader.nbytes >= pcm.nbytes
    e0 = list(loader)
    assert [tuple(x.shape) for x, _ in e0] == [(1028, 1, 99, 10), (1028, 1, 99, 10), (444, 1, 99, 10)]
    assert all(x.dtype == torch.float32 and y.dtype == torch.int64 and x.is_cuda and y.is_cuda for x, y in e0)
    assert len(list(DeviceBatchLoader.from_arrays(pcm, labels, ap, 1028, drop_last=True))) == 2

    # the same seed: the same batches, bit for bit; the next epoch: another order, other draws
    twin = DeviceBatchLoader.from_arrays(pcm, labels, ap, 1028, seed=5)
    for (x, y), (x2, y2) in zip(e0, twin):
        assert torch.equal(x, x2) and torch.equal(y, y2)
    e1 = list(loader)
    assert loader.epoch == 1
    assert not torch.equal(e0[0][1], e1[0][1]) and not torch.equal(e0[0][0], e1[0][0])
    assert not torch.equal(loader._order(0), loader._order(1))
    other_seed = next(iter(DeviceBatchLoader.from_arrays(pcm, labels, ap, 1028, seed=6)))
    assert not torch.equal(other_seed[0], e0[0][0])
    loader.set_epoch(0)
    again = list(loader)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(e0, again))
    # augmentation changes the features
    assert not torch.equal(e0[0][0], plain.index_select(0, loader._order(0)[:1028].long()))

    # un-augmented, shuffled: the epoch holds every clip exactly once (labels and first feature rows as a multiset)
    shuffled = DeviceBatchLoader.from_arrays(pcm, labels, ap, 1028, seed=5, augment=False)
    seen = sorted((int(l), r.tobytes()) for x, y in shuffled
                  for l, r in zip(y.cpu().numpy(), x[:, 0, 0, :].contiguous().cpu().numpy()))
    have = sorted((int(l), r.tobytes()) for l, r in zip(labels, plain[:, 0, 0, :].contiguous().cpu().numpy()))
    assert seen == have
    # un-augmented, in order: extract_features_batch on the rows
    ordered = DeviceBatchLoader.from_arrays(pcm, labels, ap, 1028, shuffle=False, augment=False)
    xs, ys = zip(*ordered)
    assert torch.equal(torch.cat(xs), plain)
    assert np.array_equal(torch.cat(ys).cpu().numpy(), labels)


def test_loader_draws_are_the_numpy_restatement(synthetic, dev):
    """An augmented batch of the loader is the composed route on the NumPy draws of its indices."""
    from kws.libs.data_loader import DeviceBatchLoader

    pcm, labels, ap = synthetic
    loader = DeviceBatchLoader.from_arrays(pcm, labels, ap, 300, seed=21)
    loader.set_epoch(4)
    x, y = next(iter(loader))
    index = loader._order(4)[:300].cpu().numpy()
    pool, starts, lens = ap.background_pool(N_SAMPLES)
    cfg = ap.config
    shift, off, vol, sil = draws(21, 4, index, labels, cfg.time_shift, starts, lens, N_SAMPLES, cfg.background_volume,
                                 cfg.background_frequency)
    assert sil.any() and (vol > 0).any() and (vol == 0).any() and shift.min() < 0 < shift.max()
    ctx = loader._ctx
    sig = torch.empty((300, N_SAMPLES), dtype=torch.float32, device=dev)
    ctx.augment_i16(to_dev(pcm[index], dev), sig, shift=to_dev(shift, dev), bg=to_dev(pool, dev), bg_off=to_dev(off, dev),
                    bg_vol=to_dev(vol, dev), silence=to_dev(sil, dev))
    want = torch.empty_like(x)
    ctx.mfcc_f32(sig, want)
    assert torch.equal(x, want)
    assert np.array_equal(y.cpu().numpy(), labels[index])


def write_wav(path, data, channels=1):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.ascontiguousarray(data, dtype="<i2").tobytes())


def test_loader_over_a_speech_commands_directory(tmp_path, dev):
    from kws.datasets.speech_commands import DatasetConfig, SpeechCommandDataset
    from kws.libs.audio_processor import AudioProcessor
    from kws.libs.data_loader import DeviceBatchLoader, SpeechCommandsDataLoader

    rng = np.random.default_rng(14)
    for word in ("yes", "no", "bird"):  # "bird" is not a wanted word: the unknown class
        os.makedirs(tmp_path / word)
        for i in range(13):
            n = [16000, 12000, 20000][i % 3]  # full, short (zero-padded) and long (trimmed) clips
            stereo = i == 5
            data = rng.integers(-20000, 20000, (n, 2) if stereo else n, dtype=np.int16)
            write_wav(tmp_path / word / f"{i:08x}_nohash_0.wav", data, 2 if stereo else 1)
    os.makedirs(tmp_path / "_background_noise_")
    write_wav(tmp_path / "_background_noise_" / "hum.wav", rng.integers(-3000, 3000, 9000, dtype=np.int16))  # shorter than a clip: tiled

    ds = SpeechCommandDataset(DatasetConfig(validation_percentage=0, testing_percentage=0), tmp_path)
    ap = AudioProcessor(tmp_path)
    assert len(ap.background_data) == 1 and ap.background_pool(N_SAMPLES)[2] == [27000]
    source = SpeechCommandsDataLoader(ds, ap, "training")
    assert len(source) == 39
    loader = DeviceBatchLoader(source, 16, shuffle=False, augment=False)
    assert loader.dataset is source and len(loader) == 3
    for k, (x, y) in enumerate(loader):
        want_x, want_y = source.collate_pcm16(list(range(16 * k, min(39, 16 * k + 16))))
        assert torch.equal(x, want_x) and torch.equal(y, want_y)
    # augmented batches over the same split: every clip once, labels of the split, features that differ from the plain ones
    aug = DeviceBatchLoader(source, 16, seed=3)
    ys = torch.cat([y for _, y in aug]).cpu().numpy()
    assert sorted(ys.tolist()) == sorted(source.word_to_index[s["label"]] for s in source.data)
    assert not torch.equal(next(iter(aug))[0], next(iter(loader))[0])
    with pytest.raises(Exception, match="empty"):
        DeviceBatchLoader(SpeechCommandsDataLoader(ds, ap, "validation"), 16)


@pytest.mark.parametrize("model_name", ["DepthwiseSeparableConv", "CnnTradFpool3"])
def test_reference_training_loop_over_the_loader(dev, model_name):
    """The reference's train_epoch (train.py:37-49) over a DeviceBatchLoader, augmentation on: four classes of tones that differ
    in pitch, three epochs."""
    from kws.libs import models
    from kws.libs.audio_processor import AudioProcessor
    from kws.libs.data_loader import DeviceBatchLoader

    rng = np.random.default_rng(2)
    N, classes = 512, [2, 3, 4, 5]  # word labels: index 0 is the silence class, whose clips the transform zeroes
    labels = np.repeat(classes, N // 4)
    t = np.arange(N_SAMPLES) / 16000.0
    pitch = {2: 300.0, 3: 700.0, 4: 1500.0, 5: 3000.0}
    pcm = np.stack([np.round(8000 * np.sin(2 * np.pi * pitch[int(l)] * (1 + 0.03 * rng.uniform(-1, 1)) * t + rng.uniform(0, 6.28))
                             + rng.normal(0, 200, N_SAMPLES)) for l in labels]).astype(np.int16)
    ap = AudioProcessor(None)
    ap.background_data = [(rng.standard_normal(40000) * 0.05).astype(np.float32)]
    train_loader = DeviceBatchLoader.from_arrays(pcm, labels, ap, 64, seed=1)

    torch.manual_seed(0)
    model = getattr(models, model_name)(num_classes=6).to(dev)
    criterion = torch.nn.CrossEntropyLoss()
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-3)
    epoch_loss = []
    for epoch in range(3):
        model.train()
        total_loss, correct, total = 0.0, 0, 0
        seen = []
        for inputs, targets in train_loader:
            inputs, targets = inputs.to(dev), targets.to(dev)
            optimizer.zero_grad()
            outputs = model(inputs)
            loss = criterion(outputs, targets)
            loss.backward()
            optimizer.step()
            total_loss += loss.item()
            _, predicted = torch.max(outputs, 1)
            total += targets.size(0)
            correct += (predicted == targets).sum().item()
            seen.append(targets)
        assert total == N and train_loader.epoch == epoch
        assert torch.equal(torch.cat(seen).sort().values.cpu(), torch.from_numpy(np.sort(labels)))
        assert sorted(train_loader._order(epoch).cpu().tolist()) == list(range(N))
        epoch_loss.append(total_loss / len(train_loader))
    print(f"{model_name}: mean loss per epoch {epoch_loss}, last accuracy {correct / total:.3f}")
    assert np.isfinite(epoch_loss).all() and epoch_loss[-1] < epoch_loss[0]
