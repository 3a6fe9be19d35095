"""Evaluation statistics on the GPU -- kws_eval_open / reset / close / update_f32 / read, kws.libs.evaluation.Evaluator and
evaluate() -- at wavefront and workgroup edges of B, at the class and bin counts that select each counting path (private LDS
counters where 2 C K <= 8192 of them fit, global atomics otherwise, no histograms at K = 0).

References.  Counts: the NumPy restatement of tests/_eval_ref.py fed the device's own kws_softmax_f32 output for the same logits
and the first argmax of the logits -- equal exactly.  Bins: independently, a float64 softmax; entries whose p64 K lies within
K 1e-6 (the softmax gate of tests/test_stream_decisions_gpu.py) of an interior integer are left out, no other entry may differ,
and the share left out is printed and at most 1 %.  Row losses and gradient: float64, within 4 x the error of torch-CPU float32
on the same logits + 1e-6 of the largest reference magnitude (the project's 4 x torch-f32 idiom).

Every case enqueues all its work first and then reads back once: the statistics, then one tensor holding every other output."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _eval_ref as ref
from kws import _native

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
I32_MIN = np.iinfo(np.int32).min


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    c.use_torch_stream()
    yield c
    c.close()


def _rc(c, name, *args):
    """Return code of the raw C entry (the Context methods cannot pass NULL for a required pointer)."""
    return getattr(c._lib, name)(c._h, *args)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_update(ctx, z, truth, grad_scale=None):
    """Enqueue kws_softmax_f32 and one update with both optional outputs; returns the device tensors (p, dlogits, loss_rows)."""
    B, C = z.shape
    zd, td = to_dev(z), to_dev(np.asarray(truth, dtype=np.int32))
    p = torch.full((B, C), float("nan"), device=DEV)
    dl = torch.full((B, C), float("nan"), device=DEV)
    rows = torch.full((B,), float("nan"), device=DEV)
    ctx.softmax_f32(zd, p)
    ctx.eval_update_f32(zd, td, 1.0 / B if grad_scale is None else grad_scale, dl, rows)
    return p, dl, rows


def read_all(ctx, *tensors):
    """The one read-back of a case: the statistics (kws_eval_read waits for the stream), then every tensor in one copy."""
    stats = ctx.eval_read()
    flat = torch.cat([t.reshape(-1) for t in tensors]).cpu().numpy()
    out, off = [], 0
    for t in tensors:
        out.append(flat[off:off + t.numel()].reshape(tuple(t.shape)))
        off += t.numel()
    return stats, out


def assert_stats(stats, want, K):
    counts, _, confusion, pos, neg = stats
    w_counts, w_conf, w_pos, w_neg = want
    assert np.array_equal(counts.astype(np.int64), w_counts), (counts, w_counts)
    assert np.array_equal(confusion.astype(np.int64), w_conf)
    assert pos.shape == neg.shape == (w_conf.shape[0], K)
    assert np.array_equal(pos.astype(np.int64), w_pos) and np.array_equal(neg.astype(np.int64), w_neg)


# B: wavefront (63 / 64 / 65) and workgroup (255 / 256 / 257) edges, one row, a ragged last workgroup with several partials (4099);
# 2 C K <= 8192 counters live in LDS: (2, 2), (12, 16), (64, 16), (12, 256); (12, 1024), (64, 1024) use global atomics; K = 0: none.
# The nine (4099, C in {2, 12, 64}, 1024) cases with randn x {1, 5, 30} are the inputs of the float64 bin check.
CASES = [(1, 1, 0, 5.0), (63, 2, 2, 1.0), (64, 12, 16, 5.0), (65, 64, 1024, 30.0), (255, 12, 1024, 1.0), (256, 64, 16, 5.0),
         (257, 2, 0, 30.0), (257, 1, 16, 5.0), (4099, 12, 256, 5.0), (4099, 64, 2, 30.0)]
CASES += [(4099, C, 1024, s) for C in (2, 12, 64) for s in (1.0, 5.0, 30.0)]


@pytest.mark.parametrize("B,C,K,scale", CASES)
def test_update_against_restatement_and_float64(ctx, B, C, K, scale):
    z, truth = ref.logits_for(100000 * C + 10 * B + K, B, C, scale)
    if B >= 63:  # rows outside the statistics among the others: their outputs are zeros
        truth[5], truth[40] = -1, C
        z[7, C - 1], z[41, 0] = np.nan, -np.inf
    used, ignored, nonfinite = ref.row_kinds(z, truth, C)
    ctx.eval_open(C, K)
    p_d, dl_d, rows_d = run_update(ctx, z, truth)
    stats, (p, dl, rows) = read_all(ctx, p_d, dl_d, rows_d)

    # counts: exactly the restatement on the device's own posteriors
    assert_stats(stats, ref.counts_from(p, z, truth, K), K)
    assert stats[0][0] == used.sum() and stats[0][2] == ignored.sum() and stats[0][3] == nonfinite.sum()

    # bins: independently against float64
    zu, tu = z[used].astype(np.float64), truth[used].astype(np.int64)
    p64 = ref.softmax64(zu)
    if K > 0:
        x = p64 * K
        near = np.rint(x)
        excluded = (np.abs(x - near) <= K * 1e-6) & (near >= 1) & (near <= K - 1)
        got, want = ref.bins_of(p[used], K), np.minimum(K - 1, np.floor(x).astype(np.int64))
        share = excluded.mean()
        print(f"B={B} C={C} K={K} scale={scale}: {100 * share:.4f} % of the bins within the margin, "
              f"{int(((got != want) & ~excluded).sum())} differ outside it")
        assert not ((got != want) & ~excluded).any()
        assert share <= 0.01

    # row losses: 4 x torch-f32 + 1e-6 of the largest
    n = int(used.sum())
    l64 = F.cross_entropy(torch.from_numpy(zu), torch.from_numpy(tu), reduction="none").numpy()
    l32 = F.cross_entropy(torch.from_numpy(z[used]), torch.from_numpy(tu), reduction="none").numpy()
    err32 = np.abs(l32 - l64).max()
    err = np.abs(rows[used] - l64).max()
    tol = 4 * err32 + 1e-6 * np.abs(l64).max()
    print(f"  loss rows: err {err:.3e}, torch-f32 {err32:.3e}, tol {tol:.3e}")
    assert err <= tol
    assert (rows[~used] == 0.0).all()
    loss_sum = stats[1]
    want_sum = rows.astype(np.float64).sum()
    assert abs(loss_sum - want_sum) <= 1e-12 * abs(want_sum)

    # gradient: (softmax - onehot) / B
    onehot = np.arange(C)[None, :] == tu[:, None]
    g64 = (p64 - onehot) / B
    g32 = ((torch.softmax(torch.from_numpy(z[used]), dim=1) - torch.from_numpy(onehot.astype(np.float32))) * (1.0 / B)).numpy()
    gerr32 = np.abs(g32 - g64).max()
    gerr = np.abs(dl[used] - g64).max()
    gtol = 4 * gerr32 + 1e-6 * np.abs(g64).max()
    print(f"  dlogits: err {gerr:.3e}, torch-f32 {gerr32:.3e}, tol {gtol:.3e}")
    assert gerr <= gtol
    assert (dl[~used] == 0.0).all() and not np.isnan(dl).any() and n == len(zu)


def test_optional_outputs_may_be_absent(ctx):
    """Without d_dlogits and d_loss_rows the statistics are the same (grad_scale is not read: NaN is passed)."""
    B, C, K = 300, 12, 16
    z, truth = ref.logits_for(3, B, C, 5.0)
    ctx.eval_open(C, K)
    zd, td = to_dev(z), to_dev(truth)
    p = torch.empty((B, C), device=DEV)
    ctx.softmax_f32(zd, p)
    ctx.eval_update_f32(zd, td, float("nan"))
    stats, (p,) = read_all(ctx, p)
    assert_stats(stats, ref.counts_from(p, z, truth, K), K)
    assert np.isfinite(stats[1]) and stats[1] > 0


@pytest.mark.parametrize("K", [16, 1024])
def test_accumulation_reset_and_determinism(ctx, K):
    """Updates of 257, 65 and 1 rows give the counts of their concatenation; after a reset the same sequence gives bit-identical
    loss_sum and counts; a reset zeroes everything."""
    C = 12
    z, truth = ref.logits_for(11 + K, 257 + 65 + 1, C, 5.0)
    parts = [(0, 257), (257, 322), (322, 323)]
    ctx.eval_open(C, K)
    zd, td = to_dev(z), to_dev(truth)
    p = torch.empty((len(z), C), device=DEV)
    ctx.softmax_f32(zd, p)
    rows = torch.empty((len(z),), device=DEV)

    def sequence():
        for a, b in parts:
            ctx.eval_update_f32(zd[a:b], td[a:b], 0.0, None, rows[a:b])

    sequence()
    first, (p_h, rows_h) = read_all(ctx, p, rows)
    assert_stats(first, ref.counts_from(p_h, z, truth, K), K)
    assert first[0][0] == 323
    assert abs(first[1] - rows_h.astype(np.float64).sum()) <= 1e-12 * first[1]
    # the order of the sum: every workgroup's 256 rows by its tree, the partials of a call in index order, the calls in sequence
    want = np.float64(0.0)
    for a, b in parts:
        for k in range(a, b, 256):
            want += _tree_sum(rows_h[k:min(k + 256, b)])
    assert np.float64(first[1]).tobytes() == want.tobytes()
    ctx.eval_reset()
    zeros = ctx.eval_read()
    assert not zeros[0].any() and zeros[1] == 0.0 and not zeros[2].any() and not zeros[3].any() and not zeros[4].any()
    sequence()
    second = ctx.eval_read()
    assert np.float64(second[1]).tobytes() == np.float64(first[1]).tobytes()
    for a, b in zip(first, second):
        assert np.array_equal(a, b)


def _tree_sum(v):
    """Float64 sum of up to 256 float32 values by the workgroup's fixed tree (stride 128, 64, ... 1)."""
    red = np.zeros(256, np.float64)
    red[:len(v)] = v
    s = 128
    while s:
        red[:s] += red[s:2 * s]
        s //= 2
    return red[0]


@pytest.mark.parametrize("K", [16, 1024])
def test_no_update_is_lost_under_contention(ctx, K):
    """4099 identical rows hit one confusion cell and one bin per class, through the LDS counters (K = 16) and through global
    atomics (K = 1024)."""
    B, C = 4099, 12
    row, _ = ref.logits_for(21, 1, C, 5.0)
    z = np.repeat(row, B, axis=0)
    truth = np.full(B, 3, np.int32)
    ctx.eval_open(C, K)
    p_d, dl_d, rows_d = run_update(ctx, z, truth)
    stats, (p, dl, rows) = read_all(ctx, p_d, dl_d, rows_d)
    counts, loss_sum, confusion, pos, neg = stats
    pred = int(np.argmax(row[0]))
    assert list(counts) == [B, B if pred == 3 else 0, 0, 0]
    assert confusion[3, pred] == B and confusion.sum() == B
    bins = ref.bins_of(p[0], K)
    assert (p == p[0]).all() and (rows == rows[0]).all() and (dl == dl[0]).all()
    for c in range(C):
        hit, other = (pos, neg) if c == 3 else (neg, pos)
        assert hit[c, bins[c]] == B and hit[c].sum() == B and other[c].sum() == 0
    assert abs(loss_sum - B * float(rows[0])) <= 1e-12 * loss_sum


def test_edges_of_rows_labels_and_logits(ctx):
    C, K = 4, 16
    z = np.zeros((9, C), np.float32)
    truth = np.zeros(9, np.int32)
    z[0], truth[0] = [1, 3, 3, 0], 2               # equal maxima: the first wins
    z[1], truth[1] = [100, -100, -100, -100], 0    # p = 1 lands in bin K - 1, an underflowed p in bin 0
    truth[2:6] = [-1, C, -100, I32_MIN]            # ignored
    z[2:6] = [5, 4, 3, 2]
    truth[6:9] = [1, 2, 3]                         # non-finite rows
    z[6, 1], z[7, 0], z[8, 3] = np.nan, np.inf, -np.inf
    ctx.eval_open(C, K)
    p_d, dl_d, rows_d = run_update(ctx, z, truth, grad_scale=1.0)
    stats, (p, dl, rows) = read_all(ctx, p_d, dl_d, rows_d)
    counts, loss_sum, confusion, pos, neg = stats
    assert list(counts) == [2, 1, 4, 3]
    want_conf = np.zeros((C, C), np.int64)
    want_conf[2, 1] = want_conf[0, 0] = 1
    assert np.array_equal(confusion.astype(np.int64), want_conf)
    x0 = ref.softmax64(z[0]) * K
    assert np.abs(x0 - np.rint(x0)).min() > 1e-3  # no bin of row 0 is in doubt
    want_pos, want_neg = np.zeros((C, K), np.int64), np.zeros((C, K), np.int64)
    for c in range(C):
        (want_pos if c == 2 else want_neg)[c, int(x0[c])] += 1
    want_pos[0, K - 1] += 1
    for c in (1, 2, 3):
        want_neg[c, 0] += 1
    assert np.array_equal(pos.astype(np.int64), want_pos) and np.array_equal(neg.astype(np.int64), want_neg)
    assert list(p[1]) == [1.0, 0.0, 0.0, 0.0] and rows[1] == 0.0 and list(dl[1]) == [0.0, 0.0, 0.0, 0.0]
    assert (rows[2:] == 0.0).all() and (dl[2:] == 0.0).all()
    l0 = -np.log(ref.softmax64(z[0])[2])
    assert abs(rows[0] - l0) <= 1e-6 and abs(loss_sum - float(rows[0])) <= 1e-12
    assert np.abs(dl[0] - (ref.softmax64(z[0]) - np.array([0, 0, 1, 0]))).max() <= 1e-6


def test_return_codes():
    c = _native.Context(0)
    c.use_torch_stream()
    try:
        z = torch.zeros((4, 12), device=DEV)
        t = torch.zeros((4,), dtype=torch.int32, device=DEV)
        counts = np.zeros(4, np.uint64)
        cp = counts.ctypes.data_as(_native.C.POINTER(_native.C.c_uint64))
        update = lambda zp, tp, B: _rc(c, "kws_eval_update_f32", zp, tp, B, 0.25, None, None)
        read = lambda: _rc(c, "kws_eval_read", cp, None, None, None, None)
        # before an open
        assert update(z.data_ptr(), t.data_ptr(), 4) == _native.KWS_ESTATE
        assert _rc(c, "kws_eval_reset") == _native.KWS_ESTATE
        assert read() == _native.KWS_ESTATE
        for C, K in ((0, 16), (65, 16), (-1, 16), (12, 3), (12, 2048), (12, 1), (12, -2)):
            assert _rc(c, "kws_eval_open", C, K) == _native.KWS_EINVAL, (C, K)
        assert read() == _native.KWS_ESTATE  # a refused open opens nothing
        assert _rc(c, "kws_eval_open", 12, 16) == _native.KWS_OK
        assert update(None, t.data_ptr(), 4) == _native.KWS_EINVAL
        assert update(z.data_ptr(), None, 4) == _native.KWS_EINVAL
        assert update(z.data_ptr(), t.data_ptr(), 0) == _native.KWS_EINVAL
        assert update(z.data_ptr(), t.data_ptr(), -3) == _native.KWS_EINVAL
        assert read() == _native.KWS_OK and not counts.any()  # a refused update counts nothing
        assert update(z.data_ptr(), t.data_ptr(), 4) == _native.KWS_OK
        assert read() == _native.KWS_OK and list(counts) == [4, 4, 0, 0]
        # a second open zeroes the state (here with other sizes)
        assert _rc(c, "kws_eval_open", 12, 0) == _native.KWS_OK
        assert read() == _native.KWS_OK and not counts.any()
        assert update(z.data_ptr(), t.data_ptr(), 4) == _native.KWS_OK
        assert _rc(c, "kws_eval_close") == _native.KWS_OK
        assert read() == _native.KWS_ESTATE
        assert update(z.data_ptr(), t.data_ptr(), 4) == _native.KWS_ESTATE
        assert "kws_eval_open first" in c._lib.kws_last_error(c._h).decode()
    finally:
        c.close()


def test_evaluator_and_training_by_product(ctx):
    """Evaluator.update takes the loaders' int64 labels, returns the gradient of nn.CrossEntropyLoss() when asked, and its
    report equals the raw entries' statistics."""
    from kws.common.errors import ModelError
    from kws.libs.evaluation import Evaluator

    B, C, K = 257, 12, 256
    z, truth = ref.logits_for(31, B, C, 5.0)
    ev = Evaluator(C, n_bins=K, words=[f"w{i}" for i in range(C)])
    zd = to_dev(z).requires_grad_(True)
    t64 = to_dev(truth.astype(np.int64))
    g = ev.update(zd, t64, grad_scale=1.0 / B)
    assert ev.update(zd[:65], t64[:65]) is None
    F.cross_entropy(zd, t64).backward()
    p = torch.empty((B, C), device=DEV)
    ctx.softmax_f32(zd.detach(), p)
    rep = ev.report()
    p_h, g_h, auto = (v.cpu().numpy() for v in (p, g, zd.grad))
    both_z, both_t = np.concatenate([z, z[:65]]), np.concatenate([truth, truth[:65]])
    counts, confusion, pos, neg = ref.counts_from(np.concatenate([p_h, p_h[:65]]), both_z, both_t, K)
    assert (rep.n, rep.n_correct, rep.n_ignored, rep.n_nonfinite) == tuple(counts)
    assert np.array_equal(rep.confusion, confusion) and np.array_equal(rep.hist_pos, pos) and np.array_equal(rep.hist_neg, neg)
    assert np.abs(g_h - auto).max() <= 2e-6 / B  # two float32 softmaxes, each within the project's 1e-6 gate, scaled by 1 / B
    l64 = F.cross_entropy(torch.from_numpy(both_z.astype(np.float64)), torch.from_numpy(both_t.astype(np.int64))).item()
    assert abs(rep.loss - l64) <= 1e-5 and rep.words[3] == "w3" and "w11" in rep.format()
    assert 0.5 < rep.auc(rep.roc_micro()) <= 1.0
    ev.reset()
    assert ev.report().n == 0
    with pytest.raises(ModelError, match="expects logits"):
        ev.update(zd[:, :5], t64)
    with pytest.raises(ModelError, match="CUDA/ROCm"):
        ev.update(zd.detach().cpu(), t64)
    ev.close()


def test_evaluate_end_to_end_on_the_golden_clips(e2e_golden):
    """evaluate() over a resident split of the 48 golden clips in batches of 20 + 20 + 8: the confusion matrix is the one of the
    reference model's labels, the mean loss the float64 cross-entropy of its logits within 2e-4 (the logits are gated at 1e-4
    and cross-entropy moves by at most twice the largest logit error)."""
    from _scan_ref import state_from_blob
    from kws.libs.audio_processor import AudioProcessor
    from kws.libs.data_loader import DeviceBatchLoader
    from kws.libs.evaluation import evaluate
    from kws.libs.models import DepthwiseSeparableConv

    clips = np.ascontiguousarray(e2e_golden["clips"]).astype(np.int16)
    ref_logits, ref_label = e2e_golden["he.logits"][8:], e2e_golden["he.label"][8:].astype(np.int64)
    assert len(clips) == 48 == len(ref_logits)
    truth = (np.arange(48) * 5 + 1) % 12  # assigned: the clips are synthetic signals, any truth serves
    truth[::6] = ref_label[::6]           # some of them right
    model = DepthwiseSeparableConv(num_classes=12)
    model.load_state_dict(state_from_blob(e2e_golden["he.blob"]))
    model.to(DEV).train()
    loader = DeviceBatchLoader.from_arrays(clips, truth, AudioProcessor(None), batch_size=20, shuffle=False, augment=False)
    assert [len(y) for _, y in loader] == [20, 20, 8]
    rep = evaluate(model, loader)
    assert not model.training
    want = np.zeros((12, 12), np.int64)
    np.add.at(want, (truth, ref_label), 1)
    assert np.array_equal(rep.confusion, want)
    assert (rep.n, rep.n_ignored, rep.n_nonfinite, rep.n_bins) == (48, 0, 0, 256)
    assert rep.accuracy == 100.0 * (truth == ref_label).sum() / 48
    l64 = F.cross_entropy(torch.from_numpy(ref_logits.astype(np.float64)), torch.from_numpy(truth.astype(np.int64))).item()
    print(f"mean loss {rep.loss:.6f}, float64 cross-entropy of the reference logits {l64:.6f}")
    assert abs(rep.loss - l64) <= 2e-4
    assert rep.hist_pos.sum() == 48 and rep.hist_neg.sum() == 48 * 11
