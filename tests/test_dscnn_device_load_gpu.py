"""kws_load_dscnn_device on the GPU: the image it builds from a device-resident blob equals the host image word for word and
scalar for scalar (read back with kws_dscnn_image_read), in place and after a reallocation; forwards after either load are
bit-identical; the argument checks are the host load's; DepthwiseSeparableConv trains identically through either refresh route;
a captured streaming push is retired by the device load as by the host load.  Every comparison is exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CASES = [(1, 1), (2, 1), (3, 1), (4, 1), (12, 1), (64, 1), (12, 2), (5, 64)]  # (num_classes, input_channels)


def _planted_blob(C, C_in, seed=7):
    """Finite, seeded N(0, 0.1), with a subnormal, a weight that sets its layer's scale, an all-zero layer (scale 1) and conv1's
    largest row sum in the last row."""
    from oracle import dscnn as o_dscnn

    st = {k: v.clone() for k, v in o_dscnn.random_state(seed + 100 * C + C_in, 0.1, C, C_in).items()}
    st["dsconv2.pointwise.weight"][3, 5, 0, 0] = 5e-41
    st["dsconv3.pointwise.weight"][1, 2, 0, 0] = -70000.0
    st["dsconv4.pointwise.weight"].zero_()
    st["conv1.weight"][63] *= 3.0
    rows = st["conv1.weight"].abs().double().reshape(64, -1).sum(1)
    assert int(rows.argmax()) == 63
    blob = o_dscnn.flatten_state(st)
    assert np.isfinite(blob).all() and blob.size == 6400 * C_in + 19264 + 65 * C
    return blob


def _plain_blob(C, C_in, seed=3):
    from oracle import dscnn as o_dscnn

    return o_dscnn.flatten_state(o_dscnn.random_state(seed, 0.1, C, C_in))


def _assert_image(ctx, blob, C, C_in):
    from kws import _native

    words, scalars = ctx.dscnn_image()
    want_w, want_s = _native.host_dscnn_image(blob, C, C_in)
    assert words.dtype == np.uint32 and words.shape == want_w.shape
    bad = np.flatnonzero(words != want_w)
    assert bad.size == 0, (C, C_in, bad[:8], words[bad[:8]], want_w[bad[:8]])
    assert np.array_equal(scalars.view(np.uint32), want_s.view(np.uint32)), (scalars, want_s)


@pytest.mark.parametrize("C,C_in", CASES)
def test_device_image_equals_the_host_image(C, C_in):
    from kws import _native

    blob = _planted_blob(C, C_in)
    a, b = _native.Context(0), _native.Context(0)
    try:
        a.load_dscnn_device(torch.from_numpy(blob).to(DEV), C, C_in)
        _assert_image(a, blob, C, C_in)
        _, s = a.dscnn_image()
        assert s[4] == 0.0  # k_pw of the all-zero layer: scale 1
        assert s[3] < 0  # the layer with |w| = 70000 is scaled DOWN into f16's range
        b.load_dscnn(blob, C, C_in)  # a host load reads back as the same words
        _assert_image(b, blob, C, C_in)
    finally:
        a.close()
        b.close()


def test_refresh_in_place_and_after_a_reallocation():
    from kws import _native

    c = _native.Context(0)
    try:
        for C, C_in, seed in ((12, 1, 1), (12, 1, 2), (7, 1, 3), (7, 2, 4), (12, 1, 5)):  # same size, then three other sizes
            blob = _planted_blob(C, C_in, seed)
            c.load_dscnn_device(torch.from_numpy(blob).to(DEV), C, C_in)
            _assert_image(c, blob, C, C_in)
        blob = _plain_blob(12, 1)
        c.load_dscnn(blob, 12)  # host load over a device-built image, then the device load in place over the host's
        _assert_image(c, blob, 12, 1)
        blob = _planted_blob(12, 1, 9)
        c.load_dscnn_device(torch.from_numpy(blob).to(DEV), 12, 1)
        _assert_image(c, blob, 12, 1)
    finally:
        c.close()


@pytest.mark.parametrize("C_in,T,F", [(1, 99, 10), (1, 20, 7), (2, 99, 10)])
def test_forward_is_bit_identical_after_either_load(C_in, T, F):
    from kws import _native

    C, B = 12, 64
    blob = _plain_blob(C, C_in)
    a, b = _native.Context(0), _native.Context(0)
    try:
        a.load_dscnn(blob, C, C_in)
        b.load_dscnn_device(torch.from_numpy(blob).to(DEV), C, C_in)
        x = torch.randn(B, C_in, T, F, generator=torch.Generator().manual_seed(11)).to(DEV)
        for math in (_native.PW_PAIR_F16, _native.PW_SPLIT_BF16):
            out = []
            for c in (a, b):
                c.set_pointwise_math(math)
                lg = torch.empty(B, C, device=DEV)
                lb = torch.empty(B, dtype=torch.int32, device=DEV)
                if (T, F) == (99, 10):
                    c.forward_f32(x, lg, lb)
                else:
                    c.forward_map_f32(x, lg, lb)
                c.sync()
                out.append((lg.cpu(), lb.cpu()))
            assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), math
            assert float(out[0][0].std(0).min()) > 0  # the logits depend on the input
    finally:
        a.close()
        b.close()


def test_errors():
    from kws import _native
    from kws.common.errors import ModelError

    c = _native.Context(0)
    lib, h, Cc = c._lib, c._h, _native.C
    try:
        need = Cc.c_size_t(77)
        assert lib.kws_dscnn_image_read(h, None, 0, Cc.byref(need), None) == _native.KWS_ESTATE  # no model yet
        assert need.value == 0
        with pytest.raises(ModelError):
            c.dscnn_image()
        blob = torch.from_numpy(_plain_blob(12, 1)).to(DEV)
        big = torch.zeros(6400 * 65 + 19264 + 65 * 65, device=DEV)
        assert lib.kws_load_dscnn_device(h, None, blob.numel(), 12, 1) == _native.KWS_EINVAL
        assert lib.kws_load_dscnn_device(h, blob.data_ptr(), blob.numel() - 1, 12, 1) == _native.KWS_EINVAL
        assert lib.kws_dscnn_image_read(h, None, 0, None, None) == _native.KWS_ESTATE  # a refused load leaves no model
        for C, C_in in ((0, 1), (65, 1), (12, 0), (12, 65)):  # like the host load
            n = 6400 * max(C_in, 0) + 19264 + 65 * max(C, 0)
            rc_dev = lib.kws_load_dscnn_device(h, big.data_ptr(), n, C, C_in)
            host = np.zeros(n, np.float32)
            rc_host = lib.kws_load_dscnn_ex(h, host.ctypes.data_as(Cc.POINTER(Cc.c_float)), host.size, C, C_in)
            assert rc_dev == rc_host != 0, (C, C_in)
        with pytest.raises(ModelError):
            c.load_dscnn_device(blob[:-1], 12)
        c.load_dscnn_device(blob, 12)
        assert lib.kws_dscnn_image_read(h, None, 0, Cc.byref(need), None) == _native.KWS_OK
        total = need.value
        assert total == _native.host_dscnn_image(blob.cpu().numpy(), 12)[0].size
        small = np.zeros(total - 1, np.uint32)
        need = Cc.c_size_t(0)
        assert lib.kws_dscnn_image_read(h, small.ctypes.data_as(Cc.POINTER(Cc.c_uint32)), small.size, Cc.byref(need),
                                        None) == _native.KWS_EINVAL
        assert need.value == total and not small.any()
    finally:
        c.close()


def test_training_is_identical_through_either_refresh_route():
    from kws import _native
    from kws.libs.models import DepthwiseSeparableConv

    models = []
    for device_route in (True, False):
        torch.manual_seed(5)
        m = DepthwiseSeparableConv(12).to(DEV).train()
        if not device_route:
            m._device_refresh = False
        models.append(m)
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(8, 1, 99, 10, generator=gen).to(DEV)
    y = torch.randint(0, 12, (8,), generator=gen).to(DEV)
    crit = torch.nn.CrossEntropyLoss()
    opts = [torch.optim.Adam(m.parameters(), lr=1e-3) for m in models]
    for m in models:  # count the device load's launches (one fill kernel per refresh)
        m._context(0).prof_enable(True)
    for step in range(3):
        logits = []
        for m, opt in zip(models, opts):
            opt.zero_grad()
            lg = m(x)
            crit(lg, y).backward()
            opt.step()
            logits.append(lg.detach().cpu())
        assert torch.equal(logits[0], logits[1]), step
    for p, q in zip(models[0].parameters(), models[1].parameters()):
        assert torch.equal(p.detach().cpu(), q.detach().cpu())
    dev_m, host_m = models
    for m in models:  # the refresh after the last optimizer step
        words, scalars = m._context(0).dscnn_image()
        want_w, want_s = _native.host_dscnn_image(m.packed_weights(), 12)
        assert np.array_equal(words, want_w) and np.array_equal(scalars.view(np.uint32), want_s.view(np.uint32))
    assert dev_m._ctx.prof_read(_native.KWS_K_DSCNN_LOAD_FILL)[1] == 3  # steps 2 and 3 and the last refresh (the first load preceded prof_enable)
    assert host_m._ctx.prof_read(_native.KWS_K_DSCNN_LOAD_FILL)[1] == 0

    # parameters on the CPU: inference on GPU input still works, through the host route
    torch.manual_seed(5)
    cpu_m = DepthwiseSeparableConv(12)
    torch.manual_seed(5)
    gpu_m = DepthwiseSeparableConv(12).to(DEV)
    a, b = cpu_m(x), gpu_m(x)
    assert a.is_cuda and torch.equal(a.cpu(), b.cpu())
    cpu_m._ctx.prof_enable(True)
    with torch.no_grad():
        cpu_m.fc.bias.add_(1.0)
    assert not torch.equal(cpu_m(x).cpu(), b.cpu())  # re-uploaded through the host: the logits moved
    assert cpu_m._ctx.prof_read(_native.KWS_K_DSCNN_LOAD_FILL)[1] == 0


def test_a_captured_push_is_retired_by_the_device_load():
    """A captured push holds weight pointers and scalars by value: after kws_load_dscnn_device the next push must use the new
    weights, bit for bit as after the same reload through the host."""
    from kws import _native
    from oracle import dscnn as o_dscnn

    S = 2
    st = {k: v.clone() for k, v in o_dscnn.random_state(21, 0.1, 12).items()}
    first = o_dscnn.flatten_state(st)
    st["fc.weight"] = torch.flip(st["fc.weight"], dims=[0])  # a visibly different classifier
    st["fc.bias"] = torch.flip(st["fc.bias"], dims=[0])
    st["dsconv2.pointwise.weight"] = st["dsconv2.pointwise.weight"] * 0.5  # another pointwise scale exponent
    second = o_dscnn.flatten_state(st)
    pcm = np.random.default_rng(41).integers(-20000, 20000, size=(7, S, 160), dtype=np.int16)
    ctxs = {k: _native.Context(0) for k in ("device", "host", "never")}
    try:
        out = {}
        for k, c in ctxs.items():
            c.load_dscnn(first, 12)
            c.stream_open(S)
            hop = torch.empty((S, 160), dtype=torch.int16, device=DEV)
            lg = torch.empty((S, 12), dtype=torch.float32, device=DEV)
            lb = torch.empty((S,), dtype=torch.int32, device=DEV)
            seq = []
            for t in range(7):
                if t == 6 and k == "device":
                    c.load_dscnn_device(torch.from_numpy(second).to(DEV), 12)
                if t == 6 and k == "host":
                    c.load_dscnn(second, 12)
                hop.copy_(torch.from_numpy(pcm[t]))
                torch.cuda.synchronize()
                c.stream_push_i16(hop, lg, lb, use_graph=True)
                c.sync()
                seq.append((lg.cpu().clone(), lb.cpu().clone()))
            out[k] = seq
        for t in range(7):
            assert torch.equal(out["device"][t][0], out["host"][t][0]) and torch.equal(out["device"][t][1], out["host"][t][1]), t
        for t in range(6):
            assert torch.equal(out["device"][t][0], out["never"][t][0]), t
        assert float((out["device"][6][0] - out["never"][6][0]).abs().max()) > 1e-3  # the old weights would give these
    finally:
        for c in ctxs.values():
            c.close()
