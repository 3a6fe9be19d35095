"""What of "cnn-trad-fpool3 on recordings and streams" can be checked without a GPU: the chunk constant, the hook set the spotters
run a model through, and that the refusals come from the package (ModelError / the loud no-GPU error), never an AttributeError.
tests/test_abi_cpu.py requires every new header symbol to be exported, bound and signature-matched."""
import numpy as np
import pytest
import torch

from kws import _native
from kws.common.errors import KWSError, ModelError
from kws.inference import KeywordSpotter, StreamingSpotter
from kws.libs.models import CnnTradFpool3, DepthwiseSeparableConv, DepthwiseSeparableConvBN

HOOKS = ("_native_infer_i16", "_native_infer_f32", "_native_scan", "_native_scan_ragged", "_native_stream_load", "_native_stream_push")


def test_window_chunk_is_a_multiple_of_the_dense_group():
    n = _native.host_cnn_trad_window_chunk()
    assert n > 0 and n % 16 == 0 and n <= 4096


@pytest.mark.parametrize("cls", [DepthwiseSeparableConv, DepthwiseSeparableConvBN, CnnTradFpool3])
def test_every_model_has_the_spotter_hooks(cls):
    model = cls(12)
    for name in HOOKS + ("_context", "packed_weights"):
        assert callable(getattr(model, name)), f"{cls.__name__}.{name}"
    assert model._family in ("dscnn", "cnn_trad")
    blob = model.packed_weights()
    assert blob.dtype == np.float32 and blob.ndim == 1 and blob.size > 0


def test_bn_model_serves_its_fold():
    bn = DepthwiseSeparableConvBN(12)
    assert bn._family == DepthwiseSeparableConv._family
    assert np.array_equal(bn.packed_weights(), bn.fold().packed_weights())


def test_keyword_spotter_takes_cnn_trad_and_fails_loudly_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    spotter = KeywordSpotter(model=CnnTradFpool3(12))  # constructs without a device
    pcm = np.zeros(32000, np.int16)
    with pytest.raises(KWSError, match="no CPU fallback"):
        spotter.scan(pcm, hop_frames=10)
    with pytest.raises(KWSError, match="no CPU fallback"):
        spotter.infer_pcm16(np.zeros((2, 16000), np.int16))
    with pytest.raises(KWSError, match="no CPU fallback"):
        KeywordSpotter(model=DepthwiseSeparableConvBN(12)).scan(pcm)
    with pytest.raises(ModelError, match="13 words"):
        KeywordSpotter(model=CnnTradFpool3(12), words=[str(i) for i in range(13)])


def test_streaming_spotter_refuses_a_graph_for_cnn_trad_before_any_device_call():
    """use_graph=True with a model that has no captured push: ModelError whether or not a GPU is there (no context is made)."""
    with pytest.raises(ModelError, match="use_graph"):
        StreamingSpotter(1, model=CnnTradFpool3(12), use_graph=True)
    with pytest.raises(ModelError, match="captured-graph"):
        CnnTradFpool3(12)._native_stream_push(None, None, None, None, use_graph=True)


class _NoDevice:
    """Stands where a spotter's context would: any use is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError(f"load_model touched the context ({name}) before refusing the swap")


@pytest.mark.parametrize("have,new", [(DepthwiseSeparableConv, CnnTradFpool3), (CnnTradFpool3, DepthwiseSeparableConv),
                                      (CnnTradFpool3, DepthwiseSeparableConvBN)])
def test_streaming_spotter_swaps_models_within_one_family_only(have, new):
    spotter = object.__new__(StreamingSpotter)  # load_model's refusal needs neither streams nor a device
    spotter.model, spotter._ctx = have(12), _NoDevice()
    with pytest.raises(ModelError, match="another model family"):
        spotter.load_model(new(12))
    with pytest.raises(ModelError, match="classes"):
        spotter.load_model(have(5))
