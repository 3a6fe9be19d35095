"""CPU tests of the DS-CNN device-side weight load: the C ABI declares, binds and exports kws_load_dscnn_device and
kws_dscnn_image_read with exactly these prototypes, the Python context has their methods, the profiling tables name the load's
kernels, and DepthwiseSeparableConv selects the device route by default."""
import os
import re

import pytest

from conftest import REPO

PROTOS = {
    "kws_load_dscnn_device":
        "int kws_load_dscnn_device(kws_ctx* ctx, const float* d_blob, size_t n_floats, int num_classes, int input_channels);",
    "kws_dscnn_image_read":
        "int kws_dscnn_image_read(kws_ctx* ctx, uint32_t* out_words, size_t cap_words, size_t* need_words, float* scalars);",
}


def test_header_declares_the_two_entries():
    text = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "kws_hip.h")).read())
    for name, proto in PROTOS.items():
        assert proto in text, name
    assert "#define KWS_ABI_VERSION 1" in text


def test_entries_are_bound_and_exported():
    native = pytest.importorskip("kws._native")
    C = native.C
    assert native.SIGNATURES["kws_load_dscnn_device"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int])
    assert native.SIGNATURES["kws_dscnn_image_read"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t),
                                                                   C.POINTER(C.c_float)])
    for meth in ("load_dscnn_device", "dscnn_image"):
        assert hasattr(native.Context, meth), meth
    if os.path.exists(native.LIB_PATH):
        lib = native.lib()
        for name in PROTOS:
            assert hasattr(lib, name), name


def test_the_load_kernels_have_profiling_ids_and_names():
    native = pytest.importorskip("kws._native")
    text = open(os.path.join(REPO, "include", "kws_hip.h")).read()
    ids = {"KWS_K_DSCNN_LOAD_STATS": "kws_ds_load_stats_kernel", "KWS_K_DSCNN_LOAD_PACK": "kws_ds_load_pack_kernel",
           "KWS_K_DSCNN_LOAD_FILL": "kws_ds_load_fill_kernel"}
    for const, kernel in ids.items():
        m = re.search(rf"\b{const} = (\d+)", text)
        assert m and int(m.group(1)) == getattr(native, const), const
        if os.path.exists(native.LIB_PATH):
            assert native.kernel_name(getattr(native, const)) == kernel
    assert len({getattr(native, c) for c in ids}) == 3


def test_the_model_refreshes_on_the_device_by_default():
    from kws.libs.models import DepthwiseSeparableConv

    assert DepthwiseSeparableConv._device_refresh is True
    m = DepthwiseSeparableConv(3)
    m._device_refresh = False  # an instance can ask for the host route
    assert DepthwiseSeparableConv._device_refresh is True and not m._device_refresh
    assert m.packed_weights().shape == (25664 + 65 * 3,)
