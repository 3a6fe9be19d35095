"""ctypes binding of libkws_hip.so (C ABI: include/kws_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` /
``make -C keyword-spotting_amd/csrc``; if it is missing, importing this module still works (so the
host-only classes are usable) but the first compute call raises ``KWSError`` -- loudly, never a
silent fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

from kws.common.errors import AudioProcessingError, KWSError, ModelError

# KWS_HIP_LIB selects another build of the same ABI (A/B timing of kernel variants); default is the in-tree library
LIB_PATH = os.environ.get("KWS_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libkws_hip.so")

KWS_OK, KWS_EINVAL, KWS_ENOMEM, KWS_EHIP, KWS_ESTATE, KWS_EUNSUPPORTED = 0, -1, -2, -3, -4, -5
KWS_CT_F16_PAIR, KWS_CT_BF16_TRIPLE = 0, 1  # kws_set_cnn_trad_math
KWS_K_MFCC, KWS_K_DSCNN, KWS_K_CNNTRAD_CONV, KWS_K_CNNTRAD_DENSE, KWS_K_STREAM_FRAME, KWS_K_MFCC_F64, KWS_K_MFCC_REFINE = 0, 1, 2, 3, 4, 5, 6
KWS_K_DSCNN_LOAD_STATS, KWS_K_DSCNN_LOAD_PACK, KWS_K_DSCNN_LOAD_FILL = 7, 8, 9  # the launches of kws_load_dscnn_device
KWS_K_RESAMPLE = 10  # kws_resample_i16 / kws_resample_f32
FE_REFINE_SPAN_DEFAULT = 10.2  # KWS_FE_REFINE_SPAN_DEFAULT: log(largest bin power / weakest mel band) beyond which a frame is redone in float64
FE_ROUTE_AUTO, FE_ROUTE_GENERIC = 0, 1  # KWS_FE_ROUTE_*: the kernel compiled for the reference geometry / the generic one (diagnostics)
FE_F32, FE_F64 = 0, 1  # KWS_FE_F32 (default: the fast float32 front end) / KWS_FE_F64 (float64 after framing, as psf)
ACT_FLOATS_PER_CLIP = 64 * (141 + 141 + 245 + 357) + 64 + 64 * 477  # KWS_ACT_FLOATS_PER_CLIP
PW_F32 = 1          # KWS_PW_F32: pointwise convolutions on v_mfma_f32_32x32x2_f32
PW_SPLIT_BF16 = 4   # KWS_PW_SPLIT_BF16: exact three-way bf16 split, six bf16 MFMAs per f32 product
PW_PAIR_F16 = 5     # KWS_PW_PAIR_F16 (default): f16 pairs with per-clip power-of-two scales, three f16 MFMAs per f32 product
PW_DEFAULT = PW_PAIR_F16

_c_ctx = C.c_void_p
_i16p, _f32p, _i32p = C.c_void_p, C.c_void_p, C.c_void_p  # device pointers travel as integers
_h_i32p, _h_i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)  # host tables of the ragged entries

# name -> (restype, argtypes): every symbol include/kws_hip.h declares
SIGNATURES = {
    "kws_abi_version": (C.c_int, []),
    "kws_create": (C.c_int, [C.POINTER(_c_ctx), C.c_int]),
    "kws_destroy": (None, [_c_ctx]),
    "kws_set_stream": (C.c_int, [_c_ctx, C.c_void_p, C.c_int]),
    "kws_sync": (C.c_int, [_c_ctx]),
    "kws_last_error": (C.c_char_p, [_c_ctx]),
    "kws_set_frontend": (C.c_int, [_c_ctx] + [C.c_int] * 7 + [C.c_float, C.c_int]),
    "kws_set_frontend_math": (C.c_int, [_c_ctx, C.c_int]),
    "kws_frontend_math": (C.c_int, [_c_ctx]),
    "kws_set_frontend_route": (C.c_int, [_c_ctx, C.c_int]),
    "kws_set_frontend_refine": (C.c_int, [_c_ctx, C.c_float]),
    "kws_frontend_stats": (C.c_int, [_c_ctx, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "kws_spec_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, _f32p]),
    "kws_frontend_shape": (C.c_int, [_c_ctx, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "kws_mfcc_i16": (C.c_int, [_c_ctx, _i16p, C.c_int, _f32p]),
    "kws_mfcc_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, _f32p]),
    "kws_load_dscnn": (C.c_int, [_c_ctx, C.POINTER(C.c_float), C.c_size_t, C.c_int]),
    "kws_load_dscnn_ex": (C.c_int, [_c_ctx, C.POINTER(C.c_float), C.c_size_t, C.c_int, C.c_int]),
    "kws_load_dscnn_device": (C.c_int, [_c_ctx, _f32p, C.c_size_t, C.c_int, C.c_int]),
    "kws_dscnn_image_read": (C.c_int, [_c_ctx, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_float)]),
    "kws_forward_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, _f32p, _i32p]),
    "kws_forward_map_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, C.c_int, C.c_int, _f32p, _i32p]),
    "kws_forward_map_debug_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, C.c_int, C.c_int, _f32p, _i32p, _f32p]),
    "kws_infer_i16": (C.c_int, [_c_ctx, _i16p, C.c_int, _f32p, _i32p]),
    "kws_dscnn_backward_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, C.c_int, C.c_int, _f32p, _f32p]),
    "kws_dscnn_bn_train_forward_f32": (C.c_int, [_c_ctx, _f32p, C.c_size_t, C.c_int, _f32p, C.c_int, C.c_int, C.c_int, C.c_float, _f32p, _i32p,
                                                 _f32p]),
    "kws_dscnn_bn_backward_f32": (C.c_int, [_c_ctx, _f32p, C.c_size_t, C.c_int, _f32p, C.c_int, C.c_int, C.c_int, C.c_float, _f32p, _f32p]),
    "kws_dscnn_bn_train_debug_f32": (C.c_int, [_c_ctx, _f32p, C.c_size_t, C.c_int, _f32p, C.c_int, C.c_int, C.c_int, C.c_float, _f32p, _i32p,
                                               _f32p, _f32p]),
    "kws_host_dscnn_bn_max_batch": (C.c_int, [C.c_int, C.c_int]),
    "kws_dsblock_forward_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, _f32p, _f32p, _f32p, _f32p, C.c_int, C.c_int,
                                          C.c_int, C.c_int, _f32p]),
    "kws_infer_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, _f32p, _i32p]),
    "kws_infer_host_i16": (C.c_int, [_c_ctx, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "kws_infer_host_submit_i16": (C.c_int, [_c_ctx, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "kws_infer_host_wait": (C.c_int, [_c_ctx, C.c_uint64]),
    "kws_ingest_config": (C.c_int, [_c_ctx, C.c_int, C.c_int, C.c_int]),
    "kws_reserve": (C.c_int, [_c_ctx, C.c_int]),
    "kws_set_pointwise_math": (C.c_int, [_c_ctx, C.c_int]),
    "kws_forward_debug_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, _f32p, _i32p, _f32p, C.c_int]),
    "kws_stream_open": (C.c_int, [_c_ctx, C.c_int]),
    "kws_stream_close": (C.c_int, [_c_ctx]),
    "kws_stream_reset": (C.c_int, [_c_ctx, C.c_void_p, C.c_int]),
    "kws_stream_deactivate": (C.c_int, [_c_ctx, C.c_void_p, C.c_int]),
    "kws_stream_activate": (C.c_int, [_c_ctx, C.c_void_p, C.c_int]),
    "kws_stream_active": (C.c_int, [_c_ctx, C.c_void_p, C.POINTER(C.c_int)]),
    "kws_stream_cluster": (C.c_int, [_c_ctx, C.c_int]),
    "kws_stream_host_results": (C.c_int, [_c_ctx, C.c_int]),
    "kws_stream_wait_host": (C.c_int, [_c_ctx, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "kws_stream_push_host_i16": (C.c_int, [_c_ctx, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "kws_stream_push_i16": (C.c_int, [_c_ctx, _i16p, _f32p, _i32p, C.c_int]),
    "kws_stream_state": (C.c_int, [_c_ctx, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "kws_stream_copy_features": (C.c_int, [_c_ctx, _f32p]),
    "kws_load_cnn_trad": (C.c_int, [_c_ctx, C.POINTER(C.c_float), C.c_size_t, C.c_int]),
    "kws_load_cnn_trad_device": (C.c_int, [_c_ctx, _f32p, C.c_size_t, C.c_int]),
    "kws_cnn_trad_backward_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, _f32p, _f32p]),
    "kws_cnn_trad_train_debug_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, _f32p, _i32p, _f32p, _f32p]),
    "kws_stream_vad_f32": (C.c_int, [_c_ctx, C.c_float, C.c_int, C.c_int, _i32p]),
    "kws_forward_cnn_trad_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, _f32p, _i32p]),
    "kws_forward_cnn_trad_debug_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, _f32p, _i32p, _f32p, _f32p]),
    "kws_set_cnn_trad_math": (C.c_int, [_c_ctx, C.c_int]),
    "kws_infer_cnn_trad_i16": (C.c_int, [_c_ctx, _i16p, C.c_int, _f32p, _i32p]),
    "kws_infer_cnn_trad_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, _f32p, _i32p]),
    "kws_host_cnn_trad_window_chunk": (C.c_int, []),
    "kws_forward_cnn_trad_windows_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, C.c_int, C.c_int, _f32p, _i32p]),
    "kws_scan_cnn_trad_i16": (C.c_int, [_c_ctx, _i16p, C.c_int, C.c_int, C.c_int, _f32p, _i32p, _f32p]),
    "kws_scan_cnn_trad_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, C.c_int, C.c_int, _f32p, _i32p, _f32p]),
    "kws_scan_ragged_cnn_trad_i16": (C.c_int, [_c_ctx, _i16p, C.c_int, _h_i64p, _h_i32p, C.c_int, C.c_int, _f32p, _i32p, _f32p]),
    "kws_scan_ragged_cnn_trad_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, _h_i64p, _h_i32p, C.c_int, C.c_int, _f32p, _i32p, _f32p]),
    "kws_stream_push_cnn_trad_i16": (C.c_int, [_c_ctx, _i16p, _f32p, _i32p]),
    "kws_softmax_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, C.c_int, _f32p]),
    "kws_stream_smooth_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, C.c_int, _f32p, _i32p]),
    "kws_scan_i16": (C.c_int, [_c_ctx, _i16p, C.c_int, C.c_int, C.c_int, _f32p, _i32p, _f32p]),
    "kws_scan_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, C.c_int, C.c_int, _f32p, _i32p, _f32p]),
    "kws_scan_detect_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _f32p, _i32p, _i32p,
                                      _f32p, C.c_int, _i32p]),
    "kws_frames_i16": (C.c_int, [_c_ctx, _i16p, C.c_int, C.c_int, _f32p]),
    "kws_frames_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, C.c_int, _f32p]),
    "kws_segment_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, C.c_int,
                                  _i32p]),
    "kws_cut_i16": (C.c_int, [_c_ctx, _i16p, C.c_int, C.c_int, _i32p, C.c_int, C.c_int, _i16p, C.c_int, _i32p]),
    "kws_cut_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, C.c_int, _i32p, C.c_int, C.c_float, _f32p, C.c_int, _f32p]),
    "kws_frames_ragged_i16": (C.c_int, [_c_ctx, _i16p, C.c_int, _h_i64p, _h_i32p, C.c_int, C.c_int, _f32p]),
    "kws_scan_ragged_i16": (C.c_int, [_c_ctx, _i16p, C.c_int, _h_i64p, _h_i32p, C.c_int, C.c_int, _f32p, _i32p, _f32p]),
    "kws_frames_ragged_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, _h_i64p, _h_i32p, C.c_int, C.c_int, _f32p]),
    "kws_scan_ragged_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, _h_i64p, _h_i32p, C.c_int, C.c_int, _f32p, _i32p, _f32p]),
    "kws_scan_detect_ragged_f32": (C.c_int, [_c_ctx, _f32p, _h_i32p, _h_i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _f32p,
                                             _i32p, _i32p, _f32p, C.c_int, _i32p]),
    "kws_host_score_plan": (C.c_int, [_h_i32p, C.c_int, C.c_int, C.c_int, C.c_int, _h_i32p, _h_i32p]),
    "kws_scan_score_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int,
                                     _h_i32p, C.c_int, C.c_void_p]),
    "kws_scan_score_ragged_f32": (C.c_int, [_c_ctx, _f32p, _h_i32p, _h_i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.POINTER(C.c_float), C.c_int, _h_i32p, C.c_int, C.c_void_p]),
    "kws_segment_ragged_f32": (C.c_int, [_c_ctx, _f32p, _h_i32p, _h_i32p, _h_i32p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int,
                                         _i32p, C.c_int, _i32p]),
    "kws_host_stream_utt_history": (C.c_int, [C.c_int] * 5 + [C.POINTER(C.c_int)]),
    "kws_stream_utt_open": (C.c_int, [_c_ctx, C.c_float] + [C.c_int] * 6),
    "kws_stream_utt_close": (C.c_int, [_c_ctx]),
    "kws_stream_utt_step_i16": (C.c_int, [_c_ctx, _i16p, _f32p]),
    "kws_stream_utt_flush": (C.c_int, [_c_ctx]),
    "kws_stream_utt_poll": (C.c_int, [_c_ctx, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kws_stream_utt_read": (C.c_int, [_c_ctx, C.c_uint64, C.c_int, C.POINTER(C.c_int64)]),
    "kws_stream_utt_cut_i16": (C.c_int, [_c_ctx, C.c_uint64, C.c_int, C.c_int, _i16p, C.c_int, _i32p]),
    "kws_stream_detect_open": (C.c_int, [_c_ctx, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int]),
    "kws_stream_detect_close": (C.c_int, [_c_ctx]),
    "kws_stream_detect_step_f32": (C.c_int, [_c_ctx, _f32p]),
    "kws_stream_detect_poll": (C.c_int, [_c_ctx, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kws_stream_detect_read": (C.c_int, [_c_ctx, C.c_uint64, C.c_int, C.POINTER(C.c_int64)]),
    "kws_stream_detect_smoothed": (C.c_int, [_c_ctx, _f32p, _i32p]),
    "kws_resample_i16": (C.c_int, [_c_ctx, _i16p, C.c_int, C.c_int, _i32p, C.c_int, C.c_int, _i16p, C.c_int]),
    "kws_resample_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, C.c_int, _i32p, C.c_int, C.c_int, _f32p, C.c_int]),
    "kws_host_stream_resample_plan": (C.c_int, [C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 4),
    "kws_host_stream_resample_count": (C.c_int, [C.c_int, C.c_int, C.c_uint64, C.c_int, C.POINTER(C.c_int)]),
    "kws_stream_resample_open": (C.c_int, [_c_ctx, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64]),
    "kws_stream_resample_close": (C.c_int, [_c_ctx]),
    "kws_stream_resample_i16": (C.c_int, [_c_ctx, _i16p, C.c_int, _i16p, C.c_int, C.POINTER(C.c_int)]),
    "kws_stream_push_rate_i16": (C.c_int, [_c_ctx, _i16p, C.c_int, _f32p, _i32p]),
    "kws_stream_push_host_rate_i16": (C.c_int, [_c_ctx, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "kws_eval_open": (C.c_int, [_c_ctx, C.c_int, C.c_int]),
    "kws_eval_reset": (C.c_int, [_c_ctx]),
    "kws_eval_close": (C.c_int, [_c_ctx]),
    "kws_eval_update_f32": (C.c_int, [_c_ctx, _f32p, _i32p, C.c_int, C.c_float, _f32p, _f32p]),
    "kws_eval_read": (C.c_int, [_c_ctx, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                C.POINTER(C.c_uint64)]),
    "kws_augment_i16": (C.c_int, [_c_ctx, _i16p, C.c_int, C.c_void_p, _f32p, C.c_int, C.c_void_p, _f32p, C.c_void_p, _f32p]),
    "kws_augment_draw": (C.c_int, [_c_ctx, C.c_uint64, C.c_uint32, _i32p, C.c_int, _i32p, C.c_int, C.c_int, _i32p, _i32p, C.c_int, C.c_float,
                                   C.c_float, C.c_int, C.c_int, _i32p, _i32p, _f32p, C.c_void_p]),
    "kws_mfcc_augment_i16": (C.c_int, [_c_ctx, _i16p, C.c_int, _i32p, C.c_int, C.c_void_p, _f32p, C.c_int, C.c_void_p, _f32p, C.c_void_p,
                                       _f32p]),
    "kws_forward_stamps_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, _f32p, C.c_void_p, C.c_int]),
    "kws_preemphasis_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, C.c_float, _f32p]),
    "kws_framesig_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, C.c_int, C.c_int, _f32p, _f32p]),
    "kws_spec512_f32": (C.c_int, [_c_ctx, _f32p, C.c_int, C.c_int, C.c_int, _f32p]),
    "kws_prof_enable": (C.c_int, [_c_ctx, C.c_int]),
    "kws_prof_reset": (C.c_int, [_c_ctx]),
    "kws_prof_read": (C.c_int, [_c_ctx, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "kws_kernel_name": (C.c_char_p, [C.c_int]),
    "kws_host_mel_edges": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "kws_host_mel_dense": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "kws_host_mel_layout": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                      C.POINTER(C.c_int)]),
    "kws_host_dct_lifter": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "kws_host_dscnn_image": (C.c_int, [C.POINTER(C.c_float), C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_size_t,
                                       C.POINTER(C.c_size_t), C.POINTER(C.c_float)]),
    "kws_host_cnn_trad_image": (C.c_int, [C.POINTER(C.c_float), C.c_size_t, C.c_int, C.POINTER(C.c_uint32), C.c_size_t,
                                          C.POINTER(C.c_size_t), C.POINTER(C.c_float)]),
    "kws_host_dscnn_units": (C.c_int, [C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "kws_host_scan_shape": (C.c_int, [C.c_int] * 5 + [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "kws_host_ragged_plan": (C.c_int, [_h_i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _h_i32p, _h_i32p, _h_i32p, _h_i32p,
                                       C.POINTER(C.c_int)]),
    "kws_host_resample_len": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "kws_host_resample_design": (C.c_int, [C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 4 + [C.POINTER(C.c_double), C.c_size_t,
                                           C.POINTER(C.c_size_t)]),
}

_lib = None
_lock = threading.Lock()


def lib() -> C.CDLL:
    """Load libkws_hip.so once; raise KWSError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise KWSError(
                    f"native library missing: {LIB_PATH} (build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    "or `make -C keyword-spotting_amd/csrc`); there is no CPU fallback"
                )
            try:
                h = C.CDLL(LIB_PATH)
            except OSError as e:  # pragma: no cover - depends on the host
                raise KWSError(f"cannot load {LIB_PATH}: {e}") from e
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(h, name)
                fn.restype = res
                fn.argtypes = args
            _lib = h
    return _lib


def _ptr(t) -> int:
    return int(t.data_ptr())


def _opt(t):
    """An optional device tensor -> its address or NULL."""
    return _ptr(t) if t is not None else None


class Context:
    """One kws_ctx: a GPU, its stream, front-end tables, model weights, workspace."""

    def __init__(self, device: int = 0, error_cls=KWSError):
        self._h = _c_ctx()
        self._lib = lib()
        rc = self._lib.kws_create(C.byref(self._h), int(device))
        if rc != KWS_OK:
            msg = self._lib.kws_last_error(None).decode()
            self._h = _c_ctx()
            raise error_cls(f"kws_create failed ({rc}): {msg}")
        self.device = int(device)
        self.num_classes = None
        # {ticket: (logits, label, source)} of the host batches in flight: the library holds raw pointers to them until
        # infer_host_wait retires the ticket, whatever the caller does with the tuple infer_host_submit_i16 returned
        self._host_inflight = {}

    # -- plumbing -------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.kws_destroy(self._h)
            self._h = _c_ctx()
            self._host_inflight.clear()

    def __del__(self):  # best effort
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, error_cls=KWSError):
        if rc != KWS_OK:
            raise error_cls(f"{self._lib.kws_last_error(self._h).decode()} (code {rc})")

    def use_torch_stream(self):
        """Enqueue on torch's current stream for this device, so torch sees the work in order."""
        import torch

        self._check(self._lib.kws_set_stream(self._h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), 1))

    def use_own_stream(self):
        self._check(self._lib.kws_set_stream(self._h, None, 0))

    def sync(self):
        self._check(self._lib.kws_sync(self._h))

    # -- front end ------------------------------------------------------------------------------
    def set_frontend(self, sample_rate=16000, n_samples=16000, frame_len=400, frame_step=160, nfft=512, nfilt=26,
                     numcep=10, preemph=0.97, ceplifter=22):
        self._check(
            self._lib.kws_set_frontend(self._h, sample_rate, n_samples, frame_len, frame_step, nfft, nfilt, numcep,
                                       float(preemph), ceplifter),
            AudioProcessingError,
        )

    def set_frontend_math(self, math: int):
        self._check(self._lib.kws_set_frontend_math(self._h, int(math)), AudioProcessingError)

    def set_frontend_route(self, route: int = FE_ROUTE_AUTO):
        """Diagnostics: FE_ROUTE_GENERIC keeps reference-geometry int16 calls on the generic wavefront-resident kernel (same bits)."""
        self._check(self._lib.kws_set_frontend_route(self._h, int(route)), AudioProcessingError)

    def frontend_math(self) -> int:
        """FE_F32 or FE_F64: the arithmetic kws_mfcc_* actually uses for the configured geometry."""
        return int(self._lib.kws_frontend_math(self._h))

    def set_frontend_refine(self, log_span: float = FE_REFINE_SPAN_DEFAULT):
        """Frames whose log-mel values span more than ``log_span`` are recomputed in float64 (0 switches it off)."""
        self._check(self._lib.kws_set_frontend_refine(self._h, float(log_span)), AudioProcessingError)

    def frontend_stats(self):
        """(frames through the float32 front end, frames recomputed in float64, frames the last batched call listed)."""
        total, refined, last = C.c_uint64(), C.c_uint64(), C.c_int()
        self._check(self._lib.kws_frontend_stats(self._h, C.byref(total), C.byref(refined), C.byref(last)), AudioProcessingError)
        return int(total.value), int(refined.value), int(last.value)

    def frontend_shape(self):
        nf, nc = C.c_int(), C.c_int()
        self._check(self._lib.kws_frontend_shape(self._h, C.byref(nf), C.byref(nc)), AudioProcessingError)
        return nf.value, nc.value

    def mfcc_i16(self, wav, out):
        self._check(self._lib.kws_mfcc_i16(self._h, _ptr(wav), int(wav.shape[0]), _ptr(out)), AudioProcessingError)

    def mfcc_f32(self, wav, out):
        self._check(self._lib.kws_mfcc_f32(self._h, _ptr(wav), int(wav.shape[0]), _ptr(out)), AudioProcessingError)

    # -- model ----------------------------------------------------------------------------------
    def load_dscnn(self, blob: np.ndarray, num_classes: int, input_channels: int = 1):
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        self._check(
            self._lib.kws_load_dscnn_ex(self._h, blob.ctypes.data_as(C.POINTER(C.c_float)), blob.size, int(num_classes),
                                        int(input_channels)),
            ModelError,
        )
        self.num_classes = int(num_classes)

    def load_dscnn_device(self, blob, num_classes: int, input_channels: int = 1):
        """``kws_load_dscnn_device``: ``blob`` float32 [n_floats] on this context's device (the 20 state_dict tensors in order);
        same image, scalars and forward as ``load_dscnn`` of the same values, built on the device."""
        self._check(self._lib.kws_load_dscnn_device(self._h, _ptr(blob), int(blob.numel()), int(num_classes), int(input_channels)),
                    ModelError)
        self.num_classes = int(num_classes)

    def dscnn_image(self):
        """(words uint32, scalars float32[23]) of the DS-CNN image this context holds now, in ``host_dscnn_image``'s format
        (``kws_dscnn_image_read``; waits for the context's stream)."""
        need = C.c_size_t(0)
        self._check(self._lib.kws_dscnn_image_read(self._h, None, 0, C.byref(need), None), ModelError)
        words, scalars = np.empty(need.value, np.uint32), np.empty(23, np.float32)
        self._check(self._lib.kws_dscnn_image_read(self._h, words.ctypes.data_as(C.POINTER(C.c_uint32)), words.size, None,
                                                   scalars.ctypes.data_as(C.POINTER(C.c_float))), ModelError)
        return words, scalars

    def forward_f32(self, feat, logits, label=None):
        self._check(
            self._lib.kws_forward_f32(self._h, _ptr(feat), int(feat.shape[0]), _ptr(logits), _ptr(label) if label is not None else None),
            ModelError,
        )

    def forward_map_f32(self, feat, logits, label=None, layers=None):
        """``feat`` float32 [B, C, T, F] of any size (99 x 10: the fused kernel; otherwise conv1 -> blocks -> pool + fc through
        HBM).  ``layers`` (diagnostics): every stage's output, stage after stage (``kws_forward_map_debug_f32``)."""
        B, _, T, F = (int(v) for v in feat.shape)
        lab = _ptr(label) if label is not None else None
        if layers is None:
            self._check(self._lib.kws_forward_map_f32(self._h, _ptr(feat), B, T, F, _ptr(logits), lab), ModelError)
        else:
            self._check(self._lib.kws_forward_map_debug_f32(self._h, _ptr(feat), B, T, F, _ptr(logits), lab, _ptr(layers)), ModelError)

    def dscnn_backward_f32(self, feat, T, F, dlogits, grad):
        """Gradient of a scalar loss with respect to the loaded DS-CNN's 20 state_dict tensors (``kws_dscnn_backward_f32``):
        ``feat`` float32 [B, C, T, F] and ``dlogits`` = dloss/dlogits float32 [B, num_classes] on the device; ``grad`` float32
        [n_floats] (the kws_load_dscnn blob layout) is overwritten.  Asynchronous on the context's stream."""
        self._check(self._lib.kws_dscnn_backward_f32(self._h, _ptr(feat), int(feat.shape[0]), int(T), int(F), _ptr(dlogits), _ptr(grad)),
                    ModelError)

    def dscnn_bn_train_forward_f32(self, params, num_classes, feat, eps, logits, label=None, stats=None, layers=None):
        """Train-mode forward of the BatchNorm DS-CNN at the device blob ``params`` (``DepthwiseSeparableConvBN.parameters()`` order;
        ``kws_dscnn_bn_train_forward_f32``): ``feat`` float32 [B, 1, T, F] -> ``logits``, ``label`` (optional), ``stats`` float32
        [9, 2, 64] (optional: batch mean and unbiased batch variance per layer).  ``layers`` (diagnostics): the five post-ReLU
        activations, stage after stage (``kws_dscnn_bn_train_debug_f32``)."""
        B, _, T, F = (int(v) for v in feat.shape)
        head = (self._h, _ptr(params), int(params.numel()), int(num_classes), _ptr(feat), B, T, F, float(eps), _ptr(logits), _opt(label))
        if layers is None:
            self._check(self._lib.kws_dscnn_bn_train_forward_f32(*head, _opt(stats)), ModelError)
        else:
            self._check(self._lib.kws_dscnn_bn_train_debug_f32(*head, _ptr(layers), _opt(stats)), ModelError)

    def dscnn_bn_backward_f32(self, params, num_classes, feat, eps, dlogits, grad):
        """Gradient of a scalar loss with respect to the 38 tensors of ``params`` (``kws_dscnn_bn_backward_f32``): ``dlogits`` float32
        [B, num_classes]; ``grad`` float32 [params.numel()] in the blob's layout is overwritten.  Asynchronous on the context's stream."""
        B, _, T, F = (int(v) for v in feat.shape)
        self._check(self._lib.kws_dscnn_bn_backward_f32(self._h, _ptr(params), int(params.numel()), int(num_classes), _ptr(feat), B, T, F,
                                                        float(eps), _ptr(dlogits), _ptr(grad)), ModelError)

    def load_cnn_trad(self, blob: np.ndarray, num_classes: int):
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        self._check(self._lib.kws_load_cnn_trad(self._h, blob.ctypes.data_as(C.POINTER(C.c_float)), blob.size, int(num_classes)),
                    ModelError)

    def load_cnn_trad_device(self, blob, num_classes: int):
        """``kws_load_cnn_trad_device``: ``blob`` float32 [n_floats] on this context's device (the ten state_dict tensors in
        order); same image and forward as ``load_cnn_trad`` of the same values, packed on the device."""
        self._check(self._lib.kws_load_cnn_trad_device(self._h, _ptr(blob), int(blob.numel()), int(num_classes)), ModelError)

    def cnn_trad_backward_f32(self, feat, dlogits, grad):
        """Gradient of a scalar loss with respect to the loaded cnn-trad-fpool3's ten state_dict tensors
        (``kws_cnn_trad_backward_f32``): ``feat`` float32 [B, 1, 99, 10] and ``dlogits`` float32 [B, num_classes] on the device;
        ``grad`` float32 [n_floats] (the kws_load_cnn_trad blob layout) is overwritten.  Asynchronous on the context's stream."""
        self._check(self._lib.kws_cnn_trad_backward_f32(self._h, _ptr(feat), int(feat.shape[0]), _ptr(dlogits), _ptr(grad)), ModelError)

    def cnn_trad_train_debug_f32(self, feat, conv1, winner, conv2, hidden):
        """The recompute stages of ``cnn_trad_backward_f32`` (``kws_cnn_trad_train_debug_f32``): conv1 after ReLU float32
        [B, 64, 99, 10], the pool winner int32 [B, 64, 99, 3], conv2 after ReLU float32 [B, 64, 99, 3], [h | d] float32 [B, 160]."""
        self._check(self._lib.kws_cnn_trad_train_debug_f32(self._h, _ptr(feat), int(feat.shape[0]), _ptr(conv1), _ptr(winner), _ptr(conv2),
                                                           _ptr(hidden)), ModelError)

    def set_cnn_trad_math(self, math: int):
        """KWS_CT_F16_PAIR (0, default) or KWS_CT_BF16_TRIPLE (1): arithmetic of cnn-trad-fpool3's GEMM layers."""
        self._check(self._lib.kws_set_cnn_trad_math(self._h, int(math)), ModelError)

    def forward_cnn_trad_f32(self, feat, logits, label=None):
        self._check(self._lib.kws_forward_cnn_trad_f32(self._h, _ptr(feat), int(feat.shape[0]), _ptr(logits),
                                                       _ptr(label) if label is not None else None), ModelError)

    def forward_cnn_trad_debug_f32(self, feat, logits, label, conv2, clip_scale=None):
        """``forward_cnn_trad_f32`` plus what sits between its two kernels (``kws_forward_cnn_trad_debug_f32``): ``conv2`` float32
        [B, 64, 99, 3] after ReLU and, under KWS_CT_F16_PAIR only, ``clip_scale`` float32 [B] (left untouched otherwise)."""
        self._check(self._lib.kws_forward_cnn_trad_debug_f32(self._h, _ptr(feat), int(feat.shape[0]), _ptr(logits),
                                                             _ptr(label) if label is not None else None, _ptr(conv2),
                                                             _ptr(clip_scale) if clip_scale is not None else None), ModelError)

    def infer_cnn_trad_i16(self, wav, logits, label=None):
        self._check(self._lib.kws_infer_cnn_trad_i16(self._h, _ptr(wav), int(wav.shape[0]), _ptr(logits),
                                                     _ptr(label) if label is not None else None), ModelError)

    def softmax_f32(self, logits, prob):
        self._check(self._lib.kws_softmax_f32(self._h, _ptr(logits), int(logits.shape[0]), int(logits.shape[1]), _ptr(prob)),
                    ModelError)

    def stream_smooth_f32(self, logits, window, smoothed, label=None):
        self._check(self._lib.kws_stream_smooth_f32(self._h, _ptr(logits), int(logits.shape[1]), int(window), _ptr(smoothed),
                                                    _ptr(label) if label is not None else None), ModelError)

    def stream_vad_f32(self, threshold, on_window, off_window, state):
        self._check(self._lib.kws_stream_vad_f32(self._h, float(threshold), int(on_window), int(off_window), _ptr(state)), ModelError)

    def set_pointwise_math(self, math):
        self._check(self._lib.kws_set_pointwise_math(self._h, int(math)), ModelError)

    def forward_debug_f32(self, feat, logits, label, act, use_mfma=PW_SPLIT_BF16):
        self._check(
            self._lib.kws_forward_debug_f32(self._h, _ptr(feat), int(feat.shape[0]), _ptr(logits),
                                            _ptr(label) if label is not None else None,
                                            _ptr(act) if act is not None else None, int(use_mfma)),
            ModelError,
        )

    def forward_stamps_f32(self, feat, logits, stamps, mode=PW_SPLIT_BF16):
        self._check(self._lib.kws_forward_stamps_f32(self._h, _ptr(feat), int(feat.shape[0]), _ptr(logits), _ptr(stamps), int(mode)), ModelError)

    def infer_i16(self, wav, logits, label=None):
        self._check(
            self._lib.kws_infer_i16(self._h, _ptr(wav), int(wav.shape[0]), _ptr(logits), _ptr(label) if label is not None else None),
            ModelError,
        )

    def dsblock_forward_f32(self, x, dw_w, dw_b, pw_w, pw_b, kernel_size, stride, padding, out):
        B, c_in, H, W = (int(v) for v in x.shape)
        self._check(self._lib.kws_dsblock_forward_f32(self._h, _ptr(x), B, c_in, H, W, _ptr(dw_w), _ptr(dw_b), _ptr(pw_w), _ptr(pw_b),
                                                      int(pw_w.shape[0]), int(kernel_size), int(stride), int(padding), _ptr(out)), ModelError)

    def infer_host_i16(self, wav: np.ndarray, logits: np.ndarray = None, label: np.ndarray = None):
        """Host ``int16[B,n]`` (numpy array or CPU torch tensor, pageable or pinned) -> host (logits float32[B,C], labels
        int32[B]) through the library's pack / H2D / compute / D2H pipeline (``kws_infer_host_i16``)."""
        logits, label, ticket, _keep = self.infer_host_submit_i16(wav, logits, label)
        self.infer_host_wait(ticket)
        return logits, label

    def infer_host_wait(self, ticket: int = 0):
        """Block until every submitted batch up to ``ticket`` (0: all) has its results in its host arrays."""
        ticket = int(ticket)
        self._check(self._lib.kws_infer_host_wait(self._h, C.c_uint64(ticket)), ModelError)
        # retired: the library has let go of every batch up to the ticket (after an error the arrays stay referenced, which is
        # always safe, until a later wait succeeds or the context closes)
        for t in [t for t in self._host_inflight if ticket == 0 or t <= ticket]:
            del self._host_inflight[t]

    def infer_host_submit_i16(self, wav: np.ndarray, logits: np.ndarray = None, label: np.ndarray = None):
        """Enqueue one host batch without waiting for its results (``kws_infer_host_submit_i16``).  Returns (logits, label,
        ticket, keepalive): the arrays are filled once ``infer_host_wait(ticket)`` has returned; keep ``keepalive`` (the
        source buffer -- a pinned one is read by the DMA until then) referenced until that wait.  The context itself also keeps
        the three referenced until ``infer_host_wait`` retires the ticket: the library holds raw pointers to them."""
        if self.num_classes is None:
            raise ModelError("no model loaded (kws_load_dscnn)")
        if hasattr(wav, "data_ptr"):  # CPU torch tensor (possibly pinned)
            if wav.is_cuda or wav.dtype.__str__() != "torch.int16" or not wav.is_contiguous() or wav.dim() != 2:
                raise ModelError("infer_host_i16 expects a contiguous CPU int16 tensor [B, n_samples]")
            src, B = int(wav.data_ptr()), int(wav.shape[0])
        else:
            wav = np.ascontiguousarray(wav, dtype=np.int16)
            if wav.ndim != 2:
                raise ModelError("infer_host_i16 expects int16 [B, n_samples]")
            src, B = wav.ctypes.data, int(wav.shape[0])
        if logits is None:
            logits = np.empty((B, self.num_classes), np.float32)
        if label is None:
            label = np.empty((B,), np.int32)
        assert logits.dtype == np.float32 and logits.flags.c_contiguous and logits.shape == (B, self.num_classes)
        assert label.dtype == np.int32 and label.flags.c_contiguous and label.shape == (B,)
        ticket = C.c_uint64(0)
        self._check(self._lib.kws_infer_host_submit_i16(self._h, C.c_void_p(src), B, C.c_void_p(logits.ctypes.data),
                                                        C.c_void_p(label.ctypes.data), C.byref(ticket)), ModelError)
        self._host_inflight[int(ticket.value)] = (logits, label, wav)
        return logits, label, int(ticket.value), wav

    # -- cnn-trad-fpool3 on recordings and streams ---------------------------------------------------
    def infer_cnn_trad_f32(self, wav, logits, label=None):
        """``kws_infer_cnn_trad_f32``: ``infer_cnn_trad_i16`` over ``wav`` float32 [B, n_samples] on the device."""
        self._check(self._lib.kws_infer_cnn_trad_f32(self._h, _ptr(wav), int(wav.shape[0]), _ptr(logits),
                                                     _ptr(label) if label is not None else None), ModelError)

    def forward_cnn_trad_windows_f32(self, frames, hop_frames, logits, label=None):
        """``kws_forward_cnn_trad_windows_f32``: ``frames`` float32 [R, F, 10] on the device -> ``logits`` float32 [R, W, C] (and
        ``label`` int32 [R, W]) for every window of 99 frames, ``hop_frames`` apart, read in place; W = (F - 99) // hop_frames + 1."""
        self._check(self._lib.kws_forward_cnn_trad_windows_f32(self._h, _ptr(frames), int(frames.shape[0]), int(frames.shape[1]),
                                                               int(hop_frames), _ptr(logits), _ptr(label) if label is not None else None),
                    ModelError)

    def scan_cnn_trad_i16(self, pcm, hop_frames, logits, label=None, feat=None):
        """``kws_scan_cnn_trad_i16``: ``scan_i16`` with cnn-trad-fpool3 over the windows."""
        self._scan_equal(self._lib.kws_scan_cnn_trad_i16, pcm, hop_frames, logits, label, feat)

    def scan_cnn_trad_f32(self, wav, hop_frames, logits, label=None, feat=None):
        """``kws_scan_cnn_trad_f32``: ``scan_f32`` with cnn-trad-fpool3 over the windows."""
        self._scan_equal(self._lib.kws_scan_cnn_trad_f32, wav, hop_frames, logits, label, feat)

    def scan_ragged_cnn_trad_i16(self, pcm, start, length, hop_frames, logits, label=None, feat=None):
        """``kws_scan_ragged_cnn_trad_i16``: ``scan_ragged_i16`` with cnn-trad-fpool3 over the packed windows."""
        self._scan_packed(self._lib.kws_scan_ragged_cnn_trad_i16, pcm, start, length, hop_frames, logits, label, feat)

    def scan_ragged_cnn_trad_f32(self, wav, start, length, hop_frames, logits, label=None, feat=None):
        """``kws_scan_ragged_cnn_trad_f32``: ``scan_ragged_f32`` with cnn-trad-fpool3 over the packed windows."""
        self._scan_packed(self._lib.kws_scan_ragged_cnn_trad_f32, wav, start, length, hop_frames, logits, label, feat)

    def stream_push_cnn_trad_i16(self, hop, logits, label=None):
        """``kws_stream_push_cnn_trad_i16``: one hop per stream, then cnn-trad-fpool3 over every stream's window of the feature
        ring; ``logits`` float32 [n_streams, C] is required.  Three launches; read the results after ``sync``."""
        self._check(self._lib.kws_stream_push_cnn_trad_i16(self._h, _ptr(hop), _ptr(logits), _ptr(label) if label is not None else None),
                    ModelError)

    def ingest_config(self, chunk_clips: int = 0, n_slots: int = 0, pack_threads: int = 0):
        self._check(self._lib.kws_ingest_config(self._h, int(chunk_clips), int(n_slots), int(pack_threads)), ModelError)

    def infer_f32(self, wav, logits, label=None):
        self._check(
            self._lib.kws_infer_f32(self._h, _ptr(wav), int(wav.shape[0]), _ptr(logits), _ptr(label) if label is not None else None),
            ModelError,
        )

    # -- scanning --------------------------------------------------------------------------------
    def _scan_equal(self, fn, src, hop_frames, logits, label, feat):
        """One of the four ``kws_scan_*`` entries over ``src`` [R, n_total] on the device."""
        self._check(fn(self._h, _ptr(src), int(src.shape[0]), int(src.shape[1]), int(hop_frames), _ptr(logits), _opt(label), _opt(feat)), ModelError)

    def _scan_packed(self, fn, src, start, length, hop_frames, logits, label, feat):
        """One of the four ``kws_scan_ragged_*`` entries over the packed ``src`` on the device; ``start`` / ``length`` host sequences."""
        st, ln = _host_i64(start), _host_i32(length)
        self._check(fn(self._h, _ptr(src), int(src.numel()), _as(st, C.c_int64), _as(ln, C.c_int32), len(ln), int(hop_frames), _ptr(logits),
                       _opt(label), _opt(feat)), ModelError)

    def scan_i16(self, pcm, hop_frames, logits, label=None, feat=None):
        """``kws_scan_i16``: ``pcm`` int16 [R, n_total] on the device -> ``logits`` float32 [R, W, C] (and ``label`` int32 [R, W])
        for every window of 99 frames, ``hop_frames`` frames apart, of each recording's one MFCC pass; ``feat`` float32
        [R, F_total, numcep] keeps the frames (``host_scan_shape`` gives F_total and W)."""
        self._scan_equal(self._lib.kws_scan_i16, pcm, hop_frames, logits, label, feat)

    def scan_f32(self, wav, hop_frames, logits, label=None, feat=None):
        """``kws_scan_f32``: ``scan_i16`` over ``wav`` float32 [R, n_total] on the device, the samples taken as they are."""
        self._scan_equal(self._lib.kws_scan_f32, wav, hop_frames, logits, label, feat)

    def scan_detect_f32(self, logits, smooth_window, first_keyword, threshold, refractory, event_count, event_window=None,
                        event_label=None, event_score=None, max_events=0, smoothed=None):
        """``kws_scan_detect_f32``: ``logits`` float32 [R, W, C] -> smoothed posteriors, candidates and events with a refractory
        gap.  ``event_count`` int32 [R]; the three event arrays [R, max_events]; ``smoothed`` float32 [R, W, C] or None."""
        R, W, Cn = (int(v) for v in logits.shape)
        self._check(self._lib.kws_scan_detect_f32(self._h, _ptr(logits), R, W, Cn, int(smooth_window), int(first_keyword), float(threshold),
                                                  int(refractory), _opt(smoothed), _opt(event_window), _opt(event_label), _opt(event_score),
                                                  int(max_events), _ptr(event_count)), ModelError)

    # -- utterances --------------------------------------------------------------------------------
    def frames_i16(self, pcm, feat):
        """``kws_frames_i16``: ``pcm`` int16 [R, n_total] on the device -> ``feat`` float32 [R, F_total, numcep], each recording
        one clip of the context's front end (``host_scan_shape`` gives F_total)."""
        self._check(self._lib.kws_frames_i16(self._h, _ptr(pcm), int(pcm.shape[0]), int(pcm.shape[1]), _ptr(feat)), AudioProcessingError)

    def frames_f32(self, wav, feat):
        """``kws_frames_f32``: ``frames_i16`` over ``wav`` float32 [R, n_total] on the device."""
        self._check(self._lib.kws_frames_f32(self._h, _ptr(wav), int(wav.shape[0]), int(wav.shape[1]), _ptr(feat)), AudioProcessingError)

    def segment_f32(self, feat, n_total, threshold, count, utt=None, max_utts=0, on_window=40, off_window=80, pre_roll=60,
                    max_frames=1000):
        """``kws_segment_f32``: the endpointer walked over ``feat`` float32 [R, F_total, numcep] (column 0).  ``count`` int32 [R];
        ``utt`` int32 [R, max_utts, 5] = (start_sample, end_sample, open, close, reason 0 endpoint / 1 max length / 2 end of
        recording) or None with ``max_utts`` 0."""
        self._check(self._lib.kws_segment_f32(self._h, _ptr(feat), int(feat.shape[0]), int(feat.shape[1]), int(n_total), float(threshold),
                                              int(on_window), int(off_window), int(pre_roll), int(max_frames),
                                              _ptr(utt) if utt is not None else None, int(max_utts), _ptr(count)), ModelError)

    def cut_i16(self, pcm, span, clips, normalize_to=16384, peak=None):
        """``kws_cut_i16``: normalize + fix_length of ``span`` int32 [U, 3] = (recording, start, end) over ``pcm`` int16
        [R, n_total] into ``clips`` int16 [U, n_out]; ``peak`` int32 [U] or None."""
        self._check(self._lib.kws_cut_i16(self._h, _ptr(pcm), int(pcm.shape[0]), int(pcm.shape[1]), _ptr(span), int(span.shape[0]),
                                          int(normalize_to), _ptr(clips), int(clips.shape[1]), _ptr(peak) if peak is not None else None),
                    AudioProcessingError)

    def cut_f32(self, wav, span, clips, normalize_to=0.5, peak=None):
        """``kws_cut_f32``: ``cut_i16`` over ``wav`` float32 [R, n_total] into ``clips`` float32 [U, n_out]; ``normalize_to`` and
        ``peak`` (float32 [U] or None) are in full-scale units (0.5 is the reference's 16384), and nothing is truncated."""
        self._check(self._lib.kws_cut_f32(self._h, _ptr(wav), int(wav.shape[0]), int(wav.shape[1]), _ptr(span), int(span.shape[0]),
                                          float(normalize_to), _ptr(clips), int(clips.shape[1]), _ptr(peak) if peak is not None else None),
                    AudioProcessingError)

    # -- batches of recordings of unequal length ---------------------------------------------------
    def frames_ragged_i16(self, pcm, start, length, row_multiple, feat):
        """``kws_frames_ragged_i16``: ``pcm`` int16 (any shape, contiguous) on the device holds recording r at samples
        ``[start[r], start[r] + length[r])`` (host sequences; starts multiples of 8) -> ``feat`` float32 [F_pack, numcep], every
        recording's rows rounded up to ``row_multiple`` (``host_ragged_plan(length, hop_frames=row_multiple)`` gives the rows)."""
        st, ln = _host_i64(start), _host_i32(length)
        self._check(self._lib.kws_frames_ragged_i16(self._h, _ptr(pcm), int(pcm.numel()), _as(st, C.c_int64), _as(ln, C.c_int32), len(ln),
                                                    int(row_multiple), _ptr(feat)), AudioProcessingError)

    def scan_ragged_i16(self, pcm, start, length, hop_frames, logits, label=None, feat=None):
        """``kws_scan_ragged_i16``: the ragged front end, then the DS-CNN over the packed frame array as one recording ->
        ``logits`` float32 [W_pack, C] (``label`` int32 [W_pack]); window w of recording r is row ``win_off[r] + w``."""
        self._scan_packed(self._lib.kws_scan_ragged_i16, pcm, start, length, hop_frames, logits, label, feat)

    def frames_ragged_f32(self, wav, start, length, row_multiple, feat):
        """``kws_frames_ragged_f32``: ``frames_ragged_i16`` over ``wav`` float32 (any shape, contiguous) on the device."""
        st, ln = _host_i64(start), _host_i32(length)
        self._check(self._lib.kws_frames_ragged_f32(self._h, _ptr(wav), int(wav.numel()), _as(st, C.c_int64), _as(ln, C.c_int32), len(ln),
                                                    int(row_multiple), _ptr(feat)), AudioProcessingError)

    def scan_ragged_f32(self, wav, start, length, hop_frames, logits, label=None, feat=None):
        """``kws_scan_ragged_f32``: ``scan_ragged_i16`` over ``wav`` float32 (any shape, contiguous) on the device."""
        self._scan_packed(self._lib.kws_scan_ragged_f32, wav, start, length, hop_frames, logits, label, feat)

    def scan_detect_ragged_f32(self, logits, win_off, windows, smooth_window, first_keyword, threshold, refractory, event_count,
                               event_window=None, event_label=None, event_score=None, max_events=0, smoothed=None):
        """``kws_scan_detect_ragged_f32``: ``logits`` float32 [W_pack, C]; ``win_off`` / ``windows`` host sequences [R]; the
        decisions of ``scan_detect_f32`` per recording.  ``event_count`` int32 [R]; the event arrays [R, max_events]."""
        wo, wn = _host_i32(win_off), _host_i32(windows)
        self._check(self._lib.kws_scan_detect_ragged_f32(self._h, _ptr(logits), _as(wo, C.c_int32), _as(wn, C.c_int32), len(wn),
                                                         int(logits.shape[-1]), int(smooth_window), int(first_keyword), float(threshold),
                                                         int(refractory), _opt(smoothed), _opt(event_window), _opt(event_label), _opt(event_score),
                                                         int(max_events), _ptr(event_count)), ModelError)

    # -- scoring against annotations ---------------------------------------------------------------
    def scan_score_f32(self, logits, smooth_window, first_keyword, refractory, thresholds, truth, counts):
        """``kws_scan_score_f32``: ``logits`` float32 [R, W, C] on the device scored against ``truth`` (host, int32 [N, 4] rows
        (recording, label, first_window, last_window), or None / empty) at every one of ``thresholds`` (host, float32 [K]):
        ``counts`` int64 [K, C, 4] on the device = hits, false alarms, duplicates, latency sum.  Read it after ``sync``."""
        R, W, Cn = (int(v) for v in logits.shape)
        th, tr = _host_f32(thresholds), _host_truth(truth)
        self._check(self._lib.kws_scan_score_f32(self._h, _ptr(logits), R, W, Cn, int(smooth_window), int(first_keyword), int(refractory),
                                                 _as(th, C.c_float), len(th), _as(tr, C.c_int32) if len(tr) else None, len(tr),
                                                 _ptr(counts)), ModelError)

    def scan_score_ragged_f32(self, logits, win_off, windows, smooth_window, first_keyword, refractory, thresholds, truth, counts):
        """``kws_scan_score_ragged_f32``: ``scan_score_f32`` per recording of the packed ``logits`` float32 [W_pack, C];
        ``win_off`` / ``windows`` host sequences [R]; the windows of ``truth`` are relative to their own recording."""
        wo, wn = _host_i32(win_off), _host_i32(windows)
        th, tr = _host_f32(thresholds), _host_truth(truth)
        self._check(self._lib.kws_scan_score_ragged_f32(self._h, _ptr(logits), _as(wo, C.c_int32), _as(wn, C.c_int32), len(wn),
                                                        int(logits.shape[-1]), int(smooth_window), int(first_keyword), int(refractory),
                                                        _as(th, C.c_float), len(th), _as(tr, C.c_int32) if len(tr) else None, len(tr),
                                                        _ptr(counts)), ModelError)

    def segment_ragged_f32(self, feat, frame_off, frames, length, threshold, count, utt=None, max_utts=0, on_window=40, off_window=80,
                           pre_roll=60, max_frames=1000):
        """``kws_segment_ragged_f32``: the endpointer of ``segment_f32`` per recording of the packed ``feat`` float32
        [F_pack, numcep]; ``frame_off`` / ``frames`` / ``length`` host sequences [R].  ``count`` int32 [R]; ``utt`` int32
        [R, max_utts, 5] with spans relative to each recording's own start."""
        fo, fr, ln = _host_i32(frame_off)[:len(frames)], _host_i32(frames), _host_i32(length)
        self._check(self._lib.kws_segment_ragged_f32(self._h, _ptr(feat), _as(np.ascontiguousarray(fo), C.c_int32), _as(fr, C.c_int32),
                                                     _as(ln, C.c_int32), len(ln), float(threshold), int(on_window), int(off_window),
                                                     int(pre_roll), int(max_frames), _ptr(utt) if utt is not None else None, int(max_utts),
                                                     _ptr(count)), ModelError)

    # -- live utterances ---------------------------------------------------------------------------
    def stream_utt_open(self, threshold, on_window, off_window, pre_roll, max_frames, history_samples, max_events):
        """``kws_stream_utt_open``: arm the open stream set -- every push then appends its hop to a per-stream history, walks
        one frame of the endpointer and queues the utterances that close (``host_stream_utt_history`` sizes the history)."""
        self._check(self._lib.kws_stream_utt_open(self._h, float(threshold), int(on_window), int(off_window), int(pre_roll),
                                                  int(max_frames), int(history_samples), int(max_events)), ModelError)

    def stream_utt_close(self):
        self._check(self._lib.kws_stream_utt_close(self._h), ModelError)

    def stream_utt_step_i16(self, hop=None, energy=None):
        """``kws_stream_utt_step_i16``: the explicit step; ``hop`` int16 [S, frame_step] and / or ``energy`` float32 [S], device
        tensors or raw device addresses."""
        p = lambda t: None if t is None else (int(t) if isinstance(t, int) else _ptr(t))
        self._check(self._lib.kws_stream_utt_step_i16(self._h, p(hop), p(energy)), ModelError)

    def stream_utt_flush(self):
        self._check(self._lib.kws_stream_utt_flush(self._h), ModelError)

    def stream_utt_poll(self):
        """``kws_stream_utt_poll``: wait for the newest step; (events so far, frames walked)."""
        total, steps = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.kws_stream_utt_poll(self._h, C.byref(total), C.byref(steps)), ModelError)
        return int(total.value), int(steps.value)

    def stream_utt_read(self, first_seq: int, n: int) -> np.ndarray:
        """``kws_stream_utt_read``: int64 [n, 6] = (stream, start_sample, end_sample, open_frame, close_frame, reason) of the
        sequence numbers ``first_seq`` .. ``first_seq + n - 1``, from the host mirror of the queue."""
        out = np.empty((max(int(n), 0), 6), np.int64)
        self._check(self._lib.kws_stream_utt_read(self._h, C.c_uint64(int(first_seq)), int(n), out.ctypes.data_as(C.POINTER(C.c_int64))),
                    ModelError)
        return out

    def stream_utt_cut_i16(self, first_seq: int, clips, normalize_to=16384, peak=None):
        """``kws_stream_utt_cut_i16``: the spans of ``clips.shape[0]`` consecutive sequence numbers cut from the history rings,
        normalised and padded or trimmed into ``clips`` int16 [U, n_out]; ``peak`` int32 [U] or None."""
        self._check(self._lib.kws_stream_utt_cut_i16(self._h, C.c_uint64(int(first_seq)), int(clips.shape[0]), int(normalize_to), _ptr(clips),
                                                     int(clips.shape[1]), _ptr(peak) if peak is not None else None), AudioProcessingError)

    # -- live keyword events -----------------------------------------------------------------------
    def stream_detect_open(self, num_classes, smooth_window, first_keyword, threshold, refractory, first_hop, max_events):
        """``kws_stream_detect_open``: arm the open stream set -- every push that asks for logits is then followed by one
        decision per stream (softmax, causal mean over ``smooth_window`` decisions, threshold, refractory) and the events are
        queued; pushes below hop ``first_hop`` decide nothing."""
        self._check(self._lib.kws_stream_detect_open(self._h, int(num_classes), int(smooth_window), int(first_keyword), float(threshold),
                                                     int(refractory), int(first_hop), int(max_events)), ModelError)

    def stream_detect_close(self):
        self._check(self._lib.kws_stream_detect_close(self._h), ModelError)

    def stream_detect_step_f32(self, logits):
        """``kws_stream_detect_step_f32``: the explicit step; ``logits`` float32 [S, C], a device tensor or a raw device address."""
        self._check(self._lib.kws_stream_detect_step_f32(self._h, int(logits) if isinstance(logits, int) else _ptr(logits)), ModelError)

    def stream_detect_poll(self):
        """``kws_stream_detect_poll``: wait for the newest step; (events so far, decisions made)."""
        total, decisions = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.kws_stream_detect_poll(self._h, C.byref(total), C.byref(decisions)), ModelError)
        return int(total.value), int(decisions.value)

    def stream_detect_read(self, first_seq: int, n: int) -> np.ndarray:
        """``kws_stream_detect_read``: int64 [n, 5] = (stream, decision, hop, label, score bits) of the sequence numbers
        ``first_seq`` .. ``first_seq + n - 1``, from the host mirror of the queue."""
        out = np.empty((max(int(n), 0), 5), np.int64)
        self._check(self._lib.kws_stream_detect_read(self._h, C.c_uint64(int(first_seq)), int(n), out.ctypes.data_as(C.POINTER(C.c_int64))),
                    ModelError)
        return out

    def stream_detect_smoothed(self, smoothed, label):
        """``kws_stream_detect_smoothed``: the newest decision's posteriors into ``smoothed`` float32 [S, C] and their argmax
        into ``label`` int32 [S] (device), asynchronously on the context stream."""
        self._check(self._lib.kws_stream_detect_smoothed(self._h, _ptr(smoothed), _ptr(label)), ModelError)

    # -- sample-rate conversion --------------------------------------------------------------------
    def _resample(self, fn, x, rate_in, rate_out, out, lengths):
        self._check(fn(self._h, _ptr(x), int(x.shape[0]), int(x.shape[1]), _ptr(lengths) if lengths is not None else None, int(rate_in),
                       int(rate_out), _ptr(out), int(out.shape[1])), AudioProcessingError)

    def resample_i16(self, pcm, rate_in, rate_out, out, lengths=None):
        """``kws_resample_i16``: ``pcm`` int16 [R, n_in] at ``rate_in`` -> ``out`` int16 [R, n_out] at ``rate_out``, both on the
        device; ``lengths`` int32 [R] (device) gives each row's valid samples.  Outputs beyond a row's natural length
        (``host_resample_len``) are zeros.  The first use of a rate pair designs and uploads its taps."""
        self._resample(self._lib.kws_resample_i16, pcm, rate_in, rate_out, out, lengths)

    def resample_f32(self, signal, rate_in, rate_out, out, lengths=None):
        """``kws_resample_f32``: the same for float32 [R, n_in] -> float32 [R, n_out]."""
        self._resample(self._lib.kws_resample_f32, signal, rate_in, rate_out, out, lengths)

    # -- streaming sample-rate conversion ---------------------------------------------------------
    @staticmethod
    def host_stream_resample_plan(rate_in, rate_out):
        return host_stream_resample_plan(rate_in, rate_out)

    @staticmethod
    def host_stream_resample_count(rate_in, rate_out, samples_before, n_in) -> int:
        return host_stream_resample_count(rate_in, rate_out, samples_before, n_in)

    def stream_resample_open(self, n_streams: int, rate_in: int, rate_out: int, max_in: int, first_sample: int = 0):
        """``kws_stream_resample_open``: a stateful resampler for ``n_streams`` streams in lockstep and pushes of at most ``max_in``
        samples; ``first_sample`` (a multiple of ``down``) is where the streams' signal starts."""
        self._check(self._lib.kws_stream_resample_open(self._h, int(n_streams), int(rate_in), int(rate_out), int(max_in),
                                                       C.c_uint64(int(first_sample))), AudioProcessingError)

    def stream_resample_close(self):
        self._check(self._lib.kws_stream_resample_close(self._h), AudioProcessingError)

    def stream_resample_i16(self, pcm, out) -> int:
        """``kws_stream_resample_i16``: the next ``pcm`` int16 [S, n_in] of every stream -> ``out`` int16 [S, out_cap], both on the
        device; returns the samples per stream this push emitted (known before the launch; the call is asynchronous)."""
        n = C.c_int(0)
        self._check(self._lib.kws_stream_resample_i16(self._h, _ptr(pcm), int(pcm.shape[1]), _ptr(out), int(out.shape[1]), C.byref(n)),
                    AudioProcessingError)
        return n.value

    def stream_push_rate_i16(self, pcm, logits=None, label=None):
        """``kws_stream_push_rate_i16``: one hop's worth of ``pcm`` int16 [S, n_in] at the resampler's input rate (device) ->
        resampled into the context's hop buffer -> ``stream_push_i16``."""
        self._check(self._lib.kws_stream_push_rate_i16(self._h, _ptr(pcm), int(pcm.shape[1]), _ptr(logits) if logits is not None else None,
                                                       _ptr(label) if label is not None else None), ModelError)

    def stream_push_host_rate_i16(self, pcm: np.ndarray, n_streams: int):
        """``kws_stream_push_host_rate_i16``: host int16 [S, n_in] at the resampler's input rate -> (logits, labels) host views."""
        if pcm.dtype != np.int16 or not pcm.flags.c_contiguous or pcm.ndim != 2 or pcm.shape[0] != n_streams:
            raise ModelError("stream_push_host_rate_i16 expects a C-contiguous int16 array [n_streams, n_in]")
        pl, py = C.c_void_p(), C.c_void_p()
        self._check(self._lib.kws_stream_push_host_rate_i16(self._h, pcm.ctypes.data, int(pcm.shape[1]), C.byref(pl), C.byref(py)), ModelError)
        return self._host_views_of(pl, py, n_streams)

    # -- evaluation ------------------------------------------------------------------------------
    def eval_open(self, num_classes: int, n_bins: int = 256):
        """``kws_eval_open``: allocate and zero the context's evaluation state for ``num_classes`` classes and ``n_bins``
        posterior bins (a power of two in [2, 1024], or 0: no histograms)."""
        self._check(self._lib.kws_eval_open(self._h, int(num_classes), int(n_bins)), ModelError)
        self._eval_shape = (int(num_classes), int(n_bins))

    def eval_reset(self):
        self._check(self._lib.kws_eval_reset(self._h), ModelError)

    def eval_close(self):
        self._check(self._lib.kws_eval_close(self._h), ModelError)
        self._eval_shape = None

    def eval_update_f32(self, logits, truth, grad_scale: float = 0.0, dlogits=None, loss_rows=None):
        """``kws_eval_update_f32``: ``logits`` float32 [B, C] and ``truth`` int32 [B] on the device into the statistics;
        ``dlogits`` float32 [B, C] (the cross-entropy gradient times ``grad_scale``) and ``loss_rows`` float32 [B] are optional
        outputs.  Asynchronous on the context's stream."""
        self._check(self._lib.kws_eval_update_f32(self._h, _ptr(logits), _ptr(truth), int(logits.shape[0]), float(grad_scale), _opt(dlogits),
                                                  _opt(loss_rows)), ModelError)

    def eval_read(self):
        """``kws_eval_read``: wait for the stream, then (counts uint64[4], loss_sum float, confusion uint64[C, C], hist_pos
        uint64[C, K], hist_neg uint64[C, K]) on the host; counts = rows used, correct, ignored, non-finite."""
        shape = getattr(self, "_eval_shape", None)
        if shape is None:
            raise ModelError("eval_read: call eval_open first")
        Cn, K = shape
        u64 = C.POINTER(C.c_uint64)
        counts, loss = np.zeros(4, np.uint64), C.c_double(0.0)
        confusion = np.zeros((Cn, Cn), np.uint64)
        pos, neg = np.zeros((Cn, K), np.uint64), np.zeros((Cn, K), np.uint64)
        self._check(self._lib.kws_eval_read(self._h, counts.ctypes.data_as(u64), C.byref(loss), confusion.ctypes.data_as(u64),
                                            pos.ctypes.data_as(u64) if K else None, neg.ctypes.data_as(u64) if K else None), ModelError)
        return counts, float(loss.value), confusion, pos, neg

    # -- streaming -------------------------------------------------------------------------------
    def stream_open(self, n_streams: int):
        self._check(self._lib.kws_stream_open(self._h, int(n_streams)), AudioProcessingError)

    def stream_cluster(self, workgroups_per_stream: int = 0):
        """Workgroups per stream of the one-launch push: 1, or 2 / 4 time tiles; 0 = by stream count (``kws_stream_cluster``)."""
        self._check(self._lib.kws_stream_cluster(self._h, int(workgroups_per_stream)), ModelError)

    def stream_host_results(self, enable: bool = True):
        """Zero-copy delivery of the one-launch push's logits / labels to pinned host memory (``kws_stream_host_results``)."""
        self._check(self._lib.kws_stream_host_results(self._h, 1 if enable else 0), ModelError)
        self._host_views = None

    def stream_push_host_i16(self, hop: np.ndarray, n_streams: int):
        """Host int16 [S, hop] -> (logits, labels) host views in one call (``kws_stream_push_host_i16``): no H2D submission,
        no synchronise, no D2H copy."""
        if hop.dtype != np.int16 or not hop.flags.c_contiguous:
            raise ModelError("stream_push_host_i16 expects a C-contiguous int16 array")
        pl, py = C.c_void_p(), C.c_void_p()
        self._check(self._lib.kws_stream_push_host_i16(self._h, hop.ctypes.data, C.byref(pl), C.byref(py)), ModelError)
        return self._host_views_of(pl, py, n_streams)

    def stream_wait_host(self, n_streams: int):
        """Spin until the newest push's results are in host memory; returns numpy VIEWS (logits float32[S,C], labels int32[S])
        of the context's pinned arrays -- valid until the next push."""
        pl, py = C.c_void_p(), C.c_void_p()
        self._check(self._lib.kws_stream_wait_host(self._h, C.byref(pl), C.byref(py)), ModelError)
        return self._host_views_of(pl, py, n_streams)

    def _host_views_of(self, pl, py, n_streams):
        key = (pl.value, py.value, n_streams, self.num_classes)  # a reload with another class count may get the old addresses back
        if getattr(self, "_host_views", None) is None or self._host_views[0] != key:
            lg = np.ctypeslib.as_array(C.cast(pl, C.POINTER(C.c_float)), shape=(n_streams, self.num_classes))
            lb = np.ctypeslib.as_array(C.cast(py, C.POINTER(C.c_int32)), shape=(n_streams,))
            self._host_views = (key, lg, lb)
        return self._host_views[1], self._host_views[2]

    def stream_close(self):
        self._check(self._lib.kws_stream_close(self._h))

    def stream_reset(self, streams):
        """``kws_stream_reset``: from the next push on the named streams (an int or a sequence of indices, host) behave as if they
        had received silence ever since ``stream_open``; what is armed on the set starts over for them, every other stream is
        untouched.  Enqueued on the context's stream; the indices travel inside the launch."""
        idx = np.ascontiguousarray(np.atleast_1d(np.asarray(streams, dtype=np.int64)).ravel())
        if idx.size and (idx.min() < -2**31 or idx.max() >= 2**31):
            raise ModelError("stream_reset: a stream index does not fit int32")
        idx = idx.astype(np.int32)
        self._check(self._lib.kws_stream_reset(self._h, idx.ctypes.data if idx.size else None, int(idx.size)), ModelError)

    def _stream_indices(self, streams, what):
        idx = np.ascontiguousarray(np.atleast_1d(np.asarray(streams, dtype=np.int64)).ravel())
        if idx.size and (idx.min() < -2**31 or idx.max() >= 2**31):
            raise ModelError(f"{what}: a stream index does not fit int32")
        return idx.astype(np.int32)

    def stream_deactivate(self, streams):
        """``kws_stream_deactivate``: the named streams (an int or a sequence of indices, host) leave the set -- from the next push
        on their hop rows are not read and nothing of theirs is written; an utterance open on one closes with reason 2.  Enqueued
        on the context's stream; the indices travel inside the launch."""
        idx = self._stream_indices(streams, "stream_deactivate")
        self._check(self._lib.kws_stream_deactivate(self._h, idx.ctypes.data if idx.size else None, int(idx.size)), ModelError)

    def stream_activate(self, streams):
        """``kws_stream_activate``: the named streams get the whole of ``stream_reset`` and (re)join the set."""
        idx = self._stream_indices(streams, "stream_activate")
        self._check(self._lib.kws_stream_activate(self._h, idx.ctypes.data if idx.size else None, int(idx.size)), ModelError)

    def stream_active(self, n_streams):
        """``kws_stream_active``: (bool [n_streams], active count) from the host's own record; no device work, no wait."""
        out = np.zeros(int(n_streams), np.uint8)
        n = C.c_int(0)
        self._check(self._lib.kws_stream_active(self._h, out.ctypes.data, C.byref(n)), ModelError)
        return out.astype(np.bool_), int(n.value)

    def stream_push_i16(self, hop, logits=None, label=None, use_graph=False):
        self._check(
            self._lib.kws_stream_push_i16(self._h, _ptr(hop), _ptr(logits) if logits is not None else None,
                                          _ptr(label) if label is not None else None, 1 if use_graph else 0),
            ModelError,
        )

    def stream_state(self):
        """(device address of the feature ring, pushes so far)."""
        ring, hops = C.c_void_p(), C.c_int()
        self._check(self._lib.kws_stream_state(self._h, C.byref(ring), C.byref(hops)))
        return ring.value, hops.value

    def stream_copy_features(self, out):
        self._check(self._lib.kws_stream_copy_features(self._h, _ptr(out)))

    # -- augmentation ----------------------------------------------------------------------------
    def augment_i16(self, wav, out, shift=None, bg=None, bg_off=None, bg_vol=None, silence=None):
        self._check(
            self._lib.kws_augment_i16(self._h, _ptr(wav), int(wav.shape[0]), _opt(shift), _opt(bg), int(bg.numel()) if bg is not None else 0,
                                      _opt(bg_off), _opt(bg_vol), _opt(silence), _ptr(out)),
            AudioProcessingError,
        )

    def augment_draw(self, seed, epoch, index, shift, bg_off, bg_vol, silence, labels=None, time_shift=0, bg_start=None, bg_len=None,
                     bg_volume=0.0, bg_frequency=0.0, use_background=True, n_samples=16000):
        """The training transform's random draws for the dataset indices ``index`` (int32, device), made on the device."""
        self._check(
            self._lib.kws_augment_draw(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFF, _ptr(index), int(index.numel()),
                                       _opt(labels), int(labels.numel()) if labels is not None else 0, int(time_shift), _opt(bg_start),
                                       _opt(bg_len), int(bg_start.numel()) if bg_start is not None else 0, float(bg_volume),
                                       float(bg_frequency), int(bool(use_background)), int(n_samples), _ptr(shift), _ptr(bg_off),
                                       _ptr(bg_vol), _ptr(silence)),
            AudioProcessingError,
        )

    def mfcc_augment_i16(self, pcm, index, out, shift=None, bg=None, bg_off=None, bg_vol=None, silence=None) -> int:
        """Gather + augment + MFCC in one launch.  Returns ``KWS_OK``, or ``KWS_EUNSUPPORTED`` when the configured front end
        has no fused kernel (the caller composes ``augment_i16`` and ``mfcc_f32``); every other code raises."""
        rc = self._lib.kws_mfcc_augment_i16(self._h, _ptr(pcm), int(pcm.shape[0]), _ptr(index), int(index.numel()), _opt(shift), _opt(bg),
                                            int(bg.numel()) if bg is not None else 0, _opt(bg_off), _opt(bg_vol), _opt(silence), _ptr(out))
        if rc != KWS_EUNSUPPORTED:
            self._check(rc, AudioProcessingError)
        return rc

    def reserve(self, max_batch: int):
        self._check(self._lib.kws_reserve(self._h, int(max_batch)))

    # -- sigproc operators ----------------------------------------------------------------------
    def preemphasis_f32(self, sig, coeff, out):
        self._check(self._lib.kws_preemphasis_f32(self._h, _ptr(sig), int(sig.numel()), float(coeff), _ptr(out)), AudioProcessingError)

    def framesig_f32(self, sig, frame_len, frame_step, window, frames):
        self._check(
            self._lib.kws_framesig_f32(self._h, _ptr(sig), int(sig.numel()), int(frame_len), int(frame_step),
                                       _ptr(window) if window is not None else None, _ptr(frames)),
            AudioProcessingError,
        )

    def spec_f32(self, frames, nfft, power, spec):
        self._check(
            self._lib.kws_spec_f32(self._h, _ptr(frames), int(frames.shape[0]), int(frames.shape[1]), int(nfft), 1 if power else 0, _ptr(spec)),
            AudioProcessingError,
        )

    def spec512_f32(self, frames, power, spec):
        self._check(
            self._lib.kws_spec512_f32(self._h, _ptr(frames), int(frames.shape[0]), int(frames.shape[1]), 1 if power else 0, _ptr(spec)),
            AudioProcessingError,
        )

    # -- measurement ----------------------------------------------------------------------------
    def prof_enable(self, on=True):
        """False/0 = off, True/1 = time every kernel launch, n > 1 = time every n-th launch of each kernel."""
        self._check(self._lib.kws_prof_enable(self._h, int(on)))

    def prof_reset(self):
        self._check(self._lib.kws_prof_reset(self._h))

    def prof_read(self, kernel_id: int):
        ms, n = C.c_double(), C.c_int()
        self._check(self._lib.kws_prof_read(self._h, int(kernel_id), C.byref(ms), C.byref(n)))
        return ms.value, n.value


def kernel_name(kernel_id: int) -> str:
    return lib().kws_kernel_name(int(kernel_id)).decode()


# -- host-only helpers (no GPU) --------------------------------------------------------------------
def host_mel_edges(nfilt=26, nfft=512, sample_rate=16000) -> np.ndarray:
    out = (C.c_int * (nfilt + 2))()
    rc = lib().kws_host_mel_edges(nfilt, nfft, sample_rate, out)
    if rc != KWS_OK:
        raise KWSError(f"kws_host_mel_edges failed ({rc})")
    return np.array(out[:], dtype=np.int64)


def host_mel_dense(nfilt=26, nfft=512, sample_rate=16000) -> np.ndarray:
    out = np.zeros((nfilt, nfft // 2 + 1), np.float32)
    rc = lib().kws_host_mel_dense(nfilt, nfft, sample_rate, out.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != KWS_OK:
        raise KWSError(f"kws_host_mel_dense failed ({rc})")
    return out


def host_mel_layout(nfilt=26, nfft=512, sample_rate=16000):
    """(first_lane[nfilt+1], n_lanes[nfilt+1], lanes_used, row_safe) of the sparse mel evaluation."""
    first = (C.c_int * (nfilt + 1))()
    count = (C.c_int * (nfilt + 1))()
    used, safe = C.c_int(0), C.c_int(0)
    rc = lib().kws_host_mel_layout(nfilt, nfft, sample_rate, first, count, C.byref(used), C.byref(safe))
    if rc != KWS_OK:
        raise KWSError(f"kws_host_mel_layout failed ({rc})")
    return np.array(first[:], dtype=np.int64), np.array(count[:], dtype=np.int64), int(used.value), bool(safe.value)


def host_dct_lifter(nfilt=26, numcep=10, ceplifter=22) -> np.ndarray:
    out = np.zeros((numcep, nfilt), np.float32)
    rc = lib().kws_host_dct_lifter(nfilt, numcep, ceplifter, out.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != KWS_OK:
        raise KWSError(f"kws_host_dct_lifter failed ({rc})")
    return out


def host_scan_shape(n_total, frame_len=400, frame_step=160, window_frames=99, hop_frames=1):
    """(frames_total, n_windows) of a scan over a recording of ``n_total`` samples (``kws_host_scan_shape``)."""
    frames, windows = C.c_int(0), C.c_int(0)
    rc = lib().kws_host_scan_shape(int(n_total), int(frame_len), int(frame_step), int(window_frames), int(hop_frames),
                                   C.byref(frames), C.byref(windows))
    if rc != KWS_OK:
        raise KWSError(f"kws_host_scan_shape failed ({rc}): sizes must be positive")
    return int(frames.value), int(windows.value)


def _host_i32(v) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(v, dtype=np.int32).reshape(-1))


def _host_i64(v) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(v, dtype=np.int64).reshape(-1))


def _as(a: np.ndarray, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


def _host_f32(v) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(-1))


def _host_truth(truth) -> np.ndarray:
    """An annotation table (or None) as a contiguous int32 [N, 4] copy."""
    t = np.zeros((0, 4), np.int32) if truth is None else np.array(truth, dtype=np.int32)
    if t.size == 0:
        return np.zeros((0, 4), np.int32)
    if t.ndim != 2 or t.shape[1] != 4:
        raise KWSError(f"an annotation table is int32 [N, 4] = (recording, label, first_window, last_window), got shape {t.shape}")
    return np.ascontiguousarray(t)


def host_score_plan(truth, n_recordings, num_classes, first_keyword=2):
    """``kws_host_score_plan``: the annotation table ``truth`` int32 [N, 4] = (recording, label, first_window, last_window)
    validated -> ``(sorted [N, 4], off [R * C + 1])``: the rows by (recording, label, first_window) and where each (recording,
    label) list begins.  ``KWSError`` for a bad row, overlapping rows of one recording and label, or sizes out of range."""
    t = _host_truth(truth)
    n = len(t)
    srt = np.zeros((n, 4), np.int32)
    off = np.zeros(max(int(n_recordings) * int(num_classes), 0) + 1, np.int32)
    rc = lib().kws_host_score_plan(_as(t, C.c_int32) if n else None, n, int(n_recordings), int(num_classes), int(first_keyword),
                                   _as(srt, C.c_int32) if n else None, _as(off, C.c_int32))
    if rc != KWS_OK:
        raise KWSError(f"kws_host_score_plan failed ({rc}): rows need 0 <= recording < R, first_keyword <= label < C <= 64, "
                       "0 <= first_window <= last_window and no overlap within one recording and label; at most 2^24 rows and 2^20 "
                       "recordings")
    return srt, off


def host_ragged_plan(lengths, frame_len=400, frame_step=160, window_frames=99, hop_frames=1):
    """The plan of a ragged batch (``kws_host_ragged_plan``): ``(frames [R], frame_off [R + 1], windows [R], win_off [R], W_pack)``
    as int32 arrays and an int -- each recording's frames and windows as ``host_scan_shape`` gives them, its first row in the
    packed frame array (rows rounded up to ``hop_frames``; ``frame_off[R]`` = F_pack) and its first packed window."""
    ln = _host_i32(lengths)
    R = len(ln)
    frames, frame_off = np.zeros(R, np.int32), np.zeros(R + 1, np.int32)
    windows, win_off, w_pack = np.zeros(R, np.int32), np.zeros(R, np.int32), C.c_int(0)
    rc = lib().kws_host_ragged_plan(_as(ln, C.c_int32), R, int(frame_len), int(frame_step), int(window_frames), int(hop_frames),
                                    _as(frames, C.c_int32), _as(frame_off, C.c_int32), _as(windows, C.c_int32), _as(win_off, C.c_int32),
                                    C.byref(w_pack))
    if rc != KWS_OK:
        raise KWSError(f"kws_host_ragged_plan failed ({rc}): need R >= 1, lengths >= 1 and positive sizes, at most 2^20 recordings "
                       "and 2^28 packed rows")
    return frames, frame_off, windows, win_off, int(w_pack.value)


def host_stream_utt_history(frame_len=400, frame_step=160, pre_roll=60, max_frames=1000, slack_hops=8) -> int:
    """(pre_roll + max_frames - 1 + ceil(frame_len / frame_step) + slack_hops) * frame_step: the samples of history a live
    utterance set keeps per stream (``kws_host_stream_utt_history``)."""
    n = C.c_int(0)
    rc = lib().kws_host_stream_utt_history(int(frame_len), int(frame_step), int(pre_roll), int(max_frames), int(slack_hops), C.byref(n))
    if rc != KWS_OK:
        raise ModelError(f"kws_host_stream_utt_history({frame_len}, {frame_step}, {pre_roll}, {max_frames}, {slack_hops}) failed (code {rc})")
    return int(n.value)


def host_resample_len(n_in, rate_in, rate_out) -> int:
    """ceil(n_in * up / down): the natural length of ``n_in`` samples at ``rate_in`` once at ``rate_out`` (``kws_host_resample_len``)."""
    n = C.c_int(0)
    rc = lib().kws_host_resample_len(int(n_in), int(rate_in), int(rate_out), C.byref(n))
    if rc != KWS_OK:
        raise AudioProcessingError(f"kws_host_resample_len({n_in}, {rate_in}, {rate_out}) failed (code {rc})")
    return int(n.value)


def host_stream_resample_plan(rate_in, rate_out):
    """(up, down, delay, history) of the streaming resampler: the reduced pair, the delay d in output samples and the input
    samples H a stream keeps (``kws_host_stream_resample_plan``)."""
    v = [C.c_int(0) for _ in range(4)]
    rc = lib().kws_host_stream_resample_plan(int(rate_in), int(rate_out), *(C.byref(x) for x in v))
    if rc != KWS_OK:
        raise AudioProcessingError(f"kws_host_stream_resample_plan({rate_in}, {rate_out}) failed (code {rc})")
    return tuple(x.value for x in v)


def host_stream_resample_count(rate_in, rate_out, samples_before, n_in) -> int:
    """floor((P + n_in) up / down) - floor(P up / down): what a push of ``n_in`` samples emits after ``samples_before`` = P
    samples (``kws_host_stream_resample_count``)."""
    n = C.c_int(0)
    rc = lib().kws_host_stream_resample_count(int(rate_in), int(rate_out), C.c_uint64(int(samples_before)), int(n_in), C.byref(n))
    if rc != KWS_OK:
        raise AudioProcessingError(f"kws_host_stream_resample_count({rate_in}, {rate_out}, {samples_before}, {n_in}) failed (code {rc})")
    return n.value


def host_resample_design(rate_in, rate_out):
    """(up, down, half_len, outputs_per_workgroup, taps float64 [2 * half_len + 1]) of a rate pair: the taps the device table
    holds and the tile of the kernel (``kws_host_resample_design``)."""
    up, down, half, tile, need = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_size_t(0)
    fn = lib().kws_host_resample_design
    rc = fn(int(rate_in), int(rate_out), C.byref(up), C.byref(down), C.byref(half), C.byref(tile), None, 0, C.byref(need))
    if rc == KWS_OK:
        taps = np.empty(need.value, np.float64)
        rc = fn(int(rate_in), int(rate_out), None, None, None, None, taps.ctypes.data_as(C.POINTER(C.c_double)), taps.size, None)
    if rc != KWS_OK:
        raise AudioProcessingError(f"{lib().kws_last_error(None).decode()} (code {rc})")
    return int(up.value), int(down.value), int(half.value), int(tile.value), taps


def _host_image(fn, n_scalars, blob, *dims):
    blob = np.ascontiguousarray(blob, dtype=np.float32)
    bp, need = blob.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(0)
    rc = fn(bp, blob.size, *dims, None, 0, C.byref(need), None)
    if rc != KWS_OK:
        raise ModelError(f"{lib().kws_last_error(None).decode()} (code {rc})")
    words, scalars = np.empty(need.value, np.uint32), np.empty(n_scalars, np.float32)
    rc = fn(bp, blob.size, *dims, words.ctypes.data_as(C.POINTER(C.c_uint32)), words.size, None,
            scalars.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != KWS_OK:
        raise ModelError(f"{lib().kws_last_error(None).decode()} (code {rc})")
    return words, scalars


def host_dscnn_image(blob: np.ndarray, num_classes: int, input_channels: int = 1):
    """(words uint32, scalars float32[23]): the device image ``Context.load_dscnn`` uploads for this blob and the values the context
    keeps by value -- k_c1, k_pw[4], c1_abs, c1_bmax, dw_abs[4], dw_bmax[4], pw_abs[4], pw_bmax[4] (``kws_host_dscnn_image``)."""
    return _host_image(lib().kws_host_dscnn_image, 23, blob, int(num_classes), int(input_channels))


def host_dscnn_units():
    """(words uint32 [units, 2, 64, 4], unit_base int32[5]): the unit descriptor table a DS-CNN load places behind the device image
    for the persistent batched forward, and the first unit of blocks 1..4 followed by the unit count (``kws_host_dscnn_units``)."""
    need, base = C.c_size_t(0), np.zeros(5, np.int32)
    bp = base.ctypes.data_as(C.POINTER(C.c_int))
    rc = lib().kws_host_dscnn_units(None, 0, C.byref(need), bp)
    if rc != KWS_OK:
        raise KWSError(f"kws_host_dscnn_units failed ({rc})")
    words = np.empty(need.value, np.uint32)
    rc = lib().kws_host_dscnn_units(words.ctypes.data_as(C.POINTER(C.c_uint32)), words.size, None, bp)
    if rc != KWS_OK:
        raise KWSError(f"kws_host_dscnn_units failed ({rc})")
    return words.reshape(-1, 2, 64, 4), base


def dscnn_bn_blob_layout(num_classes: int):
    """The blob of the BatchNorm DS-CNN's training entries as ``[(name, offset, floats)]`` in blob order (the mirror of
    ``DscnnBnLayout``, csrc/kws_pack.h): ``DepthwiseSeparableConvBN.named_parameters()``."""
    sizes = [("plain.conv1.weight", 6400), ("plain.conv1.bias", 64)]
    for k in range(1, 5):
        sizes += [(f"plain.dsconv{k}.depthwise.weight", 576), (f"plain.dsconv{k}.depthwise.bias", 64),
                  (f"plain.dsconv{k}.pointwise.weight", 4096), (f"plain.dsconv{k}.pointwise.bias", 64)]
    sizes += [("plain.fc.weight", 64 * int(num_classes)), ("plain.fc.bias", int(num_classes))]
    for mod in ["bn_conv1"] + [f"bn_dw.{i}" for i in range(4)] + [f"bn_pw.{i}" for i in range(4)]:
        sizes += [(f"{mod}.weight", 64), (f"{mod}.bias", 64)]
    out, off = [], 0
    for name, n in sizes:
        out.append((name, off, n))
        off += n
    return out


def host_dscnn_bn_max_batch(T: int, F: int) -> int:
    """The largest batch the BatchNorm DS-CNN's training entries take on a ``T x F`` map (``kws_host_dscnn_bn_max_batch``)."""
    return int(lib().kws_host_dscnn_bn_max_batch(int(T), int(F)))


def host_cnn_trad_window_chunk() -> int:
    """Windows per launch pair of ``Context.forward_cnn_trad_windows_f32`` (``kws_host_cnn_trad_window_chunk``)."""
    return int(lib().kws_host_cnn_trad_window_chunk())


def host_cnn_trad_image(blob: np.ndarray, num_classes: int):
    """(words uint32, scalars float32[7]): the device image ``Context.load_cnn_trad`` uploads for this blob and 1/sw of conv1,
    conv2, lin, w1_abs, b1_max, w2_abs, b2_max (``kws_host_cnn_trad_image``)."""
    return _host_image(lib().kws_host_cnn_trad_image, 7, blob, int(num_classes))


_contexts: dict = {}


def default_context(device: int = 0) -> Context:
    """Process-wide context per GPU, bound to torch's current stream at each use by the callers."""
    ctx = _contexts.get(device)
    if ctx is None:
        ctx = _contexts[device] = Context(device)
    return ctx
