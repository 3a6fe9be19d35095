// C ABI of libkws_hip.so (declared in include/kws_hip.h): context, the forward, streaming and cnn-trad-fpool3 entry points and
// per-kernel event timing.  The front end's entries are in kws_frontend.hip, the weight images in kws_weights.hip.  No torch
// types, no exceptions across the boundary, no CPU fallback.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>

#include "kws_event_queue.h"  // spin_until

namespace kws {

const char* const kKernelNames[KWS_K_COUNT] = {"kws_mfcc_i16_kernel", "kws_dscnn_fwd_kernel", "kws_cnntrad_conv_kernel",
                                               "kws_cnntrad_dense_kernel", "kws_stream_frame_kernel", "kws_mfcc_f64_kernel",
                                               "kws_mfcc_refine_kernel", "kws_ds_load_stats_kernel", "kws_ds_load_pack_kernel",
                                               "kws_ds_load_fill_kernel", "kws_resample_kernel"};

}  // namespace kws

using namespace kws;

// Streaming state: the zero-copy result buffers, then everything kws_stream_open allocates (kws_set_frontend retires it too).
static void host_results_free(kws_ctx* c) {
    if (c->h_stream_logits) (void)hipHostFree(c->h_stream_logits);
    if (c->h_stream_label) (void)hipHostFree(c->h_stream_label);
    if (c->h_stream_flag) (void)hipHostFree(c->h_stream_flag);
    if (c->h_stream_hop) (void)hipHostFree(c->h_stream_hop);
    if (c->d_hr_logits) (void)hipFree(c->d_hr_logits);
    if (c->d_hr_label) (void)hipFree(c->d_hr_label);
    c->h_stream_hop = nullptr;
    c->d_hr_logits = nullptr;
    c->d_hr_label = nullptr;
    c->h_stream_logits = nullptr;
    c->h_stream_label = nullptr;
    c->h_stream_flag = nullptr;
    c->host_results_classes = 0;
}

void stream_free(kws_ctx* c) {
    smooth_free(c);
    vad_free(c);
    stream_utt_free(c);  // live utterances (kws_live.hip)
    stream_detect_free(c);  // live keyword events (kws_live_detect.hip)
    host_results_free(c);
    if (c->stream_graph) (void)hipGraphExecDestroy(c->stream_graph);
    if (c->d_pcm_ring) (void)hipFree(c->d_pcm_ring);
    if (c->d_feat_ring) (void)hipFree(c->d_feat_ring);
    if (c->d_hops) (void)hipFree(c->d_hops);
    if (c->d_cl_part) (void)hipFree(c->d_cl_part);
    if (c->d_cl_count) (void)hipFree(c->d_cl_count);
    c->d_cl_part = nullptr;
    c->d_cl_count = nullptr;
    c->stream_graph = nullptr;
    c->d_pcm_ring = nullptr;
    c->d_feat_ring = nullptr;
    c->d_hops = nullptr;
    c->n_streams = 0;
}

#pragma GCC visibility push(default)
extern "C" {

int kws_abi_version(void) { return KWS_ABI_VERSION; }

const char* kws_last_error(kws_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

const char* kws_kernel_name(int id) { return (id >= 0 && id < KWS_K_COUNT) ? kKernelNames[id] : ""; }

int kws_create(kws_ctx** out, int device_id) {
    KWS_GUARD_BEGIN
    if (!out) return fail(nullptr, KWS_EINVAL, "kws_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, KWS_EHIP, std::string("kws_create: no HIP device (") + hipGetErrorString(e) + "); there is no CPU fallback");
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, KWS_EINVAL, "kws_create: device_id out of range");
    kws_ctx* c = new (std::nothrow) kws_ctx();
    if (!c) return fail(nullptr, KWS_ENOMEM, "kws_create: out of host memory");
    c->device = device_id;
    e = hipSetDevice(device_id);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = dscnn_init_device();
    if (e == hipSuccess) e = cnntrad_init_device();
    if (e == hipSuccess) {
        hipDeviceProp_t prop;
        e = hipGetDeviceProperties(&prop, device_id);
        if (e == hipSuccess) c->n_cu = prop.multiProcessorCount;
    }
    if (e != hipSuccess) {
        int rc = fail_hip(nullptr, e, "kws_create");
        if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
        delete c;
        return rc;
    }
    c->stream = c->own_stream;
    int rc = kws_set_frontend(c, 16000, 16000, 400, 160, 512, 26, 10, 0.97f, 22);
    if (rc != KWS_OK) {
        g_create_err = c->err;
        kws_destroy(c);
        return rc;
    }
    *out = c;
    return KWS_OK;
    KWS_GUARD_END(nullptr, "kws_create")
}

void kws_destroy(kws_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (int k = 0; k < KWS_K_COUNT; ++k)
        for (auto& p : c->ev[k]) {
            (void)hipEventDestroy(p.a);
            (void)hipEventDestroy(p.b);
        }
    if (c->d_fe) (void)hipFree(c->d_fe);
    if (c->d_spec_tw64) (void)hipFree(c->d_spec_tw64);
    if (c->d_refine) (void)hipFree(c->d_refine);
    if (c->d_model) (void)hipFree(c->d_model);
    if (c->d_cnntrad) (void)hipFree(c->d_cnntrad);
    if (c->d_ct_stats) (void)hipFree(c->d_ct_stats);
    if (c->d_ds_stats) (void)hipFree(c->d_ds_stats);
    if (c->d_conv_ws) (void)hipFree(c->d_conv_ws);
    if (c->d_train_ws) (void)hipFree(c->d_train_ws);
    if (c->d_feat_ws) (void)hipFree(c->d_feat_ws);
    if (c->d_scan_ws) (void)hipFree(c->d_scan_ws);
    if (c->d_ragged) (void)hipFree(c->d_ragged);
    stream_free(c);     // rings, hop counter, captured graph, smoothing and endpointer history (kws_decide.hip)
    eval_free(c);        // evaluation accumulators (kws_eval.hip)
    stream_resample_free(c);  // streaming resampler: history, hop buffer, pinned input (kws_resample.hip)
    resample_free(c);    // tap tables of the rate pairs (kws_resample.hip)
    ingest_free(c);      // staging rings, copy streams, pack threads
    if (c->order_ev) (void)hipEventDestroy(c->order_ev);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

// The workspaces and tables of a context are shared by everything it enqueues, so work enqueued on the new stream must
// not overtake work still pending on the old one: the new stream waits on an event recorded on the old stream.  (A
// context is still single-threaded and serves one stream at a time; this only makes the hand-over safe.)
int kws_set_stream(kws_ctx* c, void* hip_stream, int external) {
    if (!c) return KWS_EINVAL;
    hipStream_t next = external ? (hipStream_t)hip_stream : c->own_stream;
    if (next == c->stream) return KWS_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->order_ev) HIP_TRY(c, hipEventCreateWithFlags(&c->order_ev, hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(c->order_ev, c->stream));
    HIP_TRY(c, hipStreamWaitEvent(next, c->order_ev, 0));
    if (c->stream_graph) {  // a captured push replays on the stream it was captured for: retire it once it is idle
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        drop_stream_graph(c);
    }
    c->stream = next;
    return KWS_OK;
}

int kws_sync(kws_ctx* c) {
    if (!c) return KWS_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return KWS_OK;
}

static int grow_conv_ws(kws_ctx* c, size_t need, const std::string& fn);

static int forward_impl(kws_ctx* c, const float* d_feat, int B, float* d_logits, int32_t* d_label, float* d_act,
                        int mode, const char* fn, unsigned long long* d_stamps = nullptr) {
    int rc = check_batch(c, d_feat, B, fn);
    if (rc) return rc;
    if (!d_logits) return fail(c, KWS_EINVAL, std::string(fn) + ": d_logits is NULL");
    if (!c->model_ready) return fail(c, KWS_ESTATE, std::string(fn) + ": no model loaded (kws_load_dscnn)");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->mw.in_channels > 1) {
        // multi-channel input (models.py:125,135): conv1 in its own kernel through the context scratch, then the fused
        // kernel from block 1 on; the diagnostics variants exist for the single-channel model only
        if (d_act || d_stamps || (mode != KWS_PW_SPLIT_BF16 && mode != KWS_PW_PAIR_F16))
            return fail(c, KWS_EUNSUPPORTED, std::string(fn) + ": input_channels > 1 runs on the product kernels only");
        rc = grow_conv_ws(c, (size_t)B * 64 * 141, fn);
        if (rc) return rc;
        HIP_TRY(c, launch_conv1_general(c->stream, d_feat, B, c->mw.in_channels, c->mw.c1_general, c->mw.c1_b, c->d_conv_ws));
        ProfScope ps(c, KWS_K_DSCNN);
        HIP_TRY(c, launch_dscnn(c->stream, c->mw, c->d_conv_ws, B, d_logits, d_label, nullptr, mode, nullptr, nullptr, true));
        return KWS_OK;
    }
    ProfScope ps(c, KWS_K_DSCNN);
    HIP_TRY(c, launch_dscnn(c->stream, c->mw, d_feat, B, d_logits, d_label, d_act, mode, d_stamps, nullptr, false, 3, c->n_cu));
    return KWS_OK;
}

int kws_forward_f32(kws_ctx* c, const float* d_feat, int B, float* d_logits, int32_t* d_label) {
    return forward_impl(c, d_feat, B, d_logits, d_label, nullptr, c ? c->pw_math : 0, "kws_forward_f32");
}

// DepthwiseSeparableConv.forward on a feature map of any size (models.py:160-183): T x F == 99 x 10 takes the fused
// LDS-resident kernel, anything else runs composed through HBM -- conv1 -> four depthwise-separable blocks (the standalone
// block kernels, each adding its relu(bias) ring) -> global average pool + fc + argmax.
static int forward_map_impl(kws_ctx* c, const float* d_feat, int B, int T, int F, float* d_logits, int32_t* d_label, float* d_layers,
                            const char* fn) {
    int rc = check_batch(c, d_feat, B, fn);
    if (rc) return rc;
    if (!d_logits) return fail(c, KWS_EINVAL, std::string(fn) + ": d_logits is NULL");
    if (!c->model_ready) return fail(c, KWS_ESTATE, std::string(fn) + ": no model loaded (kws_load_dscnn)");
    if (T == IN_T && F == IN_F && !d_layers) return forward_impl(c, d_feat, B, d_logits, d_label, nullptr, c->pw_math, fn);
    rc = check_dscnn_map(c, fn, T, F);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const DscnnMap m(T, F);
    const int Cin = c->mw.in_channels, C = c->mw.num_classes, LAST = N_BLOCKS - 1;
    const size_t per_clip_max = CH * m.Q(LAST);                            // block 4's output, ring included
    const size_t dw_max = CH * m.P(LAST);                                  // block 4's depthwise output
    const int chunk = B < COMPOSED_MAX_CLIPS ? B : COMPOSED_MAX_CLIPS;     // a bounded workspace
    rc = grow_conv_ws(c, (size_t)chunk * (2 * per_clip_max + dw_max), fn);
    if (rc) return rc;
    float* bufs[2] = {c->d_conv_ws, c->d_conv_ws + (size_t)chunk * per_clip_max};
    float* dw_ws = c->d_conv_ws + 2 * (size_t)chunk * per_clip_max;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = B - b0 < chunk ? B - b0 : chunk;
        // the stages ping-pong between the two buffers; the diagnostics entry keeps them in d_layers instead, stage-major with the
        // batch inside: stage i of this chunk is the run [nb][per_clip] at lo * B + b0 * per_clip, lo = the per-clip floats before it
        DscnnStages st;
        size_t lo = 0;
        for (int i = 0; i <= N_BLOCKS; ++i) {
            const size_t per_clip = CH * m.P(i);
            float*& stage = i ? st.y[i - 1] : st.a0;
            stage = d_layers ? d_layers + lo * B + (size_t)b0 * per_clip : bufs[i & 1];
            if (i < N_BLOCKS) st.dw[i] = dw_ws;
            lo += per_clip;
        }
        HIP_TRY(c, launch_dscnn_composed(c->stream, c->mw, d_feat + (size_t)b0 * Cin * T * F, nb, T, F, st));
        HIP_TRY(c, launch_pool_fc(c->stream, st.y[LAST], nb, (int)m.Q(LAST), c->mw.fc_w, c->mw.fc_b, C, d_logits + (size_t)b0 * C,
                                  d_label ? d_label + b0 : nullptr));
    }
    return KWS_OK;
}

int kws_forward_map_f32(kws_ctx* c, const float* d_feat, int B, int T, int F, float* d_logits, int32_t* d_label) {
    return forward_map_impl(c, d_feat, B, T, F, d_logits, d_label, nullptr, "kws_forward_map_f32");
}

int kws_forward_map_debug_f32(kws_ctx* c, const float* d_feat, int B, int T, int F, float* d_logits, int32_t* d_label, float* d_layers) {
    if (c && !d_layers) return fail(c, KWS_EINVAL, "kws_forward_map_debug_f32: d_layers is NULL");
    return forward_map_impl(c, d_feat, B, T, F, d_logits, d_label, d_layers, "kws_forward_map_debug_f32");
}

int kws_set_pointwise_math(kws_ctx* c, int math) {
    if (!c) return KWS_EINVAL;
    if (math != KWS_PW_F32 && math != KWS_PW_SPLIT_BF16 && math != KWS_PW_PAIR_F16)
        return fail(c, KWS_EINVAL, "kws_set_pointwise_math: math must be KWS_PW_F32, KWS_PW_SPLIT_BF16 or KWS_PW_PAIR_F16");
    if (math != c->pw_math && c->stream_graph) {  // the captured graph holds the other kernel
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        drop_stream_graph(c);
    }
    c->pw_math = math;
    return KWS_OK;
}

int kws_forward_debug_f32(kws_ctx* c, const float* d_feat, int B, float* d_logits, int32_t* d_label, float* d_act,
                          int use_mfma) {
    if (c && use_mfma != 0 && use_mfma != KWS_PW_F32 && use_mfma != KWS_PW_SPLIT_BF16 && use_mfma != KWS_PW_PAIR_F16)
        return fail(c, KWS_EINVAL, "kws_forward_debug_f32: use_mfma must be 0, KWS_PW_F32, KWS_PW_SPLIT_BF16 or KWS_PW_PAIR_F16");
    return forward_impl(c, d_feat, B, d_logits, d_label, d_act, use_mfma, "kws_forward_debug_f32");
}

int kws_forward_stamps_f32(kws_ctx* c, const float* d_feat, int B, float* d_logits, uint64_t* d_stamps, int mode) {
    if (!d_stamps) return fail(c, KWS_EINVAL, "kws_forward_stamps_f32: d_stamps is NULL");
    if (mode != 0 && mode != 1 && mode != 2 && mode != 3 && mode != 4 && mode != 5 && mode != 6)
        return fail(c, KWS_EINVAL, "kws_forward_stamps_f32: unknown kernel variant");
    return forward_impl(c, d_feat, B, d_logits, nullptr, nullptr, mode, "kws_forward_stamps_f32",
                        reinterpret_cast<unsigned long long*>(d_stamps));
}

int kws_infer_i16(kws_ctx* c, const int16_t* d_wav, int B, float* d_logits, int32_t* d_label) {
    int rc = check_batch(c, d_wav, B, "kws_infer_i16");
    if (rc) return rc;
    if (!c->fe_ready || !c->model_ready) return fail(c, KWS_ESTATE, "kws_infer_i16: front end or model not configured");
    if (c->mw.in_channels != 1) return fail(c, KWS_EUNSUPPORTED, "kws_infer_i16: the MFCC front end yields one channel; the model was loaded with more");
    rc = kws_reserve(c, B);
    if (rc) return rc;
    rc = kws_mfcc_i16(c, d_wav, B, c->d_feat_ws);
    if (rc) return rc;
    // 99 x 10 (the reference geometry): the fused kernel; any other map kws_frontend_shape yields: the composed path
    return forward_map_impl(c, c->d_feat_ws, B, c->fp.num_frames, c->fp.numcep, d_logits, d_label, nullptr, "kws_infer_i16");
}

int kws_infer_f32(kws_ctx* c, const float* d_wav, int B, float* d_logits, int32_t* d_label) {
    int rc = check_batch(c, d_wav, B, "kws_infer_f32");
    if (rc) return rc;
    if (!c->fe_ready || !c->model_ready) return fail(c, KWS_ESTATE, "kws_infer_f32: front end or model not configured");
    if (c->mw.in_channels != 1) return fail(c, KWS_EUNSUPPORTED, "kws_infer_f32: the MFCC front end yields one channel; the model was loaded with more");
    rc = kws_reserve(c, B);
    if (rc) return rc;
    rc = kws_mfcc_f32(c, d_wav, B, c->d_feat_ws);
    if (rc) return rc;
    return forward_map_impl(c, c->d_feat_ws, B, c->fp.num_frames, c->fp.numcep, d_logits, d_label, nullptr, "kws_infer_f32");
}

// ---- streaming ------------------------------------------------------------------------------------
int kws_stream_open(kws_ctx* c, int n_streams) {
    if (!c) return KWS_EINVAL;
    if (n_streams <= 0) return fail(c, KWS_EINVAL, "kws_stream_open: n_streams must be positive");
    if (!c->fe_ready) return fail(c, KWS_ESTATE, "kws_stream_open: front end not configured");
    if (!c->fe_fast_ok)
        return fail(c, KWS_EUNSUPPORTED, "kws_stream_open: the streaming frame kernel is float32 only (nfft == 512, frames of at most 512 samples, a filterbank and a hop the float32 kernel covers)");
    if (c->fp.frame_step > 512) return fail(c, KWS_EUNSUPPORTED, "kws_stream_open: hops of more than 512 samples are not supported");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    stream_free(c);
    const FrontendParams& p = c->fp;
    c->ring_len = (frames_lag(p) + 1) * p.frame_step;
    const size_t pcm_b = sizeof(int16_t) * (size_t)n_streams * c->ring_len;
    const size_t feat_b = sizeof(float) * (size_t)n_streams * p.num_frames * p.numcep;
    if (hipMalloc(reinterpret_cast<void**>(&c->d_pcm_ring), pcm_b) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&c->d_feat_ring), feat_b) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&c->d_hops), 2 * sizeof(int)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&c->d_cl_part), sizeof(float) * (size_t)n_streams * 4 * 64) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&c->d_cl_count), sizeof(int) * (size_t)n_streams) != hipSuccess) {
        stream_free(c);
        return fail(c, KWS_ENOMEM, "kws_stream_open: device allocation failed");
    }
    c->n_streams = n_streams;
    c->pushes_enqueued = 0;
    c->host_push = 0;
    c->last_push_host = false;
    if (c->refine_span > 0.f) {  // the pushes count the frames they redo in float64 in the refinement counters
        int rc = ensure_refine(c, 1, c->fp.num_frames);
        if (rc) return rc;
    }
    HIP_TRY(c, hipMemsetAsync(c->d_pcm_ring, 0, pcm_b, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_feat_ring, 0, feat_b, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_hops, 0, 2 * sizeof(int), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_cl_count, 0, sizeof(int) * (size_t)n_streams, c->stream));
    return KWS_OK;
}

int kws_stream_host_results(kws_ctx* c, int enable) {
    if (!c) return KWS_EINVAL;
    if (!c->n_streams) return fail(c, KWS_ESTATE, "kws_stream_host_results: call kws_stream_open first");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    host_results_free(c);
    if (!enable) return KWS_OK;
    if (!c->model_ready) return fail(c, KWS_ESTATE, "kws_stream_host_results: no model loaded (kws_load_dscnn)");
    const int C = c->mw.num_classes;
    const unsigned flags = hipHostMallocMapped | hipHostMallocCoherent;  // fine-grained: device stores are visible to the host as they land
    if (hipHostMalloc(reinterpret_cast<void**>(&c->h_stream_logits), sizeof(float) * (size_t)c->n_streams * C, flags) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&c->h_stream_label), sizeof(int32_t) * (size_t)c->n_streams, flags) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&c->h_stream_flag), 64, flags) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&c->h_stream_hop), sizeof(int16_t) * (size_t)c->n_streams * c->fp.frame_step, flags) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&c->d_hr_logits), sizeof(float) * (size_t)c->n_streams * C) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&c->d_hr_label), sizeof(int32_t) * (size_t)c->n_streams) != hipSuccess) {
        host_results_free(c);
        return fail(c, KWS_ENOMEM, "kws_stream_host_results: pinned host allocation failed");
    }
    memset(c->h_stream_logits, 0, sizeof(float) * (size_t)c->n_streams * C);
    memset(c->h_stream_label, 0, sizeof(int32_t) * (size_t)c->n_streams);
    // the flag holds the device's push count: start it where the device stands
    int hops = 0;
    HIP_TRY(c, hipMemcpy(&hops, c->d_hops, sizeof(int), hipMemcpyDeviceToHost));
    *c->h_stream_flag = hops;
    c->pushes_enqueued = hops;
    c->host_push = hops;
    c->host_results_classes = C;
    return KWS_OK;
}

int kws_stream_wait_host(kws_ctx* c, const float** h_logits, const int32_t** h_label) {
    if (!c) return KWS_EINVAL;
    if (!c->h_stream_flag) return fail(c, KWS_ESTATE, "kws_stream_wait_host: call kws_stream_host_results(ctx, 1) first");
    // the pinned arrays hold the class count loaded when they were made: a push under another model delivered nothing to them
    if (c->host_results_classes != c->mw.num_classes)
        return fail(c, KWS_ESTATE, "kws_stream_wait_host: the class count changed (" + std::to_string(c->host_results_classes) + " -> " +
                                       std::to_string(c->mw.num_classes) + ") since kws_stream_host_results; call it again, or push with kws_stream_push_host_i16");
    // spin on the flag the last workgroup of the newest push raises; bounded: after ~2 ms without it, fall back to the stream
    if (c->host_push != c->pushes_enqueued)
        return fail(c, KWS_ESTATE, "kws_stream_wait_host: the newest push did not deliver to host memory (it asked for no logits, or took a multi-launch route)");
    volatile int* flag = c->h_stream_flag;
    const int want = c->host_push;
    if (!spin_until([&] { return *flag - want >= 0; })) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (*flag - want < 0) return fail(c, KWS_EHIP, "kws_stream_wait_host: the stream drained but the results flag never arrived");
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (h_logits) *h_logits = c->h_stream_logits;
    if (h_label) *h_label = c->h_stream_label;
    return KWS_OK;
}

int kws_stream_push_host_i16(kws_ctx* c, const int16_t* h_hop, const float** h_logits, const int32_t** h_label) {
    if (!c) return KWS_EINVAL;
    if (!c->n_streams) return fail(c, KWS_ESTATE, "kws_stream_push_host_i16: call kws_stream_open first");
    if (!h_hop) return fail(c, KWS_EINVAL, "kws_stream_push_host_i16: h_hop is NULL");
    if (int rc = host_results_ensure(c)) return rc;
    // the hop goes into pinned, device-mapped memory and the kernel reads it from there (one PCIe read of 320 bytes per stream
    // on the frame wavefront's path) -- no H2D submission in front of the launch.  One slot: this call returns after the
    // kernel's last workgroup has raised the flag, i.e. after every read of it.
    memcpy(c->h_stream_hop, h_hop, sizeof(int16_t) * (size_t)c->n_streams * c->fp.frame_step);
    int rc = kws_stream_push_i16(c, c->h_stream_hop, c->d_hr_logits, c->d_hr_label, 0);
    if (rc) return rc;
    return kws_stream_wait_host(c, h_logits, h_label);
}

int kws_stream_cluster(kws_ctx* c, int workgroups_per_stream) {
    if (!c) return KWS_EINVAL;
    if (workgroups_per_stream != 0 && workgroups_per_stream != 1 && workgroups_per_stream != 2 && workgroups_per_stream != 4)
        return fail(c, KWS_EINVAL, "kws_stream_cluster: workgroups_per_stream must be 0 (automatic), 1, 2 or 4");
    if (workgroups_per_stream != c->stream_cluster && c->stream_graph) {  // the captured graph holds the other launch shape
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        drop_stream_graph(c);
    }
    c->stream_cluster = workgroups_per_stream;
    return KWS_OK;
}

// Grow the context's float scratch (convolution outputs between two kernels of one call) to at least `need` floats.
static int grow_conv_ws(kws_ctx* c, size_t need, const std::string& fn) {
    return grow_device_buffer(c, c->d_conv_ws, c->conv_ws_floats, need, fn.c_str(), "workspace");
}

int kws_dsblock_forward_f32(kws_ctx* c, const float* d_x, int B, int C_in, int H, int W, const float* d_dw_w, const float* d_dw_b,
                            const float* d_pw_w, const float* d_pw_b, int C_out, int kernel_size, int stride, int padding,
                            float* d_out) {
    int rc = check_batch(c, d_x, B, "kws_dsblock_forward_f32");
    if (rc) return rc;
    if (!d_dw_w || !d_dw_b || !d_pw_w || !d_pw_b || !d_out) return fail(c, KWS_EINVAL, "kws_dsblock_forward_f32: NULL pointer");
    if (C_in < 1 || C_out < 1 || H < 1 || W < 1 || kernel_size < 1 || stride < 1 || padding < 0)
        return fail(c, KWS_EINVAL, "kws_dsblock_forward_f32: sizes must be positive (padding >= 0)");
    if (H + 2 * padding < kernel_size || W + 2 * padding < kernel_size)
        return fail(c, KWS_EINVAL, "kws_dsblock_forward_f32: the kernel is larger than the padded input");
    if (B > 65535) return fail(c, KWS_EUNSUPPORTED, "kws_dsblock_forward_f32: B must be <= 65535 per call");
    HIP_TRY(c, hipSetDevice(c->device));
    const int Ho = (H + 2 * padding - kernel_size) / stride + 1, Wo = (W + 2 * padding - kernel_size) / stride + 1;
    rc = grow_conv_ws(c, (size_t)B * C_in * Ho * Wo, "kws_dsblock_forward_f32");
    if (rc) return rc;
    HIP_TRY(c, launch_dsblock(c->stream, d_x, B, C_in, H, W, d_dw_w, d_dw_b, d_pw_w, d_pw_b, C_out, kernel_size, stride, padding,
                              c->d_conv_ws, d_out));
    return KWS_OK;
}

// The two launches of the cnn-trad-fpool3 forward, shared by the product entry and its parity aid (`fn` names the caller in
// error messages).  Workspace: B * 19008 floats of conv2 output, then one scale per clip (f16-pair arithmetic).
static int forward_cnn_trad(kws_ctx* c, const float* d_feat, int B, float* d_logits, int32_t* d_label, const std::string& fn) {
    int rc = check_batch(c, d_feat, B, fn.c_str());
    if (rc) return rc;
    if (!d_logits) return fail(c, KWS_EINVAL, fn + ": d_logits is NULL");
    if (!c->cnntrad_ready) return fail(c, KWS_ESTATE, fn + ": no model loaded (kws_load_cnn_trad)");
    HIP_TRY(c, hipSetDevice(c->device));
    rc = grow_conv_ws(c, (size_t)B * 64 * 297 + (size_t)B, fn);
    if (rc) return rc;
    const bool pair = c->cnntrad_math == KWS_CT_F16_PAIR;
    {
        ProfScope ps(c, KWS_K_CNNTRAD_CONV);
        HIP_TRY(c, launch_cnntrad_conv(c->stream, c->tw, d_feat, B, c->d_conv_ws, pair));
    }
    {
        ProfScope ps(c, KWS_K_CNNTRAD_DENSE);
        HIP_TRY(c, launch_cnntrad_dense(c->stream, c->tw, c->d_conv_ws, B, d_logits, d_label, pair));
    }
    return KWS_OK;
}

// cnn-trad-fpool3 behind the recording flows (kws_scan_cnn_trad_*, kws_scan_ragged_cnn_trad_*; ScanModel, kws_ctx.h)
static int cnntrad_windows_launch(kws_ctx* c, const std::string& fn, const float* d_frames, int R, int F, int W, int hop_frames,
                                  float* d_logits, int32_t* d_label);
static int cnntrad_scan_check(kws_ctx* c, const std::string& f) {
    if (!c->fe_ready || !c->cnntrad_ready) return fail(c, KWS_ESTATE, f + ": front end or model not configured (kws_load_cnn_trad)");
    if (c->fp.num_frames != IN_T || c->fp.numcep != IN_F)
        return fail(c, KWS_EUNSUPPORTED, f + ": the kernels are built for a 99 x 10 feature map");
    return KWS_OK;
}
int kws_forward_cnn_trad_f32(kws_ctx* c, const float* d_feat, int B, float* d_logits, int32_t* d_label) {
    return forward_cnn_trad(c, d_feat, B, d_logits, d_label, "kws_forward_cnn_trad_f32");
}

int kws_forward_cnn_trad_debug_f32(kws_ctx* c, const float* d_feat, int B, float* d_logits, int32_t* d_label, float* d_conv2,
                                   float* d_clip_scale) {
    const char* fn = "kws_forward_cnn_trad_debug_f32";
    if (c && !d_conv2) return fail(c, KWS_EINVAL, std::string(fn) + ": d_conv2 is NULL");
    int rc = forward_cnn_trad(c, d_feat, B, d_logits, d_label, fn);
    if (rc) return rc;
    const size_t n = (size_t)B * 64 * 297;
    HIP_TRY(c, hipMemcpyAsync(d_conv2, c->d_conv_ws, sizeof(float) * n, hipMemcpyDeviceToDevice, c->stream));
    if (d_clip_scale && c->cnntrad_math == KWS_CT_F16_PAIR)
        HIP_TRY(c, hipMemcpyAsync(d_clip_scale, c->d_conv_ws + n, sizeof(float) * (size_t)B, hipMemcpyDeviceToDevice, c->stream));
    return KWS_OK;
}

int kws_set_cnn_trad_math(kws_ctx* c, int math) {
    if (!c) return KWS_EINVAL;
    if (math != KWS_CT_F16_PAIR && math != KWS_CT_BF16_TRIPLE) return fail(c, KWS_EINVAL, "kws_set_cnn_trad_math: unknown arithmetic");
    c->cnntrad_math = math;
    return KWS_OK;
}

int kws_infer_cnn_trad_i16(kws_ctx* c, const int16_t* d_wav, int B, float* d_logits, int32_t* d_label) {
    int rc = check_batch(c, d_wav, B, "kws_infer_cnn_trad_i16");
    if (rc) return rc;
    if (!c->fe_ready || !c->cnntrad_ready)
        return fail(c, KWS_ESTATE, "kws_infer_cnn_trad_i16: front end or model not configured (kws_load_cnn_trad)");
    if (c->fp.num_frames != IN_T || c->fp.numcep != IN_F)
        return fail(c, KWS_EUNSUPPORTED, "kws_infer_cnn_trad_i16: the kernels are built for a 99 x 10 feature map");
    rc = kws_reserve(c, B);
    if (rc) return rc;
    rc = kws_mfcc_i16(c, d_wav, B, c->d_feat_ws);
    if (rc) return rc;
    return kws_forward_cnn_trad_f32(c, c->d_feat_ws, B, d_logits, d_label);
}

int kws_infer_cnn_trad_f32(kws_ctx* c, const float* d_wav, int B, float* d_logits, int32_t* d_label) {
    int rc = check_batch(c, d_wav, B, "kws_infer_cnn_trad_f32");
    if (rc) return rc;
    if (!c->fe_ready || !c->cnntrad_ready)
        return fail(c, KWS_ESTATE, "kws_infer_cnn_trad_f32: front end or model not configured (kws_load_cnn_trad)");
    if (c->fp.num_frames != IN_T || c->fp.numcep != IN_F)
        return fail(c, KWS_EUNSUPPORTED, "kws_infer_cnn_trad_f32: the kernels are built for a 99 x 10 feature map");
    rc = kws_reserve(c, B);
    if (rc) return rc;
    rc = kws_mfcc_f32(c, d_wav, B, c->d_feat_ws);
    if (rc) return rc;
    return forward_cnn_trad(c, c->d_feat_ws, B, d_logits, d_label, "kws_infer_cnn_trad_f32");
}

int kws_host_cnn_trad_window_chunk(void) { return CT_WINDOW_CHUNK; }

// The R * W windows of a frame array [R][F][10], read in place, in chunks of CT_WINDOW_CHUNK: per chunk one conv launch into the
// context workspace (a chunk's 19008 floats + 1 scale per window) and one dense launch that writes logits and labels at the
// chunk's offset.  The caller has checked the arguments and the limits (R * F <= 2^28, R * W <= 2^30).
static int cnntrad_windows_launch(kws_ctx* c, const std::string& fn, const float* d_frames, int R, int F, int W, int hop_frames,
                                  float* d_logits, int32_t* d_label) {
    const long long n = (long long)R * W;
    const int chunk = n < CT_WINDOW_CHUNK ? (int)n : CT_WINDOW_CHUNK;
    int rc = grow_conv_ws(c, (size_t)chunk * 64 * 297 + (size_t)chunk, fn);
    if (rc) return rc;
    const bool pair = c->cnntrad_math == KWS_CT_F16_PAIR;
    const int C = c->tw.num_classes;
    for (long long i0 = 0; i0 < n; i0 += chunk) {
        const int nb = n - i0 < chunk ? (int)(n - i0) : chunk;
        const CtWindows sw = {(unsigned)i0, (unsigned)W, (unsigned)F * (unsigned)IN_F, (unsigned)hop_frames * (unsigned)IN_F};
        {
            ProfScope ps(c, KWS_K_CNNTRAD_CONV);
            HIP_TRY(c, launch_cnntrad_conv_windows(c->stream, c->tw, d_frames, sw, nb, c->d_conv_ws, pair));
        }
        {
            ProfScope ps(c, KWS_K_CNNTRAD_DENSE);
            HIP_TRY(c, launch_cnntrad_dense(c->stream, c->tw, c->d_conv_ws, nb, d_logits + (size_t)i0 * C, d_label ? d_label + i0 : nullptr, pair));
        }
    }
    return KWS_OK;
}

int kws_forward_cnn_trad_windows_f32(kws_ctx* c, const float* d_frames, int R, int F, int hop_frames, float* d_logits, int32_t* d_label) {
    const std::string fn = "kws_forward_cnn_trad_windows_f32";
    if (!c) return KWS_EINVAL;
    if (!d_frames || !d_logits) return fail(c, KWS_EINVAL, fn + ": d_frames / d_logits is NULL");
    if (R < 1 || hop_frames < 1) return fail(c, KWS_EINVAL, fn + ": R and hop_frames must be positive");
    if (F < IN_T) return fail(c, KWS_EINVAL, fn + ": a recording of fewer than 99 frames has no window");
    if (!c->cnntrad_ready) return fail(c, KWS_ESTATE, fn + ": no model loaded (kws_load_cnn_trad)");
    const int W = (F - IN_T) / hop_frames + 1;
    if ((unsigned long long)R * F > (1ull << 28) || (unsigned long long)R * W > (1ull << 30))
        return fail(c, KWS_EUNSUPPORTED, fn + ": more than 2^28 frames or 2^30 windows in one call");
    HIP_TRY(c, hipSetDevice(c->device));
    return cnntrad_windows_launch(c, fn, d_frames, R, F, W, hop_frames, d_logits, d_label);
}

// The push of a cnn-trad-fpool3 context: the frame kernel advances the rings and the hop counter, the conv kernel reads every
// stream's window from the feature ring in place (RING), the dense kernel writes logits and labels.  Three launches, no graph,
// no zero-copy delivery; the armed steps run behind them as behind kws_stream_push_i16.
int kws_stream_push_cnn_trad_i16(kws_ctx* c, const int16_t* d_hop, float* d_logits, int32_t* d_label) {
    const char* fn = "kws_stream_push_cnn_trad_i16";
    if (!c) return KWS_EINVAL;
    if (!c->n_streams) return fail(c, KWS_ESTATE, std::string(fn) + ": call kws_stream_open first");
    if (!d_hop || !d_logits) return fail(c, KWS_EINVAL, std::string(fn) + ": d_hop / d_logits is NULL");
    if (!c->cnntrad_ready) return fail(c, KWS_ESTATE, std::string(fn) + ": no model loaded (kws_load_cnn_trad)");
    if (c->fp.num_frames != IN_T || c->fp.numcep != IN_F)
        return fail(c, KWS_EUNSUPPORTED, std::string(fn) + ": the kernels are built for a 99 x 10 feature map");
    if (int rc = stream_utt_push_check(c, fn)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const int S = c->n_streams;
    if (int rc = grow_conv_ws(c, (size_t)S * 64 * 297 + (size_t)S, fn)) return rc;
    const bool pair = c->cnntrad_math == KWS_CT_F16_PAIR;
    c->last_push_host = false;
    {
        ProfScope ps(c, KWS_K_STREAM_FRAME);
        HIP_TRY(c, launch_stream_frame(c->stream, c->fp, c->ft, d_hop, S, c->d_pcm_ring, c->ring_len, c->d_feat_ring, c->d_hops, c->d_refine));
    }
    {
        ProfScope ps(c, KWS_K_CNNTRAD_CONV);
        HIP_TRY(c, launch_cnntrad_conv_ring(c->stream, c->tw, c->d_feat_ring, c->d_hops, frames_lag(c->fp), S, c->d_conv_ws, pair));
    }
    {
        ProfScope ps(c, KWS_K_CNNTRAD_DENSE);
        HIP_TRY(c, launch_cnntrad_dense(c->stream, c->tw, c->d_conv_ws, S, d_logits, d_label, pair));
    }
    c->pushes_enqueued += 1;
    if (int rc = stream_utt_pushed(c)) return rc;
    return stream_detect_pushed(c, d_logits, fn, c->tw.num_classes);
}

int kws_stream_close(kws_ctx* c) {
    if (!c) return KWS_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    stream_free(c);
    return KWS_OK;
}

// timed: bracket the launches with profiling events (eager pushes only; never inside a stream capture).
// A push that asks for logits from the product DS-CNN is ONE launch: each stream's workgroup computes the stream's new
// frame in its prologue (launch_dscnn_stream).  Features-only pushes, and the diagnostic pointwise variants, take the
// frame kernel followed -- if logits are wanted -- by the DS-CNN kernel over the advanced ring.
static hipError_t stream_enqueue(kws_ctx* c, const int16_t* d_hop, float* d_logits, int32_t* d_label, bool timed) {
    hipError_t e;
    if (d_logits && (c->pw_math == KWS_PW_SPLIT_BF16 || c->pw_math == KWS_PW_PAIR_F16)) {
        const bool was = c->prof;
        c->prof = was && timed;
        ProfScope ps(c, KWS_K_DSCNN);
        c->prof = was;
        // time-tile clusters while there are CUs to spare: 4 workgroups per stream up to 64 streams, 2 up to 128 (256 CUs)
        const int cluster = c->stream_cluster ? c->stream_cluster : (c->n_streams <= 64 ? 4 : (c->n_streams <= 128 ? 2 : 1));
        const bool host = c->h_stream_flag && c->host_results_classes == c->mw.num_classes;
        const StreamPush sp = {c->fp, c->ft, d_hop, c->d_pcm_ring, c->ring_len, c->d_hops, c->d_refine, 0, cluster, c->d_cl_part, c->d_cl_count,
                               host ? c->h_stream_logits : nullptr, host ? c->h_stream_label : nullptr, host ? c->h_stream_flag : nullptr};
        c->last_push_host = host;
        return launch_dscnn_stream(c->stream, c->mw, sp, c->d_feat_ring, c->n_streams, d_logits, d_label, c->pw_math == KWS_PW_PAIR_F16);
    }
    c->last_push_host = false;
    {
        const bool was = c->prof;
        c->prof = was && timed;
        ProfScope ps(c, KWS_K_STREAM_FRAME);
        c->prof = was;
        e = launch_stream_frame(c->stream, c->fp, c->ft, d_hop, c->n_streams, c->d_pcm_ring, c->ring_len, c->d_feat_ring,
                                c->d_hops, c->d_refine);
    }
    if (e != hipSuccess) return e;
    if (d_logits) {
        const bool was = c->prof;
        c->prof = was && timed;
        ProfScope ps(c, KWS_K_DSCNN);
        c->prof = was;
        e = launch_dscnn(c->stream, c->mw, c->d_feat_ring, c->n_streams, d_logits, d_label, nullptr, c->pw_math, nullptr, c->d_hops, false,
                         frames_lag(c->fp));
    }
    return e;
}

int kws_stream_push_i16(kws_ctx* c, const int16_t* d_hop, float* d_logits, int32_t* d_label, int use_graph) {
    if (!c) return KWS_EINVAL;
    if (!c->n_streams) return fail(c, KWS_ESTATE, "kws_stream_push_i16: call kws_stream_open first");
    if (!d_hop) return fail(c, KWS_EINVAL, "kws_stream_push_i16: d_hop is NULL");
    if (d_logits) {
        if (!c->model_ready) return fail(c, KWS_ESTATE, "kws_stream_push_i16: no model loaded (kws_load_dscnn)");
        if (c->mw.in_channels != 1) return fail(c, KWS_EUNSUPPORTED, "kws_stream_push_i16: the model was loaded with more than one input channel");
        if (c->fp.num_frames != IN_T || c->fp.numcep != IN_F)
            return fail(c, KWS_EUNSUPPORTED, "kws_stream_push_i16: the DS-CNN kernel is built for a 99 x 10 feature map");
    }
    if (int rc = stream_utt_push_check(c, "kws_stream_push_i16")) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    // A push that is ONE kernel launch gains nothing from a graph -- on this stack it loses: hipGraphLaunch of a one-node graph
    // takes 6.9 us of host time against 3.0 us for the plain launch, and completion is observed 8 us later in all
    // (tools/graph_overhead.hip: 20.6 vs 12.3 us launch -> hipStreamSynchronize for a trivial kernel; still 23.6 vs 20.3 us at
    // four kernels).  use_graph is honoured for the multi-launch routes only, where it saves host time per push.
    if (use_graph && d_logits && (c->pw_math == KWS_PW_SPLIT_BF16 || c->pw_math == KWS_PW_PAIR_F16)) use_graph = 0;
    if (use_graph) {
        // one hipGraph per (hop, logits, label) pointer triple: the two launches replay as one submission
        if (!c->stream_graph || c->graph_key[0] != d_hop || c->graph_key[1] != d_logits || c->graph_key[2] != d_label) {
            if (c->stream_graph) {  // other buffers than the captured ones: retire the old graph once it is idle
                HIP_TRY(c, hipStreamSynchronize(c->stream));
                drop_stream_graph(c);
            }
            hipGraph_t g = nullptr;
            HIP_TRY(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
            hipError_t e = stream_enqueue(c, d_hop, d_logits, d_label, false);
            hipError_t e2 = hipStreamEndCapture(c->stream, &g);
            if (e != hipSuccess || e2 != hipSuccess || !g) return fail_hip(c, e != hipSuccess ? e : e2, "kws_stream_push_i16: graph capture");
            e = hipGraphInstantiate(&c->stream_graph, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (e != hipSuccess) return fail_hip(c, e, "kws_stream_push_i16: hipGraphInstantiate");
            c->graph_key[0] = d_hop;
            c->graph_key[1] = d_logits;
            c->graph_key[2] = d_label;
        }
        HIP_TRY(c, hipGraphLaunch(c->stream_graph, c->stream));
        c->pushes_enqueued += 1;
        if (int rc = stream_utt_pushed(c)) return rc;  // armed: the step kernel, behind the replay and outside the graph
        return stream_detect_pushed(c, d_logits, "kws_stream_push_i16", c->mw.num_classes);  // ... and the decision step (kws_live_detect.hip), likewise
    }
    HIP_TRY(c, stream_enqueue(c, d_hop, d_logits, d_label, true));
    c->pushes_enqueued += 1;
    if (c->last_push_host) c->host_push = c->pushes_enqueued;
    if (int rc = stream_utt_pushed(c)) return rc;
    return stream_detect_pushed(c, d_logits, "kws_stream_push_i16", c->mw.num_classes);
}

int kws_stream_state(kws_ctx* c, const float** d_feat_ring, int* hops) {
    if (!c) return KWS_EINVAL;
    if (!c->n_streams) return fail(c, KWS_ESTATE, "kws_stream_state: no open stream set");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (d_feat_ring) *d_feat_ring = c->d_feat_ring;
    if (hops) HIP_TRY(c, hipMemcpy(hops, c->d_hops, sizeof(int), hipMemcpyDeviceToHost));
    return KWS_OK;
}

int kws_stream_copy_features(kws_ctx* c, float* d_out) {
    if (!c) return KWS_EINVAL;
    if (!c->n_streams) return fail(c, KWS_ESTATE, "kws_stream_copy_features: no open stream set");
    if (!d_out) return fail(c, KWS_EINVAL, "kws_stream_copy_features: d_out is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(d_out, c->d_feat_ring, sizeof(float) * (size_t)c->n_streams * c->fp.num_frames * c->fp.numcep,
                              hipMemcpyDeviceToDevice, c->stream));
    return KWS_OK;
}

// ---- measurement ---------------------------------------------------------------------------------
int kws_prof_enable(kws_ctx* c, int on) {
    if (!c) return KWS_EINVAL;
    c->prof = on != 0;
    c->prof_every = on > 1 ? on : 1;
    return KWS_OK;
}

static int prof_drain(kws_ctx* c) {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < KWS_K_COUNT; ++k) {
        for (size_t i = 0; i < c->ev_used[k]; ++i) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, c->ev[k][i].a, c->ev[k][i].b) == hipSuccess) {
                c->ms_total[k] += ms;
                c->launches[k] += 1;
            }
        }
        c->ev_used[k] = 0;
    }
    return KWS_OK;
}

int kws_prof_reset(kws_ctx* c) {
    if (!c) return KWS_EINVAL;
    int rc = prof_drain(c);
    for (int k = 0; k < KWS_K_COUNT; ++k) {
        c->ms_total[k] = 0;
        c->launches[k] = 0;
        c->prof_seen[k] = 0;
    }
    return rc;
}

int kws_prof_read(kws_ctx* c, int kernel_id, double* total_ms, int* launches) {
    if (!c) return KWS_EINVAL;
    if (kernel_id < 0 || kernel_id >= KWS_K_COUNT) return fail(c, KWS_EINVAL, "kws_prof_read: bad kernel id");
    int rc = prof_drain(c);
    if (rc) return rc;
    if (total_ms) *total_ms = c->ms_total[kernel_id];
    if (launches) *launches = (int)c->launches[kernel_id];
    return KWS_OK;
}

}  // extern "C"
#pragma GCC visibility pop

namespace kws {
ScanModel scan_model_cnn_trad() { return {cnntrad_scan_check, cnntrad_windows_launch}; }
}  // namespace kws
