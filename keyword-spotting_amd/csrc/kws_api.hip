// C ABI of libkws_hip.so (declared in include/kws_hip.h): the context's lifetime, the DS-CNN's forwards and what the host flows
// need of that model (ModelOps, kws_ctx.h), the standalone block, the fused clip entries of both models and per-kernel event
// timing.  Streaming is in kws_stream.hip, the other model behind its kernels, the front end's entries in kws_frontend.hip, the
// weight images in kws_weights.hip.  No torch types, no exceptions across the boundary, no CPU fallback.
#include "kws_ctx.h"

namespace kws {

const char* const kKernelNames[KWS_K_COUNT] = {"kws_mfcc_i16_kernel", "kws_dscnn_fwd_kernel", "kws_cnntrad_conv_kernel",
                                               "kws_cnntrad_dense_kernel", "kws_stream_frame_kernel", "kws_mfcc_f64_kernel",
                                               "kws_mfcc_refine_kernel", "kws_ds_load_stats_kernel", "kws_ds_load_pack_kernel",
                                               "kws_ds_load_fill_kernel", "kws_resample_kernel"};

}  // namespace kws

using namespace kws;

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
        HIP_TRY(c, launch_conv1_general(c->stream, d_feat, B, c->mw.in_channels, c->mw.c1_general, c->mw.c1_b, c->d_conv_ws.get()));
        ProfScope ps(c, KWS_K_DSCNN);
        HIP_TRY(c, launch_dscnn(c->stream, c->mw, c->d_conv_ws.get(), B, d_logits, d_label, nullptr, mode, nullptr, nullptr, true));
        return KWS_OK;
    }
    ProfScope ps(c, KWS_K_DSCNN);
    HIP_TRY(c, launch_dscnn(c->stream, c->mw, d_feat, B, d_logits, d_label, d_act, mode, d_stamps, nullptr, false, 3, c->n_cu));
    return KWS_OK;
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
    float* bufs[2] = {c->d_conv_ws.get(), c->d_conv_ws.get() + (size_t)chunk * per_clip_max};
    float* dw_ws = c->d_conv_ws.get() + 2 * (size_t)chunk * per_clip_max;
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

// ---- the DS-CNN as the host flows see it (ModelOps, kws_ctx.h) --------------------------------------------------------------------
// The fused clip entries: any map the front end yields (forward_map_impl routes it), of one channel.
static int dscnn_clip_check(kws_ctx* c, const char* fn) {
    if (!c->fe_ready || !c->model_ready) return fail(c, KWS_ESTATE, std::string(fn) + ": front end or model not configured");
    if (c->mw.in_channels != 1) return fail(c, KWS_EUNSUPPORTED, std::string(fn) + ": the MFCC front end yields one channel; the model was loaded with more");
    return KWS_OK;
}
// The recording flows: kws_dscnn_fwd_kernel (SCAN) over the strided windows.  Readiness, then the geometry, then the channel count.
static int dscnn_scan_check(kws_ctx* c, const char* fn) {
    if (!c->fe_ready || !c->model_ready) return fail(c, KWS_ESTATE, std::string(fn) + ": front end or model not configured");
    if (int rc = check_ref_map(c, fn, ": the strided DS-CNN kernel is built for windows of 99 x 10 features")) return rc;
    if (int rc = dscnn_clip_check(c, fn)) return rc;
    if (c->pw_math != KWS_PW_PAIR_F16 && c->pw_math != KWS_PW_SPLIT_BF16)
        return fail(c, KWS_EUNSUPPORTED, std::string(fn) + ": needs KWS_PW_PAIR_F16 or KWS_PW_SPLIT_BF16");
    return KWS_OK;
}
static int dscnn_windows(kws_ctx* c, const char*, const float* d_frames, int R, int F, int W, int hop_frames, float* d_logits,
                         int32_t* d_label) {
    const ScanWindows sw = {(unsigned)W, W == 1 ? 0xffffffffu : (unsigned)((1ull << 32) / (unsigned)W), (unsigned)F * (unsigned)IN_F,
                            (unsigned)hop_frames * (unsigned)IN_F};
    ProfScope ps(c, KWS_K_DSCNN);
    HIP_TRY(c, launch_dscnn_scan(c->stream, c->mw, d_frames, R * W, d_logits, d_label, c->pw_math, c->n_cu, sw));
    return KWS_OK;
}
// A push that asks for logits: the kernels read the feature ring, one channel of 99 x 10.
static int dscnn_push_check(kws_ctx* c, const char* fn) {
    if (!c->model_ready) return fail(c, KWS_ESTATE, std::string(fn) + ": no model loaded (kws_load_dscnn)");
    if (c->mw.in_channels != 1) return fail(c, KWS_EUNSUPPORTED, std::string(fn) + ": the model was loaded with more than one input channel");
    return check_ref_map(c, fn, ": the DS-CNN kernel is built for a 99 x 10 feature map");
}
static int dscnn_classes(const kws_ctx* c) { return c->mw.num_classes; }
// 99 x 10 (the reference geometry): the fused kernel; any other map kws_frontend_shape yields: the composed path
static int dscnn_forward(kws_ctx* c, const float* d_feat, int B, float* d_logits, int32_t* d_label, const char* fn) {
    return forward_map_impl(c, d_feat, B, c->fp.num_frames, c->fp.numcep, d_logits, d_label, nullptr, fn);
}
static const ModelOps kDscnnOps = {dscnn_scan_check, dscnn_clip_check, dscnn_push_check, dscnn_classes, dscnn_forward, dscnn_windows, nullptr};
namespace kws {
const ModelOps& model_ops_dscnn() { return kDscnnOps; }
}  // namespace kws

// kws_infer_i16 / kws_infer_f32 and their cnn-trad-fpool3 twins: batch, the model's readiness and geometry, the feature workspace, the
// MFCC of the sample type, the model's forward.  fn names the entry in the refusals; forward_fn, where given, in the forward's own.
template <typename Sample>
static int infer_clips(kws_ctx* c, const ModelOps& m, const char* fn, int (*mfcc)(kws_ctx*, const Sample*, int, float*), const Sample* d_wav,
                       int B, float* d_logits, int32_t* d_label, const char* forward_fn = nullptr) {
    int rc = check_batch(c, d_wav, B, fn);
    if (rc) return rc;
    if ((rc = m.clip_check(c, fn))) return rc;
    if ((rc = kws_reserve(c, B))) return rc;
    if ((rc = mfcc(c, d_wav, B, c->d_feat_ws.get()))) return rc;
    return m.forward(c, c->d_feat_ws.get(), B, d_logits, d_label, forward_fn ? forward_fn : fn);
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
    stream_free(c);     // the stream set and what is armed on it: counters, captured graph, live utterances and events
    eval_free(c);        // evaluation state (kws_eval.hip)
    stream_resample_free(c);  // streaming resampler: history, hop buffer, pinned input (kws_resample.hip)
    resample_free(c);    // tap tables of the rate pairs (kws_resample.hip)
    ingest_free(c);      // staging rings, copy streams, pack threads
    const hipEvent_t order_ev = c->order_ev;
    const hipStream_t own_stream = c->own_stream;
    delete c;            // every buffer the context still owns goes here: the device is current, the stream drained and still alive
    if (order_ev) (void)hipEventDestroy(order_ev);
    if (own_stream) (void)hipStreamDestroy(own_stream);
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
    if (int rc = retire_captured_push(c)) return rc;  // a captured push replays on the stream it was captured for
    c->stream = next;
    return KWS_OK;
}

int kws_sync(kws_ctx* c) {
    if (!c) return KWS_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return KWS_OK;
}

int kws_forward_f32(kws_ctx* c, const float* d_feat, int B, float* d_logits, int32_t* d_label) {
    return forward_impl(c, d_feat, B, d_logits, d_label, nullptr, c ? c->pw_math : 0, "kws_forward_f32");
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
    if (math != c->pw_math)  // a captured push holds the other kernel
        if (int rc = retire_captured_push(c)) return rc;
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
    return infer_clips(c, model_ops_dscnn(), "kws_infer_i16", kws_mfcc_i16, d_wav, B, d_logits, d_label);
}

int kws_infer_f32(kws_ctx* c, const float* d_wav, int B, float* d_logits, int32_t* d_label) {
    return infer_clips(c, model_ops_dscnn(), "kws_infer_f32", kws_mfcc_f32, d_wav, B, d_logits, d_label);
}

// This entry used to call kws_forward_cnn_trad_f32, and the forward's own refusals (d_logits, the workspace) still speak under
// that name.
int kws_infer_cnn_trad_i16(kws_ctx* c, const int16_t* d_wav, int B, float* d_logits, int32_t* d_label) {
    return infer_clips(c, model_ops_cnn_trad(), "kws_infer_cnn_trad_i16", kws_mfcc_i16, d_wav, B, d_logits, d_label, "kws_forward_cnn_trad_f32");
}

int kws_infer_cnn_trad_f32(kws_ctx* c, const float* d_wav, int B, float* d_logits, int32_t* d_label) {
    return infer_clips(c, model_ops_cnn_trad(), "kws_infer_cnn_trad_f32", kws_mfcc_f32, d_wav, B, d_logits, d_label);
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
                              c->d_conv_ws.get(), d_out));
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

