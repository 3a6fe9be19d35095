// The stream set behind the C ABI (include/kws_hip.h: kws_stream_*): per-stream PCM and feature rings with their hop counter,
// zero-copy result delivery into pinned host memory, and the push -- one frame (stream_push) around the model's own launches:
// the DS-CNN's one-launch route, its multi-launch routes with their optional graph, cnn-trad-fpool3's three launches.  What is
// armed on a set steps behind every push: live utterances (kws_live.hip) and live keyword events (kws_live_detect.hip).
#include <atomic>
#include <cstring>

#include "kws_event_queue.h"  // spin_until

using namespace kws;

// Streaming state: the zero-copy result buffers, then everything kws_stream_open allocates (kws_set_frontend retires it too).
// The buffers are the context's own (kws_ctx.h); what is reset here with them are the counts that say a set is open.
static void host_results_free(kws_ctx* c) {
    c->h_stream_logits.reset();
    c->h_stream_label.reset();
    c->h_stream_flag.reset();
    c->h_stream_hop.reset();
    c->d_hr_logits.reset();
    c->d_hr_label.reset();
    c->host_results_classes = 0;
}

void stream_free(kws_ctx* c) {
    smooth_free(c);
    vad_free(c);
    stream_utt_free(c);  // live utterances (kws_live.hip)
    stream_detect_free(c);  // live keyword events (kws_live_detect.hip)
    host_results_free(c);
    drop_stream_graph(c);
    c->d_pcm_ring.reset();
    c->d_feat_ring.reset();
    c->d_hops.reset();
    c->d_cl_part.reset();
    c->d_cl_count.reset();
    c->d_reset_scratch.reset();
    c->reset_row_ready = false;
    stream_active_free(c);  // every stream of the next set is active (kws_stream_active.hip)
    c->n_streams = 0;
}

// The frame kernel of a multi-launch push: every stream's rings and the hop counter advance by one hop.
hipError_t stream_enqueue_frame(kws_ctx* c, const int16_t* d_hop, bool timed) {
    ProfScope ps(c, KWS_K_STREAM_FRAME, timed);
    return launch_stream_frame(c->stream, c->fp, c->ft, d_hop, c->n_streams, c->d_pcm_ring.get(), c->ring_len, c->d_feat_ring.get(),
                               c->d_hops.get(), c->d_refine.get());
}

// The route of a DS-CNN push: logits from one of the product kernels.
static bool one_launch_push(const kws_ctx* c, const float* d_logits) {
    return d_logits && (c->pw_math == KWS_PW_SPLIT_BF16 || c->pw_math == KWS_PW_PAIR_F16);
}

// timed: bracket the launches with profiling events (eager pushes only; never inside a stream capture).
// A push that asks for logits from the product DS-CNN is ONE launch: each stream's workgroup computes the stream's new
// frame in its prologue (launch_dscnn_stream).  Features-only pushes, and the diagnostic pointwise variants, take the
// frame kernel followed -- if logits are wanted -- by the DS-CNN kernel over the advanced ring.
static hipError_t stream_enqueue(kws_ctx* c, const int16_t* d_hop, float* d_logits, int32_t* d_label, bool timed) {
    if (one_launch_push(c, d_logits)) {
        ProfScope ps(c, KWS_K_DSCNN, timed);
        // time-tile clusters while there are CUs to spare: 4 workgroups per stream up to 64 streams, 2 up to 128 (256 CUs)
        // (n_active == n_streams unless streams were deactivated: a sparse set gets the cluster of the streams it serves)
        const int cluster = c->stream_cluster ? c->stream_cluster : (c->n_active <= 64 ? 4 : (c->n_active <= 128 ? 2 : 1));
        const bool host = c->h_stream_flag && c->host_results_classes == c->mw.num_classes;
        const StreamPush sp = {c->fp, c->ft, d_hop, c->d_pcm_ring.get(), c->ring_len, c->d_hops.get(), c->d_refine.get(), 0, cluster,
                               c->d_cl_part.get(), c->d_cl_count.get(), host ? c->h_stream_logits.get() : nullptr,
                               host ? c->h_stream_label.get() : nullptr, host ? c->h_stream_flag.get() : nullptr};
        c->last_push_host = host;
        if (c->sparse()) {  // the active streams' workgroups alone, their stream index from the set's list; none: the clock runs on
            if (!c->n_active) return launch_stream_tick(c->stream, sp.hops, sp.h_flag);
            return launch_dscnn_stream_active(c->stream, c->mw, sp, c->d_feat_ring.get(), c->n_streams, d_logits, d_label, c->pw_math == KWS_PW_PAIR_F16,
                                              c->d_active_list.get(), c->n_active);
        }
        return launch_dscnn_stream(c->stream, c->mw, sp, c->d_feat_ring.get(), c->n_streams, d_logits, d_label, c->pw_math == KWS_PW_PAIR_F16);
    }
    c->last_push_host = false;
    hipError_t e = stream_enqueue_frame(c, d_hop, timed);
    if (e == hipSuccess && d_logits) {
        ProfScope ps(c, KWS_K_DSCNN, timed);
        e = launch_dscnn(c->stream, c->mw, c->d_feat_ring.get(), c->n_streams, d_logits, d_label, nullptr, c->pw_math, nullptr,
                         c->d_hops.get(), false, frames_lag(c->fp));
    }
    return e;
}

// The multi-launch routes replayed as one submission: one hipGraph per (hop, logits, label) pointer triple.  A replay delivers
// nothing to host memory, whatever the push before it did.
static int stream_enqueue_graph(kws_ctx* c, const int16_t* d_hop, float* d_logits, int32_t* d_label) {
    const void* const key[3] = {d_hop, d_logits, d_label};
    if (!c->stream_graph || memcmp(c->graph_key, key, sizeof key) != 0) {
        if (int rc = retire_captured_push(c)) return rc;  // other buffers than the captured ones
        hipGraph_t g = nullptr;
        HIP_TRY(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        hipError_t e = stream_enqueue(c, d_hop, d_logits, d_label, false);
        hipError_t e2 = hipStreamEndCapture(c->stream, &g);
        if (e != hipSuccess || e2 != hipSuccess || !g) return fail_hip(c, e != hipSuccess ? e : e2, "kws_stream_push_i16: graph capture");
        e = hipGraphInstantiate(&c->stream_graph, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (e != hipSuccess) return fail_hip(c, e, "kws_stream_push_i16: hipGraphInstantiate");
        memcpy(c->graph_key, key, sizeof key);
    }
    c->last_push_host = false;
    HIP_TRY(c, hipGraphLaunch(c->stream_graph, c->stream));
    return KWS_OK;
}

// A push, whatever the model: the set, the arguments, the model's checks where logits are asked for (a features-only push needs no
// model), the armed set's driver; then `enqueue`, the model's launches; then, once, what follows every push -- the count, the newest
// push that delivers to host memory, the armed steps (outside a graph).  Nothing on the way to the launches builds a string or allocates.
template <typename Enqueue>
static int stream_push(kws_ctx* c, const ModelOps& m, const char* fn, const int16_t* d_hop, float* d_logits, bool logits_required,
                       Enqueue enqueue) {
    if (!c) return KWS_EINVAL;
    if (!c->n_streams) return fail(c, KWS_ESTATE, std::string(fn) + ": call kws_stream_open first");
    if (!d_hop || (logits_required && !d_logits))
        return fail(c, KWS_EINVAL, std::string(fn) + (logits_required ? ": d_hop / d_logits is NULL" : ": d_hop is NULL"));
    if (d_logits)
        if (int rc = m.push_check(c, fn)) return rc;
    if (int rc = stream_utt_push_check(c, fn)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = enqueue()) return rc;
    c->pushes_enqueued += 1;
    if (c->last_push_host) c->host_push = c->pushes_enqueued;
    if (int rc = stream_utt_pushed(c)) return rc;
    return stream_detect_pushed(c, d_logits, fn, m.classes(c));
}

#pragma GCC visibility push(default)
extern "C" {

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
    const size_t n = (size_t)n_streams;
    if (!(c->d_pcm_ring.alloc(n * c->ring_len) && c->d_feat_ring.alloc(n * p.num_frames * p.numcep) && c->d_hops.alloc(2) &&
          c->d_cl_part.alloc(n * 4 * 64) && c->d_cl_count.alloc(n))) {
        stream_free(c);
        return fail(c, KWS_ENOMEM, "kws_stream_open: device allocation failed");
    }
    c->n_streams = n_streams;
    c->n_active = n_streams;
    c->pushes_enqueued = 0;
    c->host_push = 0;
    c->last_push_host = false;
    if (c->refine_span > 0.f) {  // the pushes count the frames they redo in float64 in the refinement counters
        int rc = ensure_refine(c, 1, c->fp.num_frames);
        if (rc) return rc;
    }
    HIP_TRY(c, hipMemsetAsync(c->d_pcm_ring.get(), 0, sizeof(int16_t) * c->d_pcm_ring.size(), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_feat_ring.get(), 0, sizeof(float) * c->d_feat_ring.size(), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_hops.get(), 0, 2 * sizeof(int), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_cl_count.get(), 0, sizeof(int) * n, c->stream));
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
    const size_t n = (size_t)c->n_streams;
    if (!(c->h_stream_logits.alloc(n * C, flags) && c->h_stream_label.alloc(n, flags) && c->h_stream_flag.alloc(64 / sizeof(int), flags) &&
          c->h_stream_hop.alloc(n * c->fp.frame_step, flags) && c->d_hr_logits.alloc(n * C) && c->d_hr_label.alloc(n))) {
        host_results_free(c);
        return fail(c, KWS_ENOMEM, "kws_stream_host_results: pinned host allocation failed");
    }
    memset(c->h_stream_logits.get(), 0, sizeof(float) * n * C);
    memset(c->h_stream_label.get(), 0, sizeof(int32_t) * n);
    // the flag holds the device's push count: start it where the device stands
    int hops = 0;
    HIP_TRY(c, hipMemcpy(&hops, c->d_hops.get(), sizeof(int), hipMemcpyDeviceToHost));
    *c->h_stream_flag.get() = hops;
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
    volatile int* flag = c->h_stream_flag.get();
    const int want = c->host_push;
    if (!spin_until([&] { return *flag - want >= 0; })) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (*flag - want < 0) return fail(c, KWS_EHIP, "kws_stream_wait_host: the stream drained but the results flag never arrived");
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (h_logits) *h_logits = c->h_stream_logits.get();
    if (h_label) *h_label = c->h_stream_label.get();
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
    if (c->sparse()) {  // the rows of inactive streams are not read, here either
        const size_t row = (size_t)c->fp.frame_step;
        for (size_t w = 0; w < c->active_bits.size(); ++w)
            for (unsigned long long bits = c->active_bits[w]; bits; bits &= bits - 1) {
                const size_t s = 64 * w + (size_t)__builtin_ctzll(bits);
                memcpy(c->h_stream_hop.get() + s * row, h_hop + s * row, sizeof(int16_t) * row);
            }
    } else
        memcpy(c->h_stream_hop.get(), h_hop, sizeof(int16_t) * (size_t)c->n_streams * c->fp.frame_step);
    int rc = kws_stream_push_i16(c, c->h_stream_hop.get(), c->d_hr_logits.get(), c->d_hr_label.get(), 0);
    if (rc) return rc;
    return kws_stream_wait_host(c, h_logits, h_label);
}

int kws_stream_cluster(kws_ctx* c, int workgroups_per_stream) {
    if (!c) return KWS_EINVAL;
    if (workgroups_per_stream != 0 && workgroups_per_stream != 1 && workgroups_per_stream != 2 && workgroups_per_stream != 4)
        return fail(c, KWS_EINVAL, "kws_stream_cluster: workgroups_per_stream must be 0 (automatic), 1, 2 or 4");
    if (workgroups_per_stream != c->stream_cluster)  // a captured push holds the other launch shape
        if (int rc = retire_captured_push(c)) return rc;
    c->stream_cluster = workgroups_per_stream;
    return KWS_OK;
}

int kws_stream_close(kws_ctx* c) {
    if (!c) return KWS_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    stream_free(c);
    return KWS_OK;
}

int kws_stream_push_i16(kws_ctx* c, const int16_t* d_hop, float* d_logits, int32_t* d_label, int use_graph) {
    return stream_push(c, model_ops_dscnn(), "kws_stream_push_i16", d_hop, d_logits, false, [&]() -> int {
        // A push that is ONE kernel launch gains nothing from a graph -- on this stack it loses: hipGraphLaunch of a one-node graph
        // takes 6.9 us of host time against 3.0 us for the plain launch, and completion is observed 8 us later in all
        // (tools/graph_overhead.hip: 20.6 vs 12.3 us launch -> hipStreamSynchronize for a trivial kernel; still 23.6 vs 20.3 us at
        // four kernels).  use_graph is honoured for the multi-launch routes only, where it saves host time per push.
        if (c->sparse()) {  // the fused push alone takes its streams from the list
            if (use_graph) return refuse_sparse(c, "kws_stream_push_i16", "use_graph replays launches captured earlier, which");
            if (!one_launch_push(c, d_logits))
                return refuse_sparse(c, "kws_stream_push_i16", "features-only pushes and the diagnostic pointwise maths take the frame kernel and the two-launch route, which");
        }
        if (use_graph && !one_launch_push(c, d_logits)) return stream_enqueue_graph(c, d_hop, d_logits, d_label);
        HIP_TRY(c, stream_enqueue(c, d_hop, d_logits, d_label, true));
        return KWS_OK;
    });
}

// The push of a cnn-trad-fpool3 context: the frame kernel advances the rings and the hop counter, the conv kernel reads every
// stream's window from the feature ring in place (RING), the dense kernel writes logits and labels.  Three launches, no graph,
// no zero-copy delivery; the armed steps run behind them as behind kws_stream_push_i16.
int kws_stream_push_cnn_trad_i16(kws_ctx* c, const int16_t* d_hop, float* d_logits, int32_t* d_label) {
    const char* fn = "kws_stream_push_cnn_trad_i16";
    const ModelOps& m = model_ops_cnn_trad();
    return stream_push(c, m, fn, d_hop, d_logits, true, [&]() -> int {
        if (int rc = refuse_sparse(c, fn, "cnn-trad-fpool3's three launches")) return rc;
        c->last_push_host = false;
        return m.ring_push(c, fn, d_hop, d_logits, d_label);
    });
}

int kws_stream_state(kws_ctx* c, const float** d_feat_ring, int* hops) {
    if (!c) return KWS_EINVAL;
    if (!c->n_streams) return fail(c, KWS_ESTATE, "kws_stream_state: no open stream set");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (d_feat_ring) *d_feat_ring = c->d_feat_ring.get();
    if (hops) HIP_TRY(c, hipMemcpy(hops, c->d_hops.get(), sizeof(int), hipMemcpyDeviceToHost));
    return KWS_OK;
}

int kws_stream_copy_features(kws_ctx* c, float* d_out) {
    if (!c) return KWS_EINVAL;
    if (!c->n_streams) return fail(c, KWS_ESTATE, "kws_stream_copy_features: no open stream set");
    if (!d_out) return fail(c, KWS_EINVAL, "kws_stream_copy_features: d_out is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(d_out, c->d_feat_ring.get(), sizeof(float) * (size_t)c->n_streams * c->fp.num_frames * c->fp.numcep,
                              hipMemcpyDeviceToDevice, c->stream));
    return KWS_OK;
}

}  // extern "C"
#pragma GCC visibility pop
