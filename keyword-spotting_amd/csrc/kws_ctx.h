// The context behind the C ABI (include/kws_hip.h), the error plumbing and the device-memory helpers shared by the translation
// units that implement it (kws_api.hip, kws_stream.hip, kws_cnntrad.hip, kws_frontend.hip, kws_weights.hip, kws_ingest.hip,
// kws_scan.hip, kws_score.hip, kws_ragged.hip, kws_decide.hip, kws_eval.hip, kws_resample.hip, kws_live.hip, kws_live_detect.hip, kws_stream_reset.hip, kws_stream_active.hip, kws_*_bwd.hip),
// the table of what the host flows need of a model, and the event bracket of a timed launch.
// Memory: every device or pinned allocation of the context is a DeviceBuffer / PinnedBuffer member (kws_buffer.h) of kws_ctx or of
// a sub-state the context points to, and is freed by that member's destructor.  The *_free functions below reset what is not
// memory (counters, modes, the captured graph, threads and streams) and delete their sub-state; nothing frees a buffer by name.
#pragma once
#include <memory>
#include <new>

#include "kws_buffer.h"
#include "kws_endpoint_dev.h"
#include "kws_internal.h"

namespace kws {
struct Ingest;  // host-ingest pipeline state (kws_ingest.hip)
void ingest_free(kws_ctx* c);
void smooth_free(kws_ctx* c);  // posterior-smoothing and endpointer histories of the streams (kws_decide.hip)
void vad_free(kws_ctx* c);
void eval_free(kws_ctx* c);  // evaluation accumulators (kws_eval.hip)
struct ResampleCache;           // rate pairs designed so far and their device tap tables (kws_resample.hip)
void resample_free(kws_ctx* c);
struct StreamResample;          // the streaming resampler's pair, position and per-stream history (kws_resample.hip)
void stream_resample_free(kws_ctx* c);
struct StreamUtt;               // live utterances: history ring, walk state, event queue and its host mirror (kws_live.hip)
void stream_utt_free(kws_ctx* c);
int stream_utt_push_check(kws_ctx* c, const char* fn);  // a push is refused once kws_stream_utt_step_i16 has stepped the set
int stream_utt_pushed(kws_ctx* c);                      // the step behind a push's launches; nothing when the context is unarmed
struct StreamDetect;            // live keyword events: posterior ring, refractory state, event queue and its host mirror (kws_live_detect.hip)
void stream_detect_free(kws_ctx* c);
// the decision step behind a push, from that push's logits; nothing when unarmed.  fn: the push entry, named in the errors;
// model_classes: the class count of the model that made the logits (the DS-CNN's or cnn-trad-fpool3's)
int stream_detect_pushed(kws_ctx* c, const float* d_logits, const char* fn, int model_classes);
// A per-stream reset (kws_stream_reset, kws_stream_reset.hip) names its streams BY VALUE: bit s % 64 of word s / 64 of a chunk of
// 1024 streams travels inside the kernel arguments, so no later call can overtake a copy of the selection.
constexpr int RESET_CHUNK = 1024;
struct ResetMask {
    unsigned long long w[RESET_CHUNK / 64];
    __host__ __device__ bool has(int s) const { return (w[s >> 6] >> (s & 63)) & 1ull; }
};
// What the reset's ring kernel clears of the other units, each handed out by its owner: the streaming resampler's two history
// halves (kws_resample.hip), the live events' refractory word and epoch with the decision counter the epoch is read from
// (kws_live_detect.hip; from this call on the set launches the epoch instantiation of its step).  All nullptr when the unit is off.
struct ResampleResetView { int16_t* hist; long long half; int len; };  // stream s: hist + h * half + s * len, h = 0, 1
ResampleResetView stream_resample_reset_view(kws_ctx* c);
struct DetectResetView { long long* next; long long* epoch; const unsigned long long* decisions; };
DetectResetView stream_detect_reset_view(kws_ctx* c);
// live utterances: close what is open on the named streams with reason 2 and start their endpointer over -- one more tick of the
// unit's queue (kws_live.hip); nothing when the context is unarmed
int stream_utt_reset(kws_ctx* c, const ResetMask& m);
// kws_stream_reset's checks under the name `fn` of the entry that makes them (kws_stream_reset.hip; kws_stream_activate and
// kws_stream_deactivate share them, kws_stream_active.hip).  KWS_OK with *nothing = true: n == 0, the call is done.
int stream_reset_check(kws_ctx* c, const char* fn, const int32_t* streams, int n, bool* nothing);
// ... and its launches over the checked list.  only_active: inactive streams are skipped; utt_only: the rings and the other units
// stay, only what is open in the live utterances closes (a deactivation)
int stream_reset_launch(kws_ctx* c, const int32_t* streams, int n, bool only_active, bool utt_only);
// Sparse sets (kws_stream_active.hip): the launch of a push that finds no active stream -- the hop counter advances, the zero-copy
// flag follows it --, and the release of what the first deactivation allocated
hipError_t launch_stream_tick(hipStream_t s, int* d_hops, int* h_flag);
void stream_active_free(kws_ctx* c);
// What the host flows need of a model.  The recording flows (scan_recordings, kws_scan.hip; scan_ragged_entry, kws_ragged.hip), the
// fused clip entries (infer_clips, kws_api.hip) and the stream push (stream_push, kws_stream.hip) are each written once and take one
// of these.  fn names the entry: a refusal starts with it, in that model's words, and is composed on the failing branch only.
struct ModelOps {
    // readiness and geometry: front end and model for the recording flows and the clip entries, the model alone for a push with logits
    int (*scan_check)(kws_ctx* c, const char* fn);
    int (*clip_check)(kws_ctx* c, const char* fn);
    int (*push_check)(kws_ctx* c, const char* fn);
    int (*classes)(const kws_ctx* c);  // of the loaded model
    // B contiguous maps of the front end's geometry (cnn-trad-fpool3: 99 x 10 only) -> logits [B][C], labels [B] or NULL
    int (*forward)(kws_ctx* c, const float* d_feat, int B, float* d_logits, int32_t* d_label, const char* fn);
    // the R * W strided 99-frame windows of a frame array [R][F][10] -> logits [R * W][C], labels or NULL, in window order
    int (*windows)(kws_ctx* c, const char* fn, const float* d_frames, int R, int F, int W, int hop_frames, float* d_logits, int32_t* d_label);
    // the launches of a push through the feature ring: what can fail on the host, stream_enqueue_frame, the model over every stream's
    // window.  nullptr for the DS-CNN: its product push computes the frame inside the model kernel (stream_enqueue, kws_stream.hip)
    int (*ring_push)(kws_ctx* c, const char* fn, const int16_t* d_hop, float* d_logits, int32_t* d_label);
};
const ModelOps& model_ops_dscnn();     // kws_api.hip
const ModelOps& model_ops_cnn_trad();  // kws_cnntrad.hip
}  // namespace kws

using kws::FrontendParams; using kws::FrontendTables; using kws::DscnnWeights; using kws::CnnTradWeights; using kws::NFFT;
using kws::DeviceBuffer; using kws::PinnedBuffer;

// The buffers below are freed when the context is deleted: kws_destroy does that with the device current and the stream drained,
// and destroys own_stream only afterwards.
struct kws_ctx {
    int device = 0;
    int n_cu = 0;                   // compute units of the device (hipDeviceProp_t::multiProcessorCount): the persistent DS-CNN grid
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t order_ev = nullptr;  // orders the new stream behind the old one in kws_set_stream
    std::string err;

    // front end
    int sample_rate = 16000, nfft = NFFT, ceplifter = 22;
    FrontendParams fp{};
    bool fe_ready = false;
    bool fe_fast_ok = false;      // the float32 kernel covers this geometry (nfft 512, frame_len <= 512, sparse mel layout fits)
    bool fe_ref_geometry = false; // frame length, hop, filters and cepstra are the reference's: int16 PCM may take kws_mfcc_i16_ref_kernel
    int fe_route = KWS_FE_ROUTE_AUTO;  // kws_set_frontend_route (diagnostics): KWS_FE_ROUTE_GENERIC keeps such calls on the generic kernel
    int fe_math = KWS_FE_F32;     // requested arithmetic (kws_set_frontend_math); geometries without a fast kernel run in float64 anyway
    DeviceBuffer<unsigned char> d_fe;  // one allocation holding all front-end tables
    FrontendTables ft{};
    DeviceBuffer<double> d_spec_tw64;  // float64 twiddles of kws_spec_f32's last transform length
    int spec_nfft = 0;
    // selective float64 refinement of the float32 front end (kws_set_frontend_refine): worklist + counters
    float refine_span = KWS_FE_REFINE_SPAN_DEFAULT;
    DeviceBuffer<int> d_refine;       // int[8] counters followed by the list, one allocation
    int refine_cap = 0;               // frames the list holds
    unsigned long long frames_seen = 0;  // frames through the float32 kernels since kws_create

    // model
    DeviceBuffer<float> d_model;
    DscnnWeights mw{};
    bool model_ready = false;
    size_t ds_image_words = 0;        // image words in d_model, without the unit table behind them (kws_load_dscnn_device refreshes
                                      // the image in place when this matches)
    DeviceBuffer<unsigned char> d_ds_stats;  // kws_load_dscnn_device: the weight statistics read back to the host
    int pw_math = KWS_PW_PAIR_F16;    // kernel variant of the product entry points
    // cnn-trad-fpool3
    DeviceBuffer<uint32_t> d_cnntrad;
    CnnTradWeights tw{};
    bool cnntrad_ready = false;
    int cnntrad_math = KWS_CT_F16_PAIR;
    const float* ct_raw = nullptr;  // the loaded blob as float32 (state_dict layouts), inside d_cnntrad: kws_cnn_trad_backward_f32's weights
    size_t ct_image_words = 0;      // size of d_cnntrad (kws_load_cnn_trad_device refreshes it in place when the size matches)
    DeviceBuffer<float> d_ct_stats;  // kws_load_cnn_trad_device: the weight statistics read back to the host
    DeviceBuffer<float> d_conv_ws;  // scratch between two kernels of one call (grow_conv_ws)
    // training (kws_dscnn_backward_f32, kws_dscnn_bwd.hip; kws_cnn_trad_backward_f32, kws_cnntrad_bwd.hip): recomputed activations, gradients, per-workgroup partials
    DeviceBuffer<float> d_train_ws;

    // workspace (MFCC features between the two kernels of kws_infer_i16)
    DeviceBuffer<float> d_feat_ws;
    // kws_scan_i16: a recording's frames when the caller keeps none (kws_scan_detect_f32's scratch is d_conv_ws)
    DeviceBuffer<float> d_scan_ws;
    // the ragged entries' plan tables (records, per-recording offsets and counts), derived on the host per call
    DeviceBuffer<unsigned char> d_ragged;

    // streaming state (kws_stream_*): per-stream PCM ring, feature ring, hop counter, optional graph
    int n_streams = 0, ring_len = 0;
    DeviceBuffer<int16_t> d_pcm_ring;
    DeviceBuffer<float> d_feat_ring;
    DeviceBuffer<int> d_hops;
    int stream_cluster = 0;           // workgroups per stream of the fused push (kws_stream_cluster; 0 = by stream count)
    DeviceBuffer<float> d_cl_part;    // [n_streams][4][64] pooled partial sums of a stream's time tiles
    DeviceBuffer<int> d_cl_count;     // [n_streams]
    // zero-copy result delivery of the one-launch push (kws_stream_host_results): pinned, device-mapped host memory
    PinnedBuffer<float> h_stream_logits;  // [n_streams][num_classes at enable time]
    PinnedBuffer<int32_t> h_stream_label;
    PinnedBuffer<int> h_stream_flag;
    PinnedBuffer<int16_t> h_stream_hop;  // [n_streams][frame_step]: the hop of kws_stream_push_host_i16, read by the kernel over PCIe
    DeviceBuffer<float> d_hr_logits;   // device-side outputs of kws_stream_push_host_i16 (the kernel writes both copies)
    DeviceBuffer<int32_t> d_hr_label;
    int host_results_classes = 0;
    int pushes_enqueued = 0;           // pushes since kws_stream_open = the device's hop counter once the stream has drained
    int host_push = 0;                 // the newest push that delivers to host memory (the flag reads this when it is done)
    bool last_push_host = false;
    hipGraphExec_t stream_graph = nullptr;
    const void* graph_key[3] = {nullptr, nullptr, nullptr};
    // posterior smoothing history (kws_stream_smooth_f32): ring [n_streams][window][C], sum [n_streams][C], hop count
    DeviceBuffer<float> d_post_ring, d_post_sum;
    DeviceBuffer<int> d_post_count;
    int post_window = 0, post_classes = 0;
    // energy endpointer (kws_stream_vad_f32): ep_ring_push's state, bits [n_streams][EP_BIT_WORDS] and counts [n_streams][4] =
    // (c_on, c_off, triggered, cursor)
    DeviceBuffer<unsigned long long> d_vad_bits;
    DeviceBuffer<int> d_vad_counts;
    int vad_on = 0, vad_off = 0;
    // per-stream reset (kws_stream_reset): the frame kernel's scratch set of ONE stream, made at the set's first reset -- its
    // feature ring's row 0 is the row of an all-zero frame -- then the hop counter, the PCM ring and the zero hop of that run
    DeviceBuffer<float> d_reset_scratch;
    bool reset_row_ready = false;
    // sparse sets (kws_stream_activate / kws_stream_deactivate, kws_stream_active.hip).  The host mirror decides everything a launch
    // needs -- the count is the grid, the bits travel by value --; the device list is rebuilt from it at every change.
    int n_active = 0;                              // == n_streams until a stream is deactivated
    std::vector<unsigned long long> active_bits;   // bit s % 64 of word s / 64; empty until the set's first deactivation = all active
    DeviceBuffer<int32_t> d_active_list;           // [n_streams]: the first n_active entries are the active streams, ascending
    bool sparse() const { return n_active < n_streams; }
    bool is_active(int s) const { return active_bits.empty() || ((active_bits[(size_t)s >> 6] >> (s & 63)) & 1ull); }
    kws::ResetMask active_chunk(int first) const {  // the mask of streams first .. first + RESET_CHUNK - 1 (first a multiple of RESET_CHUNK)
        kws::ResetMask m{};
        for (int k = 0; k < kws::RESET_CHUNK / 64; ++k) {
            const size_t w = (size_t)first / 64 + k;
            m.w[k] = active_bits.empty() ? ~0ull : (w < active_bits.size() ? active_bits[w] : 0ull);
        }
        return m;
    }

    // evaluation statistics (kws_eval_*, kws_eval.hip): one allocation of 64-bit words -- counts[4], loss_sum (a double),
    // confusion [C][C], hist_pos [C][K], hist_neg [C][K] -- and the per-workgroup float64 loss partials of one update
    DeviceBuffer<unsigned long long> d_eval;
    int eval_classes = 0, eval_bins = 0;  // eval_classes > 0: open
    DeviceBuffer<double> d_eval_part;

    // sample-rate conversion (kws_resample_*): the tap tables of the rate pairs used so far -- created on first use
    kws::ResampleCache* resample = nullptr;
    // streaming resampler (kws_stream_resample_*, kws_stream_push_rate_i16): created by kws_stream_resample_open
    kws::StreamResample* stream_resample = nullptr;
    // live utterances (kws_stream_utt_*): created by kws_stream_utt_open, dropped with the streams
    kws::StreamUtt* stream_utt = nullptr;
    // live keyword events (kws_stream_detect_*): created by kws_stream_detect_open, dropped with the streams
    kws::StreamDetect* stream_detect = nullptr;

    // host ingest (kws_infer_host_i16): staging rings, copy streams, pack threads -- created on first use
    kws::Ingest* ingest = nullptr;

    // profiling
    bool prof = false;
    int prof_every = 1;                    // bracket every prof_every-th launch of a kernel id (kws_prof_enable)
    unsigned prof_seen[KWS_K_COUNT] = {};  // launches per kernel id since kws_prof_reset, timed or not
    struct EvPair {
        hipEvent_t a, b;
    };
    std::vector<EvPair> ev[KWS_K_COUNT];
    size_t ev_used[KWS_K_COUNT] = {};
    double ms_total[KWS_K_COUNT] = {};
    long launches[KWS_K_COUNT] = {};
};

// Front-end pieces kws_frontend.hip shares with kws_api.hip and kws_scan.hip
int frames_for(int n_samples, int frame_len, int frame_step);  // 1 + ceil((n - L) / step), 1 for n <= L (sigproc.py:31-35)
void set_clip_length(FrontendParams& p, int n_samples);
int ensure_refine(kws_ctx* c, int B, int num_frames);  // the refinement worklist holds B clips of num_frames frames
hipError_t stream_enqueue_frame(kws_ctx* c, const int16_t* d_hop, bool timed);  // kws_stream.hip: the frame kernel of a multi-launch push
void stream_free(kws_ctx* c);                          // kws_stream.hip: rings, hop counter, captured graph, smoothing and endpointer history
// The MFCC launches of B clips read from src (const int16_t*, const float* or kws::AugmentArgs; instantiated in kws_frontend.hip).
// recording_f32: float32 samples may take the wavefront-resident kernel (kws_frames_f32, kws_scan_f32).
template <typename Src>
int run_frontend(kws_ctx* c, const FrontendParams& geometry, Src src, int B, float* d_out, int refine_clips, bool recording_f32 = false);

inline thread_local std::string g_create_err;

inline int fail(kws_ctx* c, int code, const std::string& msg) {
    if (c)
        c->err = msg;
    else
        g_create_err = msg;
    return code;
}
inline int fail_hip(kws_ctx* c, hipError_t e, const char* what) {
    return fail(c, KWS_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}
// The zero-copy arrays of kws_stream_host_results (c->d_hr_logits among them) hold n_streams x the class count loaded when they
// were made, and neither DS-CNN loader retires them.  The host pushes call this before they hand c->d_hr_logits to a kernel:
// the arrays are made when absent and made again when the loaded model has another class count.
inline int host_results_ensure(kws_ctx* c) {
    if (c->h_stream_flag && c->host_results_classes == c->mw.num_classes) return KWS_OK;
    return kws_stream_host_results(c, 1);
}
// The fused kernels' one geometry; `what` is the rest of the refusal, in the words of the model and the flow.
inline int check_ref_map(kws_ctx* c, const char* fn, const char* what) {
    if (c->fp.num_frames == kws::IN_T && c->fp.numcep == kws::IN_F) return KWS_OK;
    return fail(c, KWS_EUNSUPPORTED, std::string(fn) + what);
}
inline int check_batch(kws_ctx* c, const void* in, int B, const char* fn) {
    if (!c) return KWS_EINVAL;
    if (!in) return fail(c, KWS_EINVAL, std::string(fn) + ": input pointer is NULL");
    if (B <= 0) return fail(c, KWS_EINVAL, std::string(fn) + ": B must be positive");
    return KWS_OK;
}
// The endpointer's argument checks, one text each for the entries that share them (kws_stream_vad_f32, kws_segment_f32,
// kws_stream_utt_open; kws_cut_i16, kws_stream_utt_cut_i16).
inline int check_endpoint_windows(kws_ctx* c, const char* fn, int on_window, int off_window) {
    const bool ok = on_window >= 1 && on_window <= off_window && off_window <= kws::EP_MAX_WINDOW;
    return ok ? KWS_OK : fail(c, KWS_EINVAL, std::string(fn) + ": need 1 <= on_window <= off_window <= 1024");
}
inline int check_append_energy(kws_ctx* c, const char* fn) {
    return c->fp.append_energy ? KWS_OK : fail(c, KWS_EUNSUPPORTED, std::string(fn) + ": needs cepstrum 0 = log frame energy (appendEnergy)");
}
inline int check_normalize_to(kws_ctx* c, const char* fn, int v) {
    return v >= 0 && v <= 32767 ? KWS_OK : fail(c, KWS_EINVAL, std::string(fn) + ": normalize_to must be in [0, 32767]");
}
// While a stream of the set is inactive (kws_stream_deactivate) only the fused push and the steps armed behind it are served: every
// other per-hop entry is a kernel of its own over all slots, which would need the list.  `what`: the route, in the entry's words.
inline int refuse_sparse(kws_ctx* c, const char* fn, const char* what) {
    if (!c->sparse()) return KWS_OK;
    return fail(c, KWS_EUNSUPPORTED, std::string(fn) + ": " + what + " run over every slot of the set, and " + std::to_string(c->n_streams - c->n_active) +
                                         " of its streams are inactive (kws_stream_deactivate); kws_stream_activate them first");
}
// No exception may cross the C ABI (ctypes would terminate the process): entry points that allocate host containers or
// start threads run their body between these two.
#define KWS_GUARD_BEGIN try {
#define KWS_GUARD_END(c, fn)                                                          \
    }                                                                                 \
    catch (const std::bad_alloc&) { return fail(c, KWS_ENOMEM, fn ": out of host memory"); } \
    catch (...) { return fail(c, KWS_EHIP, fn ": unexpected C++ exception"); }
#define HIP_TRY(c, expr)                                   \
    do {                                                   \
        hipError_t _e = (expr);                            \
        if (_e != hipSuccess) return fail_hip(c, _e, #expr); \
    } while (0)

// ep_ring_push's state for S streams, zeroed on the context's stream (history before the first frame is unvoiced).  On an
// error the caller resets the two (or lets them go).
inline int alloc_endpoint_state(kws_ctx* c, const char* fn, size_t S, DeviceBuffer<unsigned long long>& bits, DeviceBuffer<int>& counts) {
    if (!(bits.alloc(S * kws::EP_BIT_WORDS) && counts.alloc(S * 4))) return fail(c, KWS_ENOMEM, std::string(fn) + ": device allocation failed");
    hipError_t e = hipMemsetAsync(bits.get(), 0, sizeof(unsigned long long) * bits.size(), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(counts.get(), 0, sizeof(int) * counts.size(), c->stream);
    return e == hipSuccess ? KWS_OK : fail_hip(c, e, (std::string(fn) + ": hipMemsetAsync").c_str());
}

// Host-built plan tables of a ragged call -> context scratch (kws_ragged.hip); may wait for the stream.
int upload_ragged_tables(kws_ctx* c, const void* host, size_t bytes, const char* fn, const void** d_tables);
// What the four decision entries (kws_scan_detect_f32, kws_scan_score_f32, their ragged twins) share on the host, kws_scan.hip.
struct WindowBatch {          // the windows of R recordings among the rows of a logits array
    int R = 0;
    int W = 0;                // equal length: windows per recording; ragged: unused
    std::vector<int2> span;   // ragged: (first packed row, windows) per recording; empty for equal length
    long long first = 0, end = 0, total = 0;   // rows in use [first, end), windows of all recordings
    bool ragged() const { return !span.empty(); }
};
constexpr int MAX_RAGGED_RECORDINGS = 1 << 20;
// The two makers, each with its layout's own refusals (R >= 1 is decision_check's); fn names the entry in every refusal.
int scan_equal_windows(kws_ctx* c, const char* fn, int R, int W, WindowBatch& b);
int scan_ragged_spans(kws_ctx* c, const char* fn, const int32_t* win_off, const int32_t* windows, int R, WindowBatch& b);
// R and C, smooth_window, then refractory and first_keyword.  W: kws_scan_detect_f32 alone names its W in the first sentence (the
// score entry refuses W later, scan_equal_windows); recordings_first: kws_scan_detect_ragged_f32 alone refuses more than 2^20
// recordings ahead of smooth_window (the score entry later, scan_ragged_spans).
int decision_check(kws_ctx* c, const char* fn, int R, int C, int smooth_window, int first_keyword, int refractory, const int* W = nullptr,
                   bool recordings_first = false);
// Softmax over rows [first, end) into the context's scratch, then the layout's smoothing kernel -> per row of the logits array the
// smoothed top score and the candidate label (-1: none; at a threshold of -inf the argmax wherever it is a keyword).  d_span: b.span
// on the device -- the caller uploads it, alone or among its other tables -- or NULL for equal length.
struct ScanScratch { float* score; int32_t* cand; };
int scan_posteriors(kws_ctx* c, const char* fn, const WindowBatch& b, const int2* d_span, const float* d_logits, int C, int smooth_window,
                    int first_keyword, float threshold, float* d_smoothed, ScanScratch& out);

// Bracket a kernel launch with events when profiling is on (timed = false: never, e.g. inside a stream capture).
struct ProfScope {
    kws_ctx* c;
    int id;
    hipEvent_t stop = nullptr;
    ProfScope(kws_ctx* c_, int id_, bool timed = true) : c(c_), id(id_) {
        if (!c->prof || !timed) return;
        if (c->prof_seen[id]++ % (unsigned)c->prof_every != 0) return;  // sampling: events around every launch cost ~7 us of stream time each
        if (c->ev_used[id] == c->ev[id].size()) {
            kws_ctx::EvPair p{};
            if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) return;
            c->ev[id].push_back(p);
        }
        kws_ctx::EvPair& p = c->ev[id][c->ev_used[id]++];
        (void)hipEventRecord(p.a, c->stream);
        stop = p.b;
    }
    ~ProfScope() {
        if (stop) (void)hipEventRecord(stop, c->stream);
    }
};

// Retire the captured streaming push (it holds table and weight pointers by value); the caller has drained the stream.
inline void drop_stream_graph(kws_ctx* c) {
    if (c->stream_graph) (void)hipGraphExecDestroy(c->stream_graph);
    c->stream_graph = nullptr;
    c->graph_key[0] = c->graph_key[1] = c->graph_key[2] = nullptr;
}

// ... once the stream is idle, if there is one: what a change of anything the graph holds by value does first.
inline int retire_captured_push(kws_ctx* c) {
    if (!c->stream_graph) return KWS_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    drop_stream_graph(c);
    return KWS_OK;
}

// Swap a device allocation for a fresh copy of `bytes` host bytes (a multiple of sizeof(T)): drain the stream (kernels may be
// reading the old one), allocate, copy, and only then let the old allocation go.  On failure the context keeps what it had.
template <class T>
int replace_device_image(kws_ctx* c, DeviceBuffer<T>& buf, const void* host, size_t bytes, const char* fn) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    DeviceBuffer<T> d;
    if (!d.alloc(bytes / sizeof(T))) return fail(c, KWS_ENOMEM, std::string(fn) + ": device allocation failed");
    hipError_t e = hipMemcpy(d.get(), host, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail_hip(c, e, (std::string(fn) + ": hipMemcpy").c_str());
    buf = std::move(d);
    return KWS_OK;
}

// Grow a workspace to at least `need` elements (contents are not kept): nothing when it is large enough, else drain the
// stream, allocate, and only then let the old one go: a failed grow keeps it.  KWS_ENOMEM reads "<fn>: <what> allocation failed".
template <class T>
int grow_device_buffer(kws_ctx* c, DeviceBuffer<T>& buf, size_t need, const char* fn, const char* what) {
    if (need <= buf.size()) return KWS_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    DeviceBuffer<T> d;
    if (!d.alloc(need)) return fail(c, KWS_ENOMEM, std::string(fn) + ": " + what + " allocation failed");
    buf = std::move(d);
    return KWS_OK;
}
// Grow the context's float scratch (convolution outputs between two kernels of one call) to at least `need` floats.
inline int grow_conv_ws(kws_ctx* c, size_t need, const char* fn) {
    return grow_device_buffer(c, c->d_conv_ws, need, fn, "workspace");
}
