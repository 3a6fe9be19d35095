// Scanning recordings longer than a clip (include/kws_hip.h: kws_scan_i16 / kws_scan_f32, kws_scan_detect_f32, kws_host_scan_shape): ONE MFCC
// pass over each recording as one long clip, the DS-CNN over strided 99-frame windows of the frame array (kws_dscnn_fwd_kernel,
// SCAN), and the causal decision layer that turns the windows' logits into a short list of events.
#include "kws_ctx.h"
#include "kws_scan_dev.h"

using namespace kws;

namespace {

// The smoothing rule for row i of p, window w of its recording (the history never reaches before the recording's window 0):
// s[c] = the sum of p[v][c] over the last min(S, w + 1) windows, oldest first, divided by their number; k = first argmax.
// cand[i] = k when k is a keyword at or over the threshold, else -1; score[i] = s[k].  Shared by the equal-length and the
// ragged kernel.
__device__ __forceinline__ void scan_smooth_window(const float* p, int i, int w, int C, int S, int first_keyword,
                                                   float threshold, float* smoothed, int32_t* cand,
                                                   float* score) {
    const int terms = w + 1 < S ? w + 1 : S;
    const float* first = p + (size_t)(i - terms + 1) * C;
    const float count = (float)terms;
    float best = -1.f;
    int arg = 0;
    for (int c = 0; c < C; ++c) {
        float a = 0.f;
        for (int v = 0; v < terms; ++v) a += first[(size_t)v * C + c];
        a /= count;
        if (smoothed) smoothed[(size_t)i * C + c] = a;
        if (a > best) {
            best = a;
            arg = c;
        }
    }
    cand[i] = (arg >= first_keyword && best >= threshold) ? arg : -1;
    score[i] = best;
}

// Smoothed posteriors and candidates, one thread per window.  p: softmax rows [R * W][C] (launch_softmax).
__global__ __launch_bounds__(256) void kws_scan_smooth_kernel(const float* __restrict__ p, int n, int W, int C, int S, int first_keyword,
                                                              float threshold, float* __restrict__ smoothed, int32_t* __restrict__ cand,
                                                              float* __restrict__ score) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;  // r * W + w
    if (i >= n) return;
    scan_smooth_window(p, i, i % W, C, S, first_keyword, threshold, smoothed, cand, score);
}

// The refractory walk (scan_walk, kws_scan_dev.h), one wavefront per recording: a candidate is a window whose cand is a label;
// events land in window order with no atomics, and everything but the event stores is wave-uniform.
// cr / sr: the W candidates and scores of recording r (shared by the equal-length and the ragged kernel).
__device__ __forceinline__ void scan_events_walk(const int32_t* cr, const float* sr, int W, int refractory,
                                                 int32_t* ev_window, int32_t* ev_label,
                                                 float* ev_score, int max_events, int32_t* ev_count, int r,
                                                 int lane) {
    int k = -1;
    float sc = 0.f;
    const int count = scan_walk(
        W, refractory,
        [&](int w0) {
            const int w = w0 + lane;
            k = w < W ? cr[w] : -1;
            sc = w < W ? sr[w] : 0.f;
            return __ballot(k >= 0);
        },
        [&](int w0, int f, int n) {
            if (lane == f && n < max_events) {
                const size_t at = (size_t)r * max_events + n;
                ev_window[at] = w0 + lane;
                ev_label[at] = k;
                ev_score[at] = sc;
            }
        });
    if (lane == 0) ev_count[r] = count;
}
__global__ __launch_bounds__(64) void kws_scan_events_kernel(const int32_t* __restrict__ cand, const float* __restrict__ score, int W,
                                                             int refractory, int32_t* __restrict__ ev_window, int32_t* __restrict__ ev_label,
                                                             float* __restrict__ ev_score, int max_events, int32_t* __restrict__ ev_count) {
    const int r = blockIdx.x, lane = threadIdx.x;
    scan_events_walk(cand + (size_t)r * W, score + (size_t)r * W, W, refractory, ev_window, ev_label, ev_score, max_events, ev_count, r,
                     lane);
}

// The same two steps over the packed windows of a ragged batch (kws_scan_detect_ragged_f32).  span[r] = (first packed window,
// windows) of recording r, first windows ascending; a packed row between two recordings' windows belongs to nobody and is
// passed over.  One thread per packed row finds its recording by a binary search; one wavefront per recording walks.
__global__ __launch_bounds__(256) void kws_scan_smooth_ragged_kernel(const float* __restrict__ p, int n, const int2* __restrict__ span, int R,
                                                                     int C, int S, int first_keyword, float threshold,
                                                                     float* __restrict__ smoothed, int32_t* __restrict__ cand,
                                                                     float* __restrict__ score) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;  // packed window
    if (i >= n) return;
    int lo = 0, hi = R;  // span[lo].x <= i < span[hi].x (a row before span[0].x lands on recording 0 with w < 0)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (span[mid].x <= i) lo = mid;
        else hi = mid;
    }
    const int2 sp = span[lo];
    const int w = i - sp.x;
    if (w < 0 || w >= sp.y) return;
    scan_smooth_window(p, i, w, C, S, first_keyword, threshold, smoothed, cand, score);
}
__global__ __launch_bounds__(64) void kws_scan_events_ragged_kernel(const int32_t* __restrict__ cand, const float* __restrict__ score,
                                                                    const int2* __restrict__ span, int refractory,
                                                                    int32_t* __restrict__ ev_window, int32_t* __restrict__ ev_label,
                                                                    float* __restrict__ ev_score, int max_events,
                                                                    int32_t* __restrict__ ev_count) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const int2 sp = span[r];
    scan_events_walk(cand + sp.x, score + sp.x, sp.y, refractory, ev_window, ev_label, ev_score, max_events, ev_count, r, lane);
}

}  // namespace

static int events_check(kws_ctx* c, const char* fn, int max_events, const int32_t* d_event_window, const int32_t* d_event_label, const float* d_event_score) {
    if (max_events < 0 || (max_events > 0 && (!d_event_window || !d_event_label || !d_event_score)))
        return fail(c, KWS_EINVAL, std::string(fn) + ": max_events events need their three arrays");
    return KWS_OK;
}

int decision_check(kws_ctx* c, const char* fn, int R, int C, int smooth_window, int first_keyword, int refractory, const int* W,
                   bool recordings_first) {
    const std::string f(fn);
    if (R < 1 || (W && *W < 1) || C < 1 || C > MAX_CLASSES)
        return fail(c, KWS_EINVAL, f + (W ? ": need R >= 1, W >= 1 and C in [1, 64]" : ": need R >= 1 and C in [1, 64]"));
    if (recordings_first && R > MAX_RAGGED_RECORDINGS) return fail(c, KWS_EUNSUPPORTED, f + ": more than 2^20 recordings in one call");
    if (smooth_window < 1 || smooth_window > 256) return fail(c, KWS_EINVAL, f + ": smooth_window must be in [1, 256]");
    if (refractory < 1 || first_keyword < 0) return fail(c, KWS_EINVAL, f + ": need refractory >= 1 and first_keyword >= 0");
    return KWS_OK;
}

int scan_equal_windows(kws_ctx* c, const char* fn, int R, int W, WindowBatch& b) {
    if (W < 1) return fail(c, KWS_EINVAL, std::string(fn) + ": need W >= 1");
    if ((unsigned long long)R * W > (1ull << 30)) return fail(c, KWS_EUNSUPPORTED, std::string(fn) + ": more than 2^30 windows in one call");
    b.R = R;
    b.W = W;
    b.end = b.total = (long long)R * W;
    return KWS_OK;
}

int scan_ragged_spans(kws_ctx* c, const char* fn, const int32_t* win_off, const int32_t* windows, int R, WindowBatch& b) {
    const std::string f(fn);
    if (R > MAX_RAGGED_RECORDINGS) return fail(c, KWS_EUNSUPPORTED, f + ": more than 2^20 recordings in one call");
    b.R = R;
    b.span.resize(R);
    for (int r = 0; r < R; ++r) {
        if (windows[r] < 0 || win_off[r] < b.end)
            return fail(c, KWS_EINVAL, f + ": windows must not be negative and the recordings' windows must not overlap "
                                       "(win_off ascending, win_off[r] >= win_off[r - 1] + windows[r - 1])");
        b.span[r] = make_int2(win_off[r], windows[r]);
        b.end = (long long)win_off[r] + windows[r];
        b.total += windows[r];
        if (b.end > (1ll << 30)) return fail(c, KWS_EUNSUPPORTED, f + ": more than 2^30 packed windows in one call");
    }
    b.first = win_off[0];
    return KWS_OK;
}

// Context scratch, indexed by row of the logits array: posteriors [end][C], then per row the score and the candidate label.
int scan_posteriors(kws_ctx* c, const char* fn, const WindowBatch& b, const int2* d_span, const float* d_logits, int C, int smooth_window,
                    int first_keyword, float threshold, float* d_smoothed, ScanScratch& out) {
    const size_t n = (size_t)b.end;
    if (int rc = grow_device_buffer(c, c->d_conv_ws, n * C + 2 * n, fn, "workspace")) return rc;
    float* prob = c->d_conv_ws.get();
    float* score = prob + n * C;
    int32_t* cand = reinterpret_cast<int32_t*>(score + n);
    HIP_TRY(c, launch_softmax(c->stream, d_logits + (size_t)b.first * C, (int)(b.end - b.first), C, prob + (size_t)b.first * C));
    const dim3 grid((unsigned)((n + 255) / 256));
    if (b.ragged())
        hipLaunchKernelGGL(kws_scan_smooth_ragged_kernel, grid, dim3(256), 0, c->stream, prob, (int)n, d_span, b.R, C, smooth_window,
                           first_keyword, threshold, d_smoothed, cand, score);
    else
        hipLaunchKernelGGL(kws_scan_smooth_kernel, grid, dim3(256), 0, c->stream, prob, (int)n, b.W, C, smooth_window, first_keyword, threshold,
                           d_smoothed, cand, score);
    HIP_TRY(c, hipGetLastError());
    out = {score, cand};
    return KWS_OK;
}

// The refractory walk of every recording over what scan_posteriors left.
static hipError_t launch_scan_events(hipStream_t s, const WindowBatch& b, const int2* d_span, const int32_t* d_cand, const float* d_score,
                                     int refractory, int32_t* d_event_window, int32_t* d_event_label, float* d_event_score, int max_events,
                                     int32_t* d_event_count) {
    if (b.ragged())
        hipLaunchKernelGGL(kws_scan_events_ragged_kernel, dim3(b.R), dim3(64), 0, s, d_cand, d_score, d_span, refractory, d_event_window,
                           d_event_label, d_event_score, max_events, d_event_count);
    else
        hipLaunchKernelGGL(kws_scan_events_kernel, dim3(b.R), dim3(64), 0, s, d_cand, d_score, b.W, refractory, d_event_window,
                           d_event_label, d_event_score, max_events, d_event_count);
    return hipGetLastError();
}

// kws_scan_detect_f32 and its ragged twin behind their own pointer checks and the making of b; d_span: b.span on the device.
static int scan_detect(kws_ctx* c, const char* fn, const WindowBatch& b, const int2* d_span, const float* d_logits, int C, int smooth_window,
                       int first_keyword, float threshold, int refractory, float* d_smoothed, int32_t* d_event_window,
                       int32_t* d_event_label, float* d_event_score, int max_events, int32_t* d_event_count) {
    ScanScratch ws;
    if (int rc = scan_posteriors(c, fn, b, d_span, d_logits, C, smooth_window, first_keyword, threshold, d_smoothed, ws)) return rc;
    HIP_TRY(c, launch_scan_events(c->stream, b, d_span, ws.cand, ws.score, refractory, d_event_window, d_event_label, d_event_score, max_events,
                                  d_event_count));
    return KWS_OK;
}

// kws_scan_i16 / kws_scan_f32 and their cnn-trad-fpool3 twins: the same checks, limits and launches over int16 PCM or float32
// samples; f names the entry in the error text, src_name its source pointer, m is the model that classifies the windows.
template <typename Sample>
static int scan_recordings(kws_ctx* c, const ModelOps& m, const std::string& f, const char* src_name, const Sample* d_pcm, int R, int n_total,
                           int hop_frames, float* d_logits, int32_t* d_label, float* d_feat_out) {
    if (!c) return KWS_EINVAL;
    if (!d_pcm || !d_logits) return fail(c, KWS_EINVAL, f + ": " + src_name + " / d_logits is NULL");
    if (R < 1 || n_total < 1 || hop_frames < 1) return fail(c, KWS_EINVAL, f + ": R, n_total and hop_frames must be positive");
    if (int rc = m.scan_check(c, f.c_str())) return rc;
    if (n_total > (1 << 30)) return fail(c, KWS_EUNSUPPORTED, f + ": more than 2^30 samples per recording");
    FrontendParams p = c->fp;  // the context's geometry and arithmetic; the recording is one clip of n_total samples
    set_clip_length(p, n_total);
    const int T = c->fp.num_frames, F = p.num_frames;
    if (F < T) return fail(c, KWS_EINVAL, f + ": the recording is shorter than one window");
    const int W = (F - T) / hop_frames + 1;
    if ((unsigned long long)R * F > (1ull << 28) || (unsigned long long)R * W > (1ull << 30))
        return fail(c, KWS_EUNSUPPORTED, f + ": more than 2^28 frames or 2^30 windows in one call");
    HIP_TRY(c, hipSetDevice(c->device));
    float* feat = d_feat_out;
    if (!feat) {
        int rc = grow_device_buffer(c, c->d_scan_ws, (size_t)R * F * p.numcep, f.c_str(), "frame workspace");
        if (rc) return rc;
        feat = c->d_scan_ws.get();
    }
    // the refinement's grid: the batch in one-second clips (R * F <= 2^28 was checked above)
    int rc = run_frontend(c, p, d_pcm, R, feat, (int)((unsigned long long)R * F / T + 1), /*recording_f32=*/true);
    if (rc) return rc;
    return m.windows(c, f.c_str(), feat, R, F, W, hop_frames, d_logits, d_label);
}

#pragma GCC visibility push(default)
extern "C" {

int kws_host_scan_shape(int n_total, int frame_len, int frame_step, int window_frames, int hop_frames, int* frames_total,
                        int* n_windows) {
    if (n_total <= 0 || frame_len <= 0 || frame_step <= 0 || window_frames <= 0 || hop_frames <= 0) return KWS_EINVAL;
    const int F = frames_for(n_total, frame_len, frame_step);
    if (frames_total) *frames_total = F;
    if (n_windows) *n_windows = F < window_frames ? 0 : (F - window_frames) / hop_frames + 1;
    return KWS_OK;
}

int kws_scan_i16(kws_ctx* c, const int16_t* d_pcm, int R, int n_total, int hop_frames, float* d_logits, int32_t* d_label,
                 float* d_feat_out) {
    KWS_GUARD_BEGIN
    return scan_recordings(c, model_ops_dscnn(), "kws_scan_i16", "d_pcm", d_pcm, R, n_total, hop_frames, d_logits, d_label, d_feat_out);
    KWS_GUARD_END(c, "kws_scan_i16")
}

int kws_scan_f32(kws_ctx* c, const float* d_wav, int R, int n_total, int hop_frames, float* d_logits, int32_t* d_label,
                 float* d_feat_out) {
    KWS_GUARD_BEGIN
    return scan_recordings(c, model_ops_dscnn(), "kws_scan_f32", "d_wav", d_wav, R, n_total, hop_frames, d_logits, d_label, d_feat_out);
    KWS_GUARD_END(c, "kws_scan_f32")
}

int kws_scan_cnn_trad_i16(kws_ctx* c, const int16_t* d_pcm, int R, int n_total, int hop_frames, float* d_logits, int32_t* d_label,
                          float* d_feat_out) {
    KWS_GUARD_BEGIN
    return scan_recordings(c, model_ops_cnn_trad(), "kws_scan_cnn_trad_i16", "d_pcm", d_pcm, R, n_total, hop_frames, d_logits, d_label, d_feat_out);
    KWS_GUARD_END(c, "kws_scan_cnn_trad_i16")
}

int kws_scan_cnn_trad_f32(kws_ctx* c, const float* d_wav, int R, int n_total, int hop_frames, float* d_logits, int32_t* d_label,
                          float* d_feat_out) {
    KWS_GUARD_BEGIN
    return scan_recordings(c, model_ops_cnn_trad(), "kws_scan_cnn_trad_f32", "d_wav", d_wav, R, n_total, hop_frames, d_logits, d_label, d_feat_out);
    KWS_GUARD_END(c, "kws_scan_cnn_trad_f32")
}

int kws_scan_detect_f32(kws_ctx* c, const float* d_logits, int R, int W, int C, int smooth_window, int first_keyword, float threshold,
                        int refractory, float* d_smoothed, int32_t* d_event_window, int32_t* d_event_label, float* d_event_score,
                        int max_events, int32_t* d_event_count) {
    const char* fn = "kws_scan_detect_f32";
    KWS_GUARD_BEGIN
    if (!c) return KWS_EINVAL;
    if (!d_logits || !d_event_count) return fail(c, KWS_EINVAL, "kws_scan_detect_f32: d_logits / d_event_count is NULL");
    if (int rc = events_check(c, fn, max_events, d_event_window, d_event_label, d_event_score)) return rc;
    if (int rc = decision_check(c, fn, R, C, smooth_window, first_keyword, refractory, &W)) return rc;
    WindowBatch b;
    if (int rc = scan_equal_windows(c, fn, R, W, b)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    return scan_detect(c, fn, b, nullptr, d_logits, C, smooth_window, first_keyword, threshold, refractory, d_smoothed, d_event_window,
                       d_event_label, d_event_score, max_events, d_event_count);
    KWS_GUARD_END(c, "kws_scan_detect_f32")
}

int kws_scan_detect_ragged_f32(kws_ctx* c, const float* d_logits, const int32_t* win_off, const int32_t* windows, int R, int C,
                               int smooth_window, int first_keyword, float threshold, int refractory, float* d_smoothed,
                               int32_t* d_event_window, int32_t* d_event_label, float* d_event_score, int max_events,
                               int32_t* d_event_count) {
    const char* fn = "kws_scan_detect_ragged_f32";
    KWS_GUARD_BEGIN
    if (!c) return KWS_EINVAL;
    if (!d_logits || !d_event_count || !win_off || !windows)
        return fail(c, KWS_EINVAL, "kws_scan_detect_ragged_f32: d_logits / d_event_count / win_off / windows is NULL");
    if (int rc = events_check(c, fn, max_events, d_event_window, d_event_label, d_event_score)) return rc;
    if (int rc = decision_check(c, fn, R, C, smooth_window, first_keyword, refractory, nullptr, /*recordings_first=*/true)) return rc;
    WindowBatch b;
    if (int rc = scan_ragged_spans(c, fn, win_off, windows, R, b)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if (b.total == 0) {  // no recording has a window: every count is 0
        HIP_TRY(c, hipMemsetAsync(d_event_count, 0, sizeof(int32_t) * (size_t)R, c->stream));
        return KWS_OK;
    }
    const int2* d_span = nullptr;
    if (int rc = upload_ragged_tables(c, b.span.data(), sizeof(int2) * b.span.size(), fn, reinterpret_cast<const void**>(&d_span))) return rc;
    return scan_detect(c, fn, b, d_span, d_logits, C, smooth_window, first_keyword, threshold, refractory, d_smoothed, d_event_window,
                       d_event_label, d_event_score, max_events, d_event_count);
    KWS_GUARD_END(c, "kws_scan_detect_ragged_f32")
}

}  // extern "C"
#pragma GCC visibility pop
