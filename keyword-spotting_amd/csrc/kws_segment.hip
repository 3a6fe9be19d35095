// Utterances from recordings (include/kws_hip.h: kws_frames_i16 / _f32, kws_segment_f32, kws_cut_i16 / _f32) -- the device side of the
// reference's record-then-classify loop (kws/inference/inference_local.py:114-192): the MFCC pass of a scan on its own, the
// energy endpointer walked over a whole frame array with the reference's start point and time-out, and normalize + fix_length
// for a list of sample spans.  What follows a clip (kws_infer_i16) is elsewhere; nothing here touches another unit's kernels.
#include "kws_ctx.h"  // kws_endpoint_dev.h: the endpointer's rules and the clip cut

using namespace kws;

namespace {

constexpr int SEG_THREADS = 256;                 // frames per workgroup of the flag kernel: four ballot words
constexpr int SEG_WORDS = SEG_THREADS / 64;
constexpr int SEG_BACK_WORDS = EP_BIT_WORDS;     // ballot words of history a workgroup can need: ceil((1024 - 1) / 64)
constexpr int CUT_THREADS = 256;

// Voiced frames among the `window` frames ending at local frame `at` (bit b of words[j] = local frame 64 j + b; at >= window - 1).
__device__ __forceinline__ int voiced_in_window(const unsigned long long* words, int at, int window) {
    const int lo = at - window + 1;
    const int j0 = lo >> 6, j1 = at >> 6;
    int n = 0;
    for (int j = j0; j <= j1; ++j) {
        unsigned long long m = words[j];
        if (j == j0) m &= ~0ull << (lo & 63);
        if (j == j1) m &= ~0ull >> (63 - (at & 63));
        n += __popcll(m);
    }
    return n;
}

// Per frame: may an utterance open here, may one close here?  One thread per frame, 256 frames of one recording per workgroup.
// The workgroup first packs the voiced flags of its own frames and of the `back` words before them (frames before 0 and past
// F are unvoiced) into ballot words in LDS -- wavefront v takes words v, v + 4, ... -- then every thread counts its two
// windows as popcounts over at most 17 words and the wavefront's answers leave as two ballot words:
//   open_ok[f]  = ep_opens(c_on[f], on_window),  close_ok[f] = ep_closes(c_off[f], off_window).
// ok: [R][2][n_words], n_words = ceil(F / 64); bits at or beyond F are zero.
// segment_flags_group: the work of one workgroup -- frames f0 .. f0 + 255 of the recording whose F frames start at fr and whose
// two rows of n_words ballot words start at o (shared by the equal-length and the ragged kernel).
__device__ __forceinline__ void segment_flags_group(const float* fr, int F, int numcep, float threshold, int on_window,
                                                    int off_window, int back, int n_words, int f0, unsigned long long* o,
                                                    unsigned long long* words) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int base = f0 - back * 64;  // the frame of bit 0 of words[0]; may be negative
    for (int j = wave; j < back + SEG_WORDS; j += SEG_WORDS) {  // wave-uniform
        const int g = base + j * 64 + lane;
        const bool voiced = g >= 0 && g < F && ep_voiced(fr[(size_t)g * numcep], threshold);
        const unsigned long long b = __ballot(voiced);
        if (lane == 0) words[j] = b;
    }
    __syncthreads();
    const int f = f0 + threadIdx.x;
    const int at = back * 64 + threadIdx.x;  // back * 64 >= off_window - 1: both windows start inside words[]
    const int c_on = voiced_in_window(words, at, on_window);
    const int c_off = voiced_in_window(words, at, off_window);
    const unsigned long long open_ok = __ballot(f < F && ep_opens(c_on, on_window));
    const unsigned long long close_ok = __ballot(f < F && ep_closes(c_off, off_window));
    const int w = f0 / 64 + wave;
    if (lane == 0 && w < n_words) {
        o[w] = open_ok;
        o[n_words + w] = close_ok;
    }
}
__global__ __launch_bounds__(SEG_THREADS) void kws_segment_flags_kernel(const float* __restrict__ feat, int F, int numcep, float threshold,
                                                                        int on_window, int off_window, int back, int n_words,
                                                                        int groups_per_rec, unsigned long long* __restrict__ ok) {
    __shared__ unsigned long long words[SEG_BACK_WORDS + SEG_WORDS];
    const int r = blockIdx.x / groups_per_rec;
    segment_flags_group(feat + (size_t)r * F * numcep, F, numcep, threshold, on_window, off_window, back, n_words,
                        (blockIdx.x % groups_per_rec) * SEG_THREADS, ok + (size_t)r * 2 * n_words, words);
}

// A recording of a ragged batch as the two kernels see it (kws_segment_ragged_f32): rows [frame_off, frame_off + frames) of the
// packed frame array, len samples, its ballot words at ok + 2 * word_off, its workgroups [group_off, next record's group_off) of
// the flag launch.  R + 1 records; the last one closes the group table.
struct SegRec {
    int frame_off, frames, len, word_off, group_off;
};
__global__ __launch_bounds__(SEG_THREADS) void kws_segment_flags_ragged_kernel(const float* __restrict__ feat, const SegRec* __restrict__ rec,
                                                                               int R, int numcep, float threshold, int on_window,
                                                                               int off_window, int back, unsigned long long* __restrict__ ok) {
    __shared__ unsigned long long words[SEG_BACK_WORDS + SEG_WORDS];
    const int g = blockIdx.x;
    int lo = 0, hi = R;  // rec[lo].group_off <= g < rec[hi].group_off (workgroup-uniform)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rec[mid].group_off <= g) lo = mid;
        else hi = mid;
    }
    const SegRec rr = rec[lo];
    segment_flags_group(feat + (size_t)rr.frame_off * numcep, rr.frames, numcep, threshold, on_window, off_window, back,
                        (rr.frames + 63) / 64, (g - rr.group_off) * SEG_THREADS, ok + 2 * (size_t)rr.word_off, words);
}

// The walk, one wavefront per recording.  Every lane holds one open_ok and one close_ok word of a chunk of 64 words (4096
// frames); the walk alternates between "first open_ok at or after f" and "first close_ok after the open, or the time-out at
// open + max_frames - 1"; words without a bit are passed over through a ballot of the non-empty lanes, so a chunk costs a few
// steps per utterance, not one per word.  f moves forward in every iteration, so the loop ends for any input.  Everything is
// wave-uniform; lane 0 stores.  utt: [R][max_utts][5] = (start_sample, end_sample, open, close, reason).
// segment_walk: the walk of recording r, whose ballot words start at o (shared by the equal-length and the ragged kernel).
__device__ __forceinline__ void segment_walk(const unsigned long long* o, int F, int n_words, int n_total, int frame_len,
                                             int frame_step, int pre_roll, int max_frames, int32_t* utt, int max_utts,
                                             int32_t* count_out, int r, int lane) {
    int32_t* ur = utt + (size_t)r * max_utts * 5;
    bool triggered = false;
    int open = 0, prev_close = -1, count = 0;
    auto close_at = [&](int f, int reason) {
        const long long start = ep_span_start(open, pre_roll, prev_close);
        const long long end = (long long)f * frame_step + frame_len;
        if (lane == 0 && count < max_utts) {
            int32_t* u = ur + (size_t)count * 5;
            u[0] = (int32_t)(start * frame_step);
            u[1] = (int32_t)(end < n_total ? end : n_total);
            u[2] = open;
            u[3] = f;
            u[4] = reason;
        }
        ++count;
        prev_close = f;
        triggered = false;
    };
    int f = 0;
    for (int w0 = 0; w0 < n_words; w0 += 64) {
        const int mine = w0 + lane;
        const unsigned long long open_w = mine < n_words ? o[mine] : 0ull;
        const unsigned long long close_w = mine < n_words ? o[n_words + mine] : 0ull;
        const int chunk_end = (w0 + 64 < n_words ? w0 + 64 : n_words) * 64;  // first frame past this chunk's words
        const unsigned long long open_any = __ballot(open_w != 0), close_any = __ballot(close_w != 0);  // lanes whose word has a bit
        // the first frame of the next word of this chunk, after word w, that `any` marks; the chunk's end when there is none
        auto skip_to = [&](unsigned long long any, int w) {
            const unsigned long long rest = w - w0 < 63 ? any & (~0ull << (w - w0 + 1)) : 0ull;
            return rest ? (w0 + __builtin_ctzll(rest)) * 64 : chunk_end;
        };
        while (f < chunk_end) {  // f == w0 * 64 on entry: no step below passes the chunk's end
            const int w = f >> 6;
            const unsigned long long from = ~0ull << (f & 63);
            const int next_word = (w + 1) * 64;
            if (!triggered) {
                const unsigned long long m = __shfl(open_w, w - w0) & from;
                if (!m) {
                    f = skip_to(open_any, w);
                    continue;
                }
                open = w * 64 + __builtin_ctzll(m);
                triggered = true;
                f = open + 1;  // nothing else happens at the opening frame
                continue;
            }
            const unsigned long long m = __shfl(close_w, w - w0) & from;
            const long long limit = max_frames > 0 ? (long long)open + max_frames - 1 : (long long)F;  // >= f: max_frames >= 2
            const int cand = m ? w * 64 + __builtin_ctzll(m) : next_word;
            if (m && cand <= limit) {
                close_at(cand, 0);
                f = cand + 1;
            } else if (limit < next_word && limit < F) {
                close_at((int)limit, 1);
                f = (int)limit + 1;
            } else {  // neither in this word: on to the next word with a close_ok bit, or to the time-out's word if that comes first
                int next = skip_to(close_any, w);
                if (limit < F && (int)(limit >> 6) * 64 < next) next = (int)(limit >> 6) * 64;  // limit >= next_word here: still forward
                f = next;
            }
        }
    }
    if (triggered) close_at(F - 1, 2);  // the recording ended inside an utterance
    if (lane == 0) count_out[r] = count;
}
__global__ __launch_bounds__(64) void kws_segment_walk_kernel(const unsigned long long* __restrict__ ok, int F, int n_words, int n_total,
                                                              int frame_len, int frame_step, int pre_roll, int max_frames,
                                                              int32_t* __restrict__ utt, int max_utts, int32_t* __restrict__ count_out) {
    const int r = blockIdx.x, lane = threadIdx.x;
    segment_walk(ok + (size_t)r * 2 * n_words, F, n_words, n_total, frame_len, frame_step, pre_roll, max_frames, utt, max_utts, count_out, r,
                 lane);
}
__global__ __launch_bounds__(64) void kws_segment_walk_ragged_kernel(const unsigned long long* __restrict__ ok, const SegRec* __restrict__ rec,
                                                                     int frame_len, int frame_step, int pre_roll, int max_frames,
                                                                     int32_t* __restrict__ utt, int max_utts, int32_t* __restrict__ count_out) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const SegRec rr = rec[r];
    segment_walk(ok + 2 * (size_t)rr.word_off, rr.frames, (rr.frames + 63) / 64, rr.len, frame_len, frame_step, pre_roll, max_frames, utt,
                 max_utts, count_out, r, lane);
}

// Span u of d_span = (recording, start, end), as both cut kernels read it: start and end clamped to [0, n_total], a recording
// index outside [0, R) refused (workgroup-uniform); returns the span's first sample in the [R, n_total] buffer x.
template <typename T>
__device__ __forceinline__ const T* cut_span(const T* __restrict__ x, const int32_t* __restrict__ span, int u, int R, int n_total, bool& in_range,
                                             int& len) {
    const int r = span[3 * (size_t)u];
    int start = span[3 * (size_t)u + 1], end = span[3 * (size_t)u + 2];
    start = start < 0 ? 0 : (start > n_total ? n_total : start);
    end = end < 0 ? 0 : (end > n_total ? n_total : end);
    in_range = r >= 0 && r < R;  // workgroup-uniform
    len = in_range && end > start ? end - start : 0;
    return x + (in_range ? (size_t)r * n_total + start : 0);
}

// normalize then fix_length (ep_cut_clip) of one span per workgroup.  A span starts at any sample: 2-byte loads.
__global__ __launch_bounds__(CUT_THREADS) void kws_cut_i16_kernel(const int16_t* __restrict__ pcm, int R, int n_total,
                                                                  const int32_t* __restrict__ span, int normalize_to,
                                                                  int16_t* __restrict__ clips, int n_out, int32_t* __restrict__ peak_out) {
    const int u = blockIdx.x;
    bool in_range;
    int len;
    const int16_t* x = cut_span(pcm, span, u, R, n_total, in_range, len);
    ep_cut_clip<CUT_THREADS>([&](unsigned i) -> int { return x[i]; }, len, in_range, normalize_to, clips + (size_t)u * n_out, n_out, peak_out, u);
}
// The same over float32 samples (ep_cut_clip_f32: a float32 peak, a float64 scale, one rounding to float32 and no truncation).
__global__ __launch_bounds__(CUT_THREADS) void kws_cut_f32_kernel(const float* __restrict__ wav, int R, int n_total,
                                                                  const int32_t* __restrict__ span, float normalize_to,
                                                                  float* __restrict__ clips, int n_out, float* __restrict__ peak_out) {
    const int u = blockIdx.x;
    bool in_range;
    int len;
    const float* x = cut_span(wav, span, u, R, n_total, in_range, len);
    ep_cut_clip_f32<CUT_THREADS>([&](unsigned i) -> float { return x[i]; }, len, in_range, normalize_to, clips + (size_t)u * n_out, n_out, peak_out, u);
}

}  // namespace

// kws_frames_i16 / kws_frames_f32: the same checks, limits and launches over int16 PCM or float32 samples; f names the entry in
// the error text, src_name its source pointer.
template <typename T>
static int frames_recordings(kws_ctx* c, const std::string& f, const char* src_name, const T* d_pcm, int R, int n_total, float* d_feat_out) {
    if (!c) return KWS_EINVAL;
    if (!d_pcm || !d_feat_out) return fail(c, KWS_EINVAL, f + ": " + src_name + " / d_feat_out is NULL");
    if (R < 1 || n_total < 1) return fail(c, KWS_EINVAL, f + ": R and n_total must be positive");
    if (!c->fe_ready) return fail(c, KWS_ESTATE, f + ": front end not configured");
    if (n_total > (1 << 30)) return fail(c, KWS_EUNSUPPORTED, f + ": more than 2^30 samples per recording");
    FrontendParams p = c->fp;  // the context's geometry and arithmetic; the recording is one clip of n_total samples
    set_clip_length(p, n_total);
    const int F = p.num_frames;
    if ((unsigned long long)R * F > (1ull << 28)) return fail(c, KWS_EUNSUPPORTED, f + ": more than 2^28 frames in one call");
    // the refinement's grid: the batch in clips of the context's own length, as kws_scan_i16 sizes it
    return run_frontend(c, p, d_pcm, R, d_feat_out, (int)((unsigned long long)R * F / c->fp.num_frames + 1), /*recording_f32=*/true);
}

// What kws_segment_f32 and its ragged twin check alike, behind their own pointer and count checks and ahead of their size limits.
static int segment_check(kws_ctx* c, const char* fn, int on_window, int off_window, int pre_roll, int max_frames, const int32_t* d_utt,
                         int max_utts) {
    const std::string f(fn);
    if (int rc = check_endpoint_windows(c, fn, on_window, off_window)) return rc;
    if (pre_roll < 0 || (max_frames != 0 && max_frames < 2)) return fail(c, KWS_EINVAL, f + ": need pre_roll >= 0 and max_frames == 0 or >= 2");
    if (max_utts < 0 || (max_utts > 0 && !d_utt)) return fail(c, KWS_EINVAL, f + ": max_utts utterances need d_utt");
    if (!c->fe_ready) return fail(c, KWS_ESTATE, f + ": front end not configured");
    return check_append_energy(c, fn);
}

#pragma GCC visibility push(default)
extern "C" {

int kws_frames_i16(kws_ctx* c, const int16_t* d_pcm, int R, int n_total, float* d_feat_out) {
    KWS_GUARD_BEGIN
    return frames_recordings(c, "kws_frames_i16", "d_pcm", d_pcm, R, n_total, d_feat_out);
    KWS_GUARD_END(c, "kws_frames_i16")
}

int kws_frames_f32(kws_ctx* c, const float* d_wav, int R, int n_total, float* d_feat_out) {
    KWS_GUARD_BEGIN
    return frames_recordings(c, "kws_frames_f32", "d_wav", d_wav, R, n_total, d_feat_out);
    KWS_GUARD_END(c, "kws_frames_f32")
}

int kws_segment_f32(kws_ctx* c, const float* d_feat, int R, int F_total, int n_total, float log_energy_threshold, int on_window,
                    int off_window, int pre_roll, int max_frames, int32_t* d_utt, int max_utts, int32_t* d_count) {
    if (!c) return KWS_EINVAL;
    if (!d_feat || !d_count) return fail(c, KWS_EINVAL, "kws_segment_f32: d_feat / d_count is NULL");
    if (R < 1 || F_total < 1 || n_total < 1) return fail(c, KWS_EINVAL, "kws_segment_f32: R, F_total and n_total must be positive");
    int rc = segment_check(c, "kws_segment_f32", on_window, off_window, pre_roll, max_frames, d_utt, max_utts);
    if (rc) return rc;
    if ((unsigned long long)R * F_total > (1ull << 28)) return fail(c, KWS_EUNSUPPORTED, "kws_segment_f32: more than 2^28 frames in one call");
    HIP_TRY(c, hipSetDevice(c->device));
    // context scratch: open_ok and close_ok as ballot words, [R][2][n_words] of 64 bits
    const int n_words = (F_total + 63) / 64;
    rc = grow_device_buffer(c, c->d_conv_ws, (size_t)R * 2 * n_words * 2, "kws_segment_f32", "workspace");
    if (rc) return rc;
    unsigned long long* ok = reinterpret_cast<unsigned long long*>(c->d_conv_ws.get());
    const int back = (off_window - 1 + 63) / 64;  // words of history before a workgroup's first frame: <= 16
    const int groups_per_rec = (F_total + SEG_THREADS - 1) / SEG_THREADS;  // R * groups_per_rec <= 2^28 / 256 + R workgroups
    hipLaunchKernelGGL(kws_segment_flags_kernel, dim3((unsigned)R * (unsigned)groups_per_rec), dim3(SEG_THREADS), 0, c->stream, d_feat,
                       F_total, c->fp.numcep, log_energy_threshold, on_window, off_window, back, n_words, groups_per_rec, ok);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(kws_segment_walk_kernel, dim3(R), dim3(64), 0, c->stream, ok, F_total, n_words, n_total, c->fp.frame_len,
                       c->fp.frame_step, pre_roll, max_frames, d_utt, max_utts, d_count);
    HIP_TRY(c, hipGetLastError());
    return KWS_OK;
}

int kws_segment_ragged_f32(kws_ctx* c, const float* d_feat, const int32_t* frame_off, const int32_t* frames, const int32_t* len, int R,
                           float log_energy_threshold, int on_window, int off_window, int pre_roll, int max_frames, int32_t* d_utt,
                           int max_utts, int32_t* d_count) {
    KWS_GUARD_BEGIN
    if (!c) return KWS_EINVAL;
    if (!d_feat || !d_count || !frame_off || !frames || !len)
        return fail(c, KWS_EINVAL, "kws_segment_ragged_f32: d_feat / d_count / frame_off / frames / len is NULL");
    if (R < 1) return fail(c, KWS_EINVAL, "kws_segment_ragged_f32: R must be positive");
    if (R > (1 << 20)) return fail(c, KWS_EUNSUPPORTED, "kws_segment_ragged_f32: more than 2^20 recordings in one call");
    int rc = segment_check(c, "kws_segment_ragged_f32", on_window, off_window, pre_roll, max_frames, d_utt, max_utts);
    if (rc) return rc;
    std::vector<SegRec> rec(R + 1);
    long long words = 0, groups = 0, rows_end = 0;
    for (int r = 0; r < R; ++r) {
        if (frames[r] < 1 || len[r] < 1 || frame_off[r] < rows_end)
            return fail(c, KWS_EINVAL, "kws_segment_ragged_f32: frames and len must be positive and the recordings' rows must not overlap "
                                       "(frame_off ascending)");
        rows_end = (long long)frame_off[r] + frames[r];
        if (rows_end > (1ll << 28)) return fail(c, KWS_EUNSUPPORTED, "kws_segment_ragged_f32: more than 2^28 rows in the packed frame array");
        rec[r] = {frame_off[r], frames[r], len[r], (int)words, (int)groups};
        words += (frames[r] + 63) / 64;
        groups += (frames[r] + SEG_THREADS - 1) / SEG_THREADS;
    }
    rec[R] = {0, 0, 0, (int)words, (int)groups};
    HIP_TRY(c, hipSetDevice(c->device));
    // context scratch: per recording open_ok and close_ok as ballot words, [2][n_words_r] of 64 bits, one recording after another
    rc = grow_device_buffer(c, c->d_conv_ws, (size_t)words * 2 * 2, "kws_segment_ragged_f32", "workspace");
    if (rc) return rc;
    const SegRec* d_rec = nullptr;
    if ((rc = upload_ragged_tables(c, rec.data(), sizeof(SegRec) * rec.size(), "kws_segment_ragged_f32", reinterpret_cast<const void**>(&d_rec))))
        return rc;
    unsigned long long* ok = reinterpret_cast<unsigned long long*>(c->d_conv_ws.get());
    const int back = (off_window - 1 + 63) / 64;
    hipLaunchKernelGGL(kws_segment_flags_ragged_kernel, dim3((unsigned)groups), dim3(SEG_THREADS), 0, c->stream, d_feat, d_rec, R,
                       c->fp.numcep, log_energy_threshold, on_window, off_window, back, ok);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(kws_segment_walk_ragged_kernel, dim3(R), dim3(64), 0, c->stream, ok, d_rec, c->fp.frame_len, c->fp.frame_step, pre_roll,
                       max_frames, d_utt, max_utts, d_count);
    HIP_TRY(c, hipGetLastError());
    return KWS_OK;
    KWS_GUARD_END(c, "kws_segment_ragged_f32")
}

int kws_cut_i16(kws_ctx* c, const int16_t* d_pcm, int R, int n_total, const int32_t* d_span, int U, int normalize_to, int16_t* d_clips,
                int n_out, int32_t* d_peak) {
    if (!c) return KWS_EINVAL;
    if (!d_pcm || !d_span || !d_clips) return fail(c, KWS_EINVAL, "kws_cut_i16: d_pcm / d_span / d_clips is NULL");
    if (U < 1 || R < 1 || n_total < 1 || n_out < 1) return fail(c, KWS_EINVAL, "kws_cut_i16: U, R, n_total and n_out must be positive");
    if (int rc = check_normalize_to(c, "kws_cut_i16", normalize_to)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(kws_cut_i16_kernel, dim3(U), dim3(CUT_THREADS), 0, c->stream, d_pcm, R, n_total, d_span, normalize_to, d_clips,
                       n_out, d_peak);
    HIP_TRY(c, hipGetLastError());
    return KWS_OK;
}

int kws_cut_f32(kws_ctx* c, const float* d_wav, int R, int n_total, const int32_t* d_span, int U, float normalize_to, float* d_clips,
                int n_out, float* d_peak) {
    if (!c) return KWS_EINVAL;
    if (!d_wav || !d_span || !d_clips) return fail(c, KWS_EINVAL, "kws_cut_f32: d_wav / d_span / d_clips is NULL");
    if (U < 1 || R < 1 || n_total < 1 || n_out < 1) return fail(c, KWS_EINVAL, "kws_cut_f32: U, R, n_total and n_out must be positive");
    if (!(normalize_to >= 0.f) || normalize_to > 3.402823466e38f) return fail(c, KWS_EINVAL, "kws_cut_f32: normalize_to must be finite and not negative");
    HIP_TRY(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(kws_cut_f32_kernel, dim3(U), dim3(CUT_THREADS), 0, c->stream, d_wav, R, n_total, d_span, normalize_to, d_clips,
                       n_out, d_peak);
    HIP_TRY(c, hipGetLastError());
    return KWS_OK;
}

}  // extern "C"
#pragma GCC visibility pop
