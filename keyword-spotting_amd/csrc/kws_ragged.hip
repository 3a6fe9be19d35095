// Batches of recordings of unequal length (include/kws_hip.h: kws_host_ragged_plan, kws_frames_ragged_i16 / _f32, kws_scan_ragged_i16 / _f32):
// the plan of a packed batch on the host, the ragged front end (kws_mfcc_i16_ragged_kernel, kws_mfcc.hip, and the refinement of
// its flagged frames, kws_mfcc_f64.hip) and the scan of the packed frame array as ONE recording by the strided DS-CNN launch.
// The decisions and the endpointer of a ragged batch are beside their equal-length families (kws_scan.hip, kws_segment.hip).
#include "kws_ctx.h"

using namespace kws;

namespace {

constexpr int RAGGED_MAX_R = 1 << 20;
constexpr long long RAGGED_MAX_FRAMES = 1ll << 28, RAGGED_MAX_WINDOWS = 1ll << 30, RAGGED_MAX_PCM = 1ll << 30;

// Rows of the packed frame array: frames[r] = frames_for(len[r]), each recording's row count rounded up to a multiple of
// row_multiple; frame_off has R + 1 entries, the last one F_pack.  Returns F_pack, or -1 when it passes 2^28.
long long ragged_rows(const int32_t* len, int R, int frame_len, int frame_step, int row_multiple, int32_t* frames, int32_t* frame_off) {
    long long at = 0;
    for (int r = 0; r < R; ++r) {
        const int F = frames_for(len[r], frame_len, frame_step);
        if (frames) frames[r] = F;
        if (frame_off) frame_off[r] = (int32_t)at;
        at += ((long long)F + row_multiple - 1) / row_multiple * row_multiple;
        if (at > RAGGED_MAX_FRAMES) return -1;
    }
    if (frame_off) frame_off[R] = (int32_t)at;
    return at;
}

// The argument checks of the two device entries; nothing is launched before they pass.
// src: the buffer's name in the entry's prototype ("pcm" for int16, "wav" for float32: d_pcm / n_pcm, d_wav / n_wav).
int check_ragged_batch(kws_ctx* c, const char* fn, const char* src, const void* d_pcm, int n_pcm, const int64_t* start, const int32_t* len,
                       int R) {
    const std::string f(fn), d_src = std::string("d_") + src, n_src = std::string("n_") + src;
    if (!d_pcm || !start || !len) return fail(c, KWS_EINVAL, f + ": " + d_src + " / start / len is NULL");
    if (R < 1 || n_pcm < 1) return fail(c, KWS_EINVAL, f + ": R and " + n_src + " must be positive");
    if (R > RAGGED_MAX_R) return fail(c, KWS_EUNSUPPORTED, f + ": more than 2^20 recordings in one call");
    if (n_pcm > RAGGED_MAX_PCM) return fail(c, KWS_EUNSUPPORTED, f + ": more than 2^30 samples in the buffer");
    if ((reinterpret_cast<uintptr_t>(d_pcm) & 15) != 0) return fail(c, KWS_EINVAL, f + ": " + d_src + " must be 16-byte aligned");
    for (int r = 0; r < R; ++r) {
        if (len[r] < 1) return fail(c, KWS_EINVAL, f + ": recording " + std::to_string(r) + " has no samples");
        if (start[r] < 0 || start[r] % 8 != 0)
            return fail(c, KWS_EINVAL, f + ": start of recording " + std::to_string(r) + " must be a non-negative multiple of 8 samples");
        if (start[r] + (int64_t)len[r] > (int64_t)n_pcm)
            return fail(c, KWS_EINVAL, f + ": recording " + std::to_string(r) + " runs past the buffer's " + n_src + " samples");
    }
    return KWS_OK;
}

// The ragged front end: plan, tables into context scratch, the float32 kernel and the refinement of what it flagged.
// frames_total (may be NULL) receives the sum of the recordings' own frame counts.
// T: int16 PCM or float32 samples -- the same plan, records and launches (launch_mfcc_ragged / launch_mfcc_refine_ragged overloads).
template <typename T>
int frames_ragged(kws_ctx* c, const char* fn, const T* d_pcm, const int64_t* start, const int32_t* len, int R, int row_multiple,
                  float* d_feat_out, long long* frames_total) {
    const std::string f(fn);
    FrontendParams p = c->fp;
    set_clip_length(p, 8);  // the recordings' own lengths reach the kernel through the records; any multiple of 8 asks about the geometry alone
    if (c->fe_math == KWS_FE_F64 || !c->fe_fast_ok || !mfcc_wave_resident_ok(p))
        return fail(c, KWS_EUNSUPPORTED, f + ": needs KWS_FE_F32 at a geometry of the wavefront-resident kernel (frame_len in (384, 448], "
                                             "4 * frame_step a multiple of 8 and 3 * frame_step + 448 <= 1024)");
    std::vector<int32_t> frames(R), frame_off(R + 1);
    if (ragged_rows(len, R, p.frame_len, p.frame_step, row_multiple, frames.data(), frame_off.data()) < 0)
        return fail(c, KWS_EUNSUPPORTED, f + ": more than 2^28 rows in the packed frame array");
    long total_chunks = 0, total_frames = 0;
    for (int r = 0; r < R; ++r) {
        total_chunks += (frames[r] + MFCC_WR_FRAMES - 1) / MFCC_WR_FRAMES;
        total_frames += frames[r];
    }
    std::vector<RaggedRec> rec(R + 1);
    long waves = 0, pairs = 0;
    for (int r = 0; r < R; ++r) {
        const int n_chunks = (frames[r] + MFCC_WR_FRAMES - 1) / MFCC_WR_FRAMES;
        const int cpw = mfcc_wr_chunks_per_wave(total_chunks, n_chunks);
        rec[r] = {start[r], len[r], frames[r], frame_off[r], (int)pairs, (int)waves, cpw};
        waves += (n_chunks + cpw - 1) / cpw;
        pairs += (frames[r] + 1) / 2;
    }
    rec[R] = {0, 0, 0, frame_off[R], (int)pairs, (int)waves, 1};
    HIP_TRY(c, hipSetDevice(c->device));
    const RaggedRec* d_rec = nullptr;
    int rc = upload_ragged_tables(c, rec.data(), sizeof(RaggedRec) * rec.size(), fn, reinterpret_cast<const void**>(&d_rec));
    if (rc) return rc;
    const RaggedArgs rg = {d_rec, R};
    c->frames_seen += (unsigned long long)total_frames;
    if (frames_total) *frames_total = total_frames;
    RefineList rl{};
    if (p.refine_span > 0.f) {
        if ((rc = ensure_refine(c, 1, (int)(2 * pairs)))) return rc;  // one entry per frame pair of the packed numbering
        rl = {c->d_refine.get(), c->d_refine.get() + 8, c->refine_cap, 0};
    }
    {
        ProfScope ps(c, KWS_K_MFCC);
        HIP_TRY(c, launch_mfcc_ragged(c->stream, p, c->ft, d_pcm, rg, (int)waves, d_feat_out, rl));
    }
    if (rl.ctr) {
        ProfScope ps(c, KWS_K_MFCC_REFINE);
        // the refinement's grid: the batch in clips of the context's own length, as kws_frames_i16 sizes it
        HIP_TRY(c, launch_mfcc_refine_ragged(c->stream, p, c->ft, d_pcm, rg, d_feat_out, rl, (int)(total_frames / c->fp.num_frames + 1)));
    }
    return KWS_OK;
}

}  // namespace

// Host-built tables of a ragged call -> context scratch.  The copy is ordered on the context's stream behind the kernels that
// still read the previous tables, and the stream is drained before the host's copy may go.
int upload_ragged_tables(kws_ctx* c, const void* host, size_t bytes, const char* fn, const void** d_tables) {
    int rc = grow_device_buffer(c, c->d_ragged, bytes, fn, "plan table");
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_ragged.get(), host, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *d_tables = c->d_ragged.get();
    return KWS_OK;
}

// The device entries, shared by the int16 and the float32 source (fn / src: the entry's and its buffer's names in the error text).
template <typename T>
static int frames_ragged_entry(kws_ctx* c, const char* fn, const char* src, const T* d_pcm, int n_pcm, const int64_t* start, const int32_t* len,
                               int R, int row_multiple, float* d_feat_out) {
    const std::string f(fn);
    if (!c) return KWS_EINVAL;
    int rc = check_ragged_batch(c, fn, src, d_pcm, n_pcm, start, len, R);
    if (rc) return rc;
    if (!d_feat_out) return fail(c, KWS_EINVAL, f + ": d_feat_out is NULL");
    if (row_multiple < 1) return fail(c, KWS_EINVAL, f + ": row_multiple must be positive");
    if (!c->fe_ready) return fail(c, KWS_ESTATE, f + ": front end not configured");
    return frames_ragged(c, fn, d_pcm, start, len, R, row_multiple, d_feat_out, nullptr);
}

template <typename Sample>
static int scan_ragged_entry(kws_ctx* c, const ModelOps& m, const char* fn, const char* src, const Sample* d_pcm, int n_pcm, const int64_t* start, const int32_t* len,
                             int R, int hop_frames, float* d_logits, int32_t* d_label, float* d_feat_out) {
    const std::string f(fn);
    if (!c) return KWS_EINVAL;
    int rc = check_ragged_batch(c, fn, src, d_pcm, n_pcm, start, len, R);
    if (rc) return rc;
    if (!d_logits) return fail(c, KWS_EINVAL, f + ": d_logits is NULL");
    if (hop_frames < 1) return fail(c, KWS_EINVAL, f + ": hop_frames must be positive");
    if ((rc = m.scan_check(c, fn))) return rc;
    const int T = c->fp.num_frames;
    std::vector<int32_t> windows(R);
    std::vector<int32_t> frame_off(R + 1);
    int W_pack = 0;
    rc = kws_host_ragged_plan(len, R, c->fp.frame_len, c->fp.frame_step, T, hop_frames, nullptr, frame_off.data(), windows.data(), nullptr, &W_pack);
    if (rc) return fail(c, rc, f + ": more than 2^28 rows in the packed frame array");
    const long long F_pack = frame_off[R];
    if ((long long)W_pack > RAGGED_MAX_WINDOWS) return fail(c, KWS_EUNSUPPORTED, f + ": more than 2^30 packed windows");
    long long any_window = 0;
    for (int r = 0; r < R; ++r) any_window += windows[r];
    HIP_TRY(c, hipSetDevice(c->device));
    float* feat = d_feat_out;
    if (!feat) {
        rc = grow_device_buffer(c, c->d_scan_ws, (size_t)F_pack * c->fp.numcep, fn, "frame workspace");
        if (rc) return rc;
        feat = c->d_scan_ws.get();
    }
    rc = frames_ragged(c, fn, d_pcm, start, len, R, hop_frames, feat, nullptr);
    if (rc) return rc;
    if (any_window == 0) return KWS_OK;  // every recording is shorter than a window: the frames are all there is
    // the packed frame array as ONE recording of F_pack frames: window win_off[r] + w is window w of recording r
    return m.windows(c, fn, feat, 1, (int)F_pack, W_pack, hop_frames, d_logits, d_label);
}

#pragma GCC visibility push(default)
extern "C" {

int kws_host_ragged_plan(const int32_t* len, int R, int frame_len, int frame_step, int window_frames, int hop_frames, int32_t* frames,
                         int32_t* frame_off, int32_t* windows, int32_t* win_off, int* W_pack) {
    if (!len || R < 1 || frame_len <= 0 || frame_step <= 0 || window_frames <= 0 || hop_frames < 1) return KWS_EINVAL;
    if (R > RAGGED_MAX_R) return KWS_EUNSUPPORTED;
    for (int r = 0; r < R; ++r)
        if (len[r] < 1) return KWS_EINVAL;
    KWS_GUARD_BEGIN
    std::vector<int32_t> F(R), off(R + 1);
    const long long F_pack = ragged_rows(len, R, frame_len, frame_step, hop_frames, F.data(), off.data());
    if (F_pack < 0) return KWS_EUNSUPPORTED;
    for (int r = 0; r < R; ++r) {
        if (frames) frames[r] = F[r];
        if (frame_off) frame_off[r] = off[r];
        if (windows) windows[r] = F[r] < window_frames ? 0 : (F[r] - window_frames) / hop_frames + 1;
        if (win_off) win_off[r] = off[r] / hop_frames;
    }
    if (frame_off) frame_off[R] = off[R];
    if (W_pack) *W_pack = F_pack < window_frames ? 0 : (int)((F_pack - window_frames) / hop_frames + 1);
    return KWS_OK;
    KWS_GUARD_END(nullptr, "kws_host_ragged_plan")
}

int kws_frames_ragged_i16(kws_ctx* c, const int16_t* d_pcm, int n_pcm, const int64_t* start, const int32_t* len, int R, int row_multiple,
                          float* d_feat_out) {
    KWS_GUARD_BEGIN
    return frames_ragged_entry(c, "kws_frames_ragged_i16", "pcm", d_pcm, n_pcm, start, len, R, row_multiple, d_feat_out);
    KWS_GUARD_END(c, "kws_frames_ragged_i16")
}

int kws_frames_ragged_f32(kws_ctx* c, const float* d_wav, int n_wav, const int64_t* start, const int32_t* len, int R, int row_multiple,
                          float* d_feat_out) {
    KWS_GUARD_BEGIN
    return frames_ragged_entry(c, "kws_frames_ragged_f32", "wav", d_wav, n_wav, start, len, R, row_multiple, d_feat_out);
    KWS_GUARD_END(c, "kws_frames_ragged_f32")
}

int kws_scan_ragged_i16(kws_ctx* c, const int16_t* d_pcm, int n_pcm, const int64_t* start, const int32_t* len, int R, int hop_frames,
                        float* d_logits, int32_t* d_label, float* d_feat_out) {
    KWS_GUARD_BEGIN
    return scan_ragged_entry(c, model_ops_dscnn(), "kws_scan_ragged_i16", "pcm", d_pcm, n_pcm, start, len, R, hop_frames, d_logits, d_label, d_feat_out);
    KWS_GUARD_END(c, "kws_scan_ragged_i16")
}

int kws_scan_ragged_f32(kws_ctx* c, const float* d_wav, int n_wav, const int64_t* start, const int32_t* len, int R, int hop_frames,
                        float* d_logits, int32_t* d_label, float* d_feat_out) {
    KWS_GUARD_BEGIN
    return scan_ragged_entry(c, model_ops_dscnn(), "kws_scan_ragged_f32", "wav", d_wav, n_wav, start, len, R, hop_frames, d_logits, d_label, d_feat_out);
    KWS_GUARD_END(c, "kws_scan_ragged_f32")
}

int kws_scan_ragged_cnn_trad_i16(kws_ctx* c, const int16_t* d_pcm, int n_pcm, const int64_t* start, const int32_t* len, int R, int hop_frames,
                                 float* d_logits, int32_t* d_label, float* d_feat_out) {
    KWS_GUARD_BEGIN
    return scan_ragged_entry(c, model_ops_cnn_trad(), "kws_scan_ragged_cnn_trad_i16", "pcm", d_pcm, n_pcm, start, len, R, hop_frames, d_logits, d_label,
                             d_feat_out);
    KWS_GUARD_END(c, "kws_scan_ragged_cnn_trad_i16")
}

int kws_scan_ragged_cnn_trad_f32(kws_ctx* c, const float* d_wav, int n_wav, const int64_t* start, const int32_t* len, int R, int hop_frames,
                                 float* d_logits, int32_t* d_label, float* d_feat_out) {
    KWS_GUARD_BEGIN
    return scan_ragged_entry(c, model_ops_cnn_trad(), "kws_scan_ragged_cnn_trad_f32", "wav", d_wav, n_wav, start, len, R, hop_frames, d_logits, d_label,
                             d_feat_out);
    KWS_GUARD_END(c, "kws_scan_ragged_cnn_trad_f32")
}

}  // extern "C"
#pragma GCC visibility pop
