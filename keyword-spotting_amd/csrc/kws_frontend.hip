// The front end's part of the C ABI (include/kws_hip.h): configuration, the MFCC entries over their three sources (int16 PCM,
// float32 samples, the augmented view of a resident split), the stand-alone augmentation and the sigproc operators.  Every MFCC
// entry runs the one flow below, run_frontend; the kernels and their launchers are in kws_mfcc.hip, kws_mfcc_f64.hip,
// kws_augment.hip and kws_sigproc.hip, the tables in kws_tables.hip.
#include <type_traits>

#include "kws_ctx.h"
#include "kws_tables.h"

using namespace kws;

int frames_for(int n_samples, int frame_len, int frame_step) {
    if (n_samples <= frame_len) return 1;
    return 1 + (n_samples - frame_len + frame_step - 1) / frame_step;  // 1 + ceil((n - L)/step)
}

// What of a front end's launch parameters depends on the clip length (p.frame_len and p.frame_step are set): kws_set_frontend
// for the context's clips, kws_scan_i16 for a whole recording as one clip.
void set_clip_length(FrontendParams& p, int n_samples) {
    p.n_samples = n_samples;
    p.num_frames = frames_for(n_samples, p.frame_len, p.frame_step);
    // 16-byte PCM loads: every clip base and every workgroup's first sample must be multiples of 8 samples
    // (the pointer itself is checked per call; the tail of a clip falls back to guarded scalar loads)
    p.vec_ok = (n_samples % 8 == 0) && ((MFCC_FRAMES_PER_WG * p.frame_step) % 8 == 0);
}

// Worklist of the selective refinement for batches of up to B clips of num_frames frames: int[8] counters + one entry per frame
// pair.  The counters (running totals included) move to the new allocation.
int ensure_refine(kws_ctx* c, int B, int num_frames) {
    const size_t frames = (size_t)B * ((num_frames + 1) / 2);  // one entry per frame pair
    if (frames > 0x1fffffffu) return fail(c, KWS_EUNSUPPORTED, "refinement worklist: more than 2^29 frame pairs in one call");
    if (c->d_refine && (int)frames <= c->refine_cap) return KWS_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // not grow_device_buffer: the eight counters in front of the list (kws_frontend_stats reads them) move to the new allocation
    DeviceBuffer<int> d;
    if (!d.alloc(8 + frames)) return fail(c, KWS_ENOMEM, "refinement worklist: device allocation failed");
    hipError_t e = c->d_refine ? hipMemcpy(d.get(), c->d_refine.get(), sizeof(int) * 8, hipMemcpyDeviceToDevice)
                               : hipMemset(d.get(), 0, sizeof(int) * 8);
    if (e != hipSuccess) return fail_hip(c, e, "refinement worklist");
    c->d_refine = std::move(d);
    c->refine_cap = (int)frames;
    return KWS_OK;
}

// The launches of an MFCC entry for B clips of the geometry p (the context's own, or kws_scan_i16's recording-long clips) read
// from src: float64, or float32 with the flagged frames redone.  refine_clips sizes the refinement's grid: the batch in
// one-second clips.  int16 PCM off a 16-byte boundary takes the kernels' scalar loads; kws_mfcc_augment_i16 refuses such a
// split, and the float64 route, before it gets here.
// recording_f32: float32 samples of a recording entry (kws_frames_f32, kws_scan_f32) ask for the wavefront-resident float kernel;
// off a 16-byte boundary, or at a length that is no multiple of 8, the tile kernel serves them as it serves kws_mfcc_f32.
template <typename Src>
int run_frontend(kws_ctx* c, const FrontendParams& geometry, Src src, int B, float* d_out, int refine_clips, bool recording_f32) {
    HIP_TRY(c, hipSetDevice(c->device));
    FrontendParams p = geometry;
    if constexpr (std::is_pointer<Src>::value)  // (the float tile and float64 kernels read samples one by one and never ask)
        if ((reinterpret_cast<uintptr_t>(src) & 15) != 0) p.vec_ok = 0;
    if constexpr (std::is_pointer<Src>::value)
        if (c->fe_math == KWS_FE_F64 || !c->fe_fast_ok) {
            ProfScope ps(c, KWS_K_MFCC_F64);
            HIP_TRY(c, launch_mfcc_f64(c->stream, p, c->ft, src, B, d_out));
            return KWS_OK;
        }
    c->frames_seen += (unsigned long long)B * p.num_frames;
    // the launch's one routing flag: the reference-geometry kernel for int16 PCM, the wavefront-resident kernel for float32 samples
    const bool ref_route = std::is_same<Src, const float*>::value ? recording_f32 : c->fe_ref_geometry && c->fe_route == KWS_FE_ROUTE_AUTO;
    if (p.refine_span > 0.f) {
        int rc = ensure_refine(c, B, p.num_frames);
        if (rc) return rc;
        const RefineList rl = {c->d_refine.get(), c->d_refine.get() + 8, c->refine_cap, 0};
        {
            ProfScope ps(c, KWS_K_MFCC);
            HIP_TRY(c, launch_mfcc(c->stream, p, c->ft, src, B, d_out, rl, ref_route));
        }
        ProfScope ps(c, KWS_K_MFCC_REFINE);
        HIP_TRY(c, launch_mfcc_refine(c->stream, p, c->ft, src, d_out, rl, refine_clips));
        return KWS_OK;
    }
    ProfScope ps(c, KWS_K_MFCC);
    HIP_TRY(c, launch_mfcc(c->stream, p, c->ft, src, B, d_out, RefineList{}, ref_route));
    return KWS_OK;
}
template int run_frontend(kws_ctx*, const FrontendParams&, const int16_t*, int, float*, int, bool);
template int run_frontend(kws_ctx*, const FrontendParams&, const float*, int, float*, int, bool);
template int run_frontend(kws_ctx*, const FrontendParams&, AugmentArgs, int, float*, int, bool);

#pragma GCC visibility push(default)
extern "C" {

int kws_set_frontend(kws_ctx* c, int sample_rate, int n_samples, int frame_len, int frame_step, int nfft, int nfilt,
                     int numcep, float preemph, int ceplifter) {
    KWS_GUARD_BEGIN
    if (!c) return KWS_EINVAL;
    if (sample_rate <= 0 || n_samples <= 0 || frame_len <= 0 || frame_step <= 0 || nfilt <= 0 || numcep <= 0 || nfft < 2)
        return fail(c, KWS_EINVAL, "kws_set_frontend: sizes must be positive");
    if (nfilt > MAX_NFILT || numcep > MAX_NUMCEP || numcep > nfilt)
        return fail(c, KWS_EUNSUPPORTED, "kws_set_frontend: need nfilt <= 64 and numcep <= min(nfilt, 32)");
    int log2n = 0;
    if ((nfft & (nfft - 1)) == 0)
        for (int v = nfft; v > 1; v >>= 1) ++log2n;
    if (nfft > 4096 || (log2n == 0 && nfft > 2048) || (log2n > 0 && nfft < 64))
        return fail(c, KWS_EUNSUPPORTED, "kws_set_frontend: nfft must be a power of two in [64, 4096] or any value in [2, 2048]");
    FrontendImage im;
    if (!build_frontend_image(sample_rate, frame_len, nfft, nfilt, numcep, ceplifter, im))
        return fail(c, KWS_EUNSUPPORTED, "kws_set_frontend: mel edges are not monotone inside [0, nfft/2]");

    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // tables of the previous configuration may be in use
    if (c->n_streams) stream_free(c);             // ring geometry depends on the front end
    int rc = replace_device_image(c, c->d_fe, im.bytes.data(), im.bytes.size(), "kws_set_frontend");
    if (rc) return rc;
    c->ft = im.tables(c->d_fe.get());

    FrontendParams& p = c->fp;
    p.frame_len = frame_len;
    p.frame_step = frame_step;
    set_clip_length(p, n_samples);
    p.nfilt = nfilt;
    p.numcep = numcep;
    p.append_energy = 1;
    p.preemph = preemph;
    p.chunk_samples = (MFCC_FRAMES_PER_WG - 1) * frame_step + frame_len;
    p.nfft = nfft;
    p.log2_nfft = log2n;
    p.refine_span = c->refine_span;
    c->sample_rate = sample_rate;
    c->nfft = nfft;
    c->ceplifter = ceplifter;
    // a hop so long that the tile kernels' staged span (23 hops + one frame) does not fit the LDS: the float64 kernel, which
    // reads its frames from global memory, serves the geometry (kws_frontend_math reports it; kws_stream_open refuses)
    c->fe_fast_ok = im.fast && mfcc_tile_lds_bytes(p) <= MFCC_TILE_LDS_MAX;
    // the reference configuration has a wavefront-resident kernel with its constants compiled in (kws_set_frontend_route)
    // (whether a call's clips suit a wavefront-resident kernel at all -- their length, the pointer -- is asked per launch, as before)
    c->fe_ref_geometry = c->fe_fast_ok && mfcc_reference_geometry(p);
    c->fe_ready = true;
    return KWS_OK;
    KWS_GUARD_END(c, "kws_set_frontend")
}

int kws_set_frontend_math(kws_ctx* c, int math) {
    if (!c) return KWS_EINVAL;
    if (math != KWS_FE_F32 && math != KWS_FE_F64) return fail(c, KWS_EINVAL, "kws_set_frontend_math: math must be KWS_FE_F32 or KWS_FE_F64");
    c->fe_math = math;
    return KWS_OK;
}

int kws_set_frontend_route(kws_ctx* c, int route) {
    if (!c) return KWS_EINVAL;
    if (route != KWS_FE_ROUTE_AUTO && route != KWS_FE_ROUTE_GENERIC)
        return fail(c, KWS_EINVAL, "kws_set_frontend_route: route must be KWS_FE_ROUTE_AUTO or KWS_FE_ROUTE_GENERIC");
    c->fe_route = route;
    return KWS_OK;
}

int kws_frontend_math(kws_ctx* c) {
    if (!c || !c->fe_ready) return KWS_EINVAL;
    return (c->fe_math == KWS_FE_F64 || !c->fe_fast_ok) ? KWS_FE_F64 : KWS_FE_F32;
}

int kws_set_frontend_refine(kws_ctx* c, float log_span) {
    if (!c) return KWS_EINVAL;
    if (!(log_span == log_span)) return fail(c, KWS_EINVAL, "kws_set_frontend_refine: log_span is NaN");
    c->refine_span = log_span > 0.f ? log_span : 0.f;
    c->fp.refine_span = c->refine_span;
    return retire_captured_push(c);  // a captured push holds the front-end parameters by value
}

int kws_frontend_stats(kws_ctx* c, uint64_t* frames_total, uint64_t* frames_refined, int* last_call_refined) {
    if (!c) return KWS_EINVAL;
    int ctr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->d_refine) HIP_TRY(c, hipMemcpy(ctr, c->d_refine.get(), sizeof ctr, hipMemcpyDeviceToHost));
    if (frames_total) *frames_total = c->frames_seen;
    if (frames_refined) *frames_refined = ((uint64_t)(uint32_t)ctr[3] << 32 | (uint32_t)ctr[2]) + (uint64_t)(uint32_t)ctr[5];
    if (last_call_refined) *last_call_refined = ctr[4];
    return KWS_OK;
}

int kws_frontend_shape(kws_ctx* c, int* num_frames, int* numcep) {
    if (!c) return KWS_EINVAL;
    if (!c->fe_ready) return fail(c, KWS_ESTATE, "front end not configured");
    if (num_frames) *num_frames = c->fp.num_frames;
    if (numcep) *numcep = c->fp.numcep;
    return KWS_OK;
}

int kws_reserve(kws_ctx* c, int max_batch) {
    if (!c) return KWS_EINVAL;
    if (max_batch <= 0) return fail(c, KWS_EINVAL, "kws_reserve: max_batch must be positive");
    if (!c->fe_ready) return fail(c, KWS_ESTATE, "front end not configured");
    if (c->refine_span > 0.f && c->fe_fast_ok) {
        int rc = ensure_refine(c, max_batch, c->fp.num_frames);
        if (rc) return rc;
    }
    const size_t need = (size_t)max_batch * c->fp.num_frames * c->fp.numcep;
    if (need <= c->d_feat_ws.size()) return KWS_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    return grow_device_buffer(c, c->d_feat_ws, need, "kws_reserve", "device");
}

int kws_mfcc_i16(kws_ctx* c, const int16_t* d_wav, int B, float* d_out) {
    int rc = check_batch(c, d_wav, B, "kws_mfcc_i16");
    if (rc) return rc;
    if (!d_out) return fail(c, KWS_EINVAL, "kws_mfcc_i16: d_out is NULL");
    if (!c->fe_ready) return fail(c, KWS_ESTATE, "kws_mfcc_i16: front end not configured");
    return run_frontend(c, c->fp, d_wav, B, d_out, B);
}

int kws_mfcc_f32(kws_ctx* c, const float* d_wav, int B, float* d_out) {
    int rc = check_batch(c, d_wav, B, "kws_mfcc_f32");
    if (rc) return rc;
    if (!d_out) return fail(c, KWS_EINVAL, "kws_mfcc_f32: d_out is NULL");
    if (!c->fe_ready) return fail(c, KWS_ESTATE, "kws_mfcc_f32: front end not configured");
    return run_frontend(c, c->fp, d_wav, B, d_out, B);
}

// ---- augmentation ---------------------------------------------------------------------------------
int kws_augment_i16(kws_ctx* c, const int16_t* d_wav, int B, const int32_t* d_shift, const float* d_bg, int bg_len,
                    const int32_t* d_bg_off, const float* d_bg_vol, const uint8_t* d_silence, float* d_out) {
    int rc = check_batch(c, d_wav, B, "kws_augment_i16");
    if (rc) return rc;
    if (!d_out) return fail(c, KWS_EINVAL, "kws_augment_i16: d_out is NULL");
    if (d_bg && (bg_len <= 0 || !d_bg_off || !d_bg_vol)) return fail(c, KWS_EINVAL, "kws_augment_i16: background pool needs length, offsets and volumes");
    if (!c->fe_ready) return fail(c, KWS_ESTATE, "kws_augment_i16: front end not configured");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_augment(c->stream, d_wav, B, c->fp.n_samples, d_shift, d_bg, bg_len, d_bg_off, d_bg_vol, d_silence, d_out));
    return KWS_OK;
}

// ---- resident training loader -----------------------------------------------------------------------
int kws_augment_draw(kws_ctx* c, uint64_t seed, uint32_t epoch, const int32_t* d_index, int B, const int32_t* d_label, int N,
                     int time_shift, const int32_t* d_bg_start, const int32_t* d_bg_len, int K, float bg_volume,
                     float bg_frequency, int use_background, int n_samples, int32_t* d_shift, int32_t* d_bg_off,
                     float* d_bg_vol, uint8_t* d_silence) {
    int rc = check_batch(c, d_index, B, "kws_augment_draw");
    if (rc) return rc;
    if (!d_shift || !d_bg_off || !d_bg_vol || !d_silence) return fail(c, KWS_EINVAL, "kws_augment_draw: an output pointer is NULL");
    if (K < 0 || (K > 0 && (!d_bg_start || !d_bg_len))) return fail(c, KWS_EINVAL, "kws_augment_draw: K files need their start and length tables");
    if (time_shift < 0 || time_shift > (1 << 30)) return fail(c, KWS_EINVAL, "kws_augment_draw: time_shift must be in [0, 2^30]");
    if (N < 0 || n_samples < 0) return fail(c, KWS_EINVAL, "kws_augment_draw: N and n_samples must not be negative");
    HIP_TRY(c, hipSetDevice(c->device));
    const kws::DrawArgs d = {seed, epoch, d_index, d_label, N, time_shift, d_bg_start, d_bg_len, K, bg_volume, bg_frequency,
                             use_background, n_samples, d_shift, d_bg_off, d_bg_vol, d_silence};
    HIP_TRY(c, kws::launch_augment_draw(c->stream, d, B));
    return KWS_OK;
}

int kws_mfcc_augment_i16(kws_ctx* c, const int16_t* d_pcm, int N, const int32_t* d_index, int B, const int32_t* d_shift,
                         const float* d_bg, int bg_len, const int32_t* d_bg_off, const float* d_bg_vol,
                         const uint8_t* d_silence, float* d_out) {
    int rc = check_batch(c, d_pcm, B, "kws_mfcc_augment_i16");
    if (rc) return rc;
    if (!d_index || !d_out) return fail(c, KWS_EINVAL, "kws_mfcc_augment_i16: d_index or d_out is NULL");
    if (N <= 0) return fail(c, KWS_EINVAL, "kws_mfcc_augment_i16: N must be positive");
    if (d_bg && (bg_len <= 0 || !d_bg_off || !d_bg_vol)) return fail(c, KWS_EINVAL, "kws_mfcc_augment_i16: background pool needs length, offsets and volumes");
    if (!c->fe_ready) return fail(c, KWS_ESTATE, "kws_mfcc_augment_i16: front end not configured");
    FrontendParams p = c->fp;
    if ((reinterpret_cast<uintptr_t>(d_pcm) & 15) != 0) p.vec_ok = 0;
    if (c->fe_math == KWS_FE_F64 || !c->fe_fast_ok || !kws::mfcc_wave_resident_ok(p))
        return fail(c, KWS_EUNSUPPORTED, "kws_mfcc_augment_i16: needs KWS_FE_F32 at a geometry of the wavefront-resident kernel and 16-byte "
                                         "aligned PCM; compose kws_augment_i16 and kws_mfcc_f32 instead");
    const kws::AugmentArgs a = {d_pcm, d_index, N, d_shift, d_bg, bg_len, d_bg_off, d_bg_vol, d_silence};
    return run_frontend(c, p, a, B, d_out, B);
}

// ---- sigproc operators --------------------------------------------------------------------------
int kws_preemphasis_f32(kws_ctx* c, const float* d_signal, int n, float coeff, float* d_out) {
    int rc = check_batch(c, d_signal, n, "kws_preemphasis_f32");
    if (rc) return rc;
    if (!d_out) return fail(c, KWS_EINVAL, "kws_preemphasis_f32: d_out is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_preemphasis(c->stream, d_signal, n, coeff, d_out));
    return KWS_OK;
}

int kws_framesig_f32(kws_ctx* c, const float* d_signal, int n, int frame_len, int frame_step, const float* d_window,
                     float* d_frames) {
    int rc = check_batch(c, d_signal, n, "kws_framesig_f32");
    if (rc) return rc;
    if (!d_frames || frame_len <= 0 || frame_step <= 0) return fail(c, KWS_EINVAL, "kws_framesig_f32: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_framesig(c->stream, d_signal, n, frame_len, frame_step, frames_for(n, frame_len, frame_step), d_window, d_frames));
    return KWS_OK;
}

int kws_spec512_f32(kws_ctx* c, const float* d_frames, int num_frames, int frame_len, int power, float* d_spec) {
    int rc = check_batch(c, d_frames, num_frames, "kws_spec512_f32");
    if (rc) return rc;
    if (!d_spec || frame_len <= 0) return fail(c, KWS_EINVAL, "kws_spec512_f32: bad argument");
    if (!c->fe_ready) return fail(c, KWS_ESTATE, "kws_spec512_f32: front end tables not built");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_spec512(c->stream, c->ft, d_frames, num_frames, frame_len, power, d_spec));
    return KWS_OK;
}

int kws_spec_f32(kws_ctx* c, const float* d_frames, int num_frames, int frame_len, int nfft, int power, float* d_spec) {
    KWS_GUARD_BEGIN
    int rc = check_batch(c, d_frames, num_frames, "kws_spec_f32");
    if (rc) return rc;
    if (!d_spec || frame_len <= 0 || nfft < 2) return fail(c, KWS_EINVAL, "kws_spec_f32: bad argument");
    if (nfft == NFFT) return kws_spec512_f32(c, d_frames, num_frames, frame_len, power, d_spec);
    int log2n = 0;
    if ((nfft & (nfft - 1)) == 0)
        for (int v = nfft; v > 1; v >>= 1) ++log2n;
    if (nfft > 4096 || (log2n == 0 && nfft > 2048) || (log2n > 0 && nfft < 64))
        return fail(c, KWS_EUNSUPPORTED, "kws_spec_f32: NFFT must be a power of two in [64, 4096] or any value in [2, 2048]");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->spec_nfft != nfft) {  // float64 twiddles of this transform length, kept until another length is asked for
        const std::vector<double> tw = build_twiddle64(nfft);
        rc = replace_device_image(c, c->d_spec_tw64, tw.data(), sizeof(double) * tw.size(), "kws_spec_f32");
        if (rc) return rc;
        c->spec_nfft = nfft;
    }
    HIP_TRY(c, launch_spec_f64(c->stream, c->d_spec_tw64.get(), d_frames, num_frames, frame_len, nfft, log2n, power, d_spec));
    return KWS_OK;
    KWS_GUARD_END(c, "kws_spec_f32")
}

}  // extern "C"
#pragma GCC visibility pop
