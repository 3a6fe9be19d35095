// The decision layer behind the logits (include/kws_hip.h: kws_softmax_f32, kws_stream_smooth_f32, kws_stream_vad_f32):
// posteriors, their moving average per stream and the energy endpointer, each kernel with the entry point that drives it and
// the history it keeps in the context.  (the reference's scripts take argmax of the logits.)
#include "kws_ctx.h"
#include "kws_softmax_dev.h"  // softmax_row: one thread per clip / stream, shared with kws_eval.hip

namespace kws {
namespace {

__global__ void kws_softmax_f32_kernel(const float* __restrict__ logits, int B, int C, float* __restrict__ prob) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) softmax_row(logits + (size_t)b * C, C, prob + (size_t)b * C);
}

// Moving average of the last `window` posterior vectors per stream (ring [S][window][C], running sum [S][C]),
// then argmax of the smoothed vector (first maximum wins).  count = hops smoothed so far, before this one.
// The running sum is updated incrementally (sum += p - oldest) and REBUILT from the ring every `window` hops (when the
// write slot wraps to 0), so its float32 rounding error is bounded by one window's worth of updates instead of growing
// over the life of a stream (10 ms hops = 8.6 M updates a day).
__global__ void kws_smooth_posteriors_kernel(const float* __restrict__ logits, int S, int C, int window,
                                             float* __restrict__ ring, float* __restrict__ sum, int* __restrict__ count_ptr,
                                             float* __restrict__ smoothed, int32_t* __restrict__ label) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    const int count = count_ptr[0];
    // every workgroup has read the hop count; the one that finishes last advances it (count_ptr[1] = done counter)
    auto finish = [&]() {
        __syncthreads();
        if (threadIdx.x == 0) {
            __threadfence();
            if (atomicAdd(&count_ptr[1], 1) == (int)gridDim.x - 1) {
                count_ptr[1] = 0;
                count_ptr[0] = count + 1;
            }
        }
    };
    if (s >= S) {
        finish();
        return;
    }
    const int slot = count % window;
    float p[MAX_CLASSES];
    softmax_row(logits + (size_t)s * C, C, p);
    float* r = ring + ((size_t)s * window + slot) * C;
    float* acc = sum + (size_t)s * C;
    const float inv = 1.0f / (float)((count + 1 < window) ? count + 1 : window);
    float best = -1.f;
    int arg = 0;
    const bool rebuild = count >= window && slot == 0;
    for (int i = 0; i < C; ++i) {
        const float old = count >= window ? r[i] : 0.f;
        r[i] = p[i];
        float a;
        if (rebuild) {
            a = 0.f;
            for (int k = 0; k < window; ++k) a += ring[((size_t)s * window + k) * C + i];
        } else {
            a = acc[i] + (p[i] - old);
        }
        acc[i] = a;
        const float v = a * inv;
        smoothed[(size_t)s * C + i] = v;
        if (v > best) {
            best = v;
            arg = i;
        }
    }
    if (label) label[s] = arg;
    finish();
}

}  // namespace

hipError_t launch_softmax(hipStream_t s, const float* d_logits, int B, int C, float* d_prob) {
    hipLaunchKernelGGL(kws_softmax_f32_kernel, dim3((B + 255) / 256), dim3(256), 0, s, d_logits, B, C, d_prob);
    return hipGetLastError();
}

// Energy endpointer per stream (the gate that replaces webrtcvad in the reference's live loop,
// kws/inference/inference_local.py:131-166 -- same hysteresis, at hop granularity).  The newest frame's log energy
// (cepstrum 0 with appendEnergy) above the threshold marks the hop voiced; an utterance OPENS when more than 80 % of the
// last `on_window` hops are voiced (:151) and CLOSES when more than 90 % of the last `off_window` hops are unvoiced
// (:161); hops before the stream began count as unvoiced (the reference's rings start as zeros).  One thread per stream, the
// rules and the O(1) flag ring of kws_endpoint_dev.h; counts[s] = (c_on, c_off, triggered, frames walked so far).
// state[s] = triggered | event << 1, event 1 = opened at this hop, 2 = closed at this hop.
__global__ void kws_stream_vad_kernel(const float* __restrict__ feat_ring, const int* __restrict__ hops_ptr, int n_streams,
                                      int num_frames, int numcep, int lag, float threshold, int on_window, int off_window,
                                      unsigned long long* __restrict__ bits, int* __restrict__ counts, int32_t* __restrict__ state) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_streams) return;
    const int hops = *hops_ptr;  // already advanced by the push this call follows: the newest frame is hops - lag
    if (hops < lag) {            // no complete frame yet
        state[s] = 0;
        return;
    }
    const float c0 = feat_ring[((size_t)s * num_frames + (hops - lag) % num_frames) * numcep];
    int* cnt = counts + 4 * s;
    const int cur = cnt[3];
    int trig = cnt[2], event = 0;
    const EpCounts n = ep_ring_push(bits + (size_t)s * EP_BIT_WORDS, cnt, cur, ep_voiced(c0, threshold) ? 1 : 0, on_window, off_window);
    if (!trig) {
        if (ep_opens(n.on, on_window)) trig = 1, event = 1;
    } else if (ep_closes(n.off, off_window)) {
        trig = 0, event = 2;
    }
    cnt[2] = trig;
    cnt[3] = cur + 1;
    state[s] = trig | (event << 1);
}

hipError_t launch_smooth_posteriors(hipStream_t s, const float* d_logits, int S, int C, int window, float* d_ring,
                                    float* d_sum, int* d_count, float* d_smoothed, int32_t* d_label) {
    hipLaunchKernelGGL(kws_smooth_posteriors_kernel, dim3((S + 63) / 64), dim3(64), 0, s, d_logits, S, C, window, d_ring, d_sum,
                       d_count, d_smoothed, d_label);
    return hipGetLastError();
}

// The histories of the two streaming entry points below; stream_free (kws_stream.hip) drops them with the streams.  The window
// sizes say whether a history is running.
void smooth_free(kws_ctx* c) {
    c->d_post_ring.reset();
    c->d_post_sum.reset();
    c->d_post_count.reset();
    c->post_window = c->post_classes = 0;
}

void vad_free(kws_ctx* c) {
    c->d_vad_bits.reset();
    c->d_vad_counts.reset();
    c->vad_on = c->vad_off = 0;
}

}  // namespace kws

using namespace kws;

#pragma GCC visibility push(default)
extern "C" {

int kws_stream_vad_f32(kws_ctx* c, float log_energy_threshold, int on_window, int off_window, int32_t* d_state) {
    if (!c) return KWS_EINVAL;
    if (!c->n_streams) return fail(c, KWS_ESTATE, "kws_stream_vad_f32: call kws_stream_open first");
    if (!d_state) return fail(c, KWS_EINVAL, "kws_stream_vad_f32: d_state is NULL");
    int rc = check_endpoint_windows(c, "kws_stream_vad_f32", on_window, off_window);
    if (!rc) rc = check_append_energy(c, "kws_stream_vad_f32");
    if (!rc) rc = refuse_sparse(c, "kws_stream_vad_f32", "the endpointer's frames");
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if (on_window != c->vad_on || off_window != c->vad_off) {  // (re)start the history
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        vad_free(c);
        if ((rc = alloc_endpoint_state(c, "kws_stream_vad_f32", (size_t)c->n_streams, c->d_vad_bits, c->d_vad_counts))) {
            vad_free(c);
            return rc;
        }
        c->vad_on = on_window;
        c->vad_off = off_window;
    }
    hipLaunchKernelGGL(kws_stream_vad_kernel, dim3((c->n_streams + 63) / 64), dim3(64), 0, c->stream, c->d_feat_ring.get(), c->d_hops.get(),
                       c->n_streams, c->fp.num_frames, c->fp.numcep, frames_lag(c->fp), log_energy_threshold, on_window, off_window,
                       c->d_vad_bits.get(), c->d_vad_counts.get(), d_state);
    HIP_TRY(c, hipGetLastError());
    return KWS_OK;
}

int kws_softmax_f32(kws_ctx* c, const float* d_logits, int B, int C, float* d_prob) {
    int rc = check_batch(c, d_logits, B, "kws_softmax_f32");
    if (rc) return rc;
    if (!d_prob) return fail(c, KWS_EINVAL, "kws_softmax_f32: d_prob is NULL");
    if (C < 1 || C > MAX_CLASSES) return fail(c, KWS_EUNSUPPORTED, "kws_softmax_f32: C must be in [1, 64]");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_softmax(c->stream, d_logits, B, C, d_prob));
    return KWS_OK;
}

int kws_stream_smooth_f32(kws_ctx* c, const float* d_logits, int C, int window, float* d_smoothed, int32_t* d_label) {
    if (!c) return KWS_EINVAL;
    if (!c->n_streams) return fail(c, KWS_ESTATE, "kws_stream_smooth_f32: call kws_stream_open first");
    if (!d_logits || !d_smoothed) return fail(c, KWS_EINVAL, "kws_stream_smooth_f32: d_logits / d_smoothed is NULL");
    if (C < 1 || C > MAX_CLASSES) return fail(c, KWS_EUNSUPPORTED, "kws_stream_smooth_f32: C must be in [1, 64]");
    if (window < 1 || window > 4096) return fail(c, KWS_EINVAL, "kws_stream_smooth_f32: window must be in [1, 4096]");
    HIP_TRY(c, hipSetDevice(c->device));
    if (window != c->post_window || C != c->post_classes) {  // (re)start the history
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        smooth_free(c);
        const size_t sums = (size_t)c->n_streams * C;
        if (!(c->d_post_ring.alloc(sums * window) && c->d_post_sum.alloc(sums) && c->d_post_count.alloc(2))) {
            smooth_free(c);
            return fail(c, KWS_ENOMEM, "kws_stream_smooth_f32: device allocation failed");
        }
        HIP_TRY(c, hipMemsetAsync(c->d_post_ring.get(), 0, sizeof(float) * sums * window, c->stream));
        HIP_TRY(c, hipMemsetAsync(c->d_post_sum.get(), 0, sizeof(float) * sums, c->stream));
        HIP_TRY(c, hipMemsetAsync(c->d_post_count.get(), 0, 2 * sizeof(int), c->stream));
        c->post_window = window;
        c->post_classes = C;
    }
    HIP_TRY(c, launch_smooth_posteriors(c->stream, d_logits, c->n_streams, C, window, c->d_post_ring.get(), c->d_post_sum.get(),
                                        c->d_post_count.get(), d_smoothed, d_label));
    return KWS_OK;
}

}  // extern "C"
#pragma GCC visibility pop
