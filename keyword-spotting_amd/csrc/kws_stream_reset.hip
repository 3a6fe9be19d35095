// Reset single streams of the open set (include/kws_hip.h: kws_stream_reset): from the next push on a named stream behaves as if it
// had received digital silence ever since kws_stream_open, what is armed on the set starts over for it, and every other stream keeps
// its bits.  The set's counters run on.  One kernel here, one workgroup per named stream, fills the stream's rows of the context's
// rings and of the other units' per-stream state; the live utterances close what is open in a launch of their own (kws_live.hip),
// and the live events switch to the epoch instantiation of their step (kws_live_detect.hip).  The streams travel BY VALUE, as a
// 1024-bit mask per launch: nothing is copied to the device that a later call could overtake, nothing waits, and after the set's
// first reset nothing is allocated.
#include <cstring>

#include "kws_ctx.h"

namespace kws {
namespace {

constexpr int RESET_THREADS = 256;

struct ResetArgs {
    ResetMask m;              // the chunk's named streams; stream = first + bit index
    int first, n_streams;
    const int* hops;          // the context's hop counter: h0 = pushes so far
    int16_t* pcm;             // [n_streams][ring_len]
    int ring_len;
    float* feat;              // [n_streams][T][numcep]
    int T, numcep, K;
    const float* z;           // [numcep]: the row the frame kernel writes for an all-zero frame
    ResampleResetView rs;
    unsigned long long* vad_bits;  // kws_stream_vad_f32's state, nullptr when it has none
    int* vad_counts;
    DetectResetView dv;
};

// n int16 from p on, 16 bytes at a time between the two ends that are not 16-byte aligned (each shorter than 8 elements)
__device__ __forceinline__ void zero_i16(int16_t* p, int n, int tid) {
    int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 1);
    head = head < n ? head : n;
    const int body = (n - head) >> 3;
    if (tid < head) p[tid] = 0;
    uint4* q = reinterpret_cast<uint4*>(p + head);
    for (int i = tid; i < body; i += RESET_THREADS) q[i] = make_uint4(0u, 0u, 0u, 0u);
    const int tail = head + 8 * body;
    if (tid < n - tail) p[tail + tid] = 0;
}

// Workgroup b serves the b-th named stream of the chunk (the grid is the mask's popcount).
__global__ __launch_bounds__(RESET_THREADS) void kws_stream_reset_kernel(const ResetArgs a) {
    const int tid = threadIdx.x;
    int s = -1, left = (int)blockIdx.x;  // workgroup-uniform
#pragma unroll
    for (int k = 0; k < RESET_CHUNK / 64; ++k) {
        unsigned long long w = a.m.w[k];
        const int n = __popcll(w);
        if (s < 0 && left < n) {
            for (int j = 0; j < left; ++j) w &= w - 1;
            s = a.first + 64 * k + (int)__ffsll((long long)w) - 1;
        }
        left -= n;
    }
    if (s < 0 || s >= a.n_streams) return;

    zero_i16(a.pcm + (size_t)s * a.ring_len, a.ring_len, tid);
    if (a.rs.hist) {
        zero_i16(a.rs.hist + (size_t)s * a.rs.len, a.rs.len, tid);
        zero_i16(a.rs.hist + a.rs.half + (size_t)s * a.rs.len, a.rs.len, tid);
    }

    // Feature ring of a stream that has heard silence for h0 pushes: frames 0 .. h0 - K exist, frame f in row f mod T, so the
    // first min(h0 - K + 1, T) rows hold the silence row and the others what kws_stream_open left, zeros.
    const int h0 = a.hops[0];
    const int frames = h0 >= a.K ? h0 - a.K + 1 : 0;
    const int live = (frames < a.T ? frames : a.T) * a.numcep;  // elements below it hold z
    const int n = a.T * a.numcep;
    float* f = a.feat + (size_t)s * n;
    auto value = [&](int i) -> float { return i < live ? a.z[i % a.numcep] : 0.f; };
    int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(f) & 15u)) & 15u) >> 2);
    head = head < n ? head : n;
    const int body = (n - head) >> 2;
    if (tid < head) f[tid] = value(tid);
    float4* q = reinterpret_cast<float4*>(f + head);
    for (int i = tid; i < body; i += RESET_THREADS) {
        const int e = head + 4 * i;
        q[i] = make_float4(value(e), value(e + 1), value(e + 2), value(e + 3));
    }
    const int tail = head + 4 * body;
    if (tid < n - tail) f[tail + tid] = value(tail + tid);

    if (a.vad_bits) {  // all flags unvoiced, both window counts zero, not triggered; the frame cursor is the set's and runs on
        if (tid < EP_BIT_WORDS / 2) reinterpret_cast<ulonglong2*>(a.vad_bits + (size_t)s * EP_BIT_WORDS)[tid] = make_ulonglong2(0ull, 0ull);
        if (tid < 3) a.vad_counts[4 * s + tid] = 0;
    }
    if (a.dv.next && tid == 0) {
        a.dv.next[s] = 0;
        a.dv.epoch[s] = (long long)a.dv.decisions[0];
    }
}

// The silence row, once per open set: the project's own frame kernel over the scratch set of ONE stream -- zeroed rings, a zero
// hop, K launches; the K-th completes frame 0 into row 0 of the scratch feature ring.  No refinement counters (kws_frontend_stats
// does not move) and no profiling bracket.
int ensure_silence_row(kws_ctx* c) {
    if (c->reset_row_ready) return KWS_OK;
    const FrontendParams& p = c->fp;
    const size_t feat_n = (size_t)p.num_frames * p.numcep;
    const size_t pcm_n = (size_t)c->ring_len + p.frame_step;                  // int16: the ring, then the hop
    const size_t total = feat_n + 2 + (pcm_n + 1) / 2;                        // in floats
    if (!c->d_reset_scratch.alloc(total)) return fail(c, KWS_ENOMEM, "kws_stream_reset: device allocation failed");
    float* feat = c->d_reset_scratch.get();
    int* hops = reinterpret_cast<int*>(feat + feat_n);
    int16_t* pcm = reinterpret_cast<int16_t*>(hops + 2);
    const int16_t* hop = pcm + c->ring_len;
    hipError_t e = hipMemsetAsync(feat, 0, sizeof(float) * total, c->stream);
    for (int k = 0; e == hipSuccess && k < frames_lag(p); ++k)
        e = launch_stream_frame(c->stream, p, c->ft, hop, 1, pcm, c->ring_len, feat, hops, nullptr);
    if (e != hipSuccess) return fail_hip(c, e, "kws_stream_reset: the silence row");
    c->reset_row_ready = true;
    return KWS_OK;
}

}  // namespace

int stream_reset_check(kws_ctx* c, const char* fn, const int32_t* streams, int n, bool* nothing) {
    *nothing = false;
    if (!c) return KWS_EINVAL;
    const std::string f(fn);
    if (!c->n_streams) return fail(c, KWS_ESTATE, f + ": call kws_stream_open first");
    if (n < 0) return fail(c, KWS_EINVAL, f + ": n must not be negative");
    if (n == 0) {
        *nothing = true;
        return KWS_OK;
    }
    if (!streams) return fail(c, KWS_EINVAL, f + ": streams is NULL");
    for (int i = 0; i < n; ++i)
        if (streams[i] < 0 || streams[i] >= c->n_streams)
            return fail(c, KWS_EINVAL, f + ": stream " + std::to_string(streams[i]) + " is outside [0, " + std::to_string(c->n_streams) + ")");
    if (c->post_window)
        return fail(c, KWS_EUNSUPPORTED, f + ": kws_stream_smooth_f32 keeps a running sum and ONE hop count for all streams, which no single stream can leave; smooth with kws_stream_detect_* (a ring and an epoch per stream) on sets that reset streams");
    return KWS_OK;
}

int stream_reset_launch(kws_ctx* c, const int32_t* streams, int n, bool only_active, bool utt_only) {
    HIP_TRY(c, hipSetDevice(c->device));
    if (!utt_only)
        if (int rc = ensure_silence_row(c)) return rc;

    ResetArgs a{};
    a.n_streams = c->n_streams;
    a.hops = c->d_hops.get();
    a.pcm = c->d_pcm_ring.get();
    a.ring_len = c->ring_len;
    a.feat = c->d_feat_ring.get();
    a.T = c->fp.num_frames;
    a.numcep = c->fp.numcep;
    a.K = frames_lag(c->fp);
    a.z = c->d_reset_scratch.get();
    a.rs = stream_resample_reset_view(c);
    a.vad_bits = c->d_vad_bits.get();
    a.vad_counts = c->d_vad_counts.get();
    if (!utt_only) a.dv = stream_detect_reset_view(c);  // (switches the set's event steps to their epoch instantiation)
    for (int first = 0; first < c->n_streams; first += RESET_CHUNK) {
        memset(&a.m, 0, sizeof a.m);
        int named = 0;
        for (int i = 0; i < n; ++i) {
            const int r = streams[i] - first;
            if (r < 0 || r >= RESET_CHUNK || a.m.has(r)) continue;  // another chunk's, or a duplicate
            if (only_active && !c->is_active(streams[i])) continue;  // left alone until it is activated, which resets it
            a.m.w[r >> 6] |= 1ull << (r & 63);
            named += 1;
        }
        if (!named) continue;
        a.first = first;
        if (!utt_only) {
            hipLaunchKernelGGL(kws_stream_reset_kernel, dim3(named), dim3(RESET_THREADS), 0, c->stream, a);
            HIP_TRY(c, hipGetLastError());
        }
        if (first == 0)  // the live units hold at most 1024 streams: theirs are all in the first chunk
            if (int rc = stream_utt_reset(c, a.m)) return rc;
    }
    return KWS_OK;
}

}  // namespace kws

using namespace kws;

#pragma GCC visibility push(default)
extern "C" {

int kws_stream_reset(kws_ctx* c, const int32_t* streams, int n) {
    KWS_GUARD_BEGIN
    bool nothing = false;
    if (int rc = stream_reset_check(c, "kws_stream_reset", streams, n, &nothing)) return rc;
    if (nothing) return KWS_OK;
    return stream_reset_launch(c, streams, n, true, false);
    KWS_GUARD_END(c, "kws_stream_reset")
}

}  // extern "C"
#pragma GCC visibility pop
