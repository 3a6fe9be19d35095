// Live utterances (include/kws_hip.h: kws_stream_utt_*) -- the reference's one live loop (kws/inference/inference_local.py:
// 114-192) for the streams of kws_stream_open: a per-stream PCM history ring, the walk of kws_segment_f32 taken one frame per
// hop with O(1) window counts, an event queue mirrored in pinned host memory (kws_event_queue.h), and kws_cut_i16 with a ring
// origin.  Everything here is new kernels launched BEHIND a push; no other unit's kernel changes, and an unarmed context never
// gets here.
#include <climits>

#include "kws_event_queue.h"

namespace kws {

constexpr int LIVE_MAX_STREAMS = 1024;  // one workgroup walks every stream: one thread each
constexpr int LIVE_REC = 6;             // int64 words per record
constexpr int LIVE_CUT_THREADS = 256;
static_assert(LIVE_MAX_STREAMS <= EQ_MAX_THREADS, "eq_emit counts one ballot per wavefront of the step's workgroup");

namespace {

// What a step reads.  The first group is set per launch (utt_args); the set's own size, rules and buffers below it are filled
// once by kws_stream_utt_open.  The unit's device counters q.unit()[2] = frames walked, hops appended; the queue's progress word
// (h_ctr[1]) is the frames walked.
struct LiveArgs {
    const int16_t* hop;       // append source (nullptr: no append): stream s at hop + s * hop_stride (+ the ring offset with ctx_hops)
    long long hop_stride;
    const int* ctx_hops;      // stepped by a push: the context's hop counter (already advanced); nullptr: explicit step
    int ring_len;             // of the context's PCM ring
    const float* energy;      // explicit step: [S] (nullptr: no walk); push: the context's feature ring
    int num_frames, numcep, K;
    int S, step, frame_len, H;
    int on_window, off_window, pre_roll, max_frames;
    float threshold;
    int vec;                  // the hop may be copied 16 bytes at a time
    int16_t* hist;            // [S][H]
    unsigned long long* bits; // [S][EP_BIT_WORDS], counts [S][4] = c_on, c_off, triggered, unused: ep_ring_push's state
    int* counts;
    long long* pos;           // [S][2]: open, prev_close
    EventQueue q;             // records of LIVE_REC words
};

}  // namespace

// Everything kws_stream_utt_open allocates: as the step kernel takes it (a), and the owners a's pointers are filled from.
struct StreamUtt {
    LiveArgs a{};
    int mode = 0;  // 0: not stepped yet, 1: stepped by pushes, 2: stepped by kws_stream_utt_step_i16
    DeviceBuffer<int16_t> hist;
    DeviceBuffer<unsigned long long> bits;
    DeviceBuffer<int> counts;
    DeviceBuffer<long long> pos;
    EventQueueMem queue;
};

namespace {

// One hop of every stream: append, walk one frame of the endpointer, close and emit, publish -- the body of the four step kernels
// below.  ONE workgroup, thread s = stream s (threads at or beyond S only help with the copy, the ballots and the barriers).  The
// streams that closed at this step emit their records and thread 0 publishes the totals as kws_event_queue.h lays down (eq_emit,
// eq_publish): every thread gets there in every instantiation -- no early return, and the mask below gates only the copy, the
// walk and `closed`.
// FLUSH: no append and no walk -- every stream inside an utterance closes at the newest walked frame with reason 2.
// MASKED: `m` names the streams that take part; a stream outside it appends nothing, pushes no flag, walks nothing and emits
// nothing, while its thread takes part in the ballots and the barriers.  The unit's two counters run on for the whole set.
// RESET (a masked flush): the named streams then start over -- flag ring, window counts and the open frame as
// kws_stream_utt_open leaves them, prev_close = hops appended - 1, so that ep_span_start keeps a later utterance of the stream
// from starting before the first sample pushed after the reset.  The history ring stays: what closed before the reset remains
// cuttable.  The unit's own counters stand.
// `a` by value: by reference the compiler schedules the dense step differently.
template <bool FLUSH, bool MASKED, bool RESET = false>
__device__ __forceinline__ void live_step(const LiveArgs a, const ResetMask* m = nullptr) {
    static_assert(!RESET || (FLUSH && MASKED), "a reset is the flush of the streams a mask names");
    auto mine = [&](int s) { return !MASKED || m->has(s); };
    const int tid = threadIdx.x;
    const EqCounts was = eq_counts(a.q);
    const unsigned long long frames = was.unit[0], appended = was.unit[1];
    bool do_append = false, do_walk = false;  // workgroup-uniform
    const int16_t* src = a.hop;
    const float* energy = a.energy;
    long long e_stride = 1;
    if constexpr (!FLUSH) {
        if (a.ctx_hops) {
            // push number h left its hop at [((h - 1) step) mod ring_len, + step) of the context's ring (kws_mfcc_dev.h) and
            // completed the frame of feature row (h - K) mod num_frames; this set's own K - 1 first hops walk nothing
            const int h = a.ctx_hops[0];  // >= 1 behind a push
            do_append = h >= 1;
            do_walk = do_append && appended + 1 >= (unsigned long long)a.K && h >= a.K;
            if (do_append) src += (int)(((long long)(h - 1) * a.step) % a.ring_len);
            if (do_walk) energy += (size_t)((h - a.K) % a.num_frames) * a.numcep;
            e_stride = (long long)a.num_frames * a.numcep;
        } else {
            do_append = a.hop != nullptr;
            do_walk = a.energy != nullptr;
        }
    }
    if (do_append) {  // a hop never straddles the seam: H is a multiple of step
        const int at = (int)((appended * (unsigned long long)a.step) % (unsigned long long)a.H);
        if (a.vec) {
            const int per = a.step >> 3;
            for (int i = tid; i < a.S * per; i += (int)blockDim.x) {
                const int s = i / per, j = i - s * per;
                if (mine(s)) reinterpret_cast<uint4*>(a.hist + (size_t)s * a.H + at)[j] = reinterpret_cast<const uint4*>(src + (size_t)s * a.hop_stride)[j];
            }
        } else {
            for (int i = tid; i < a.S * a.step; i += (int)blockDim.x) {
                const int s = i / a.step, j = i - s * a.step;
                if (mine(s)) a.hist[(size_t)s * a.H + at + j] = src[(size_t)s * a.hop_stride + j];
            }
        }
    }
    bool closed = false;
    long long open = 0, start_frame = 0, close_frame = 0;
    int reason = 0;
    if (tid < a.S && (FLUSH || do_walk) && mine(tid)) {
        int* cnt = a.counts + 4 * tid;
        long long* ps = a.pos + 2 * tid;
        int trig = cnt[2];
        open = ps[0];
        const long long prev_close = ps[1];
        if constexpr (FLUSH) {
            if (trig) {
                closed = true;
                reason = 2;
                close_frame = (long long)frames - 1;  // triggered: at least one frame was walked
            }
        } else {
            const long long f = (long long)frames;
            const int v = ep_voiced(energy[(size_t)tid * e_stride], a.threshold) ? 1 : 0;
            const EpCounts n = ep_ring_push(a.bits + (size_t)tid * EP_BIT_WORDS, cnt, f, v, a.on_window, a.off_window);
            if (!trig) {
                if (ep_opens(n.on, a.on_window)) {  // the utterance opens; nothing else happens at this frame
                    trig = 1;
                    open = f;
                    ps[0] = f;
                    cnt[2] = 1;
                }
            } else if (ep_closes(n.off, a.off_window)) {
                closed = true;
                reason = 0;
                close_frame = f;
            } else if (f - open + 1 >= a.max_frames) {
                closed = true;
                reason = 1;
                close_frame = f;
            }
        }
        if (closed) {
            start_frame = ep_span_start(open, a.pre_roll, prev_close);
            ps[1] = close_frame;
            cnt[2] = 0;
        }
        if constexpr (RESET) {
            ulonglong2* row = reinterpret_cast<ulonglong2*>(a.bits + (size_t)tid * EP_BIT_WORDS);
#pragma unroll
            for (int k = 0; k < EP_BIT_WORDS / 2; ++k) row[k] = make_ulonglong2(0ull, 0ull);
            cnt[0] = cnt[1] = cnt[2] = 0;
            ps[0] = -1;
            ps[1] = (long long)appended - 1;
        }
    }
    const long long rec[LIVE_REC] = {(long long)tid, start_frame * a.step, close_frame * a.step + a.frame_len, open, close_frame, (long long)reason};
    const int all = eq_emit(a.q, was, closed, rec);
    const unsigned long long frames_now = frames + (do_walk ? 1 : 0);
    eq_publish(a.q, was, all, frames_now);
    if constexpr (!RESET) {
        if (tid == 0) {
            a.q.unit()[0] = frames_now;
            a.q.unit()[1] = appended + (do_append ? 1 : 0);
        }
    }
}

// The step of a dense set (a push, kws_stream_utt_step_i16) and kws_stream_utt_flush.
template <bool FLUSH>
__global__ __launch_bounds__(LIVE_MAX_STREAMS) void kws_live_step_kernel(const LiveArgs a) {
    live_step<FLUSH, false>(a);
}

// kws_stream_reset's step (and a deactivation's): one more tick of the queue.
__global__ __launch_bounds__(LIVE_MAX_STREAMS) void kws_live_reset_kernel(const LiveArgs a, const ResetMask m) {
    live_step<true, true, true>(a, &m);
}

// The step behind a push of a set with inactive streams (kws_stream_deactivate; `m`: the active ones, by value): an active
// stream's records are those of a dense set.  Only ever stepped by a push (explicit steps are refused while a stream is inactive).
__global__ __launch_bounds__(LIVE_MAX_STREAMS) void kws_live_step_masked_kernel(const LiveArgs a, const ResetMask m) {
    live_step<false, true>(a, &m);
}

// kws_cut_i16_kernel (kws_segment.hip) with a ring origin: one workgroup per sequence number, the record read from the device
// queue (q.ctr[0]: events so far; q.unit()[1]: hops appended).  The span [start, end) of stream r lies in the history ring from
// start mod H on and crosses the seam at most once (end - start <= H): element i is at p0 + i, minus H from the seam on.  The
// cut itself is the linear kernel's (ep_cut_clip).  Refused (zero clip, peak -1): a sequence number not issued yet or already
// overwritten in the queue, a span whose start has left the ring, a span that ends beyond what was appended.
__global__ __launch_bounds__(LIVE_CUT_THREADS) void kws_live_cut_kernel(const int16_t* __restrict__ hist, int S, int H, int step,
                                                                        const EventQueue q, unsigned long long first_seq, int normalize_to,
                                                                        int16_t* __restrict__ clips, int n_out, int32_t* __restrict__ peak_out) {
    const int u = blockIdx.x;
    const unsigned long long seq = first_seq + (unsigned long long)u, total = q.ctr[0];
    const long long have = (long long)(q.unit()[1] * (unsigned long long)step);  // samples appended so far
    bool ok = seq < total && seq + (unsigned long long)q.max_events >= total;  // workgroup-uniform throughout
    long long r = 0, start = 0, end = 0;
    if (ok) {
        const long long* rec = q.queue + (size_t)(seq % (unsigned long long)q.max_events) * LIVE_REC;
        r = rec[0];
        start = rec[1];
        end = rec[2];
        ok = r >= 0 && r < S && start >= 0 && end >= start && end <= have && start + H >= have;
    }
    const int len = ok ? (int)(end - start) : 0;  // <= H
    const int p0 = ok ? (int)(start % H) : 0;
    const int16_t* x = hist + (ok ? (size_t)r * H : 0);
    auto at = [&](unsigned i) -> int {
        int p = p0 + (int)i;
        p -= p >= H ? H : 0;
        return x[p];
    };
    ep_cut_clip<LIVE_CUT_THREADS>(at, len, ok, normalize_to, clips + (size_t)u * n_out, n_out, peak_out, u);
}

int history_for(int frame_len, int frame_step, int pre_roll, int max_frames, int slack_hops, long long* out) {
    if (frame_len < 1 || frame_step < 1 || pre_roll < 0 || max_frames < 2 || slack_hops < 0) return KWS_EINVAL;
    const long long K = frames_lag(frame_len, frame_step);
    *out = ((long long)pre_roll + max_frames - 1 + K + slack_hops) * frame_step;
    return *out > INT_MAX ? KWS_EINVAL : KWS_OK;
}

// The set's state with a launch's own fields; hop / energy / ctx_hops as LiveArgs describes them.
LiveArgs utt_args(kws_ctx* c, const int16_t* hop, long long hop_stride, const int* ctx_hops, const float* energy) {
    const FrontendParams& p = c->fp;
    LiveArgs a = c->stream_utt->a;
    a.hop = hop;
    a.hop_stride = hop_stride;
    a.ctx_hops = ctx_hops;
    a.ring_len = c->ring_len;
    a.energy = energy;
    a.num_frames = p.num_frames;
    a.numcep = p.numcep;
    a.K = frames_lag(p);
    a.step = p.frame_step;
    a.frame_len = p.frame_len;
    // 16-byte copies: whole hops of 8 samples, every stream's hop and ring row on a 16-byte boundary (the ring offset and the
    // ring's write position are multiples of step)
    a.vec = hop && p.frame_step % 8 == 0 && hop_stride % 8 == 0 && reinterpret_cast<uintptr_t>(hop) % 16 == 0;
    return a;
}

// One launch of a step kernel, with its mask where it takes one, and the queue's tick.  Threads: one per stream, in whole wavefronts.
template <class... Mask>
int utt_launch(kws_ctx* c, void (*kernel)(LiveArgs, Mask...), const LiveArgs& a, const Mask&... m) {
    int threads = (a.S + 63) / 64 * 64;
    if (a.hop && threads < 256) threads = 256;  // the copy is the workgroup's bulk
    hipLaunchKernelGGL(kernel, dim3(1), dim3(threads), 0, c->stream, a, m...);
    HIP_TRY(c, hipGetLastError());
    eq_enqueued(c->stream_utt->a.q);
    return KWS_OK;
}

}  // namespace

void stream_utt_free(kws_ctx* c) {
    delete c->stream_utt;
    c->stream_utt = nullptr;
}

// The push entries' side (kws_stream.hip): the check in front of a push's launches, the step behind them.
int stream_utt_push_check(kws_ctx* c, const char* fn) {
    if (c->stream_utt && c->stream_utt->mode == 2)
        return fail(c, KWS_ESTATE, std::string(fn) + ": this utterance set was stepped by kws_stream_utt_step_i16; a push would let its two counters drift apart");
    return KWS_OK;
}

int stream_utt_reset(kws_ctx* c, const ResetMask& m) {
    if (!c->stream_utt) return KWS_OK;
    return utt_launch(c, kws_live_reset_kernel, utt_args(c, nullptr, 0, nullptr, nullptr), m);
}

int stream_utt_pushed(kws_ctx* c) {
    if (!c->stream_utt) return KWS_OK;
    c->stream_utt->mode = 1;
    const LiveArgs a = utt_args(c, c->d_pcm_ring.get(), c->ring_len, c->d_hops.get(), c->d_feat_ring.get());
    // some stream is inactive: the masked step, its active streams by value (the unit holds at most one chunk)
    return c->sparse() ? utt_launch(c, kws_live_step_masked_kernel, a, c->active_chunk(0)) : utt_launch(c, kws_live_step_kernel<false>, a);
}

}  // namespace kws

using namespace kws;

#pragma GCC visibility push(default)
extern "C" {

int kws_host_stream_utt_history(int frame_len, int frame_step, int pre_roll, int max_frames, int slack_hops, int* history_samples) {
    long long h = 0;
    if (!history_samples || history_for(frame_len, frame_step, pre_roll, max_frames, slack_hops, &h) != KWS_OK) return KWS_EINVAL;
    *history_samples = (int)h;
    return KWS_OK;
}

int kws_stream_utt_open(kws_ctx* c, float log_energy_threshold, int on_window, int off_window, int pre_roll, int max_frames,
                        int history_samples, int max_events) {
    KWS_GUARD_BEGIN
    if (!c) return KWS_EINVAL;
    if (!c->n_streams) return fail(c, KWS_ESTATE, "kws_stream_utt_open: call kws_stream_open first");
    int rc = check_append_energy(c, "kws_stream_utt_open");
    if (!rc) rc = check_endpoint_windows(c, "kws_stream_utt_open", on_window, off_window);
    if (rc) return rc;
    if (pre_roll < 0 || max_frames < 2)
        return fail(c, KWS_EINVAL, "kws_stream_utt_open: need pre_roll >= 0 and max_frames >= 2 (a live ring is bounded: there is no \"no time-out\")");
    long long need = 0;
    if (history_for(c->fp.frame_len, c->fp.frame_step, pre_roll, max_frames, 0, &need) != KWS_OK)
        return fail(c, KWS_EINVAL, "kws_stream_utt_open: pre_roll + max_frames is beyond what a ring of int samples holds");
    if (history_samples < need || history_samples % c->fp.frame_step != 0)
        return fail(c, KWS_EINVAL, "kws_stream_utt_open: history_samples must be a multiple of frame_step and at least kws_host_stream_utt_history(..., slack_hops = 0)");
    if (max_events < c->n_streams) return fail(c, KWS_EINVAL, "kws_stream_utt_open: max_events must be at least n_streams (all may close at one step)");
    if (c->n_streams > LIVE_MAX_STREAMS)
        return fail(c, KWS_EUNSUPPORTED, "kws_stream_utt_open: more than 1024 streams (one workgroup walks them all)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    stream_utt_free(c);
    std::unique_ptr<StreamUtt> u(new StreamUtt());
    LiveArgs& a = u->a;
    const size_t S = (size_t)c->n_streams;
    a.S = c->n_streams;
    a.H = history_samples;
    a.on_window = on_window;
    a.off_window = off_window;
    a.pre_roll = pre_roll;
    a.max_frames = max_frames;
    a.threshold = log_energy_threshold;
    const size_t hist_b = sizeof(int16_t) * S * (size_t)a.H, pos_b = sizeof(long long) * S * 2;
    if (!(u->hist.alloc(S * (size_t)a.H) && u->pos.alloc(S * 2))) return fail(c, KWS_ENOMEM, "kws_stream_utt_open: allocation failed");
    a.hist = u->hist.get();
    a.pos = u->pos.get();
    rc = eq_open(c, "kws_stream_utt_open", u->queue, a.q, LIVE_REC, max_events);
    if (!rc) rc = alloc_endpoint_state(c, "kws_stream_utt_open", S, u->bits, u->counts);
    if (!rc) {
        a.bits = u->bits.get();
        a.counts = u->counts.get();
        hipError_t e = hipMemsetAsync(a.hist, 0, hist_b, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(a.pos, 0xFF, pos_b, c->stream);  // open = prev_close = -1
        if (e != hipSuccess) rc = fail_hip(c, e, "kws_stream_utt_open: hipMemsetAsync");
    }
    if (rc) {  // the clears enqueued so far finish before u's memory goes
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    c->stream_utt = u.release();
    return KWS_OK;
    KWS_GUARD_END(c, "kws_stream_utt_open")
}

int kws_stream_utt_close(kws_ctx* c) {
    if (!c) return KWS_EINVAL;
    if (!c->stream_utt) return KWS_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    stream_utt_free(c);
    return KWS_OK;
}

int kws_stream_utt_step_i16(kws_ctx* c, const int16_t* d_hop, const float* d_energy) {
    if (!c) return KWS_EINVAL;
    StreamUtt* u = c->stream_utt;
    if (!u) return fail(c, KWS_ESTATE, "kws_stream_utt_step_i16: call kws_stream_utt_open first");
    if (!d_hop && !d_energy) return fail(c, KWS_EINVAL, "kws_stream_utt_step_i16: d_hop and d_energy are both NULL");
    if (u->mode == 1) return fail(c, KWS_ESTATE, "kws_stream_utt_step_i16: this utterance set is stepped by the pushes");
    if (int rc = refuse_sparse(c, "kws_stream_utt_step_i16", "explicit steps")) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    u->mode = 2;
    return utt_launch(c, kws_live_step_kernel<false>, utt_args(c, d_hop, c->fp.frame_step, nullptr, d_energy));
}

int kws_stream_utt_flush(kws_ctx* c) {
    if (!c) return KWS_EINVAL;
    if (!c->stream_utt) return fail(c, KWS_ESTATE, "kws_stream_utt_flush: call kws_stream_utt_open first");
    HIP_TRY(c, hipSetDevice(c->device));
    return utt_launch(c, kws_live_step_kernel<true>, utt_args(c, nullptr, 0, nullptr, nullptr));
}

int kws_stream_utt_poll(kws_ctx* c, uint64_t* total_events, uint64_t* steps) {
    if (!c) return KWS_EINVAL;
    StreamUtt* u = c->stream_utt;
    if (!u) return fail(c, KWS_ESTATE, "kws_stream_utt_poll: call kws_stream_utt_open first");
    return eq_wait(c, "kws_stream_utt_poll", u->a.q, total_events, steps);
}

int kws_stream_utt_read(kws_ctx* c, uint64_t first_seq, int n, int64_t* out_records) {
    if (!c) return KWS_EINVAL;
    StreamUtt* u = c->stream_utt;
    if (!u) return fail(c, KWS_ESTATE, "kws_stream_utt_read: call kws_stream_utt_open first");
    return eq_read(c, "kws_stream_utt_read", u->a.q, LIVE_REC, first_seq, n, out_records);
}

int kws_stream_utt_cut_i16(kws_ctx* c, uint64_t first_seq, int U, int normalize_to, int16_t* d_clips, int n_out, int32_t* d_peak) {
    if (!c) return KWS_EINVAL;
    StreamUtt* u = c->stream_utt;
    if (!u) return fail(c, KWS_ESTATE, "kws_stream_utt_cut_i16: call kws_stream_utt_open first");
    if (!d_clips) return fail(c, KWS_EINVAL, "kws_stream_utt_cut_i16: d_clips is NULL");
    if (U < 1 || n_out < 1) return fail(c, KWS_EINVAL, "kws_stream_utt_cut_i16: U and n_out must be positive");
    if (int rc = check_normalize_to(c, "kws_stream_utt_cut_i16", normalize_to)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(kws_live_cut_kernel, dim3(U), dim3(LIVE_CUT_THREADS), 0, c->stream, u->a.hist, u->a.S, u->a.H, c->fp.frame_step,
                       u->a.q, (unsigned long long)first_seq, normalize_to, d_clips, n_out, d_peak);
    HIP_TRY(c, hipGetLastError());
    return KWS_OK;
}

}  // extern "C"
#pragma GCC visibility pop
