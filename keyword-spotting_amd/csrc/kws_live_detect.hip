// Live keyword events (include/kws_hip.h: kws_stream_detect_*) -- the decision layer of kws_scan_detect_f32 taken one decision
// per push for the streams of kws_stream_open: softmax, a posterior ring per stream, the direct causal sum, threshold and
// refractory, and an event queue mirrored in pinned host memory (kws_event_queue.h).  Everything here is a new kernel launched
// BEHIND a push; no other unit's kernel changes, and an unarmed context never gets here.
#include "kws_event_queue.h"
#include "kws_softmax_dev.h"

namespace kws {

constexpr int DETECT_MAX_STREAMS = 1024;  // one workgroup decides for every stream: one thread each
constexpr int DETECT_REC = 5;             // int64 words per record
constexpr int DETECT_MAX_WINDOW = 256;    // kws_scan_detect_f32's bound
static_assert(DETECT_MAX_STREAMS <= EQ_MAX_THREADS, "eq_emit counts one ballot per wavefront of the step's workgroup");

namespace {

// What a step reads.  logits and ctx_hops are set per launch (detect_launch); the rest is filled once by
// kws_stream_detect_open.  The unit's device counter q.unit()[0] = decisions made, which is also the queue's progress word
// (h_ctr[1]).
struct DetectArgs {
    const float* logits;      // [S][C]
    const int* ctx_hops;      // stepped by a push: the context's hop counter (already advanced); nullptr: explicit step
    int S, C, W, first_keyword, refractory, first_hop;
    float threshold;
    float* ring;              // [S][W][C] posteriors, decision d at slot d mod W
    float* smoothed;          // [S][C] of the newest decision, label [S] its first argmax
    int32_t* label;
    long long* next;          // [S]: the first decision at which stream s may fire again
    EventQueue q;             // records of DETECT_REC words
};

}  // namespace

// Everything kws_stream_detect_open allocates: as the step kernel takes it (a), and the owners a's pointers are filled from.
struct StreamDetect {
    DetectArgs a{};
    int mode = 0;  // 0: not stepped yet, 1: stepped by pushes, 2: stepped by kws_stream_detect_step_f32
    DeviceBuffer<float> ring, smoothed;
    DeviceBuffer<int32_t> label;
    DeviceBuffer<long long> next;
    DeviceBuffer<long long> epoch;  // [S]: decisions made when stream s was last reset (kws_stream_reset); 0 in a fresh set
    bool was_reset = false;         // a reset was issued on this set: its steps launch the epoch instantiation from then on
    EventQueueMem queue;
};

namespace {

// One decision of every stream.  ONE workgroup.  (1) thread s = stream s: softmax_row of the stream's logits into slot d mod W of
// its ring.  (2) behind a barrier the S * C sums are spread over ALL threads, one (stream, class) pair at a time with the class
// fastest (a wavefront's loads of one term are contiguous runs of C floats): the mean over the last min(W, d + 1) slots,
// oldest first -- scan_smooth_window's sum, no running sum.  The rule is restated here and not shared through a header: moving
// it out of kws_scan.hip changed that unit's generated code (register allocation of both smooth kernels), which this unit must
// not do; tests/test_live_detect_gpu.py holds the two to the same bits.  (3) behind another barrier thread s takes the first
// argmax of its row, the threshold and the refractory rule.
// The streams that fired emit their records and thread 0 publishes the totals as kws_event_queue.h lays down (eq_emit,
// eq_publish).  A push below first_hop decides nothing and advances nothing but the kernel count.
// EPOCH (a set on which kws_stream_reset was called): stream s's mean runs over the last min(W, d - epoch[s] + 1) slots -- the
// decisions since its reset --, same order of addition, same single division; the term count is then the pair's own, no longer
// the workgroup's.  The body of two kernels: a set that was never reset launches kws_live_detect_step_kernel, under the name and
// with the code it had before there was a reset (DESIGN 4.32 holds its listing to that).
// MASKED (a set with inactive streams, kws_stream_deactivate; `active`: the active ones): the epoch step in which an inactive
// stream writes no posterior, gets no mean, takes no decision and emits nothing; the decision counter runs on for the whole set.  A
// stream that joins again has its epoch at the decision count of its activation, so no mean reads a slot of its idle time.  A third
// kernel: the two above keep their code.
template <bool EPOCH, bool MASKED = false>
__device__ __forceinline__ void detect_step(const DetectArgs& a, const long long* __restrict__ epoch, const ResetMask* active = nullptr) {
    auto mine = [&](int s) { return !MASKED || active->has(s); };
    const int tid = threadIdx.x;
    const EqCounts was = eq_counts(a.q);
    const unsigned long long d = was.unit[0];
    long long h = (long long)d;  // explicit steps: the record's hop is the decision
    bool decide = true;          // workgroup-uniform
    if (a.ctx_hops) {
        h = a.ctx_hops[0];  // >= 1 behind a push
        decide = h >= a.first_hop;
    }
    bool fired = false;
    int arg = 0;
    float best = -1.f;
    if (decide) {
        const int C = a.C, W = a.W;
        const int slot = (int)(d % (unsigned long long)W);
        if (tid < a.S && mine(tid)) softmax_row(a.logits + (size_t)tid * C, C, a.ring + ((size_t)tid * W + slot) * C);
        __syncthreads();
        int terms = d + 1 < (unsigned long long)W ? (int)d + 1 : W;
        int oldest = slot - terms + 1 + (slot - terms + 1 < 0 ? W : 0);
        float count = (float)terms;
        for (int i = tid; i < a.S * C; i += (int)blockDim.x) {
            const int s = i / C, c = i - s * C;
            if constexpr (MASKED)
                if (!mine(s)) continue;
            if constexpr (EPOCH) {
                const long long since = (long long)d - epoch[s] + 1;  // >= 1: an epoch is a decision count already reached
                terms = since < (long long)W ? (int)since : W;
                oldest = slot - terms + 1 + (slot - terms + 1 < 0 ? W : 0);
                count = (float)terms;
            }
            const float* row = a.ring + (size_t)s * W * C + c;
            // scan_smooth_window's rule (kws_scan.hip), restated: float32 additions from 0, oldest first, then ONE division
            // The ring's slots from `oldest` to its end, then from slot 0: two linear runs, each taken eight loads at a time so that
            // a pair waits for memory once per eight terms (the additions stay one chain, in order).
            float acc = 0.f;
            auto run = [&](const float* p, int n) {
                int v = 0;
                for (; v + 8 <= n; v += 8) {
                    float t[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) t[j] = p[(size_t)(v + j) * C];
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc += t[j];
                }
                for (; v < n; ++v) acc += p[(size_t)v * C];
            };
            const int head = terms < W - oldest ? terms : W - oldest;
            run(row + (size_t)oldest * C, head);
            run(row, terms - head);
            acc /= count;
            a.smoothed[i] = acc;
        }
        __syncthreads();
        if (tid < a.S && mine(tid)) {
            const float* sm = a.smoothed + (size_t)tid * C;
            for (int c = 0; c < C; ++c) {
                const float v = sm[c];
                if (v > best) {
                    best = v;
                    arg = c;
                }
            }
            a.label[tid] = arg;
            if (arg >= a.first_keyword && best >= a.threshold && (long long)d >= a.next[tid]) {
                fired = true;
                a.next[tid] = (long long)d + a.refractory;
            }
        }
    }
    const long long rec[DETECT_REC] = {(long long)tid, (long long)d, h, (long long)arg, (long long)__float_as_uint(best)};
    const int all = eq_emit(a.q, was, fired, rec);
    const unsigned long long decisions = d + (decide ? 1 : 0);
    eq_publish(a.q, was, all, decisions);
    if (tid == 0) a.q.unit()[0] = decisions;
}

__global__ __launch_bounds__(DETECT_MAX_STREAMS) void kws_live_detect_step_kernel(const DetectArgs a) {
    detect_step<false>(a, nullptr);
}

__global__ __launch_bounds__(DETECT_MAX_STREAMS) void kws_live_detect_step_epoch_kernel(const DetectArgs a, const long long* __restrict__ epoch) {
    detect_step<true>(a, epoch);
}

__global__ __launch_bounds__(DETECT_MAX_STREAMS) void kws_live_detect_step_masked_kernel(const DetectArgs a, const long long* __restrict__ epoch,
                                                                                         const ResetMask active) {
    detect_step<true, true>(a, epoch, &active);
}

// One launch of the step kernel with the set's state.  Threads: one per stream at least, and up to one per (stream, class) pair
// for the sums.
int detect_launch(kws_ctx* c, const float* d_logits, const int* ctx_hops) {
    StreamDetect* u = c->stream_detect;
    DetectArgs a = u->a;
    a.logits = d_logits;
    a.ctx_hops = ctx_hops;
    const long long pairs = (long long)a.S * a.C;
    const int threads = pairs >= DETECT_MAX_STREAMS ? DETECT_MAX_STREAMS : (int)((pairs + 63) / 64 * 64);  // >= S rounded up: C >= 1
    if (c->sparse())  // (an epoch of 0, where no stream was reset yet, is the plain step's term count)
        hipLaunchKernelGGL(kws_live_detect_step_masked_kernel, dim3(1), dim3(threads), 0, c->stream, a, (const long long*)u->epoch.get(), c->active_chunk(0));
    else if (u->was_reset)
        hipLaunchKernelGGL(kws_live_detect_step_epoch_kernel, dim3(1), dim3(threads), 0, c->stream, a, (const long long*)u->epoch.get());
    else
        hipLaunchKernelGGL(kws_live_detect_step_kernel, dim3(1), dim3(threads), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    eq_enqueued(u->a.q);
    return KWS_OK;
}

}  // namespace

void stream_detect_free(kws_ctx* c) {
    delete c->stream_detect;
    c->stream_detect = nullptr;
}

// kws_stream_reset's side: what its kernel writes for the streams it names (next = 0, epoch = decisions made), and the switch
// of this set's steps to the epoch instantiation.
DetectResetView stream_detect_reset_view(kws_ctx* c) {
    StreamDetect* u = c->stream_detect;
    if (!u) return {nullptr, nullptr, nullptr};
    u->was_reset = true;
    return {u->a.next, u->epoch.get(), u->a.q.unit()};
}

// The push entries' side (kws_stream.hip): the step behind a push's launches, from that push's logits.
int stream_detect_pushed(kws_ctx* c, const float* d_logits, const char* fn, int model_classes) {
    StreamDetect* u = c->stream_detect;
    if (!u) return KWS_OK;
    const std::string f(fn);
    if (!d_logits)
        return fail(c, KWS_ESTATE, f + ": the context is armed for detection (kws_stream_detect_open) and this push asked for no logits; its hop was taken, no decision was made");
    if (u->mode == 2)
        return fail(c, KWS_ESTATE, f + ": this detection set was stepped by kws_stream_detect_step_f32; its hop was taken, no decision was made");
    if (u->a.C != model_classes)
        return fail(c, KWS_EINVAL, f + ": kws_stream_detect_open was given another class count than the loaded model's; the hop was taken, no decision was made");
    u->mode = 1;
    return detect_launch(c, d_logits, c->d_hops.get());
}

}  // namespace kws

using namespace kws;

#pragma GCC visibility push(default)
extern "C" {

int kws_stream_detect_open(kws_ctx* c, int C, int smooth_window, int first_keyword, float threshold, int refractory, int first_hop,
                           int max_events) {
    KWS_GUARD_BEGIN
    if (!c) return KWS_EINVAL;
    if (!c->n_streams) return fail(c, KWS_ESTATE, "kws_stream_detect_open: call kws_stream_open first");
    if (C < 1 || C > MAX_CLASSES) return fail(c, KWS_EINVAL, "kws_stream_detect_open: C must be in [1, 64]");
    if (smooth_window < 1 || smooth_window > DETECT_MAX_WINDOW) return fail(c, KWS_EINVAL, "kws_stream_detect_open: smooth_window must be in [1, 256]");
    if (refractory < 1 || first_keyword < 0 || first_hop < 0)
        return fail(c, KWS_EINVAL, "kws_stream_detect_open: need refractory >= 1, first_keyword >= 0 and first_hop >= 0");
    if (max_events < c->n_streams) return fail(c, KWS_EINVAL, "kws_stream_detect_open: max_events must be at least n_streams (all may fire at one step)");
    if (c->n_streams > DETECT_MAX_STREAMS)
        return fail(c, KWS_EUNSUPPORTED, "kws_stream_detect_open: more than 1024 streams (one workgroup decides for them all)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    stream_detect_free(c);
    std::unique_ptr<StreamDetect> u(new StreamDetect());
    DetectArgs& a = u->a;
    const size_t S = (size_t)c->n_streams;
    a.S = c->n_streams;
    a.C = C;
    a.W = smooth_window;
    a.first_keyword = first_keyword;
    a.refractory = refractory;
    a.first_hop = first_hop;
    a.threshold = threshold;
    const size_t sm_b = sizeof(float) * S * C, label_b = sizeof(int32_t) * S, next_b = sizeof(long long) * S;
    if (!(u->ring.alloc(S * (size_t)smooth_window * C) && u->smoothed.alloc(S * C) && u->label.alloc(S) && u->next.alloc(S) && u->epoch.alloc(S)))
        return fail(c, KWS_ENOMEM, "kws_stream_detect_open: allocation failed");
    a.ring = u->ring.get();
    a.smoothed = u->smoothed.get();
    a.label = u->label.get();
    a.next = u->next.get();
    int rc = eq_open(c, "kws_stream_detect_open", u->queue, a.q, DETECT_REC, max_events);
    if (!rc) {
        // the ring needs no clearing: a decision reads only slots written since the arming
        hipError_t e = hipMemsetAsync(a.smoothed, 0, sm_b, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(a.label, 0, label_b, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(a.next, 0, next_b, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(u->epoch.get(), 0, next_b, c->stream);
        if (e != hipSuccess) rc = fail_hip(c, e, "kws_stream_detect_open: hipMemsetAsync");
    }
    if (rc) {  // the clears enqueued so far finish before u's memory goes
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    c->stream_detect = u.release();
    return KWS_OK;
    KWS_GUARD_END(c, "kws_stream_detect_open")
}

int kws_stream_detect_close(kws_ctx* c) {
    if (!c) return KWS_EINVAL;
    if (!c->stream_detect) return KWS_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    stream_detect_free(c);
    return KWS_OK;
}

int kws_stream_detect_step_f32(kws_ctx* c, const float* d_logits) {
    if (!c) return KWS_EINVAL;
    StreamDetect* u = c->stream_detect;
    if (!u) return fail(c, KWS_ESTATE, "kws_stream_detect_step_f32: call kws_stream_detect_open first");
    if (!d_logits) return fail(c, KWS_EINVAL, "kws_stream_detect_step_f32: d_logits is NULL");
    if (u->mode == 1) return fail(c, KWS_ESTATE, "kws_stream_detect_step_f32: this detection set is stepped by the pushes");
    if (int rc = refuse_sparse(c, "kws_stream_detect_step_f32", "explicit steps")) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    u->mode = 2;
    return detect_launch(c, d_logits, nullptr);
}

int kws_stream_detect_poll(kws_ctx* c, uint64_t* total_events, uint64_t* decisions) {
    if (!c) return KWS_EINVAL;
    StreamDetect* u = c->stream_detect;
    if (!u) return fail(c, KWS_ESTATE, "kws_stream_detect_poll: call kws_stream_detect_open first");
    return eq_wait(c, "kws_stream_detect_poll", u->a.q, total_events, decisions);
}

int kws_stream_detect_read(kws_ctx* c, uint64_t first_seq, int n, int64_t* out_records) {
    if (!c) return KWS_EINVAL;
    StreamDetect* u = c->stream_detect;
    if (!u) return fail(c, KWS_ESTATE, "kws_stream_detect_read: call kws_stream_detect_open first");
    return eq_read(c, "kws_stream_detect_read", u->a.q, DETECT_REC, first_seq, n, out_records);
}

int kws_stream_detect_smoothed(kws_ctx* c, float* d_smoothed, int32_t* d_label) {
    if (!c) return KWS_EINVAL;
    StreamDetect* u = c->stream_detect;
    if (!u) return fail(c, KWS_ESTATE, "kws_stream_detect_smoothed: call kws_stream_detect_open first");
    if (!d_smoothed || !d_label) return fail(c, KWS_EINVAL, "kws_stream_detect_smoothed: d_smoothed / d_label is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(d_smoothed, u->a.smoothed, sizeof(float) * (size_t)u->a.S * u->a.C, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_label, u->a.label, sizeof(int32_t) * (size_t)u->a.S, hipMemcpyDeviceToDevice, c->stream));
    return KWS_OK;
}

}  // extern "C"
#pragma GCC visibility pop
