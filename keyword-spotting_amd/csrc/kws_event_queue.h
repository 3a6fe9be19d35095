// The host-mirrored event queue of the live units (kws_live.hip: utterances, kws_live_detect.hip: keyword events): a step kernel
// of ONE workgroup numbers the events of its step, writes them to a device queue and to a pinned host mirror, and raises a
// kernel count the host spins on.  Inline functions only: the device half is the tail of both step kernels, the host half what
// their open, poll and read entries do with the queue; kws_stream_wait_host (kws_stream.hip) shares the bounded spin.  The queue's
// memory is owned by an EventQueueMem beside the EventQueue that travels to the kernels, and goes with its unit.
// What the two halves keep, and what every change here must keep:
//  1. Every thread reads the counters at the top of the kernel (eq_counts); thread 0 overwrites them only behind the last
//     barrier (eq_publish, and the unit's own words after it).
//  2. A firing lane's sequence number is the total before the step + the firing lanes of the lower wavefronts (their ballots'
//     popcounts, through LDS) + the lower firing lanes of its own ballot: consecutive, ascending by stream, no atomics.  Its
//     slot is seq % max_events.
//  3. Word by word, a record goes to the device queue as plain stores and to the mirror as relaxed system-scope stores.
//  4. Each wavefront waits for vmcnt(0), then the barrier; thread 0 then writes the device counters, h_ctr[0] and h_ctr[1],
//     waits for vmcnt(0) again and only then stores h_ctr[2].
//  5. The host spins on h_ctr[2] >= ticks_enqueued; after the bound it falls back to hipStreamSynchronize and fails with
//     KWS_EHIP if the flag is still missing.  It issues an acquire fence before it reads the totals.  A read checks "landed"
//     before the copy and "not overwritten" against a re-read total after it.
//  6. The hardware assumption: a store a wavefront has waited for (vmcnt 0) is acknowledged -- it is on its way, and such stores
//     arrive in order --, so the records and the totals are in host memory before the kernel count that follows them: the
//     discipline of the push's zero-copy results (kws_dscnn.hip), in one workgroup.  This is an assumption about the hardware,
//     outside the HSA memory model, which orders nothing between relaxed stores (first finding).
#pragma once

#include <atomic>
#include <chrono>
#include <cstring>

#include "kws_ctx.h"

namespace kws {

constexpr int EQ_MAX_THREADS = 1024;  // of the one workgroup that emits

// Travels by value inside a step kernel's arguments.  ctr is ONE zeroed 64-byte device block: the queue's two words, then the
// unit's own counters (unit(); eq_counts reads the first two).  h_ctr[3] = events so far, the unit's progress, kernels finished.
struct EventQueue {
    unsigned long long* ctr;    // [0] events so far, [1] kernels finished
    long long* queue;           // [max_events][REC]
    long long* h_queue;         // pinned, device-mapped mirror of queue
    unsigned long long* h_ctr;  // pinned, device-mapped
    int max_events;
    unsigned long long ticks_enqueued;  // host only: kernels enqueued so far; h_ctr[2] reads this once the newest has landed
    __host__ __device__ unsigned long long* unit() const { return ctr + 2; }
};

// ---- device half ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void store_host(long long* p, long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// What every thread reads at the top of the kernel: events so far, kernels finished and the unit's first two words -- ONE 32-byte
// load, so that the words a kernel needs last do not become a second round trip to memory --, the queue's size, the wavefronts.
struct EqCounts { unsigned long long total, ticks, unit[2]; int max_events, n_waves; };
__device__ __forceinline__ EqCounts eq_counts(const EventQueue& q) {
    const ulonglong4 w = *reinterpret_cast<const ulonglong4*>(q.ctr);
    return {w.x, w.y, {w.z, w.w}, q.max_events, (int)blockDim.x >> 6};
}

// Called by every thread of the workgroup.  The lanes with `fires` get consecutive sequence numbers from was.total on and store
// their record; returns the number of events of this step.
template <int REC>
__device__ __forceinline__ int eq_emit(const EventQueue& q, const EqCounts& was, bool fires, const long long (&rec)[REC]) {
    __shared__ int wave_n[EQ_MAX_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(fires);
    if (lane == 0) wave_n[wave] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < was.n_waves; ++k) {
        before += k < wave ? wave_n[k] : 0;
        all += wave_n[k];
    }
    if (fires) {
        const unsigned long long seq = was.total + (unsigned long long)before + (unsigned long long)__popcll(b & ((1ull << lane) - 1ull));
        const size_t at = (size_t)(seq % (unsigned long long)was.max_events) * REC;
#pragma unroll
        for (int k = 0; k < REC; ++k) {
            q.queue[at + k] = rec[k];
            store_host(q.h_queue + at + k, rec[k]);
        }
    }
    return all;
}

// Called by every thread behind eq_emit: the counts read at the top, this step's events, the unit's progress for h_ctr[1].
__device__ __forceinline__ void eq_publish(const EventQueue& q, EqCounts was, int events, unsigned long long progress) {
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wavefront's stores, the host's among them, are acknowledged
    __syncthreads();                     // ... and so are every other wavefront's; all have read ctr[]
    if (threadIdx.x == 0) {
        const unsigned long long total = was.total + (unsigned long long)events;
        q.ctr[0] = total;
        q.ctr[1] = was.ticks + 1;
        store_host(reinterpret_cast<long long*>(q.h_ctr), (long long)total);
        store_host(reinterpret_cast<long long*>(q.h_ctr) + 1, (long long)progress);
        __builtin_amdgcn_s_waitcnt(0x0F70);
        store_host(reinterpret_cast<long long*>(q.h_ctr) + 2, (long long)(was.ticks + 1));
    }
}

// ---- host half --------------------------------------------------------------------------------------------------------------------
// Spin until seen(), a pause between looks; bounded: false after ~2 ms without it (the clock is read every 1024 spins).
template <class Seen>
inline bool spin_until(Seen seen) {
    const auto t0 = std::chrono::steady_clock::now();
    for (long spin = 1;; ++spin) {
        if (seen()) return true;
        __builtin_ia32_pause();
        if ((spin & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) return false;
    }
}

// What an EventQueue points into.
struct EventQueueMem {
    DeviceBuffer<unsigned long long> ctr;
    DeviceBuffer<long long> queue;
    PinnedBuffer<long long> h_queue;
    PinnedBuffer<unsigned long long> h_ctr;
};

// Allocate a queue of max_events records of `rec` words into m and point q at it; the mirror zeroed here, the device side on the
// context's stream.  On a failure the caller lets m go, after the stream has drained.
inline int eq_open(kws_ctx* c, const char* fn, EventQueueMem& m, EventQueue& q, int rec, int max_events) {
    q = EventQueue{};
    const size_t words = (size_t)max_events * rec, queue_b = sizeof(long long) * words;
    const unsigned flags = hipHostMallocMapped | hipHostMallocCoherent;  // fine-grained: device stores are visible to the host as they land
    if (!(m.ctr.alloc(8) && m.queue.alloc(words) && m.h_queue.alloc(words, flags) && m.h_ctr.alloc(8, flags)))
        return fail(c, KWS_ENOMEM, std::string(fn) + ": allocation failed");
    q.ctr = m.ctr.get();
    q.queue = m.queue.get();
    q.h_queue = m.h_queue.get();
    q.h_ctr = m.h_ctr.get();
    q.max_events = max_events;
    memset(q.h_queue, 0, queue_b);
    memset(q.h_ctr, 0, 64);
    hipError_t e = hipMemsetAsync(q.ctr, 0, 64, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(q.queue, 0, queue_b, c->stream);
    return e == hipSuccess ? KWS_OK : fail_hip(c, e, (std::string(fn) + ": hipMemsetAsync").c_str());
}

inline void eq_enqueued(EventQueue& q) { q.ticks_enqueued += 1; }

// Wait for the newest enqueued kernel, then the totals: events so far and the unit's progress.
inline int eq_wait(kws_ctx* c, const char* fn, const EventQueue& q, uint64_t* total_events, uint64_t* progress) {
    volatile unsigned long long* h = q.h_ctr;
    const unsigned long long want = q.ticks_enqueued;
    if (!spin_until([&] { return h[2] >= want; })) {  // fall back to the stream
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (h[2] < want) return fail(c, KWS_EHIP, std::string(fn) + ": the stream drained but the step's flag never arrived");
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (total_events) *total_events = h[0];
    if (progress) *progress = h[1];
    return KWS_OK;
}

// Records first_seq .. first_seq + n - 1 of `rec` words each out of the mirror.
inline int eq_read(kws_ctx* c, const char* fn, const EventQueue& q, int rec, uint64_t first_seq, int n, int64_t* out_records) {
    if (n < 1 || !out_records) return fail(c, KWS_EINVAL, std::string(fn) + ": n must be positive and out_records not NULL");
    volatile unsigned long long* h = q.h_ctr;
    unsigned long long total = h[0];
    std::atomic_thread_fence(std::memory_order_acquire);
    if (first_seq + (unsigned long long)n > total) return fail(c, KWS_EINVAL, std::string(fn) + ": sequence numbers beyond the events landed so far");
    for (int i = 0; i < n; ++i) {
        const volatile long long* r = q.h_queue + (size_t)((first_seq + i) % (unsigned long long)q.max_events) * rec;
        for (int k = 0; k < rec; ++k) out_records[(size_t)i * rec + k] = r[k];
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    total = h[0];  // again: a step that landed during the copy may have overwritten the oldest
    if (first_seq + (unsigned long long)q.max_events < total) return fail(c, KWS_EINVAL, std::string(fn) + ": the sequence number is no longer in the queue");
    return KWS_OK;
}

}  // namespace kws
