// Host ingest for the fused path: kws_infer_host_i16 takes a HOST batch of PCM clips and
// returns HOST logits / labels.  It replaces what the reference does between the decoded audio and the model input --
// DataLoader workers collating batches into pinned memory and `inputs.to(device)` (kws/libs/data_loader.py:96-105,
// train.py:108-121, kws/libs/training.py:286) -- with a three-stage pipeline inside the library:
//
//   pack   the batch is cut into chunks of `chunk` clips; a pool of host threads copies chunk k+1 from the caller's
//          (pageable) memory into a pinned staging slot while
//   H2D    chunk k travels to the device on a copy stream (hipMemcpyAsync from pinned memory = one DMA), while
//   run    chunk k-1 runs MFCC + DS-CNN on the context's stream, and
//   D2H    the 52 bytes per clip of results of chunk k-2 return on a second copy stream into pinned memory.
//
// Events order the streams; the host thread blocks only when it needs a slot that is still in flight.  With S slots up
// to S chunks are in flight.  A caller buffer that is already pinned (hipHostMalloc / hipHostRegister / torch
// pin_memory) skips the pack stage: the DMA reads it directly.  The PCIe-inclusive rate of this path is reported by
// tools/bench_ingest.py, never as bench.py's `value`.
#include <algorithm>
#include <cstring>
#include <new>
#include <thread>

#include "kws_ctx.h"
#include "kws_pack_pool.h"

namespace kws {

struct IngestSlot {
    PinnedBuffer<int16_t> h_in;      // pinned [chunk][n_samples]
    DeviceBuffer<int16_t> d_in;      // device
    DeviceBuffer<float> d_logits;    // device [chunk][C]
    DeviceBuffer<int32_t> d_label;   // device [chunk]
    PinnedBuffer<float> h_logits;    // pinned
    PinnedBuffer<int32_t> h_label;   // pinned
    hipEvent_t staged = nullptr, computed = nullptr, drained = nullptr;
    int count = 0;                // clips this slot currently carries (0: free)
    float* dst_logits = nullptr;  // where its results go in the submitting call's host arrays (already offset to the chunk)
    int32_t* dst_label = nullptr;
    uint64_t ticket = 0;          // the submit call it belongs to
};

struct Ingest {
    int chunk = 0, n_slots = 0, n_samples = 0, classes = 0;
    hipStream_t copy_in[2] = {nullptr, nullptr}, copy_out = nullptr;  // two H2D streams: consecutive chunks ride different DMA engines
    std::vector<IngestSlot> slots;
    PackPool* pool = nullptr;
    int pool_threads = 0;
    uint64_t next_ticket = 1;
    int next_slot = 0, lane = 0;   // ring position and H2D stream of the next chunk (they persist across submit calls)
    // tickets whose chunks were dropped after a HIP failure and that no kws_infer_host_wait has reported yet, with the code of
    // the failure: their callers' arrays are incomplete, and a wait that covers one must say so
    struct Dropped {
        uint64_t ticket;
        int code;
    };
    std::vector<Dropped> dropped;
    // configuration requested through kws_ingest_config (0 = default)
    int want_chunk = 0, want_slots = 0, want_threads = 0;
};

static void ingest_release(Ingest* g) {
    if (!g) return;
    for (auto& s : g->slots) {
        if (s.staged) (void)hipEventDestroy(s.staged);
        if (s.computed) (void)hipEventDestroy(s.computed);
        if (s.drained) (void)hipEventDestroy(s.drained);
    }
    g->slots.clear();  // the slots' staging memory goes with them
    for (auto& st : g->copy_in) {
        if (st) (void)hipStreamDestroy(st);
        st = nullptr;
    }
    if (g->copy_out) (void)hipStreamDestroy(g->copy_out);
    g->copy_out = nullptr;
    g->chunk = g->n_slots = 0;
}

void ingest_free(kws_ctx* c) {
    if (!c || !c->ingest) return;
    ingest_release(c->ingest);
    delete c->ingest->pool;
    delete c->ingest;
    c->ingest = nullptr;
}

// (Re)build the staging rings for the current front end / model geometry and the requested configuration.
static int ingest_prepare(kws_ctx* c) {
    if (!c->ingest) c->ingest = new (std::nothrow) Ingest();
    Ingest* g = c->ingest;
    if (!g) return fail(c, KWS_ENOMEM, "kws_infer_host_i16: out of host memory");
    const int chunk = g->want_chunk > 0 ? g->want_chunk : 1024;
    const int n_slots = g->want_slots > 0 ? g->want_slots : 3;
    int threads = g->want_threads > 0 ? g->want_threads : (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency() / 2));
    if (g->want_threads < 0) threads = 0;  // pack on the calling thread
    const int n_samples = c->fp.n_samples, classes = c->mw.num_classes;
    if (!g->pool || g->pool_threads != threads) {
        delete g->pool;
        g->pool = new (std::nothrow) PackPool(threads);
        g->pool_threads = threads;
        if (!g->pool) return fail(c, KWS_ENOMEM, "kws_infer_host_i16: out of host memory");
    }
    if (g->chunk == chunk && g->n_slots == n_slots && g->n_samples == n_samples && g->classes == classes) return KWS_OK;
    for (auto& s : g->slots)
        if (s.count) return fail(c, KWS_ESTATE, "kws_infer_host_i16: the ingest geometry changed while batches are in flight (kws_infer_host_wait first)");
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    ingest_release(g);
    g->next_slot = g->lane = 0;
    HIP_TRY(c, hipStreamCreateWithFlags(&g->copy_in[0], hipStreamNonBlocking));
    HIP_TRY(c, hipStreamCreateWithFlags(&g->copy_in[1], hipStreamNonBlocking));
    HIP_TRY(c, hipStreamCreateWithFlags(&g->copy_out, hipStreamNonBlocking));
    g->slots.resize(n_slots);
    const size_t in_n = (size_t)chunk * n_samples, lg_n = (size_t)chunk * classes, lb_n = (size_t)chunk;
    for (auto& s : g->slots) {
        if (!(s.h_in.alloc(in_n, hipHostMallocDefault) && s.d_in.alloc(in_n) && s.d_logits.alloc(lg_n) && s.d_label.alloc(lb_n) &&
              s.h_logits.alloc(lg_n, hipHostMallocDefault) && s.h_label.alloc(lb_n, hipHostMallocDefault)) ||
            hipEventCreateWithFlags(&s.staged, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&s.computed, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&s.drained, hipEventDisableTiming) != hipSuccess) {
            ingest_release(g);
            return fail(c, KWS_ENOMEM, "kws_infer_host_i16: staging allocation failed");
        }
    }
    g->chunk = chunk;
    g->n_slots = n_slots;
    g->n_samples = n_samples;
    g->classes = classes;
    return kws_reserve(c, chunk);
}

// Results of the chunk a slot carries: wait for its D2H, hand them to the caller, mark the slot free.
static int ingest_collect(kws_ctx* c, IngestSlot& s) {
    if (s.count == 0) return KWS_OK;
    HIP_TRY(c, hipEventSynchronize(s.drained));
    const int C = c->ingest->classes;
    memcpy(s.dst_logits, s.h_logits.get(), sizeof(float) * (size_t)s.count * C);
    if (s.dst_label) memcpy(s.dst_label, s.h_label.get(), sizeof(int32_t) * (size_t)s.count);
    s.count = 0;
    return KWS_OK;
}

// 0: ordinary (pageable) host memory, 1: pinned / registered host memory (the DMA can read it), -1: not host memory at all
static int host_pointer_kind(const void* p) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // an ordinary malloc'ed pointer is "invalid value" for the query: not an error here
        return 0;
    }
    if (a.type == hipMemoryTypeHost) return 1;
    if (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeArray) return -1;
    return 0;  // unregistered / managed: treated as pageable
}

// Let the pipeline's own streams run dry before chunks are forgotten: a forgotten slot's staging memory is packed into by the
// host and its device buffers are written by the next chunk that takes it, on whichever H2D stream comes next.
static void ingest_quiesce(kws_ctx* c) {
    Ingest* g = c->ingest;
    for (hipStream_t st : {g->copy_in[0], g->copy_in[1], c->stream, g->copy_out}) (void)hipStreamSynchronize(st);
    (void)hipGetLastError();
}

// Forget every chunk of `ticket` that the ring still carries and remember the ticket, so that kws_infer_host_wait reports it
// instead of returning KWS_OK over rows nobody filled.  (The streams have been quiesced by the caller.)
static void ingest_drop(Ingest* g, uint64_t ticket, int code) {
    for (auto& s : g->slots)
        if (s.count && s.ticket == ticket) s.count = 0;
    for (const auto& d : g->dropped)
        if (d.ticket == ticket) return;
    g->dropped.push_back({ticket, code});
}

// Deliver every chunk of the tickets up to `limit`, oldest first.  A chunk whose D2H failed takes its whole ticket with it
// (ingest_drop) -- and only that ticket: the chunks of the others are still delivered.
static void ingest_drain(kws_ctx* c, uint64_t limit) {
    Ingest* g = c->ingest;
    bool quiet = false;
    for (int i = 0; i < g->n_slots; ++i) {
        IngestSlot& s = g->slots[(g->next_slot + i) % g->n_slots];
        if (!s.count || s.ticket > limit) continue;
        const int rc = ingest_collect(c, s);
        if (rc == KWS_OK) continue;
        if (!quiet) ingest_quiesce(c);
        quiet = true;
        ingest_drop(g, s.ticket, rc);
    }
}

// The unreported dropped tickets up to `limit`: none -> KWS_OK; else they are taken off the list and named in the error text,
// with the code of the first one's failure.
static int ingest_report_dropped(kws_ctx* c, uint64_t limit) {
    Ingest* g = c->ingest;
    std::string names;
    int code = KWS_OK, n = 0;
    for (size_t i = 0; i < g->dropped.size();) {
        if (g->dropped[i].ticket > limit) {
            ++i;
            continue;
        }
        if (!n++) code = g->dropped[i].code;
        names += (names.empty() ? "" : ", ") + std::to_string(g->dropped[i].ticket);
        g->dropped.erase(g->dropped.begin() + (std::ptrdiff_t)i);
    }
    if (!n) return KWS_OK;
    return fail(c, code, std::string("kws_infer_host_wait: the results of ") + (n > 1 ? "tickets " : "ticket ") + names +
                             " were dropped after a failure (code " + std::to_string(code) + "): their h_logits / h_label are incomplete");
}

}  // namespace kws

using namespace kws;

#pragma GCC visibility push(default)
extern "C" {

int kws_ingest_config(kws_ctx* c, int chunk_clips, int n_slots, int pack_threads) {
    if (!c) return KWS_EINVAL;
    if (c->ingest)
        for (auto& s : c->ingest->slots)
            if (s.count) return fail(c, KWS_ESTATE, "kws_ingest_config: batches are in flight (kws_infer_host_wait first)");
    if (chunk_clips < 0 || n_slots < 0 || (n_slots > 0 && n_slots < 2) || n_slots > 16 || pack_threads > 64)
        return fail(c, KWS_EINVAL, "kws_ingest_config: chunk_clips >= 0, n_slots 0 or 2..16, pack_threads <= 64");
    if (!c->ingest) c->ingest = new (std::nothrow) Ingest();
    if (!c->ingest) return fail(c, KWS_ENOMEM, "kws_ingest_config: out of host memory");
    c->ingest->want_chunk = chunk_clips;
    c->ingest->want_slots = n_slots;
    c->ingest->want_threads = pack_threads;
    return KWS_OK;
}

// Enqueue one host batch: every chunk is packed (pageable input), sent, computed and its results started on their way back;
// slots still carrying an older chunk are collected (results copied to THAT chunk's destination) as the ring comes round.
// Every argument and state check comes before the call takes its ticket, and a call refused by one has touched nothing: the
// ring, the slots and the tickets in flight are as they were.  *began is the call's ticket once it has one (0 before): an
// error with *began != 0 may have left chunks of this call in the ring (ingest_abandon).
static int ingest_submit(kws_ctx* c, const int16_t* h_wav, int B, float* h_logits, int32_t* h_label, uint64_t* ticket_out, uint64_t* began) {
    if (!h_wav || !h_logits) return fail(c, KWS_EINVAL, "kws_infer_host_submit_i16: h_wav and h_logits must not be NULL");
    if (B <= 0) return fail(c, KWS_EINVAL, "kws_infer_host_submit_i16: B must be positive");
    if (!c->fe_ready || !c->model_ready) return fail(c, KWS_ESTATE, "kws_infer_host_submit_i16: front end or model not configured");
    HIP_TRY(c, hipSetDevice(c->device));
    const int kind = host_pointer_kind(h_wav);
    if (kind < 0 || host_pointer_kind(h_logits) < 0 || (h_label && host_pointer_kind(h_label) < 0))
        return fail(c, KWS_EINVAL, "kws_infer_host_submit_i16: h_wav / h_logits / h_label must be HOST pointers (device tensors go to kws_infer_i16)");
    int rc = ingest_prepare(c);  // rebuilds the ring only when nothing is in flight, refuses (KWS_ESTATE) otherwise
    if (rc) return rc;
    Ingest* g = c->ingest;
    const int n = g->n_samples, C = g->classes;
    const bool direct = kind == 1;  // the DMA can read the caller's buffer: no pack stage
    // Chunk size of THIS batch: a batch smaller than the ring (the reference's own batch_size = 1028, train.py:110, against
    // 3 x 1024) would otherwise be one chunk plus a tail, its pack / H2D / compute / D2H strictly one after the other; cut
    // into as many chunks as there are slots (not below 128 clips: a launch pair per chunk costs ~0.1 ms of fixed time).
    int chunk = (B + g->n_slots - 1) / g->n_slots;
    chunk = std::min(g->chunk, std::max(chunk, std::min(B, 128)));  // never above what the staging slots hold
    const uint64_t ticket = g->next_ticket++;
    *began = ticket;
    for (int first = 0; first < B; first += chunk, g->next_slot = (g->next_slot + 1) % g->n_slots, g->lane ^= 1) {
        IngestSlot& s = g->slots[g->next_slot];
        rc = ingest_collect(c, s);  // blocks only if this slot's previous chunk is still in flight
        if (rc) return rc;
        const int count = std::min(chunk, B - first);
        const size_t bytes = sizeof(int16_t) * (size_t)count * n;
        const int16_t* src = h_wav + (size_t)first * n;
        if (!direct) {
            g->pool->copy(s.h_in.get(), src, bytes);
            src = s.h_in.get();
        }
        HIP_TRY(c, hipMemcpyAsync(s.d_in.get(), src, bytes, hipMemcpyHostToDevice, g->copy_in[g->lane]));
        HIP_TRY(c, hipEventRecord(s.staged, g->copy_in[g->lane]));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, s.staged, 0));
        rc = kws_infer_i16(c, s.d_in.get(), count, s.d_logits.get(), s.d_label.get());
        if (rc) return rc;
        HIP_TRY(c, hipEventRecord(s.computed, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(g->copy_out, s.computed, 0));
        HIP_TRY(c, hipMemcpyAsync(s.h_logits.get(), s.d_logits.get(), sizeof(float) * (size_t)count * C, hipMemcpyDeviceToHost, g->copy_out));
        HIP_TRY(c, hipMemcpyAsync(s.h_label.get(), s.d_label.get(), sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost, g->copy_out));
        HIP_TRY(c, hipEventRecord(s.drained, g->copy_out));
        s.dst_logits = h_logits + (size_t)first * C;
        s.dst_label = h_label ? h_label + first : nullptr;
        s.ticket = ticket;
        s.count = count;
    }
    if (ticket_out) *ticket_out = ticket;
    return KWS_OK;
}

// A submit failed with `code` after it took `ticket` (a HIP error mid-batch): the callers of the OLDER tickets get their
// results first, then the streams run dry and only this call's own chunks are forgotten; the ticket is remembered as dropped.
// The error text of the failure itself is kept.
static void ingest_abandon(kws_ctx* c, uint64_t ticket, int code) {
    const std::string err = c->err;
    ingest_drain(c, ticket - 1);
    ingest_quiesce(c);
    ingest_drop(c->ingest, ticket, code);
    c->err = err;
}

// Collect every chunk of the batches up to `ticket` (0: everything in flight), oldest first, then report the tickets among
// them whose chunks were dropped: never KWS_OK over rows nobody filled.
static int ingest_wait(kws_ctx* c, uint64_t ticket) {
    Ingest* g = c->ingest;
    if (!g) return KWS_OK;
    const uint64_t limit = ticket ? ticket : UINT64_MAX;
    if (!g->slots.empty()) {
        HIP_TRY(c, hipSetDevice(c->device));
        ingest_drain(c, limit);
    }
    return ingest_report_dropped(c, limit);
}

int kws_infer_host_submit_i16(kws_ctx* c, const int16_t* h_wav, int B, float* h_logits, int32_t* h_label, uint64_t* ticket) {
    if (!c) return KWS_EINVAL;
    uint64_t began = 0;
    // failed half-way: chunks of this call may be in flight (a refusal, began == 0, has touched nothing)
    auto failed = [&](int code) noexcept {
        if (!began) return;
        try {
            ingest_abandon(c, began, code);
        } catch (...) {
        }
        if (ticket) *ticket = began;  // the number kws_infer_host_wait will name
    };
    try {
        const int rc = ingest_submit(c, h_wav, B, h_logits, h_label, ticket, &began);
        if (rc) failed(rc);
        return rc;
    } catch (const std::bad_alloc&) {
        failed(KWS_ENOMEM);
        return fail(c, KWS_ENOMEM, "kws_infer_host_submit_i16: out of host memory");
    } catch (...) {
        failed(KWS_EHIP);
        return fail(c, KWS_EHIP, "kws_infer_host_submit_i16: unexpected C++ exception");
    }
}

int kws_infer_host_wait(kws_ctx* c, uint64_t ticket) {
    if (!c) return KWS_EINVAL;
    try {
        return ingest_wait(c, ticket);
    } catch (...) {
        return fail(c, KWS_EHIP, "kws_infer_host_wait: unexpected C++ exception");
    }
}

int kws_infer_host_i16(kws_ctx* c, const int16_t* h_wav, int B, float* h_logits, int32_t* h_label) {
    if (!c) return KWS_EINVAL;
    uint64_t ticket = 0;
    int rc = kws_infer_host_submit_i16(c, h_wav, B, h_logits, h_label, &ticket);
    if (rc) {  // this return reports the failure: a dropped ticket of this very call is not reported to a later wait again
        if (ticket && c->ingest) {
            auto& d = c->ingest->dropped;
            d.erase(std::remove_if(d.begin(), d.end(), [&](const Ingest::Dropped& x) { return x.ticket == ticket; }), d.end());
        }
        return rc;
    }
    return kws_infer_host_wait(c, ticket);
}

}  // extern "C"
#pragma GCC visibility pop
