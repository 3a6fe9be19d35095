// Sparse live sets (include/kws_hip.h: kws_stream_deactivate, kws_stream_activate, kws_stream_active): a stream of the open set that
// nobody is using leaves the set, and from then on a push launches, reads and writes for the active streams alone -- the fused
// push on a grid of n_active * cluster workgroups whose stream index comes from a list (kws_dscnn.hip, ACTIVE), the armed steps
// in their masked kernels (kws_live.hip, kws_live_detect.hip).  An idle stream needs no bookkeeping: after kws_stream_reset a
// stream's state is that of a stream that has heard digital silence since kws_stream_open, whatever the hop counter says, so a
// stream is left alone while it is idle and reset when it joins again.
// The host mirror (kws_ctx: active_bits, n_active) decides every launch: the count is the grid, the bits travel BY VALUE in chunks
// of RESET_CHUNK streams (the ResetMask discipline of kws_stream_reset.hip) -- nothing is copied to the device that a later call
// could overtake, nothing waits, and after the set's first deactivation nothing is allocated.  The device list is rebuilt from the
// mirror at every change, so the two cannot drift.
#include "kws_ctx.h"

namespace kws {
namespace {

struct ActiveListArgs {
    ResetMask m;       // the chunk's active streams; stream = first + bit index
    int first, base;   // base: active streams of the chunks before this one (the host knows it)
    int n_streams;
    int32_t* list;     // [n_streams]
};

// One workgroup per chunk, thread r = stream first + r: an active stream writes its index at base + the active streams below it in
// the chunk.  tests/test_stream_active_cpu.py restates the rule.
__global__ __launch_bounds__(RESET_CHUNK) void kws_stream_active_list_kernel(const ActiveListArgs a) {
    const int r = threadIdx.x, s = a.first + r;
    if (s >= a.n_streams || !a.m.has(r)) return;
    int at = a.base + __popcll(a.m.w[r >> 6] & ((1ull << (r & 63)) - 1ull));
    for (int k = 0; k < (r >> 6); ++k) at += __popcll(a.m.w[k]);
    a.list[at] = s;  // at < n_active <= n_streams: the mirror's bits at or beyond n_streams are clear
}

// A push with no active stream: the set's clock runs on.  What the fused push's last workgroup does, alone.
__global__ void kws_stream_tick_kernel(int* hops, int* h_flag) {
    if (threadIdx.x != 0) return;
    const int h = hops[0] + 1;
    hops[0] = h;
    if (h_flag) __hip_atomic_store(h_flag, h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

int rebuild_list(kws_ctx* c) {
    ActiveListArgs a{};
    a.n_streams = c->n_streams;
    a.list = c->d_active_list.get();
    int base = 0;
    for (int first = 0; first < c->n_streams; first += RESET_CHUNK) {
        a.m = c->active_chunk(first);
        int n = 0;
        for (unsigned long long w : a.m.w) n += __builtin_popcountll(w);
        if (!n) continue;
        a.first = first;
        a.base = base;
        hipLaunchKernelGGL(kws_stream_active_list_kernel, dim3(1), dim3(RESET_CHUNK), 0, c->stream, a);
        HIP_TRY(c, hipGetLastError());
        base += n;
    }
    return KWS_OK;
}

// The two entries: checks, what the device does for the named streams, then the mirror and the list.
int set_active(kws_ctx* c, const char* fn, const int32_t* streams, int n, bool on) {
    bool nothing = false;
    if (int rc = stream_reset_check(c, fn, streams, n, &nothing)) return rc;
    if (nothing) return KWS_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!on && c->active_bits.empty()) {  // the set's first deactivation: mirror and list
        if (!c->d_active_list.alloc((size_t)c->n_streams)) return fail(c, KWS_ENOMEM, std::string(fn) + ": device allocation failed");
        c->active_bits.assign(((size_t)c->n_streams + 63) / 64, ~0ull);
        if (c->n_streams % 64) c->active_bits.back() = (1ull << (c->n_streams % 64)) - 1ull;
    }
    // activate: the whole of kws_stream_reset, on active and inactive streams alike.  deactivate: what is open in the live
    // utterances on a named ACTIVE stream closes with reason 2; the rings stay as they are until the stream joins again
    if (int rc = stream_reset_launch(c, streams, n, !on, !on)) return rc;
    if (c->active_bits.empty()) return KWS_OK;  // never deactivated: an activation is a plain reset
    int changed = 0;
    for (int i = 0; i < n; ++i) {
        if (c->is_active(streams[i]) == on) continue;
        c->active_bits[(size_t)streams[i] >> 6] ^= 1ull << (streams[i] & 63);
        changed += 1;
    }
    if (!changed) return KWS_OK;
    c->n_active += on ? changed : -changed;
    return rebuild_list(c);
}

}  // namespace

hipError_t launch_stream_tick(hipStream_t s, int* d_hops, int* h_flag) {
    hipLaunchKernelGGL(kws_stream_tick_kernel, dim3(1), dim3(64), 0, s, d_hops, h_flag);
    return hipGetLastError();
}

void stream_active_free(kws_ctx* c) {
    c->d_active_list.reset();
    c->active_bits.clear();
    c->n_active = 0;
}

}  // namespace kws

using namespace kws;

#pragma GCC visibility push(default)
extern "C" {

int kws_stream_deactivate(kws_ctx* c, const int32_t* streams, int n) {
    KWS_GUARD_BEGIN
    return set_active(c, "kws_stream_deactivate", streams, n, false);
    KWS_GUARD_END(c, "kws_stream_deactivate")
}

int kws_stream_activate(kws_ctx* c, const int32_t* streams, int n) {
    KWS_GUARD_BEGIN
    return set_active(c, "kws_stream_activate", streams, n, true);
    KWS_GUARD_END(c, "kws_stream_activate")
}

int kws_stream_active(kws_ctx* c, uint8_t* out, int* n_active) {
    if (!c) return KWS_EINVAL;
    if (!c->n_streams) return fail(c, KWS_ESTATE, "kws_stream_active: call kws_stream_open first");
    if (out)
        for (int s = 0; s < c->n_streams; ++s) out[s] = c->is_active(s) ? 1 : 0;
    if (n_active) *n_active = c->n_active;
    return KWS_OK;
}

}  // extern "C"
#pragma GCC visibility pop
