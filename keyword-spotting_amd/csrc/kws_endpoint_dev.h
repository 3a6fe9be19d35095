// The energy endpointer's one statement on the device (the reference's live loop, kws/inference/inference_local.py:131-166):
// what a voiced frame is, when an utterance opens and closes, the flag ring with O(1) window counts, where a span starts, and
// normalize + fix_length of a span into a clip.  No kernels here: kws_stream_vad_kernel (kws_decide.hip), the flag and walk
// kernels (kws_segment.hip), the live step (kws_live.hip) and the cut kernels are the callers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kws {

constexpr int EP_MAX_WINDOW = 1024;                // off_window's limit: the flag ring holds this many frames
constexpr int EP_BIT_WORDS = EP_MAX_WINDOW / 64;   // 64-bit words of one stream's flag ring

// float32, strict; a NaN compares false: unvoiced
__host__ __device__ __forceinline__ bool ep_voiced(float energy, float threshold) { return energy > threshold; }
// more than 80 % of the last on_window frames are voiced (:151)
__host__ __device__ __forceinline__ bool ep_opens(int c_on, int on_window) { return 10 * c_on > 8 * on_window; }
// more than 90 % of the last off_window frames are unvoiced (:161)
__host__ __device__ __forceinline__ bool ep_closes(int c_off, int off_window) { return 10 * (off_window - c_off) > 9 * off_window; }

// Frame f of one stream arrives with voiced flag v (0 / 1): bits_row[EP_BIT_WORDS] keeps the flag of frame g at bit g mod 1024,
// counts_row[0..1] the two window counts; frames before 0 are unvoiced.  O(1): each count gains v and loses the flag that
// leaves its window.  The leaving flags are read BEFORE the new one is stored: with a window of 1024 they share its slot.
struct EpCounts { int on, off; };  // returned: voiced frames among the last on_window / off_window, frame f included
__host__ __device__ __forceinline__ EpCounts ep_ring_push(unsigned long long* bits_row, int* counts_row, long long f, int v,
                                                          int on_window, int off_window) {
    auto flag_at = [&](long long g) -> int { return g < 0 ? 0 : (int)((bits_row[(g & (EP_MAX_WINDOW - 1)) >> 6] >> (g & 63)) & 1ull); };
    const int c_on = counts_row[0] + v - flag_at(f - on_window);
    const int c_off = counts_row[1] + v - flag_at(f - off_window);
    const int slot = (int)(f & (EP_MAX_WINDOW - 1));
    bits_row[slot >> 6] = (bits_row[slot >> 6] & ~(1ull << (slot & 63))) | ((unsigned long long)v << (slot & 63));
    counts_row[0] = c_on;
    counts_row[1] = c_off;
    return {c_on, c_off};
}

// First frame of the utterance that opened at `open`: pre_roll frames early, but not before the frame after the previous close
// (prev_close = -1 when there was none, so prev_close + 1 >= 0).  T: the caller's frame index type (int or long long).
template <typename T>
__host__ __device__ __forceinline__ long long ep_span_start(T open, int pre_roll, T prev_close) {
    long long start = (long long)open - pre_roll;
    if (start < prev_close + 1) start = prev_close + 1;
    return start;
}

// normalize (:102-109) then fix_length (:70) of one span by one workgroup of Threads: the peak over the WHOLE span of `len`
// samples (the reference normalises before it trims), then n_out samples, scaled in float64 and truncated towards zero as
// int(i * times), zero beyond the span.  at(i): sample i of the span as int; ok, len: workgroup-uniform; peak_out[u] = the
// peak, -1 for a refused span (!ok, len 0: a zero clip).
template <int Threads, typename At>
__device__ __forceinline__ void ep_cut_clip(At at, int len, bool ok, int normalize_to, int16_t* out, int n_out,
                                            int32_t* peak_out, int u) {
    __shared__ int wave_peak[Threads / 64];
    const int tid = threadIdx.x;
    int peak = 0;
    for (unsigned i = tid; i < (unsigned)len; i += Threads) {
        const int v = at(i);
        const int m = v < 0 ? -v : v;  // |-32768| = 32768
        peak = m > peak ? m : peak;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const int other = __shfl_xor(peak, d);
        peak = other > peak ? other : peak;
    }
    if ((tid & 63) == 0) wave_peak[tid >> 6] = peak;
    __syncthreads();
    peak = wave_peak[0];
    for (int k = 1; k < Threads / 64; ++k) peak = wave_peak[k] > peak ? wave_peak[k] : peak;
    if (tid == 0 && peak_out) peak_out[u] = ok ? peak : -1;
    const int body = len < n_out ? len : n_out;
    if (normalize_to > 0) {
        const double times = peak > 0 ? (double)normalize_to / (double)peak : 0.0;  // peak 0: the span is all zeros anyway
        for (unsigned i = tid; i < (unsigned)n_out; i += Threads) out[i] = i < (unsigned)body ? (int16_t)(int)((double)at(i) * times) : (int16_t)0;
    } else {
        for (unsigned i = tid; i < (unsigned)n_out; i += Threads) out[i] = i < (unsigned)body ? (int16_t)at(i) : (int16_t)0;
    }
}

// The same for float32 samples (kws_cut_f32): peak = the largest |x| of the whole span in float32, compared with m > peak, so a NaN
// never raises it; normalize_to > 0 and peak > 0: out[i] = (float)((double)x[i] * ((double)normalize_to / (double)peak)) -- a
// float64 divide and multiply, one rounding to float32, no truncation; peak == 0: zeros; normalize_to == 0: the samples' own bits.
// at(i): sample i of the span as float; peak_out[u] = the peak, -1 for a refused span.
template <int Threads, typename At>
__device__ __forceinline__ void ep_cut_clip_f32(At at, int len, bool ok, float normalize_to, float* out, int n_out, float* peak_out,
                                                int u) {
    __shared__ float wave_peak[Threads / 64];
    const int tid = threadIdx.x;
    float peak = 0.f;
    for (unsigned i = tid; i < (unsigned)len; i += Threads) {
        const float m = fabsf(at(i));
        peak = m > peak ? m : peak;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const float other = __shfl_xor(peak, d);
        peak = other > peak ? other : peak;
    }
    if ((tid & 63) == 0) wave_peak[tid >> 6] = peak;
    __syncthreads();
    peak = wave_peak[0];
    for (int k = 1; k < Threads / 64; ++k) peak = wave_peak[k] > peak ? wave_peak[k] : peak;
    if (tid == 0 && peak_out) peak_out[u] = ok ? peak : -1.f;
    const int body = len < n_out ? len : n_out;
    if (normalize_to > 0.f) {
        const bool scale = peak > 0.f;
        const double times = scale ? (double)normalize_to / (double)peak : 0.0;
        for (unsigned i = tid; i < (unsigned)n_out; i += Threads) out[i] = scale && i < (unsigned)body ? (float)((double)at(i) * times) : 0.f;
    } else {
        for (unsigned i = tid; i < (unsigned)n_out; i += Threads) out[i] = i < (unsigned)body ? at(i) : 0.f;
    }
}

}  // namespace kws
