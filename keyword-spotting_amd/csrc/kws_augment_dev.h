// Device side of the resident training loader for gfx950: the per-clip view of kws_mfcc_augment_i16's arguments and the ONE
// per-sample function (gather, time shift, silence, background mix) that the fused float32 kernel (kws_mfcc.hip) and the
// refinement instantiation (kws_mfcc_f64.hip) share, so that both see the same augmented float32 samples -- the ones
// kws_augment_i16 writes to memory on the composed route (reference kws/libs/audio_processor.py:151-159, 172-233).
// Anonymous namespace: each translation unit gets its own inlined copy.
#pragma once
#include "kws_internal.h"

namespace kws {
namespace {

__device__ __forceinline__ float pcm_unit(int16_t s) { return (float)s * (1.0f / 32768.0f); }

// One clip of the batch.  Every member is wave-uniform when the batch row is (readfirstlane: scalar registers).
struct AugClip {
    const int16_t* x;    // the clip's own row of the resident split: nothing outside [x, x + n_samples) is read
    const float* bg;     // background pool, or nullptr: no mix
    int bg_len;
    int shift, off;
    float vol;
    bool silence;
};

__device__ __forceinline__ int uniform_i(int v) { return __builtin_amdgcn_readfirstlane(v); }

// b: batch row (the same for every lane of the wavefront).  A dataset index outside [0, n_rows) is never dereferenced: the
// row is clamped to 0 and that batch row's output is unspecified.
__device__ __forceinline__ AugClip aug_clip(const AugmentArgs& a, int b, int n_samples) {
    b = uniform_i(b);
    int row = uniform_i(a.index[b]);
    row = (unsigned)row < (unsigned)a.n_rows ? row : 0;
    AugClip c;
    c.x = a.pcm + (size_t)row * n_samples;
    c.bg = a.bg;
    c.bg_len = a.bg_len;
    c.shift = a.shift ? uniform_i(a.shift[b]) : 0;
    c.silence = a.silence && uniform_i(a.silence[b]) != 0;
    c.off = (a.bg && a.bg_off) ? uniform_i(a.bg_off[b]) : 0;
    c.vol = (a.bg && a.bg_vol) ? __builtin_bit_cast(float, uniform_i(__builtin_bit_cast(int, a.bg_vol[b]))) : 0.f;
    return c;
}

// Augmented sample i of the clip, 0 <= i < n: the arithmetic of kws_augment_i16_kernel, rounding for rounding.
__device__ __forceinline__ float aug_sample(const AugClip& c, int i, int n) {
    const int j = i - c.shift;
    float a = (!c.silence && j >= 0 && j < n) ? pcm_unit(c.x[j]) : 0.f;
    if (c.bg) {
        const int k = c.off + i;
        const float g = (k >= 0 && k < c.bg_len) ? c.bg[k] : 0.f;
        a = __fadd_rn(a, __fmul_rn(g, c.vol));
    }
    return a;
}

// sample m of the augmented clip after pre-emphasis (float32, two roundings, as NumPy does it), 0 outside the clip
__device__ __forceinline__ float preemph_sample(const AugClip& x, long m, int n_samples, float c) {
    if (m < 0 || m >= n_samples) return 0.f;
    const float cur = aug_sample(x, (int)m, n_samples);
    return m > 0 ? __fsub_rn(cur, __fmul_rn(c, aug_sample(x, (int)m - 1, n_samples))) : cur;
}

}  // namespace
}  // namespace kws
