// Training-time augmentation as kernels of its own: the transform of a batch (kws_augment_i16) and its random draws
// (kws_augment_draw).  The fused loader kernel, which augments on the way into the MFCC, is in kws_mfcc.hip; the per-sample
// function the two share is in kws_augment_dev.h.
#include "kws_augment_dev.h"
#include "kws_internal.h"

namespace kws {
namespace {

// Augmentation of the reference's training transform (kws/libs/audio_processor.py:151-159, 172-233) for a whole
// batch: out[b][i] = (silence_b ? 0 : x_b[i - shift_b] / 32768, zero outside the clip) + vol_b * bg[off_b + i],
// float32 with the same two roundings NumPy makes.
__global__ void kws_augment_i16_kernel(const int16_t* __restrict__ wav, int B, int n, const int32_t* __restrict__ shift,
                                       const float* __restrict__ bg, int bg_len, const int32_t* __restrict__ bg_off,
                                       const float* __restrict__ bg_vol, const uint8_t* __restrict__ silence,
                                       float* __restrict__ out) {
    const int b = blockIdx.y;
    const int sh = shift ? shift[b] : 0;
    const bool sil = silence && silence[b];
    const float vol = (bg && bg_vol) ? bg_vol[b] : 0.f;
    const int off = (bg && bg_off) ? bg_off[b] : 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int j = i - sh;
        float a = (!sil && j >= 0 && j < n) ? pcm_unit(wav[(size_t)b * n + j]) : 0.f;
        if (bg) {
            const int k = off + i;
            const float g = (k >= 0 && k < bg_len) ? bg[k] : 0.f;
            a = __fadd_rn(a, __fmul_rn(g, vol));
        }
        out[(size_t)b * n + i] = a;
    }
}

// The four random draws of the training transform (kws/libs/audio_processor.py:172-233) for a batch of dataset indices, made
// on the device.  Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), key = the 64-bit seed,
// counter = (dataset index, epoch, 0, 0): one call yields the four words of a clip, so a clip's draws are a pure function of
// (seed, epoch, dataset index) -- whatever the batch size, the other clips of the batch or the order inside it.
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0, c[1] = lo1, c[2] = n2, c[3] = lo0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
}
// word -> integer in [0, m): (u * m) >> 32; word -> float in [0, 1): (u >> 8) * 2^-24, exact in float32
__device__ __forceinline__ int draw_below(uint32_t u, int m) { return (int)(((unsigned long long)u * (unsigned)m) >> 32); }
__device__ __forceinline__ float draw_unit(uint32_t u) { return (float)(u >> 8) * (1.0f / 16777216.0f); }

__global__ void kws_augment_draw_kernel(DrawArgs d, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int idx = d.index[b];
    uint32_t w[4] = {(uint32_t)idx, d.epoch, 0u, 0u};
    philox4x32_10(w, (uint32_t)d.seed, (uint32_t)(d.seed >> 32));
    const bool in_split = (unsigned)idx < (unsigned)d.n_rows;  // a label outside the split is never read
    const bool sil = d.label && in_split && d.label[idx] == KWS_SILENCE_INDEX;
    // time shift: uniform on the integers [-S, S) (np.random.randint(-S, S), :174)
    d.shift[b] = d.time_shift > 0 ? draw_below(w[0], 2 * d.time_shift) - d.time_shift : 0;
    int off = 0;
    float vol = 0.f;
    if (d.n_files > 0 && (d.use_background || sil)) {  // (:158: without use_background_noise only silence clips get noise)
        const int k = draw_below(w[1], d.n_files);       // random.choice(background_data), :205
        const int room = d.bg_len[k] - d.n_samples;      // np.random.randint(0, len - n), :214 (the pool's files are tiled beyond n)
        off = d.bg_start[k] + (room > 0 ? draw_below(w[2], room) : 0);
        // the reference draws a Bernoulli(background_frequency) variable and then the volume (:218-223); the one word left serves
        // both: u < frequency decides, and given that, u / frequency is again uniform on [0, 1)
        const float u = draw_unit(w[3]);
        if (sil)
            vol = u;
        else if (u < d.bg_frequency)
            vol = __fmul_rn(__fdiv_rn(u, d.bg_frequency), d.bg_volume);
    }
    d.bg_off[b] = off;
    d.bg_vol[b] = vol;
    d.silence[b] = sil ? 1 : 0;
}

}  // namespace

hipError_t launch_augment(hipStream_t s, const int16_t* d_wav, int B, int n, const int32_t* d_shift, const float* d_bg,
                          int bg_len, const int32_t* d_bg_off, const float* d_bg_vol, const uint8_t* d_silence,
                          float* d_out) {
    int bx = (n + 255) / 256;
    if (bx > 64) bx = 64;
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const int nb = (B - b0 < 65535) ? (B - b0) : 65535;
        hipLaunchKernelGGL(kws_augment_i16_kernel, dim3(bx, nb), dim3(256), 0, s, d_wav + (size_t)b0 * n, nb, n,
                           d_shift ? d_shift + b0 : nullptr, d_bg, bg_len, d_bg_off ? d_bg_off + b0 : nullptr,
                           d_bg_vol ? d_bg_vol + b0 : nullptr, d_silence ? d_silence + b0 : nullptr, d_out + (size_t)b0 * n);
    }
    return hipGetLastError();
}

hipError_t launch_augment_draw(hipStream_t s, const DrawArgs& d, int B) {
    hipLaunchKernelGGL(kws_augment_draw_kernel, dim3((B + 255) / 256), dim3(256), 0, s, d, B);
    return hipGetLastError();
}

}  // namespace kws
