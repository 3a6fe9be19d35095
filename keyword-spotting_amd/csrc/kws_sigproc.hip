// sigproc operators (kws/libs/speech_features/sigproc.py) as device kernels: preemphasis, framesig, and magspec / powspec for
// any NFFT in float64 (the transform of kws_mfcc_f64_dev.h).  NFFT = 512 has a float32 kernel built from the MFCC kernels'
// transform, kws_spec512_f32_kernel: it stays in their unit, kws_mfcc.hip -- compiled apart from the wavefront-resident kernels
// its instructions come out in another order.
// Entries: kws_preemphasis_f32, kws_framesig_f32, kws_spec_f32 (kws_frontend.hip).
#include "kws_internal.h"
#include "kws_mfcc_f64_dev.h"

namespace kws {
namespace {

__global__ void kws_preemphasis_f32_kernel(const float* __restrict__ in, int n, float coeff, float* __restrict__ out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        out[i] = (i > 0) ? __fsub_rn(in[i], __fmul_rn(coeff, in[i - 1])) : in[i];
}

__global__ void kws_framesig_f32_kernel(const float* __restrict__ in, int n, int frame_len, int frame_step,
                                        int num_frames, const float* __restrict__ window,
                                        float* __restrict__ frames) {
    const long total = (long)num_frames * frame_len;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int f = (int)(idx / frame_len), i = (int)(idx % frame_len);
        const long s = (long)f * frame_step + i;
        float v = (s < n) ? in[s] : 0.f;
        if (window) v *= window[i];
        frames[idx] = v;
    }
}

// magspec / powspec for any NFFT (kws/libs/speech_features/sigproc.py:55-90): frames float32 [num_frames][frame_len]
// (zero-padded to nfft, or truncated), one wavefront per pair of frames, float64 inside, float32 out.
template <bool POW2>
__global__ __launch_bounds__(64) void kws_spec_f64_kernel(const float* __restrict__ frames, int num_frames, int frame_len, int nfft,
                                                         int log2n, int power, const d2* __restrict__ tw, float* __restrict__ spec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem64[];
    const int nb = nfft / 2 + 1;
    d2* X = reinterpret_cast<d2*>(smem64);
    d2* P = X + nfft;
    d2* tw_lds = P + nb;
    const int lane = threadIdx.x;
    const int fa = 2 * blockIdx.x;
    const bool has_b = fa + 1 < num_frames;
    const int n_used = frame_len < nfft ? frame_len : nfft;
    bool nza = false, nzb = false;
    for (int n = lane; n < nfft; n += 64) {
        double a = 0.0, b = 0.0;
        if (n < n_used) {
            a = (double)frames[(size_t)fa * frame_len + n];
            if (has_b) b = (double)frames[(size_t)(fa + 1) * frame_len + n];
        }
        nza |= a != 0.0;
        nzb |= b != 0.0;
        X[n] = d2{a, b};
    }
    nza = __any(nza);
    nzb = __any(nzb);
    for (int i = lane; i < (POW2 ? nfft / 2 : nfft); i += 64) tw_lds[i] = tw[i];
    wave_order();
    spectrum_pair<POW2, 0>(X, P, tw_lds, nfft, log2n, n_used, power ? 1.0 / (double)nfft : 1.0, lane);
    for (int k = lane; k < nb; k += 64) {
        d2 pw = P[k];
        if (!nza) pw.x = 0.0;  // an all-zero frame has an exactly zero spectrum, whatever shares its transform
        if (!nzb) pw.y = 0.0;
        spec[(size_t)fa * nb + k] = (float)(power ? pw.x : sqrt(pw.x));
        if (has_b) spec[(size_t)(fa + 1) * nb + k] = (float)(power ? pw.y : sqrt(pw.y));
    }
}

size_t spec_lds_bytes(int nfft, bool pow2) {
    const size_t nb = nfft / 2 + 1;
    return sizeof(d2) * ((size_t)nfft + nb + (pow2 ? (size_t)nfft / 2 : (size_t)nfft));
}

}  // namespace

hipError_t launch_preemphasis(hipStream_t s, const float* d_in, int n, float coeff, float* d_out) {
    const int blocks = (n + 255) / 256;
    hipLaunchKernelGGL(kws_preemphasis_f32_kernel, dim3(blocks < 2048 ? blocks : 2048), dim3(256), 0, s, d_in, n, coeff, d_out);
    return hipGetLastError();
}

hipError_t launch_framesig(hipStream_t s, const float* d_in, int n, int frame_len, int frame_step, int num_frames,
                           const float* d_window, float* d_frames) {
    const long total = (long)num_frames * frame_len;
    long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(kws_framesig_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, s, d_in, n, frame_len, frame_step,
                       num_frames, d_window, d_frames);
    return hipGetLastError();
}

hipError_t launch_spec_f64(hipStream_t s, const double* d_tw64, const float* d_frames, int num_frames, int frame_len, int nfft,
                           int log2n, int power, float* d_spec) {
    const bool pow2 = log2n > 0;
    const size_t lds = spec_lds_bytes(nfft, pow2);
    auto kernel = pow2 ? kws_spec_f64_kernel<true> : kws_spec_f64_kernel<false>;
    hipError_t e = raise_lds_limit(kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3((num_frames + 1) / 2), dim3(64), lds, s, d_frames, num_frames, frame_len, nfft, log2n, power,
                       reinterpret_cast<const d2*>(d_tw64), d_spec);
    return hipGetLastError();
}

}  // namespace kws
