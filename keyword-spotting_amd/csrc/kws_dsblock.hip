// Standalone depthwise-separable block for an arbitrary [B, C_in, H, W] map -- the drop-in for
// DepthwiseSeparableConvBlock.forward (reference kws/libs/models.py:108-119) outside the fused DS-CNN:
//     depthwise Conv2d(C_in, C_in, k, stride, padding, groups=C_in) + bias          (:96-103, :117)
//     pointwise Conv2d(C_in, C_out, 1, stride 1, padding=padding) + bias, ReLU      (:104-106, :118-119)
// The pointwise padding surrounds its output with a ring of `padding` positions equal to relu(bias) -- reference
// behaviour (defect 8), reproduced on purpose.
//
// Not the hot path (the four blocks of the DS-CNN run fused and LDS-resident in kws_dscnn.hip); this is the general-shape
// operator, so it is two plain kernels through a context workspace:
//   kws_dsblock_depthwise_kernel   one thread per output element, taps in registers per channel
//   kws_dsblock_pointwise_kernel   64 positions x 64 output channels per workgroup, the depthwise tile staged through
//                                  LDS in slabs of 16 input channels, 4 x 4 outputs per thread, f32 FMA in channel
//                                  order; ring positions are written by the same kernel (relu(bias), no arithmetic)
// kws_dsblock_pointwise_pre_kernel and kws_conv1_any_pre_kernel are the pointwise and the conv1 kernel without the ReLU (the ring
// is then the bias): the pre-activations of the train-mode BatchNorm path (kws_dscnn_bn.hip).  Each pair shares one body, included
// as text (kws_dsblock_pointwise_body.h, kws_conv1_any_body.h).
#include <algorithm>

#include "kws_ctx.h"
#include "kws_dscnn_geom.h"
#include "kws_pack.h"
#include "kws_split_mfma.h"

namespace kws {
namespace {

__global__ __launch_bounds__(256) void kws_dsblock_depthwise_kernel(const float* __restrict__ x, int C, int H, int W,
                                                                    const float* __restrict__ w, const float* __restrict__ b,
                                                                    int k, int stride, int pad, int Ho, int Wo,
                                                                    float* __restrict__ y, long total) {
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int wo = (int)(idx % Wo);
        const int ho = (int)((idx / Wo) % Ho);
        const long bc = idx / ((long)Wo * Ho);  // b * C + c
        const int c = (int)(bc % C);
        const float* xp = x + bc * (long)H * W;
        const float* wp = w + (long)c * k * k;
        float acc = b[c];
        for (int kh = 0; kh < k; ++kh) {
            const int hi = ho * stride - pad + kh;
            if ((unsigned)hi >= (unsigned)H) continue;
            for (int kw = 0; kw < k; ++kw) {
                const int wi = wo * stride - pad + kw;
                if ((unsigned)wi < (unsigned)W) acc = fmaf(wp[kh * k + kw], xp[(long)hi * W + wi], acc);
            }
        }
        y[idx] = acc;
    }
}

constexpr int TP = 64, TC = 64, TK = 16;  // positions x output channels per workgroup, input channels per slab

__global__ __launch_bounds__(256) void kws_dsblock_pointwise_kernel(const float* __restrict__ dw, int C_in, int P /*Ho*Wo*/,
                                                                    const float* __restrict__ w, const float* __restrict__ bias,
                                                                    int C_out, int Ho, int Wo, int pad, float* __restrict__ out) {
    constexpr bool RELU_OUT = true;
#include "kws_dsblock_pointwise_body.h"
}
// no ReLU: conv + bias, the ring equal to the bias
__global__ __launch_bounds__(256) void kws_dsblock_pointwise_pre_kernel(const float* __restrict__ dw, int C_in, int P /*Ho*Wo*/,
                                                                    const float* __restrict__ w, const float* __restrict__ bias,
                                                                    int C_out, int Ho, int Wo, int pad, float* __restrict__ out) {
    constexpr bool RELU_OUT = false;
#include "kws_dsblock_pointwise_body.h"
}

// ------------------------------------------------------------------------------------------------
// The rest of DepthwiseSeparableConv.forward for feature maps other than 99 x 10 (reference kws/libs/models.py:160-183 takes
// any [B, C, T, F]: AudioConfig.clip_duration_ms / num_cepstral_coeffs change T and F, audio_processor.py:37-46).  The
// fused LDS-resident kernel is built for the reference geometry; any other map runs composed and HBM-resident:
// conv1 (below) -> 4 x launch_dsblock -> pool + fc (below).
//
// conv1: Conv2d(C_in, 64, 10, stride 2, padding 2) + bias + ReLU (models.py:135,170).  One workgroup per (clip, tile of 64
// output positions); thread (co = tid & 63, pg = tid >> 6) owns output channel co at positions pg, pg + 4, ... of the tile.
// Per input channel the zero-padded plane goes through LDS (every lane of a wavefront reads the same address: a
// broadcast) and the 100 taps come from the [ci][tap][co] weight image (coalesced).
constexpr int C1A_POS = 64, C1A_PER = C1A_POS / 4;
__global__ __launch_bounds__(256) void kws_conv1_any_kernel(const float* __restrict__ x, int C_in, int T, int F, const float* __restrict__ wt,
                                                            const float* __restrict__ bias, int Ho, int Wo, float* __restrict__ out) {
    constexpr bool RELU_OUT = true;
#include "kws_conv1_any_body.h"
}
// no ReLU: conv1 + bias
__global__ __launch_bounds__(256) void kws_conv1_any_pre_kernel(const float* __restrict__ x, int C_in, int T, int F, const float* __restrict__ wt,
                                                            const float* __restrict__ bias, int Ho, int Wo, float* __restrict__ out) {
    constexpr bool RELU_OUT = false;
#include "kws_conv1_any_body.h"
}

// conv1 for input_channels > 1 on the 99 x 10 map, in front of the fused kernel's PRECONV entry (kws_dscnn.hip; reference
// kws/libs/models.py:125,135: Conv2d(input_channels, 64, 10, stride 2, padding 2)):
// one 512-thread workgroup per clip; thread (co = tid & 63, group g = tid >> 6) owns output channel co at positions
// g, g + 8, ...; per input channel the zero-padded plane goes through LDS (every lane of a wavefront reads the same
// address: a broadcast) and the 100 taps come from a [ci][tap][co] weight image (coalesced).  ReLU(bias + sum) -> [64][141].
__global__ __launch_bounds__(NT) void kws_conv1_general_kernel(const float* __restrict__ x, int C_in, const float* __restrict__ wt,
                                                               const float* __restrict__ bias, float* __restrict__ out) {
    __shared__ float plane[FEAT_H * FEAT_W];
    const int tid = threadIdx.x, co = tid & 63, g = tid >> 6;
    constexpr int PER = (P0 + NW - 1) / NW;  // positions per thread
    float acc[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) acc[k] = 0.f;
    const float* xc = x + (size_t)blockIdx.x * C_in * (IN_T * IN_F);
    for (int ci = 0; ci < C_in; ++ci) {
        __syncthreads();
        for (int i = tid; i < FEAT_H * FEAT_W; i += NT) {
            const int r = i / FEAT_W - 2, cidx = i % FEAT_W - 2;
            plane[i] = ((unsigned)r < (unsigned)IN_T && (unsigned)cidx < (unsigned)IN_F) ? xc[(size_t)ci * (IN_T * IN_F) + r * IN_F + cidx] : 0.f;
        }
        __syncthreads();
        const float* wc = wt + (size_t)ci * (C1_K * C1_K) * CH + co;
        for (int tap = 0; tap < C1_K * C1_K; ++tap) {
            const float wv_ = wc[(size_t)tap * CH];
            const int kh = tap / C1_K, kw = tap % C1_K;
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int pos = g + NW * k;
                if (pos < P0) acc[k] = fmaf(wv_, plane[(2 * (pos / C1_W) + kh) * FEAT_W + 2 * (pos % C1_W) + kw], acc[k]);
            }
        }
    }
    float* o = out + (size_t)blockIdx.x * (CH * P0) + (size_t)co * P0;
    const float bv = bias[co];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int pos = g + NW * k;
        if (pos < P0) o[pos] = relu(acc[k] + bv);
    }
}

// F.adaptive_avg_pool2d(x, (1, 1)) + view + fc (models.py:179-181) + argmax, first maximum wins (training.py:371).
// x: [B][64][HW] (the last block's output, ring included).  One workgroup per clip: four partial sums per channel, fc and
// argmax on wavefront 0.
__global__ __launch_bounds__(256) void kws_pool_fc_kernel(const float* __restrict__ x, int HW, const float* __restrict__ fc_w,
                                                          const float* __restrict__ fc_b, int C, float* __restrict__ logits,
                                                          int32_t* __restrict__ label) {
    __shared__ float part[4][64];
    __shared__ float pooled[64];
    __shared__ float lg[MAX_CLASSES];
    const int tid = threadIdx.x, c = tid & 63, q = tid >> 6;
    const float* xp = x + ((size_t)blockIdx.x * 64 + c) * HW;
    float s = 0.f;
    for (int i = q; i < HW; i += 4) s += xp[i];
    part[q][c] = s;
    __syncthreads();
    if (tid < 64) pooled[tid] = ((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid])) * (1.0f / (float)HW);
    __syncthreads();
    if (tid < C) {
        float acc = fc_b[tid];
        for (int k = 0; k < 64; ++k) acc = fmaf(fc_w[tid * 64 + k], pooled[k], acc);
        logits[(size_t)blockIdx.x * C + tid] = acc;
        lg[tid] = acc;
    }
    __syncthreads();
    if (tid == 0 && label) {
        int best = 0;
        for (int k = 1; k < C; ++k)
            if (lg[k] > lg[best]) best = k;  // strict: the first maximum wins
        label[blockIdx.x] = best;
    }
}

}  // namespace

hipError_t launch_conv1_any(hipStream_t s, const float* d_x, int B, int C_in, int T, int F, const float* d_wt, const float* d_bias,
                            float* d_out, bool relu_out) {
    const int Ho = (T + 4 - 10) / 2 + 1, Wo = (F + 4 - 10) / 2 + 1;
    const size_t lds = sizeof(float) * (size_t)(T + 4) * (F + 4);
    const auto kernel = relu_out ? kws_conv1_any_kernel : kws_conv1_any_pre_kernel;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3((Ho * Wo + C1A_POS - 1) / C1A_POS, B), dim3(256), lds, s, d_x, C_in, T, F, d_wt, d_bias, Ho, Wo, d_out);
    return hipGetLastError();
}

hipError_t launch_conv1_general(hipStream_t s, const float* d_x, int B, int C_in, const float* d_wt, const float* d_bias, float* d_out) {
    hipLaunchKernelGGL(kws_conv1_general_kernel, dim3(B), dim3(NT), 0, s, d_x, C_in, d_wt, d_bias, d_out);
    return hipGetLastError();
}

hipError_t launch_pool_fc(hipStream_t s, const float* d_x, int B, int HW, const float* d_fc_w, const float* d_fc_b, int C,
                          float* d_logits, int32_t* d_label) {
    hipLaunchKernelGGL(kws_pool_fc_kernel, dim3(B), dim3(256), 0, s, d_x, HW, d_fc_w, d_fc_b, C, d_logits, d_label);
    return hipGetLastError();
}

hipError_t launch_dsblock_depthwise(hipStream_t s, const float* d_x, int B, int C_in, int H, int W, const float* d_dw_w,
                                    const float* d_dw_b, int k, int stride, int pad, float* d_out) {
    const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    const long total = (long)B * C_in * Ho * Wo;
    const int blocks = (int)std::min<long>((total + 255) / 256, 1 << 20);
    hipLaunchKernelGGL(kws_dsblock_depthwise_kernel, dim3(blocks), dim3(256), 0, s, d_x, C_in, H, W, d_dw_w, d_dw_b, k, stride, pad,
                       Ho, Wo, d_out, total);
    return hipGetLastError();
}

hipError_t launch_dsblock_pointwise(hipStream_t s, const float* d_dw, int B, int C_in, int Ho, int Wo, const float* d_pw_w,
                                    const float* d_pw_b, int C_out, int pad, float* d_out, bool relu_out) {
    const int P = Ho * Wo;
    hipLaunchKernelGGL(relu_out ? kws_dsblock_pointwise_kernel : kws_dsblock_pointwise_pre_kernel,
                       dim3((P + TP - 1) / TP, (C_out + TC - 1) / TC, B), dim3(256), 0, s, d_dw, C_in, P, d_pw_w, d_pw_b, C_out, Ho, Wo, pad,
                       d_out);
    return hipGetLastError();
}

hipError_t launch_dsblock(hipStream_t s, const float* d_x, int B, int C_in, int H, int W, const float* d_dw_w, const float* d_dw_b,
                          const float* d_pw_w, const float* d_pw_b, int C_out, int k, int stride, int pad, float* d_ws,
                          float* d_out) {
    const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    hipError_t e = launch_dsblock_depthwise(s, d_x, B, C_in, H, W, d_dw_w, d_dw_b, k, stride, pad, d_ws);
    if (e != hipSuccess) return e;
    return launch_dsblock_pointwise(s, d_ws, B, C_in, Ho, Wo, d_pw_w, d_pw_b, C_out, pad, d_out, true);
}

int check_dscnn_map(kws_ctx* c, const char* fn, int T, int F) {
    if (T < 6 || F < 6) return fail(c, KWS_EINVAL, std::string(fn) + ": the 10 x 10 first convolution (padding 2) needs T >= 6 and F >= 6");
    if ((size_t)(T + 4) * (F + 4) * sizeof(float) > 160 * 1024)
        return fail(c, KWS_EUNSUPPORTED, std::string(fn) + ": the padded feature map must fit 160 KB of LDS ((T + 4) * (F + 4) <= 40960)");
    return KWS_OK;
}

hipError_t launch_dscnn_composed(hipStream_t s, const DscnnWeights& w, const float* d_feat, int nb, int T, int F, const DscnnStages& st) {
    const DscnnMap m(T, F);
    const DscnnLayout L(w.num_classes, w.in_channels);
    hipError_t e = launch_conv1_any(s, d_feat, nb, w.in_channels, T, F, w.c1_general, w.c1_b, st.a0);
    for (int k = 0; k < N_BLOCKS && e == hipSuccess; ++k) {
        const float* prm = w.raw + L.block(k);  // the block's parameters in state_dict order
        e = launch_dsblock(s, k ? st.y[k - 1] : st.a0, nb, CH, m.H(k), m.W(k), prm, prm + L.B_DWB, prm + L.B_PWW, prm + L.B_PWB, CH, 3, 1,
                           1, st.dw[k], st.y[k]);
    }
    return e;
}

}  // namespace kws
