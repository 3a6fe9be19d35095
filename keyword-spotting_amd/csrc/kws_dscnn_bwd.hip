// Training: the backward pass of DepthwiseSeparableConv.forward (reference kws/libs/models.py:160-183) -- the gradient of a
// scalar loss with respect to all 20 state_dict tensors, given dloss/dlogits (kws_dscnn_backward_f32, include/kws_hip.h).
// It replaces loss.backward() of the reference trainer (train.py:48, kws/libs/training.py:296) for this model.
//
// Recompute, not save: the forward activations are recomputed at the start of the call by the composed fp32 path
// (launch_conv1_any + 4 x launch_dsblock, exactly the kernels of kws_forward_map_f32), every stage kept in the context's
// training workspace.  The inference kernels stay untouched and a forward under autograd costs what it costs without it.
//
// Geometry per block k (0-based): input H x W (H = H1 + 2k, W = W1 + 2k), depthwise output H x W, pointwise output
// (H + 2) x (W + 2) whose ring is relu(b_pw).  At 99 x 10: H x W = 47x3, 49x5, 51x7, 53x9, and block 4's output is 55 x 11.
//
// Kernels (one launch each per stage, all fp32, stable names for rocprofv3 --kernel-trace):
//   kws_bwd_fc_kernel          global average pool + fc: dY4 = (W_fc^T dl) / (H4 W4) per (clip, channel), partials of
//                              g_fc_w = sum_b dl (x) pooled and g_fc_b = sum_b dl
//   kws_bwd_pointwise_kernel   dZ = dY [Y > 0]; g_pw_b = sum dZ over ALL positions (ring included); the two 64 x 64 GEMMs on
//                              the exact f32-input MFMA v_mfma_f32_32x32x2_f32: g_pw_w += dZ X_dw^T (K = positions,
//                              accumulated in registers over the workgroup's clips) and dX_dw = W_pw^T dZ (K = 64 output
//                              channels) on the interior positions
//   kws_bwd_depthwise_kernel   g_dw_b = sum dX_dw, g_dw_w[c][tap] = sum dX_dw * X_in(shifted), dX_in = correlation of dX_dw
//                              with the flipped 3x3 kernel over the whole input (= the gradient of the previous block's output,
//                              ring included)
//   kws_bwd_conv1_kernel       dZ1 = dA0 [A0 > 0]; g_c1_b = sum dZ1, g_c1_w as an implicit GEMM (M = 64, N = 100, K = B H1 W1)
//                              on the VALU; no input gradient
//   kws_bwd_reduce_kernel      fixed-order sum of the per-workgroup partials into d_grad
//   kws_bwd_pointwise_dz_kernel, kws_bwd_conv1_dz_kernel   the same two kernels fed with a finished dZ instead of dY and the mask
//                              Y > 0: what a BatchNorm between the convolution and its ReLU hands back (kws_dscnn_bn.hip, through
//                              the launch_bwd_* functions of kws_train.h).  Each pair shares one body, included as text
//                              (kws_bwd_pointwise_body.h, kws_bwd_conv1_body.h).
//
// Deterministic: no float atomics, but the clip groups of kws_train.h with at most 1024 groups per chunk (chunks after the first
// add onto d_grad in chunk order).  G, cpg and the chunking depend on B and the map only, so the same inputs and B give
// bit-identical gradients on every call.
//
// input_channels > 1 returns KWS_EUNSUPPORTED: conv1's weight gradient is written for one input channel (N = 100 taps).
//
// Memory is written with plain vector stores only; there is no inline assembly in this unit.
#include "kws_train.h"

namespace kws {
namespace {

using DL = DscnnLayout;
constexpr int PW_TP = 64;                     // interior positions per tile of the pointwise backward

// ---- global average pool + fc ---------------------------------------------------------------------------------------------
// One workgroup per clip group.  Per clip: pooled = mean of the block-4 output over its Q4 positions (ring included),
// dpool = W_fc^T dl, dY4[b][c] = dpool[c] / Q4 (the same value at every position); partial sums of dl (x) pooled and dl.
__global__ __launch_bounds__(256) void kws_bwd_fc_kernel(const float* __restrict__ y4, const float* __restrict__ dl,
                                                         const float* __restrict__ fc_w, int Q4, int C, int nb, int cpg,
                                                         float* __restrict__ dy4, float* __restrict__ part) {
    constexpr int PER = (fc_part(MAX_CLASSES) + 255) / 256;  // partial entries per thread
    __shared__ float s_sum[4][64];
    __shared__ float s_pool[64];
    __shared__ float s_dl[MAX_CLASSES];
    const int tid = threadIdx.x, c = tid & 63, q0 = tid >> 6, g = blockIdx.x;
    const int n_part = C * DL::CO + C;  // fc_part(C), spelled out: the call moves instructions in this kernel
    float acc[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) acc[k] = 0.f;
    const int b_end = group_end(g, cpg, nb);
    for (int b = g * cpg; b < b_end; ++b) {
        const float* yp = y4 + ((size_t)b * 64 + c) * Q4;
        float s = 0.f;
        for (int r0 = q0; r0 < Q4; r0 += 4 * RUN) {  // runs of RUN positions, each summed from zero
            const int r1 = min(Q4, r0 + 4 * RUN);
            float t = 0.f;
            for (int q = r0; q < r1; q += 4) t += yp[q];
            s += t;
        }
        s_sum[q0][c] = s;
        if (tid < C) s_dl[tid] = dl[(size_t)b * C + tid];
        __syncthreads();
        if (tid < 64) {
            s_pool[tid] = ((s_sum[0][tid] + s_sum[1][tid]) + (s_sum[2][tid] + s_sum[3][tid])) / (float)Q4;
            float dp = 0.f;
            for (int j = 0; j < C; ++j) dp = fmaf(fc_w[j * 64 + tid], s_dl[j], dp);
            dy4[(size_t)b * 64 + tid] = dp / (float)Q4;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int e = tid + 256 * k;
            if (e < C * 64) acc[k] = fmaf(s_dl[e >> 6], s_pool[e & 63], acc[k]);
            else if (e < n_part) acc[k] += s_dl[e - C * 64];
        }
        __syncthreads();
    }
    float* pg = part + (size_t)g * n_part;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int e = tid + 256 * k;
        if (e < n_part) pg[e] = acc[k];
    }
}

// ---- pointwise 1x1 (padding 1) + ReLU ------------------------------------------------------------------------------------
// One workgroup (4 waves) per clip group.  dY of the block output is read as dy[b * dy_clip + co * dy_plane + q * dy_qstep]
// (block 4: dy_qstep = 0, one value per (clip, channel)).  Per clip: the bias sum over all Q = (H+2)(W+2) positions, then
// tiles of 64 interior positions staged in LDS as dZ [64 co][64 p] and X_dw [64 ci][64 p]; wave w, with u = w >> 1, v = w & 1:
//   g_pw_w tile (co 32 u .., ci 32 v ..) += dZ X_dw^T    32 x v_mfma_f32_32x32x2_f32 per tile (K = 64 positions)
//   dX_dw tile (ci 32 v .., p 32 u ..) = W^T dZ           32 x v_mfma_f32_32x32x2_f32 per tile (K = 64 output channels)
// (the 16x16x4 form would need no more LDS traffic, but the ISA hazard lint calibrates the 32x32x2 wait states only)
__global__ __launch_bounds__(256) void kws_bwd_pointwise_kernel(const float* __restrict__ dy, long dy_clip, int dy_plane, int dy_qstep,
                                                                const float* __restrict__ y, const float* __restrict__ xdw,
                                                                const float* __restrict__ w, int H, int W, int nb, int cpg,
                                                                float* __restrict__ dxdw, float* __restrict__ part) {
    constexpr bool MASK = true;
#include "kws_bwd_pointwise_body.h"
}
// dy = the finished dZ [nb][64][Q] (dy_clip = 64 Q, dy_plane = Q, dy_qstep = 1); y is not read
__global__ __launch_bounds__(256) void kws_bwd_pointwise_dz_kernel(const float* __restrict__ dy, long dy_clip, int dy_plane, int dy_qstep,
                                                                const float* __restrict__ y, const float* __restrict__ xdw,
                                                                const float* __restrict__ w, int H, int W, int nb, int cpg,
                                                                float* __restrict__ dxdw, float* __restrict__ part) {
    constexpr bool MASK = false;
#include "kws_bwd_pointwise_body.h"
}

// ---- depthwise 3x3 (padding 1, groups 64) --------------------------------------------------------------------------------
// Grid (16 channel quads, G clip groups); wave w of workgroup (cq, g) owns channel 4 cq + w, its lanes walk the H x W
// positions.  Per position p = (h, x) of the depthwise output: g_w[kh][kw] += dX_dw[h][x] X_in[h + kh - 1][x + kw - 1];
// per input position i = (h, x): dX_in[h][x] = sum w[kh][kw] dX_dw[h - kh + 1][x - kw + 1] (inside the map).
__global__ __launch_bounds__(256) void kws_bwd_depthwise_kernel(const float* __restrict__ dxdw, const float* __restrict__ xin,
                                                                const float* __restrict__ w, int H, int W, int nb, int cpg,
                                                                float* __restrict__ dxin, float* __restrict__ part) {
    __shared__ float s_red[4][10][64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = 4 * blockIdx.x + wv, g = blockIdx.y;
    const int P = H * W;
    float wk[9], gk[10];
#pragma unroll
    for (int t = 0; t < 9; ++t) wk[t] = w[c * 9 + t];
#pragma unroll
    for (int t = 0; t < 10; ++t) gk[t] = 0.f;
    const int b_end = group_end(g, cpg, nb);
    for (int b = g * cpg; b < b_end; ++b) {
        const float* dp = dxdw + ((size_t)b * 64 + c) * P;
        const float* xp = xin + ((size_t)b * 64 + c) * P;
        float* op = dxin + ((size_t)b * 64 + c) * P;
        for (int p = lane; p < P; p += 64) {
            const int h = p / W, x = p % W;
            const float d = dp[p];
            gk[9] += d;
            float gi = 0.f;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int hi = h + kh - 1, xi = x + kw - 1;  // input tap of output p
                    if ((unsigned)hi < (unsigned)H && (unsigned)xi < (unsigned)W) gk[kh * 3 + kw] = fmaf(d, xp[hi * W + xi], gk[kh * 3 + kw]);
                    const int ho = h - kh + 1, xo = x - kw + 1;  // output that sees input p through tap (kh, kw)
                    if ((unsigned)ho < (unsigned)H && (unsigned)xo < (unsigned)W) gi = fmaf(wk[kh * 3 + kw], dp[ho * W + xo], gi);
                }
            }
            op[p] = gi;
        }
    }
#pragma unroll
    for (int t = 0; t < 10; ++t) s_red[wv][t][lane] = gk[t];
    __syncthreads();
    if (lane < 10) {
        float s = 0.f;
        for (int l = 0; l < 64; ++l) s += s_red[wv][lane][l];
        float* pg = part + (size_t)g * DW_PART;
        if (lane < 9) pg[c * 9 + lane] = s;
        else pg[DL::DW_W + c] = s;
    }
}

// ---- conv1 (10x10, stride 2, padding 2) + ReLU, one input channel --------------------------------------------------------
// One workgroup per clip group.  Thread (co = tid & 63, r0 = tid >> 6) owns output channel co and the kernel rows
// r0, r0 + 4, r0 + 8 (< 10): 30 accumulators.  Tiles of 64 output positions of dZ1 = dA0 [A0 > 0] go through LDS as
// [p][co]; the input taps are wave-uniform loads (every lane of a wave reads the same feature value).
constexpr int C1B_TP = 64;
__global__ __launch_bounds__(256) void kws_bwd_conv1_kernel(const float* __restrict__ da, const float* __restrict__ a,
                                                            const float* __restrict__ x, int T, int F, int H1, int W1, int nb,
                                                            int cpg, float* __restrict__ part) {
    constexpr bool MASK = true;
#include "kws_bwd_conv1_body.h"
}
// da = the finished dZ1; a is not read
__global__ __launch_bounds__(256) void kws_bwd_conv1_dz_kernel(const float* __restrict__ da, const float* __restrict__ a,
                                                            const float* __restrict__ x, int T, int F, int H1, int W1, int nb,
                                                            int cpg, float* __restrict__ part) {
    constexpr bool MASK = false;
#include "kws_bwd_conv1_body.h"
}

// out[i] (+)= sum over g = 0 .. G-1 of part[g][i], in the fixed order of reduce_partials (kws_train.h)
__global__ __launch_bounds__(256) void kws_bwd_reduce_kernel(const float* __restrict__ part, int G, int n, float* __restrict__ out,
                                                             int accumulate) {
    reduce_partials<false>(part, G, n, 0, out, accumulate);
}

hipError_t reduce(hipStream_t s, const float* part, int G, int n, float* out, bool accumulate) {
    hipLaunchKernelGGL(kws_bwd_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, s, part, G, n, out, accumulate ? 1 : 0);
    return hipGetLastError();
}

}  // namespace

// The launches the train-mode BatchNorm backward (kws_dscnn_bn.hip) shares with this unit; `part` holds G rows of the stage's
// partials, reduced in fixed order into `out` (bwd_reduce).
hipError_t bwd_reduce(hipStream_t s, const float* part, int G, int n, float* out) { return reduce(s, part, G, n, out, false); }
hipError_t launch_bwd_fc(hipStream_t s, const float* y4, const float* dl, const float* fc_w, int Q4, int C, int nb, int cpg, int G,
                         float* dy4, float* part) {
    hipLaunchKernelGGL(kws_bwd_fc_kernel, dim3(G), dim3(256), 0, s, y4, dl, fc_w, Q4, C, nb, cpg, dy4, part);
    return hipGetLastError();
}
hipError_t launch_bwd_pointwise_dz(hipStream_t s, const float* dz, const float* xdw, const float* w, int H, int W, int nb, int cpg, int G,
                                   float* dxdw, float* part) {
    const int Q = (H + 2) * (W + 2);
    hipLaunchKernelGGL(kws_bwd_pointwise_dz_kernel, dim3(G), dim3(256), 0, s, dz, (long)CH * Q, Q, 1, (const float*)nullptr, xdw, w, H, W, nb, cpg,
                       dxdw, part);
    return hipGetLastError();
}
hipError_t launch_bwd_depthwise(hipStream_t s, const float* dxdw, const float* xin, const float* w, int H, int W, int nb, int cpg, int G,
                                float* dxin, float* part) {
    hipLaunchKernelGGL(kws_bwd_depthwise_kernel, dim3(CH / 4, G), dim3(256), 0, s, dxdw, xin, w, H, W, nb, cpg, dxin, part);
    return hipGetLastError();
}
hipError_t launch_bwd_conv1_dz(hipStream_t s, const float* dz, const float* x, int T, int F, int H1, int W1, int nb, int cpg, int G,
                               float* part) {
    hipLaunchKernelGGL(kws_bwd_conv1_dz_kernel, dim3(G), dim3(256), 0, s, dz, (const float*)nullptr, x, T, F, H1, W1, nb, cpg, part);
    return hipGetLastError();
}

}  // namespace kws

using namespace kws;

#pragma GCC visibility push(default)
extern "C" {

int kws_dscnn_backward_f32(kws_ctx* c, const float* d_feat, int B, int T, int F, const float* d_dlogits, float* d_grad) {
    static const char* fn = "kws_dscnn_backward_f32";
    KWS_GUARD_BEGIN
    int rc = check_backward_args(c, d_feat, B, d_dlogits, d_grad, fn);
    if (rc) return rc;
    if (!c->model_ready) return fail(c, KWS_ESTATE, std::string(fn) + ": no model loaded (kws_load_dscnn)");
    if (c->mw.in_channels != 1)
        return fail(c, KWS_EUNSUPPORTED, std::string(fn) + ": the backward is implemented for input_channels == 1 only");
    rc = check_dscnn_map(c, fn, T, F);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const int C = c->mw.num_classes, LAST = N_BLOCKS - 1;
    const DscnnMap m(T, F);
    const DL L(C, 1);
    DscnnStages st;
    float *gin, *gdw, *dy4, *part;
    auto carve = [&](Carver& w) {
        st.a0 = w.per(CH * m.P(0));
        for (int k = 0; k < N_BLOCKS; ++k) {
            st.dw[k] = w.per(CH * m.P(k));
            st.y[k] = w.per(CH * m.Q(k));
        }
        gin = w.per(CH * m.P(LAST));  // dloss / d(block input) = dloss / d(previous block's output, or conv1's)
        gdw = w.per(CH * m.P(LAST));  // dloss / d(depthwise output)
        dy4 = w.per(CH);
        // partial rows: G = ceil(nb / ceil(nb / 1024)) <= min(nb, 1024), the widest row is conv1's
        part = w.flat(std::min<size_t>(w.clips, BWD_MAX_GROUPS) * C1_PART);
    };
    Carver per_clip(0);
    carve(per_clip);
    // clip chunks: at most as many clips as the composed forward takes and at most 2^31 floats of activations and gradients
    const size_t by_budget = std::max<size_t>(1, ((size_t)1 << 31) / per_clip.per_clip);
    const int chunk = (int)std::min<size_t>({(size_t)B, COMPOSED_MAX_CLIPS, by_budget});
    Carver need(chunk);
    carve(need);
    rc = grow_device_buffer(c, c->d_train_ws, need.floats(), fn, "workspace");
    if (rc) return rc;
    Carver ws(chunk, c->d_train_ws.get());
    carve(ws);
    const float* raw = c->mw.raw;
    hipStream_t s = c->stream;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = std::min(chunk, B - b0);
        const auto [cpg, G] = clip_groups(nb, BWD_MAX_GROUPS);
        const bool acc = b0 > 0;
        const float* feat = d_feat + (size_t)b0 * T * F;
        // recompute: the composed forward of kws_forward_map_f32, every stage kept
        HIP_TRY(c, launch_dscnn_composed(s, c->mw, feat, nb, T, F, st));
        // pool + fc
        hipLaunchKernelGGL(kws_bwd_fc_kernel, dim3(G), dim3(256), 0, s, st.y[LAST], d_dlogits + (size_t)b0 * C, raw + L.b_fcw,
                           (int)m.Q(LAST), C, nb, cpg, dy4, part);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, reduce(s, part, G, fc_part(C), d_grad + L.b_fcw, acc));
        // blocks 4 .. 1
        for (int k = LAST; k >= 0; --k) {
            const float* prm = raw + L.block(k);
            float* gk = d_grad + L.block(k);
            const int Q = (int)m.Q(k);
            const bool last = k == LAST;
            hipLaunchKernelGGL(kws_bwd_pointwise_kernel, dim3(G), dim3(256), 0, s, last ? dy4 : gin, last ? (long)CH : (long)CH * Q,
                               last ? 1 : Q, last ? 0 : 1, st.y[k], st.dw[k], prm + DL::B_PWW, m.H(k), m.W(k), nb, cpg, gdw, part);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, reduce(s, part, G, PW_PART, gk + DL::B_PWW, acc));
            hipLaunchKernelGGL(kws_bwd_depthwise_kernel, dim3(CH / 4, G), dim3(256), 0, s, gdw, k ? st.y[k - 1] : st.a0, prm, m.H(k), m.W(k),
                               nb, cpg, gin, part);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, reduce(s, part, G, DW_PART, gk, acc));
        }
        // conv1
        hipLaunchKernelGGL(kws_bwd_conv1_kernel, dim3(G), dim3(256), 0, s, gin, st.a0, feat, T, F, m.H1, m.W1, nb, cpg, part);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, reduce(s, part, G, C1_PART, d_grad, acc));
    }
    return KWS_OK;
    KWS_GUARD_END(c, "kws_dscnn_backward_f32")
}

}  // extern "C"
#pragma GCC visibility pop
