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
constexpr int BWD_MAX_GROUPS = 1024;          // partial rows per stage and chunk
constexpr int PW_TP = 64;                     // interior positions per tile of the pointwise backward
constexpr int PW_PART = DL::PW_W + DL::CO;    // pointwise.weight [co][ci] | pointwise.bias
constexpr int DW_PART = DL::DW_W + DL::CO;    // depthwise.weight [c][3][3] | depthwise.bias
constexpr int C1_PART = DL::C1_W + DL::CO;    // conv1.weight [co][10][10] | conv1.bias
constexpr int fc_part(int C) { return C * DL::CO + C; }  // fc.weight [C][64] | fc.bias

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
    __shared__ float s_w[64][65];        // W[co][ci]
    __shared__ float s_dz[64][PW_TP + 1];  // dZ[co][p]
    __shared__ float s_x[64][PW_TP + 1];   // X_dw[ci][p]
    __shared__ float s_b[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = blockIdx.x;
    const int P = H * W, Wq = W + 2, Q = (H + 2) * Wq;
    for (int e = tid; e < DL::PW_W; e += 256) s_w[e >> 6][e & 63] = w[e];
    __syncthreads();
    const int co0 = 32 * (wv >> 1), ci0 = 32 * (wv & 1), pt0 = 32 * (wv >> 1);
    // A operand of dX_dw = W^T dZ (32x32x2: A[i = l & 31][k = l >> 5]): A[ci][co] = W[co][ci], k-step s covers co 2s, 2s + 1
    float wa[32];
#pragma unroll
    for (int s = 0; s < 32; ++s) wa[s] = s_w[2 * s + (lane >> 5)][ci0 + (lane & 31)];
    // the MFMA calls, zero fills and D rows stay spelled out in this kernel: through kws_train.h's mfma32 / zero16 / drow it
    // took 176 VGPRs for 168
    f32x16 gw;
#pragma unroll
    for (int r = 0; r < 16; ++r) gw[r] = 0.f;
    float bsum = 0.f;
    const int b_end = group_end(g, cpg, nb);
    for (int b = g * cpg; b < b_end; ++b) {
        const float* dyb = dy + (size_t)b * dy_clip;
        const float* yb = y + (size_t)b * 64 * Q;
        const float* xb = xdw + (size_t)b * 64 * P;
        {
            const float* yc = yb + (size_t)lane * Q;
            const float* dc = dyb + (size_t)lane * dy_plane;
            for (int r0 = wv; r0 < Q; r0 += 4 * RUN) {  // runs of RUN positions, each summed from zero
                const int r1 = min(Q, r0 + 4 * RUN);
                float t = 0.f;
                for (int q = r0; q < r1; q += 4)
                    if (yc[q] > 0.f) t += dc[(size_t)q * dy_qstep];
                bsum += t;
            }
        }
        for (int p0 = 0; p0 < P; p0 += PW_TP) {
            for (int e = tid; e < 64 * PW_TP; e += 256) {
                const int row = e / PW_TP, pp = e % PW_TP, p = p0 + pp;
                float dz = 0.f, xv = 0.f;
                if (p < P) {
                    const int q = (p / W + 1) * Wq + p % W + 1;
                    const float yv = yb[(size_t)row * Q + q];
                    dz = yv > 0.f ? dyb[(size_t)row * dy_plane + (size_t)q * dy_qstep] : 0.f;
                    xv = xb[(size_t)row * P + p];
                }
                s_dz[row][pp] = dz;
                s_x[row][pp] = xv;
            }
            __syncthreads();
            // g_pw_w: A[i = co][k = p] = dZ, B[k = p][j = ci] = X_dw (32x32x2: lane l holds k = l >> 5); the tile's sum starts
            // from zero and is added to the running one, so no f32 chain runs longer than 64 positions
            f32x16 gt;
#pragma unroll
            for (int r = 0; r < 16; ++r) gt[r] = 0.f;
#pragma unroll
            for (int s = 0; s < PW_TP / 2; ++s) {
                const float a = s_dz[co0 + (lane & 31)][2 * s + (lane >> 5)];
                const float bb = s_x[ci0 + (lane & 31)][2 * s + (lane >> 5)];
                gt = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, gt, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) gw[r] += gt[r];
            // dX_dw: B[k = co][j = p] = dZ
            f32x16 d;
#pragma unroll
            for (int r = 0; r < 16; ++r) d[r] = 0.f;
#pragma unroll
            for (int s = 0; s < 32; ++s) d = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[s], s_dz[2 * s + (lane >> 5)][pt0 + (lane & 31)], d, 0, 0, 0);
            // C/D: col = l & 31 (position), row = (r & 3) + 8 (r >> 2) + 4 (l >> 5) (input channel)
            const int p = p0 + pt0 + (lane & 31);
            if (p < P) {
                float* o = dxdw + (size_t)b * 64 * P + (size_t)ci0 * P + p;
#pragma unroll
                for (int r = 0; r < 16; ++r) o[(size_t)((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * P] = d[r];
            }
            __syncthreads();
        }
    }
    float* pg = part + (size_t)g * PW_PART;
    // C/D of 32x32: col = l & 31 (ci), row = (r & 3) + 8 (r >> 2) + 4 (l >> 5) (co)
#pragma unroll
    for (int r = 0; r < 16; ++r) pg[(co0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * 64 + ci0 + (lane & 31)] = gw[r];
    s_b[wv][lane] = bsum;
    __syncthreads();
    if (tid < 64) pg[DL::PW_W + tid] = (s_b[0][tid] + s_b[1][tid]) + (s_b[2][tid] + s_b[3][tid]);
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
    __shared__ float s_dz[C1B_TP][65];
    __shared__ float s_b[4][64];
    const int tid = threadIdx.x, co = tid & 63, r0 = tid >> 6, g = blockIdx.x;
    const int P = H1 * W1;
    float acc[3][10];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 10; ++k) acc[i][k] = 0.f;
    float bsum = 0.f;
    const int b_end = group_end(g, cpg, nb);
    for (int b = g * cpg; b < b_end; ++b) {
        const float* dab = da + (size_t)b * 64 * P;
        const float* ab = a + (size_t)b * 64 * P;
        const float* xb = x + (size_t)b * T * F;
        for (int p0 = 0; p0 < P; p0 += C1B_TP) {
            for (int e = tid; e < 64 * C1B_TP; e += 256) {
                const int ch = e / C1B_TP, pp = e % C1B_TP, p = p0 + pp;
                float dz = 0.f;
                if (p < P && ab[(size_t)ch * P + p] > 0.f) dz = dab[(size_t)ch * P + p];
                s_dz[pp][ch] = dz;
            }
            __syncthreads();
            const int n = min(C1B_TP, P - p0);
            for (int pp = 0; pp < n; ++pp) {
                const int p = p0 + pp, oh = p / W1, ow = p % W1;
                const float dz = s_dz[pp][co];
                if (r0 == 0) bsum += dz;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const int kh = r0 + 4 * i;
                    const int ih = 2 * oh - 2 + kh;
                    if (kh < 10 && (unsigned)ih < (unsigned)T) {
                        const float* xr = xb + (size_t)ih * F;
#pragma unroll
                        for (int kw = 0; kw < 10; ++kw) {
                            const int iw = 2 * ow - 2 + kw;
                            if ((unsigned)iw < (unsigned)F) acc[i][kw] = fmaf(dz, xr[iw], acc[i][kw]);
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
    float* pg = part + (size_t)g * C1_PART;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int kh = r0 + 4 * i;
        if (kh < 10) {
#pragma unroll
            for (int kw = 0; kw < 10; ++kw) pg[co * DL::C1_TAPS + kh * 10 + kw] = acc[i][kw];
        }
    }
    s_b[r0][co] = bsum;
    __syncthreads();
    if (tid < 64) pg[DL::C1_W + tid] = s_b[0][tid];
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
