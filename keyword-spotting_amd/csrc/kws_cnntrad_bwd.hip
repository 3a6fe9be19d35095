// Training: the backward pass of cnn-trad-fpool3 (kws_cnntrad.hip, oracle/cnn_trad.py) -- the gradient of a scalar loss with
// respect to all ten state_dict tensors, given dloss/dlogits (kws_cnn_trad_backward_f32, include/kws_hip.h).  It replaces
// loss.backward() of the reference trainer (train.py:48, kws/libs/training.py:296) for this model.
//
// Recompute, not save: the activations are recomputed at the start of the call by this unit's own f32 forward (the inference
// kernels kws_cnntrad_conv_kernel / kws_cnntrad_dense_kernel are not used and not changed), so the gradients do not depend on
// kws_set_cnn_trad_math.  Only the pooled conv1 map and its winners are kept of conv1: the ReLU mask of conv1 at a winner is
// pooled > 0, so conv1's full 64 x 99 x 10 output never reaches memory.
//
// Kernels (stable names for rocprofv3 --kernel-trace), per chunk of clips:
//   kws_ct_bwd_prep_kernel         conv2.weight as the two A-operand tables [kk][k channel][m channel] (once per call)
//   kws_ct_bwd_conv1_kernel        conv1 + ReLU + 1x3 max-pool on the VALU (fmaf, rows of 8 taps summed from zero):
//                                  pooled map yp and the winner (first maximum, torch's rule) per pooled position
//   kws_ct_bwd_conv2_fwd_kernel    conv2 + ReLU: implicit GEMM M = 64, N = 297, K = 2560 on v_mfma_f32_32x32x2_f32
//   kws_ct_bwd_lin_fwd_kernel      h = lin(y2) (K = 19008 on the f32 MFMA) and d = relu(dnn(h))
//   kws_ct_bwd_tail_kernel         dd = fc.w^T dl [d > 0], dh = dnn.w^T dd; partials of g_fc, g_dnn, g_lin.b
//   kws_ct_bwd_lin_kernel          dz2 = (lin.w^T dh) [y2 > 0] and g_lin.w = sum_b dh (x) y2, both on the f32 MFMA; every wave owns
//                                  32 columns of lin.weight over the whole chunk, so g_lin.w needs no partials
//   kws_ct_bwd_conv2_wgrad_kernel  g_conv2.w (M = 64, N = 2560, K = 297 per clip) on the f32 MFMA, g_conv2.b
//   kws_ct_bwd_conv2_dgrad_kernel  dyp = correlation of dz2 with the flipped, transposed kernel (K = 2560) on the f32 MFMA; the
//                                  epilogue keeps it where the pooled value is > 0 (dz1 at the winners)
//   kws_ct_bwd_conv1_wgrad_kernel  g_conv1.w (M = 64, N = 160, K = 297 winners per clip) and g_conv1.b on the VALU
//   kws_ct_bwd_reduce_kernel       fixed-order sum of the per-workgroup partials into d_grad
//
// Deterministic: no float atomics.  Clip ownership is fixed by the chunk size alone (conv groups: cpg = ceil(nb / 256) clips,
// tail groups: 64 clips), partial rows are reduced in a fixed order, and chunks after the first add onto d_grad in chunk order.
// Every long sum runs in runs of at most 64 terms, each started from zero: positions of a clip in runs of 64, clips of a group
// one clip sum at a time (cpg <= 32), clip blocks of lin.weight's gradient in blocks of 32 (blocks of blocks of 32), partial rows
// in runs of 32.
//
// Memory is written with plain vector stores only; there is no inline assembly in this unit.
#include "kws_train.h"

namespace kws {
namespace {

using CL = CtLayout;
constexpr int CT_T = 99, CT_F = 10, CT_P = 297, CT_FLAT = (int)CL::FLAT;  // pooled map: 64 x 99 x 3
static_assert(CT_FLAT == CH * CT_P, "lin's inputs are the pooled map");
constexpr int XP_H = 118, XP_W = 17;                                      // conv1's zero-padded input (pad 9/10 x 3/4)
constexpr int W2_N = CL::N_C2;                                            // conv2.weight floats
constexpr int MAX_CHUNK = 8192;                // clips per chunk (the workspace is about 324 KB per clip)
constexpr int CONV_GROUPS = 256;               // clip groups of the two weight-gradient kernels
constexpr int TAIL_CPG = 64;                   // clips per group of the tail kernel
constexpr int C2W_PART = W2_N + (int)CL::CO;   // [kk][co][ci] | conv2.bias
constexpr int C1W_PART = CL::N_C1 + (int)CL::CO;
constexpr int HD = CL::LIN_OUT + CL::DNN_OUT;  // [h | d] per clip
constexpr int LIN_TILES = CT_FLAT / 32;  // 594 column tiles of lin.weight
constexpr int LF_WAVES = 6, LF_BLOCKS = LIN_TILES / LF_WAVES;  // h = lin(y2): 99 blocks of 32 k per wave
static_assert(LF_BLOCKS * LF_WAVES == LIN_TILES && LF_BLOCKS % 3 == 0, "K of lin must divide among the waves");
// the tail's partial row, in the blob's order from lin.bias on: lin.b | dnn.w | dnn.b | fc.w | fc.b
constexpr int TP_DW = CL::LIN_OUT, TP_DB = TP_DW + CL::N_DNN, TP_FW = TP_DB + CL::DNN_OUT;
constexpr int tail_part_floats(int C) { return TP_FW + CL::DNN_OUT * C + C; }
constexpr int CONV2_LDS = CT_FLAT * 4;                           // one map [64][297]
constexpr int C2W_LDS = 2 * CT_FLAT * 4;                         // dz2 | yp
constexpr int C1W_X = 2048;                                      // floats reserved for the padded input (118 x 17 = 2006)
constexpr int C1W_LDS = (C1W_X + CT_FLAT) * 4 + CT_FLAT;         // padded input | dz1 | winners (bytes)

__device__ __forceinline__ float relu0(float v) { return v > 0.f ? v : 0.f; }

// ---- conv2.weight [co][ci][kk] as A-operand tables ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kws_ct_bwd_prep_kernel(const float* __restrict__ w2, float* __restrict__ w2t, float* __restrict__ w2u) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= W2_N) return;
    const int co = i / 2560, ci = (i / 40) % 64, kk = i % 40;
    const float v = w2[i];
    w2t[(kk * 64 + ci) * 64 + co] = v;  // forward: A[m = co][k = ci]
    w2u[(kk * 64 + co) * 64 + ci] = v;  // input gradient: A[m = ci][k = co]
}

// ---- conv1 + ReLU + max-pool ------------------------------------------------------------------------------------------------
// One workgroup per clip.  Wave w owns channels w, w + 4, ..; lane = time row (two passes: 0..63, 64..98).  Per (channel, row):
// the ten outputs of the row, each sum taken as 20 kernel-row sums of 8 taps (from zero) added in kernel-row order.
__global__ __launch_bounds__(256) void kws_ct_bwd_conv1_kernel(const float* __restrict__ feat, const float* __restrict__ w1,
                                                               const float* __restrict__ b1, float* __restrict__ yp,
                                                               unsigned char* __restrict__ win, float* __restrict__ dbg_conv1,
                                                               int32_t* __restrict__ dbg_win) {
    __shared__ float s_x[XP_H * XP_W];
    __shared__ float s_w[CL::N_C1];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x;
    const float* xb = feat + (size_t)b * (CT_T * CT_F);
    for (int i = tid; i < XP_H * XP_W; i += 256) {
        const int r = i / XP_W - 9, c = i % XP_W - 3;
        s_x[i] = ((unsigned)r < (unsigned)CT_T && (unsigned)c < (unsigned)CT_F) ? xb[r * CT_F + c] : 0.f;
    }
    for (int i = tid; i < CL::N_C1; i += 256) s_w[i] = w1[i];
    __syncthreads();
    for (int co = wv; co < 64; co += 4) {
        const float bias = b1[co];
        const float* wc = s_w + co * 160;
        for (int t = lane; t < CT_T; t += 64) {
            float acc[CT_F];
#pragma unroll
            for (int f = 0; f < CT_F; ++f) acc[f] = 0.f;
            for (int kh = 0; kh < 20; ++kh) {
                float xr[XP_W], rs[CT_F];
#pragma unroll
                for (int j = 0; j < XP_W; ++j) xr[j] = s_x[(t + kh) * XP_W + j];
#pragma unroll
                for (int f = 0; f < CT_F; ++f) rs[f] = 0.f;
#pragma unroll
                for (int kw = 0; kw < 8; ++kw) {
                    const float wt = wc[kh * 8 + kw];
#pragma unroll
                    for (int f = 0; f < CT_F; ++f) rs[f] = fmaf(wt, xr[f + kw], rs[f]);
                }
#pragma unroll
                for (int f = 0; f < CT_F; ++f) acc[f] += rs[f];
            }
            float v[CT_F];
#pragma unroll
            for (int f = 0; f < CT_F; ++f) v[f] = relu0(acc[f] + bias);
            const size_t o = ((size_t)b * 64 + co) * CT_P + t * 3;
#pragma unroll
            for (int fp = 0; fp < 3; ++fp) {  // first maximum wins (torch's max_pool2d); column 9 is dropped
                float m = v[3 * fp];
                int wi = 0;
                if (v[3 * fp + 1] > m) {
                    m = v[3 * fp + 1];
                    wi = 1;
                }
                if (v[3 * fp + 2] > m) {
                    m = v[3 * fp + 2];
                    wi = 2;
                }
                yp[o + fp] = m;
                win[o + fp] = (unsigned char)wi;
                if (dbg_win) dbg_win[o + fp] = wi;
            }
            if (dbg_conv1) {
                float* d = dbg_conv1 + (((size_t)b * 64 + co) * CT_T + t) * CT_F;
#pragma unroll
                for (int f = 0; f < CT_F; ++f) d[f] = v[f];
            }
        }
    }
}

// ---- conv2 as an implicit GEMM on the map in LDS ----------------------------------------------------------------------------
// out[m][p] = sum over kk = (kh, kw) and k channels of tab[kk][k][m] * map[k][p shifted], p = (t, f) over 99 x 3:
//   forward (FWD):        map = yp,  shift (t + kh - 4, f + kw - 1), tab = w2t  -> relu(. + b2) = y2
//   input gradient:       map = dz2, shift (t - kh + 4, f - kw + 1), tab = w2u  -> dyp, kept where yp > 0 (= dz1 at the winners)
// One workgroup (4 waves) per clip; wave w takes m tile w & 1 and the position tiles (w >> 1) + 2i, i < 5.  Per kk, the 32
// k-steps (64 products) are summed from zero and added to the running sum.
template <bool FWD>
__device__ __forceinline__ void conv2_body(const float* __restrict__ map, const float* __restrict__ tab, const float* __restrict__ bias,
                                           const float* __restrict__ ypmask, float* __restrict__ out, float* smem) {
    constexpr int NT = 5;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, half = lane >> 5, col = lane & 31, b = blockIdx.x;
    const float4* src = reinterpret_cast<const float4*>(map + (size_t)b * CT_FLAT);
    for (int i = tid; i < CT_FLAT / 4; i += 256) reinterpret_cast<float4*>(smem)[i] = src[i];
    __syncthreads();
    const int mt = wv & 1;
    int t[NT], f[NT], p[NT];
    f32x16 run[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        p[i] = ((wv >> 1) + 2 * i) * 32 + col;
        t[i] = p[i] / 3;
        f[i] = p[i] % 3;
        zero16(run[i]);
    }
    for (int kk = 0; kk < 40; ++kk) {
        const int kh = kk >> 2, kw = kk & 3;
        const int dt = FWD ? kh - 4 : 4 - kh, df = FWD ? kw - 1 : 1 - kw;
        int q[NT];
        bool ok[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int ti = t[i] + dt, fi = f[i] + df;
            ok[i] = p[i] < CT_P && (unsigned)ti < (unsigned)CT_T && (unsigned)fi < 3u;
            q[i] = ok[i] ? ti * 3 + fi : 0;
        }
        f32x16 blk[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) zero16(blk[i]);
        const float* ta = tab + (size_t)kk * 4096 + mt * 32 + col;
#pragma unroll 8
        for (int s = 0; s < 32; ++s) {
            const int kc = 2 * s + half;  // A[i = m][k = kc], B[k = kc][j = p]
            const float a = ta[kc * 64];
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const float bv = smem[kc * CT_P + q[i]];
                blk[i] = mfma32(a, ok[i] ? bv : 0.f, blk[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) run[i] += blk[i];
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        if (p[i] >= CT_P) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = mt * 32 + drow(r, half);
            const size_t o = (size_t)b * CT_FLAT + (size_t)m * CT_P + p[i];
            if constexpr (FWD)
                out[o] = relu0(run[i][r] + bias[m]);
            else
                out[o] = ypmask[o] > 0.f ? run[i][r] : 0.f;
        }
    }
}
__global__ __launch_bounds__(256) void kws_ct_bwd_conv2_fwd_kernel(const float* __restrict__ yp, const float* __restrict__ w2t,
                                                                   const float* __restrict__ b2, float* __restrict__ y2) {
    extern __shared__ float smem[];
    conv2_body<true>(yp, w2t, b2, nullptr, y2, smem);
}
__global__ __launch_bounds__(256) void kws_ct_bwd_conv2_dgrad_kernel(const float* __restrict__ dz2, const float* __restrict__ w2u,
                                                                     const float* __restrict__ yp, float* __restrict__ dz1) {
    extern __shared__ float smem[];
    conv2_body<false>(dz2, w2u, nullptr, yp, dz1, smem);
}

// ---- h = lin(y2), d = relu(dnn(h)) ------------------------------------------------------------------------------------------
// 32 clips per workgroup (the MFMA rows; rows past the batch repeat its last clip and are not written), K = 19008 split among six
// waves, 99 blocks of 32 k each.  In block k0, k-step s covers k0 + 16 half + s, so a lane reads 16 consecutive floats of its
// clip's y2 row and of its output's weight row.  Block sums start from zero; 33 of them make a third, three thirds the wave's sum;
// the six wave sums are added in wave order, then the bias.
__global__ __launch_bounds__(LF_WAVES * 64) void kws_ct_bwd_lin_fwd_kernel(const float* __restrict__ y2, const float* __restrict__ wl,
                                                                           const float* __restrict__ bl, const float* __restrict__ wd,
                                                                           const float* __restrict__ bd, int nb, float* __restrict__ hd) {
    __shared__ float s_part[LF_WAVES][32][33];
    __shared__ float s_h[32][33];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, half = lane >> 5, col = lane & 31;
    const int b0 = blockIdx.x * 32;
    const int ba = min(b0 + col, nb - 1);
    const float* xa = y2 + (size_t)ba * CT_FLAT + half * 16;
    const float* wb = wl + (size_t)col * CT_FLAT + half * 16;
    f32x16 run;
    zero16(run);
    for (int g = 0; g < 3; ++g) {
        f32x16 mid;
        zero16(mid);
        for (int n = 0; n < LF_BLOCKS / 3; ++n) {
            const int k0 = (wv * LF_BLOCKS + g * (LF_BLOCKS / 3) + n) * 32;
            float av[16], bv[16];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 x4 = *reinterpret_cast<const float4*>(xa + k0 + 4 * j);
                const float4 w4 = *reinterpret_cast<const float4*>(wb + k0 + 4 * j);
                av[4 * j] = x4.x; av[4 * j + 1] = x4.y; av[4 * j + 2] = x4.z; av[4 * j + 3] = x4.w;
                bv[4 * j] = w4.x; bv[4 * j + 1] = w4.y; bv[4 * j + 2] = w4.z; bv[4 * j + 3] = w4.w;
            }
            f32x16 blk;
            zero16(blk);
#pragma unroll
            for (int s = 0; s < 16; ++s) blk = mfma32(av[s], bv[s], blk);
            mid += blk;
        }
        run += mid;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) s_part[wv][drow(r, half)][col] = run[r];  // D[row = clip slot][column = output]
    __syncthreads();
    for (int i = tid; i < 32 * 32; i += LF_WAVES * 64) {
        const int s = i >> 5, j = i & 31;
        float a = 0.f;
#pragma unroll
        for (int w = 0; w < LF_WAVES; ++w) a += s_part[w][s][j];
        a += bl[j];
        s_h[s][j] = a;
        if (b0 + s < nb) hd[(size_t)(b0 + s) * HD + j] = a;
    }
    __syncthreads();
    for (int i = tid; i < 32 * 128; i += LF_WAVES * 64) {
        const int s = i >> 7, j = i & 127;
        float a = bd[j];
        for (int k = 0; k < 32; ++k) a = fmaf(s_h[s][k], wd[j * 32 + k], a);
        if (b0 + s < nb) hd[(size_t)(b0 + s) * HD + CL::LIN_OUT + j] = relu0(a);
    }
}

// ---- the dense tail -----------------------------------------------------------------------------------------------------------
// One workgroup per group of TAIL_CPG clips.  Per clip: dd = (fc.w^T dl) [d > 0], dh = dnn.w^T dd (two runs of 64); partial sums
// in the blob's order from lin.bias on: g_lin.b = sum dh, g_dnn.w = sum dd (x) h, g_dnn.b = sum dd, g_fc.w = sum dl (x) d,
// g_fc.b = sum dl.
__global__ __launch_bounds__(256) void kws_ct_bwd_tail_kernel(const float* __restrict__ hd, const float* __restrict__ dl,
                                                              const float* __restrict__ wd, const float* __restrict__ wf, int C, int nb,
                                                              float* __restrict__ dh, float* __restrict__ part) {
    constexpr int PER = (tail_part_floats(MAX_CLASSES) + 255) / 256;
    __shared__ float s_h[32], s_d[128], s_dl[MAX_CLASSES], s_dd[128], s_dh[32];
    const int tid = threadIdx.x, g = blockIdx.x;
    const int n_part = tail_part_floats(C);
    float acc[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) acc[k] = 0.f;
    const int b_end = group_end(g, TAIL_CPG, nb);
    for (int b = g * TAIL_CPG; b < b_end; ++b) {
        if (tid < HD) {
            const float v = hd[(size_t)b * HD + tid];
            if (tid < 32)
                s_h[tid] = v;
            else
                s_d[tid - 32] = v;
        }
        if (tid < C) s_dl[tid] = dl[(size_t)b * C + tid];
        __syncthreads();
        if (tid < 128) {
            float a = 0.f;
            for (int c = 0; c < C; ++c) a = fmaf(wf[c * 128 + tid], s_dl[c], a);
            s_dd[tid] = s_d[tid] > 0.f ? a : 0.f;
        }
        __syncthreads();
        if (tid < 32) {
            float a0 = 0.f, a1 = 0.f;
            for (int j = 0; j < 64; ++j) a0 = fmaf(wd[j * 32 + tid], s_dd[j], a0);
            for (int j = 64; j < 128; ++j) a1 = fmaf(wd[j * 32 + tid], s_dd[j], a1);
            s_dh[tid] = a0 + a1;
            dh[(size_t)b * 32 + tid] = a0 + a1;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int e = tid + 256 * k;
            if (e < TP_DW)
                acc[k] += s_dh[e];
            else if (e < TP_DB)
                acc[k] = fmaf(s_dd[(e - TP_DW) >> 5], s_h[(e - TP_DW) & 31], acc[k]);
            else if (e < TP_FW)
                acc[k] += s_dd[e - TP_DB];
            else if (e < TP_FW + CL::DNN_OUT * C)
                acc[k] = fmaf(s_dl[(e - TP_FW) >> 7], s_d[(e - TP_FW) & 127], acc[k]);
            else if (e < n_part)
                acc[k] += s_dl[e - TP_FW - CL::DNN_OUT * C];
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

// ---- lin backward: dz2 and lin.weight's gradient --------------------------------------------------------------------------------
// Wave = one tile of 32 columns of lin.weight, over every clip of the chunk in blocks of 32:
//   dY2 tile D[clip][col] = sum_j dh[clip][j] W[j][col]   (K = 32 outputs), dz2 = dY2 [y2 > 0]
//   gW  tile D[j][col]   += sum_clip dh[clip][j] y2[clip][col]   (K = 32 clips per block; 32 blocks per mid sum)
// The wave owns its columns, so the gradient goes straight to d_grad (added to it after the first chunk).
__global__ __launch_bounds__(256) void kws_ct_bwd_lin_kernel(const float* __restrict__ y2, const float* __restrict__ dh,
                                                             const float* __restrict__ wl, int nb, int accumulate, float* __restrict__ dz2,
                                                             float* __restrict__ g_wl) {
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, col = lane & 31;
    const int tile = blockIdx.x * 4 + (tid >> 6);
    if (tile >= LIN_TILES) return;  // whole waves; no barrier in this kernel
    const int c0 = tile * 32;
    float wb[16];  // B[k = j][col]: k-step s covers outputs 2s + half
#pragma unroll
    for (int s = 0; s < 16; ++s) wb[s] = wl[(size_t)(2 * s + half) * CT_FLAT + c0 + col];
    f32x16 run, mid;
    zero16(run);
    zero16(mid);
    int nblk = 0;
    for (int b0 = 0; b0 < nb; b0 += 32) {
        const int ba = b0 + col;
        f32x16 d;
        zero16(d);
#pragma unroll
        for (int s = 0; s < 16; ++s) d = mfma32(ba < nb ? dh[(size_t)ba * 32 + 2 * s + half] : 0.f, wb[s], d);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int bb = b0 + drow(r, half);
            if (bb < nb) {
                const size_t o = (size_t)bb * CT_FLAT + c0 + col;
                dz2[o] = y2[o] > 0.f ? d[r] : 0.f;
            }
        }
        f32x16 blk;
        zero16(blk);
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int bs = b0 + 2 * s + half;  // A[i = j][k = clip], B[k = clip][j = col]
            const bool v = bs < nb;
            const float a = v ? dh[(size_t)bs * 32 + col] : 0.f;
            const float bv = v ? y2[(size_t)bs * CT_FLAT + c0 + col] : 0.f;
            blk = mfma32(a, bv, blk);
        }
        mid += blk;
        if (++nblk == 32) {
            run += mid;
            zero16(mid);
            nblk = 0;
        }
    }
    run += mid;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float* o = g_wl + (size_t)drow(r, half) * CT_FLAT + c0 + col;
        *o = accumulate ? *o + run[r] : run[r];
    }
}

// ---- conv2 weight gradient -----------------------------------------------------------------------------------------------------
// Grid (10 slices of 4 kk, clip groups), 8 waves.  Wave w: kk = 4 slice + (w >> 1), co tile w & 1, both ci tiles:
//   D[co][ci] += sum_p dz2[co][p] yp[ci][(t + kh - 4, f + kw - 1)]   (A[i = co][k = p], B[k = p][j = ci]; k-step s: p = 2s + half)
// Runs of 64 positions from zero -> the clip's sum -> the group's sum.  Slice 0 also sums conv2.bias: thread (co, part) over its
// part's <= 38 positions per clip, the eight parts added in order at the end.  Partial row: [kk][co][ci] | bias.
__global__ __launch_bounds__(512) void kws_ct_bwd_conv2_wgrad_kernel(const float* __restrict__ dz2, const float* __restrict__ yp, int nb,
                                                                     int cpg, float* __restrict__ part) {
    extern __shared__ float smem[];
    float* s_dz = smem;
    float* s_y = smem + CT_FLAT;
    __shared__ float s_b[8][64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, half = lane >> 5, col = lane & 31, g = blockIdx.y;
    const int kk = blockIdx.x * 4 + (wv >> 1), mt = wv & 1, kh = kk >> 2, kw = kk & 3;
    const bool do_bias = blockIdx.x == 0;
    f32x16 grp[2];
    zero16(grp[0]);
    zero16(grp[1]);
    float bgrp = 0.f;
    const int b_end = group_end(g, cpg, nb);
    for (int b = g * cpg; b < b_end; ++b) {
        __syncthreads();
        const float4* s1 = reinterpret_cast<const float4*>(dz2 + (size_t)b * CT_FLAT);
        const float4* s2 = reinterpret_cast<const float4*>(yp + (size_t)b * CT_FLAT);
        for (int i = tid; i < CT_FLAT / 4; i += 512) {
            reinterpret_cast<float4*>(s_dz)[i] = s1[i];
            reinterpret_cast<float4*>(s_y)[i] = s2[i];
        }
        __syncthreads();
        if (do_bias) {
            const int p0 = wv * 38, p1 = min(CT_P, p0 + 38);
            float t = 0.f;
            for (int p = p0; p < p1; ++p) t += s_dz[lane * CT_P + p];
            bgrp += t;
        }
        f32x16 clp[2];
        zero16(clp[0]);
        zero16(clp[1]);
        for (int s0 = 0; s0 < (CT_P + 1) / 2; s0 += RUN / 2) {
            const int s1e = min((CT_P + 1) / 2, s0 + RUN / 2);
            f32x16 blk[2];
            zero16(blk[0]);
            zero16(blk[1]);
            for (int s = s0; s < s1e; ++s) {
                const int p = 2 * s + half;
                const int t = p / 3, f = p % 3, ti = t + kh - 4, fi = f + kw - 1;
                const bool pv = p < CT_P;
                const bool ok = pv && (unsigned)ti < (unsigned)CT_T && (unsigned)fi < 3u;
                const int q = ok ? ti * 3 + fi : 0;
                const float av = s_dz[(mt * 32 + col) * CT_P + (pv ? p : 0)];
                const float a = pv ? av : 0.f;
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const float bv = s_y[(ct * 32 + col) * CT_P + q];
                    blk[ct] = mfma32(a, ok ? bv : 0.f, blk[ct]);
                }
            }
            clp[0] += blk[0];
            clp[1] += blk[1];
        }
        grp[0] += clp[0];
        grp[1] += clp[1];
    }
    float* pg = part + (size_t)g * C2W_PART;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) pg[(kk * 64 + mt * 32 + drow(r, half)) * 64 + ct * 32 + col] = grp[ct][r];
    if (do_bias) {
        s_b[wv][lane] = bgrp;
        __syncthreads();
        if (tid < 64) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < 8; ++w) s += s_b[w][tid];
            pg[W2_N + tid] = s;
        }
    }
}

// ---- conv1 weight gradient --------------------------------------------------------------------------------------------------------
// One workgroup (8 waves) per clip group.  Thread (co = lane, r0 = wave) owns kernel rows r0, r0 + 8, r0 + 16 (< 20), 8 columns
// each.  Per pooled position p = (t, fp) with gradient dz1[co][p] (zero unless the pooled value is > 0) at the winner column
// f = 3 fp + win: g[kh][kw] += dz1 * xpad[t + kh][f + kw].  Runs of 64 positions -> clip -> group.
__global__ __launch_bounds__(512) void kws_ct_bwd_conv1_wgrad_kernel(const float* __restrict__ feat, const float* __restrict__ dz1,
                                                                     const unsigned char* __restrict__ win, int nb, int cpg,
                                                                     float* __restrict__ part) {
    extern __shared__ float smem[];
    float* s_x = smem;
    float* s_dz = smem + C1W_X;
    unsigned char* s_w = reinterpret_cast<unsigned char*>(smem + C1W_X + CT_FLAT);
    const int tid = threadIdx.x, co = tid & 63, r0 = tid >> 6, g = blockIdx.x;
    float grp[3][8], bgrp = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 8; ++k) grp[i][k] = 0.f;
    const int b_end = group_end(g, cpg, nb);
    for (int b = g * cpg; b < b_end; ++b) {
        __syncthreads();
        const float* xb = feat + (size_t)b * (CT_T * CT_F);
        for (int i = tid; i < XP_H * XP_W; i += 512) {
            const int r = i / XP_W - 9, c = i % XP_W - 3;
            s_x[i] = ((unsigned)r < (unsigned)CT_T && (unsigned)c < (unsigned)CT_F) ? xb[r * CT_F + c] : 0.f;
        }
        const float4* sd = reinterpret_cast<const float4*>(dz1 + (size_t)b * CT_FLAT);
        for (int i = tid; i < CT_FLAT / 4; i += 512) reinterpret_cast<float4*>(s_dz)[i] = sd[i];
        const uint32_t* sw = reinterpret_cast<const uint32_t*>(win + (size_t)b * CT_FLAT);
        for (int i = tid; i < CT_FLAT / 4; i += 512) reinterpret_cast<uint32_t*>(s_w)[i] = sw[i];
        __syncthreads();
        float clp[3][8], bclp = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 8; ++k) clp[i][k] = 0.f;
        for (int p0 = 0; p0 < CT_P; p0 += RUN) {
            const int p1 = min(CT_P, p0 + RUN);
            float run[3][8], brun = 0.f;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int k = 0; k < 8; ++k) run[i][k] = 0.f;
            for (int p = p0; p < p1; ++p) {
                const float dz = s_dz[co * CT_P + p];
                const int t = p / 3, f = 3 * (p % 3) + s_w[co * CT_P + p];
                brun += dz;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const int kh = r0 + 8 * i;
                    if (kh < 20) {
                        const float* xr = s_x + (t + kh) * XP_W + f;
#pragma unroll
                        for (int kw = 0; kw < 8; ++kw) run[i][kw] = fmaf(dz, xr[kw], run[i][kw]);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int k = 0; k < 8; ++k) clp[i][k] += run[i][k];
            bclp += brun;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 8; ++k) grp[i][k] += clp[i][k];
        bgrp += bclp;
    }
    float* pg = part + (size_t)g * C1W_PART;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int kh = r0 + 8 * i;
        if (kh < 20) {
#pragma unroll
            for (int kw = 0; kw < 8; ++kw) pg[co * 160 + kh * 8 + kw] = grp[i][kw];
        }
    }
    if (r0 == 0) pg[CL::N_C1 + co] = bgrp;
}

// out (+)= sum over g < G of part[g], in the fixed order of reduce_partials (kws_train.h).  perm_c2: the rows are conv2 partials
// ([kk][co][ci] | bias), written to the blob's [co][ci][kk] | bias.
__global__ __launch_bounds__(256) void kws_ct_bwd_reduce_kernel(const float* __restrict__ part, int G, int n, int perm_c2,
                                                                float* __restrict__ out, int accumulate) {
    reduce_partials<true>(part, G, n, perm_c2, out, accumulate);
}

hipError_t reduce(hipStream_t s, const float* part, int G, int n, bool perm_c2, float* out, bool accumulate) {
    hipLaunchKernelGGL(kws_ct_bwd_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, s, part, G, n, perm_c2 ? 1 : 0, out, accumulate ? 1 : 0);
    return hipGetLastError();
}

hipError_t set_lds_limits() {
    const struct {
        const void* fn;
        int bytes;
    } k[] = {{reinterpret_cast<const void*>(kws_ct_bwd_conv2_fwd_kernel), CONV2_LDS},
             {reinterpret_cast<const void*>(kws_ct_bwd_conv2_dgrad_kernel), CONV2_LDS},
             {reinterpret_cast<const void*>(kws_ct_bwd_conv2_wgrad_kernel), C2W_LDS},
             {reinterpret_cast<const void*>(kws_ct_bwd_conv1_wgrad_kernel), C1W_LDS}};
    for (const auto& e : k) {
        hipError_t r = hipFuncSetAttribute(e.fn, hipFuncAttributeMaxDynamicSharedMemorySize, e.bytes);
        if (r != hipSuccess) return r;
    }
    return hipSuccess;
}

// The recompute (and, with d_dl, the backward) in chunks of at most MAX_CHUNK clips.  Debug mode (d_dl == NULL): conv2's output
// goes to dbg_conv2 and [h | d] to dbg_hidden instead of the workspace, conv1's output and the winners to dbg_conv1 / dbg_win.
int run(kws_ctx* c, const char* fn, const float* d_feat, int B, const float* d_dl, float* d_grad, float* dbg_conv1, int32_t* dbg_win,
        float* dbg_conv2, float* dbg_hidden) {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, set_lds_limits());
    const int C = c->tw.num_classes;
    const CL L(C);
    const int chunk = std::min(B, MAX_CHUNK);
    const int g_conv = std::min(chunk, CONV_GROUPS), g_tail = (chunk + TAIL_CPG - 1) / TAIL_CPG;
    float *yp, *y2, *dz2, *dz1, *hd, *dh, *w2t, *w2u, *part;
    unsigned char* win;
    auto carve = [&](Carver& w) {
        yp = w.per(CT_FLAT);
        y2 = w.per(CT_FLAT);
        dz2 = w.per(CT_FLAT);
        dz1 = w.per(CT_FLAT);
        win = reinterpret_cast<unsigned char*>(w.per(CT_FLAT / 4));  // one byte per pooled position
        hd = w.per(HD);
        dh = w.per(CL::LIN_OUT);
        w2t = w.flat(W2_N);
        w2u = w.flat(W2_N);
        part = w.flat(std::max({(size_t)g_conv * C2W_PART, (size_t)g_tail * tail_part_floats(C), (size_t)g_conv * C1W_PART}));
    };
    Carver need(chunk);
    carve(need);
    // the training workspace is shared with kws_dscnn_backward_f32
    int rc = grow_device_buffer(c, c->d_train_ws, need.floats(), fn, "workspace");
    if (rc) return rc;
    Carver ws(chunk, c->d_train_ws.get());
    carve(ws);
    const float* raw = c->ct_raw;
    hipStream_t s = c->stream;
    hipLaunchKernelGGL(kws_ct_bwd_prep_kernel, dim3(W2_N / 256), dim3(256), 0, s, raw + L.b_w2, w2t, w2u);
    HIP_TRY(c, hipGetLastError());
    const bool debug = d_dl == nullptr;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = std::min(chunk, B - b0);
        const bool acc = b0 > 0;
        const auto [cpg, G] = clip_groups(nb, CONV_GROUPS);
        const int Gt = (nb + TAIL_CPG - 1) / TAIL_CPG;
        const float* feat = d_feat + (size_t)b0 * CT_T * CT_F;
        hipLaunchKernelGGL(kws_ct_bwd_conv1_kernel, dim3(nb), dim3(256), 0, s, feat, raw + L.b_w1, raw + L.b_b1, yp, win,
                           dbg_conv1 ? dbg_conv1 + (size_t)b0 * CH * CT_T * CT_F : nullptr, dbg_win ? dbg_win + (size_t)b0 * CT_FLAT : nullptr);
        HIP_TRY(c, hipGetLastError());
        float* y2c = debug ? dbg_conv2 + (size_t)b0 * CT_FLAT : y2;
        hipLaunchKernelGGL(kws_ct_bwd_conv2_fwd_kernel, dim3(nb), dim3(256), CONV2_LDS, s, yp, w2t, raw + L.b_b2, y2c);
        HIP_TRY(c, hipGetLastError());
        float* hdc = debug ? dbg_hidden + (size_t)b0 * HD : hd;
        hipLaunchKernelGGL(kws_ct_bwd_lin_fwd_kernel, dim3((nb + 31) / 32), dim3(LF_WAVES * 64), 0, s, y2c, raw + L.b_wl, raw + L.b_bl,
                           raw + L.b_wd, raw + L.b_bd, nb, hdc);
        HIP_TRY(c, hipGetLastError());
        if (debug) continue;
        hipLaunchKernelGGL(kws_ct_bwd_tail_kernel, dim3(Gt), dim3(256), 0, s, hd, d_dl + (size_t)b0 * C, raw + L.b_wd, raw + L.b_wf, C, nb, dh, part);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, reduce(s, part, Gt, tail_part_floats(C), false, d_grad + L.b_bl, acc));
        hipLaunchKernelGGL(kws_ct_bwd_lin_kernel, dim3((LIN_TILES + 3) / 4), dim3(256), 0, s, y2, dh, raw + L.b_wl, nb, acc ? 1 : 0, dz2,
                           d_grad + L.b_wl);
        HIP_TRY(c, hipGetLastError());
        hipLaunchKernelGGL(kws_ct_bwd_conv2_wgrad_kernel, dim3(10, G), dim3(512), C2W_LDS, s, dz2, yp, nb, cpg, part);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, reduce(s, part, G, C2W_PART, true, d_grad + L.b_w2, acc));
        hipLaunchKernelGGL(kws_ct_bwd_conv2_dgrad_kernel, dim3(nb), dim3(256), CONV2_LDS, s, dz2, w2u, yp, dz1);
        HIP_TRY(c, hipGetLastError());
        hipLaunchKernelGGL(kws_ct_bwd_conv1_wgrad_kernel, dim3(G), dim3(512), C1W_LDS, s, feat, dz1, win, nb, cpg, part);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, reduce(s, part, G, C1W_PART, false, d_grad + L.b_w1, acc));
    }
    return KWS_OK;
}

}  // namespace
}  // namespace kws

using namespace kws;

#pragma GCC visibility push(default)
extern "C" {

int kws_cnn_trad_backward_f32(kws_ctx* c, const float* d_feat, int B, const float* d_dlogits, float* d_grad) {
    static const char* fn = "kws_cnn_trad_backward_f32";
    KWS_GUARD_BEGIN
    int rc = check_backward_args(c, d_feat, B, d_dlogits, d_grad, fn);
    if (rc) return rc;
    if (!c->cnntrad_ready) return fail(c, KWS_ESTATE, std::string(fn) + ": no model loaded (kws_load_cnn_trad)");
    return run(c, fn, d_feat, B, d_dlogits, d_grad, nullptr, nullptr, nullptr, nullptr);
    KWS_GUARD_END(c, "kws_cnn_trad_backward_f32")
}

int kws_cnn_trad_train_debug_f32(kws_ctx* c, const float* d_feat, int B, float* d_conv1, int32_t* d_winner, float* d_conv2,
                                 float* d_hidden) {
    static const char* fn = "kws_cnn_trad_train_debug_f32";
    KWS_GUARD_BEGIN
    int rc = check_batch(c, d_feat, B, fn);
    if (rc) return rc;
    if (!d_conv1 || !d_winner || !d_conv2 || !d_hidden) return fail(c, KWS_EINVAL, std::string(fn) + ": an output pointer is NULL");
    if (!c->cnntrad_ready) return fail(c, KWS_ESTATE, std::string(fn) + ": no model loaded (kws_load_cnn_trad)");
    return run(c, fn, d_feat, B, nullptr, nullptr, d_conv1, d_winner, d_conv2, d_hidden);
    KWS_GUARD_END(c, "kws_cnn_trad_train_debug_f32")
}

}  // extern "C"
#pragma GCC visibility pop
