// Training the BatchNorm DS-CNN (DepthwiseSeparableConvBN, kws/libs/models.py): the train-mode forward with batch statistics and
// the gradient of a scalar loss with respect to all 38 parameters (kws_dscnn_bn_train_forward_f32, kws_dscnn_bn_backward_f32,
// kws_dscnn_bn_train_debug_f32, include/kws_hip.h).  The entries take the parameters as a device blob (DscnnBnLayout, kws_pack.h)
// and neither need nor touch the context's loaded model.
//
// Forward, nine times conv -> BatchNorm (-> ReLU), every stage kept in the context's training workspace:
//   z0 = conv1(x) + b                      kws_conv1_any_pre_kernel (kws_dsblock.hip)            a0 = relu(BN(z0))
//   z  = depthwise_k(a_{k-1}) + b          kws_dsblock_depthwise_kernel                          u  = BN(z)          (no ReLU)
//   z  = pointwise_k(u) + b, ring = b      kws_dsblock_pointwise_pre_kernel                      a_k = relu(BN(z))   (ring counted)
//   logits = fc(mean of a_4)               kws_pool_fc_kernel
// A BatchNorm layer is three launches:
//   kws_bn_stats_kernel      sum z and sum z^2 per channel in float64: wave = channel, lanes walk the positions of the clips of one
//                            clip group (kws_train.h) -> partial row g
//   kws_bn_finish_kernel     the G partial rows summed in a fixed order (16 segments of consecutive rows, then the 16 segment sums),
//                            mean, biased variance, 1 / sqrt(var + eps) -> the layer's coefficients (and d_stats)
//   kws_bn_apply_kernel      y = (z - mean) * rstd * gamma + beta, ReLU where one follows
// Backward (recompute, not save: the call redoes the forward above, which is deterministic, so it sees the forward call's bits), per
// BatchNorm layer, with dy^ = dy [a > 0] where a ReLU follows:
//   kws_bn_bwd_stats_kernel  S1 = sum dy^, S2 = sum dy^ x^ in float64, partial rows as above
//   kws_bn_bwd_finish_kernel g_beta = S1, g_gamma = S2, and gamma * rstd, S1 / N, S2 / N for the next kernel
//   kws_bn_bwd_apply_kernel  dz = gamma * rstd * (dy^ - S1 / N - x^ S2 / N), written over z
// and dz goes through the plain model's convolution backward (kws_dscnn_bwd.hip): kws_bwd_pointwise_dz_kernel,
// kws_bwd_depthwise_kernel, kws_bwd_conv1_dz_kernel, kws_bwd_fc_kernel, kws_bwd_reduce_kernel.
//
// Deterministic: no float atomics; the clip groups depend on B only and every reduction runs in a fixed order, so the same inputs
// give bit-identical logits, statistics and gradients on every call.  Statistics span the batch, so there is no chunking: the
// whole batch lives in the workspace (kws_host_dscnn_bn_max_batch).
//
// Memory is written with plain vector stores only; there is no inline assembly in this unit.
#include <cmath>

#include "kws_train.h"

namespace kws {
namespace {

using DL = DscnnLayout;
using BL = DscnnBnLayout;
constexpr int N_BN = BL::N_BN;
constexpr int FIN_SEG = 16;                          // row segments of the finish kernels
constexpr size_t PART64_FLOATS = (size_t)BWD_MAX_GROUPS * CH * 2 * 2;  // [G][64][2] doubles, counted in floats
constexpr size_t WS_LIMIT = (size_t)1 << 31;         // floats of workspace

// conv1.weight [co][tap] -> [tap][co], the layout kws_conv1_any_kernel reads
__global__ __launch_bounds__(256) void kws_bn_c1_transpose_kernel(const float* __restrict__ w, float* __restrict__ wt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < DL::C1_W) wt[(i % DL::C1_TAPS) * CH + i / DL::C1_TAPS] = w[i];
}

// Grid (16 channel quads, G clip groups); wave w of workgroup (cq, g) owns channel 4 cq + w over the group's clips, its lanes walk
// the n positions of a plane.  The 64 lane sums are added in lane order.
__device__ __forceinline__ void write_partial(double (&s_red)[4][2][64], double s0, double s1, int wv, int lane, int c, int g,
                                              double* __restrict__ part) {
    s_red[wv][0][lane] = s0;
    s_red[wv][1][lane] = s1;
    __syncthreads();
    if (lane < 2) {
        double t = 0.0;
        for (int l = 0; l < 64; ++l) t += s_red[wv][lane][l];
        part[((size_t)g * CH + c) * 2 + lane] = t;
    }
}

__global__ __launch_bounds__(256) void kws_bn_stats_kernel(const float* __restrict__ z, int n, int nb, int cpg, double* __restrict__ part) {
    __shared__ double s_red[4][2][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = 4 * blockIdx.x + wv, g = blockIdx.y;
    double s = 0.0, ss = 0.0;
    const int b_end = group_end(g, cpg, nb);
    for (int b = g * cpg; b < b_end; ++b) {
        const float* zp = z + ((size_t)b * CH + c) * n;
        for (int p = lane; p < n; p += 64) {
            const double v = (double)zp[p];
            s += v;
            ss += v * v;
        }
    }
    write_partial(s_red, s, ss, wv, lane, c, g, part);
}

// One workgroup of 64 channels x FIN_SEG segments: thread (c, seg) sums its consecutive partial rows in order, thread (c, 0) the
// segment sums in order -> sum[0], sum[1] of channel c.
__device__ __forceinline__ bool sum_partials(const double* __restrict__ part, int G, double (&sum)[2]) {
    __shared__ double s_seg[FIN_SEG][2][64];
    const int c = threadIdx.x & 63, seg = threadIdx.x >> 6;
    const int per = (G + FIN_SEG - 1) / FIN_SEG, g1 = min(G, (seg + 1) * per);
    double a = 0.0, b = 0.0;
    for (int g = seg * per; g < g1; ++g) {
        a += part[((size_t)g * CH + c) * 2];
        b += part[((size_t)g * CH + c) * 2 + 1];
    }
    s_seg[seg][0][c] = a;
    s_seg[seg][1][c] = b;
    __syncthreads();
    if (seg != 0) return false;
    sum[0] = sum[1] = 0.0;
    for (int k = 0; k < FIN_SEG; ++k) {
        sum[0] += s_seg[k][0][c];
        sum[1] += s_seg[k][1][c];
    }
    return true;
}

// coef: [mean 64 | rstd 64] of the layer; stats (may be NULL): [mean 64 | unbiased variance 64]
__global__ __launch_bounds__(64 * FIN_SEG) void kws_bn_finish_kernel(const double* __restrict__ part, int G, double N, float eps,
                                                                     float* __restrict__ coef, float* __restrict__ stats) {
    double sum[2];
    if (!sum_partials(part, G, sum)) return;
    const int c = threadIdx.x;
    const double mean = sum[0] / N;
    const double var = fmax(sum[1] / N - mean * mean, 0.0);
    coef[c] = (float)mean;
    coef[CH + c] = (float)(1.0 / sqrt(var + (double)eps));
    if (stats) {
        stats[c] = (float)mean;
        stats[CH + c] = (float)(var * (N / (N - 1.0)));
    }
}

// y = (z - mean) * rstd * gamma + beta over [planes][n], plane = clip * 64 + channel
template <bool RELU>
__global__ __launch_bounds__(256) void kws_bn_apply_kernel(const float* __restrict__ z, const float* __restrict__ coef,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, int n,
                                                           size_t total, float* __restrict__ y) {
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)((i / (size_t)n) & 63);
        const float xh = (z[i] - coef[c]) * coef[CH + c];
        const float v = xh * gamma[c] + beta[c];
        y[i] = RELU ? fmaxf(v, 0.f) : v;
    }
}

// dy of plane pl, position q: dy[pl * dy_plane + q * dy_q] (the last block: one value per plane, dy_plane = 1, dy_q = 0)
template <bool RELU>
__global__ __launch_bounds__(256) void kws_bn_bwd_stats_kernel(const float* __restrict__ dy, int dy_plane, int dy_q,
                                                               const float* __restrict__ a, const float* __restrict__ z,
                                                               const float* __restrict__ coef, int n, int nb, int cpg,
                                                               double* __restrict__ part) {
    __shared__ double s_red[4][2][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = 4 * blockIdx.x + wv, g = blockIdx.y;
    const float mean = coef[c], rstd = coef[CH + c];
    double s1 = 0.0, s2 = 0.0;
    const int b_end = group_end(g, cpg, nb);
    for (int b = g * cpg; b < b_end; ++b) {
        const size_t pl = (size_t)b * CH + c;
        const float* dp = dy + pl * dy_plane;
        const float* zp = z + pl * n;
        const float* ap = a + pl * n;
        for (int p = lane; p < n; p += 64) {
            float d = dp[(size_t)p * dy_q];
            if (RELU && !(ap[p] > 0.f)) d = 0.f;
            const float xh = (zp[p] - mean) * rstd;
            s1 += (double)d;
            s2 += (double)d * (double)xh;
        }
    }
    write_partial(s_red, s1, s2, wv, lane, c, g, part);
}

// g_gamma = S2, g_beta = S1; bcoef: [gamma * rstd 64 | S1 / N 64 | S2 / N 64]
__global__ __launch_bounds__(64 * FIN_SEG) void kws_bn_bwd_finish_kernel(const double* __restrict__ part, int G, double N,
                                                                         const float* __restrict__ coef, const float* __restrict__ gamma,
                                                                         float* __restrict__ g_gamma, float* __restrict__ g_beta,
                                                                         float* __restrict__ bcoef) {
    double sum[2];
    if (!sum_partials(part, G, sum)) return;
    const int c = threadIdx.x;
    g_beta[c] = (float)sum[0];
    g_gamma[c] = (float)sum[1];
    bcoef[c] = gamma[c] * coef[CH + c];
    bcoef[CH + c] = (float)(sum[0] / N);
    bcoef[2 * CH + c] = (float)(sum[1] / N);
}

// dz = gamma * rstd * (dy^ - S1 / N - x^ S2 / N); dz may be z itself (an element is read before it is written, by one thread)
template <bool RELU>
__global__ __launch_bounds__(256) void kws_bn_bwd_apply_kernel(const float* __restrict__ dy, int dy_plane, int dy_q,
                                                               const float* __restrict__ a, const float* z,
                                                               const float* __restrict__ coef, const float* __restrict__ bcoef, int n,
                                                               size_t total, float* dz) {
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t pl = i / (size_t)n;
        const int q = (int)(i - pl * n), c = (int)(pl & 63);
        float d = dy[pl * dy_plane + (size_t)q * dy_q];
        if (RELU && !(a[i] > 0.f)) d = 0.f;
        const float xh = (z[i] - coef[c]) * coef[CH + c];
        dz[i] = bcoef[c] * ((d - bcoef[CH + c]) - xh * bcoef[2 * CH + c]);
    }
}

int elementwise_blocks(size_t total) { return (int)std::min<size_t>((total + 255) / 256, (size_t)1 << 20); }

// ---- the workspace and the two passes ---------------------------------------------------------------------------------------
struct BnStages {
    double* part64;       // [G][64][2] partial sums of a BatchNorm layer
    float* coef;          // [9][mean 64 | rstd 64]
    float* bcoef;         // the backward's coefficients of the layer at hand
    float* c1t;           // conv1.weight as [tap][co]
    float *z0, *a0;       // conv1: pre-activation, relu(BN)
    float *zdw[N_BLOCKS], *u[N_BLOCKS];  // depthwise: pre-activation, BN
    float *zpw[N_BLOCKS], *a[N_BLOCKS];  // pointwise (ring included): pre-activation, relu(BN)
    float *gin, *gdw, *dy4, *part;       // the backward's gradients and partial rows
};

void carve(Carver& w, const DscnnMap& m, BnStages& st) {
    st.part64 = reinterpret_cast<double*>(w.flat(PART64_FLOATS));  // first: 8-byte aligned
    st.coef = w.flat(N_BN * 2 * CH);
    st.bcoef = w.flat(3 * CH);
    st.c1t = w.flat(DL::C1_W);
    st.part = w.flat(std::min<size_t>(w.clips, BWD_MAX_GROUPS) * C1_PART);  // the widest row is conv1's
    st.z0 = w.per(CH * m.P(0));
    st.a0 = w.per(CH * m.P(0));
    for (int k = 0; k < N_BLOCKS; ++k) {
        st.zdw[k] = w.per(CH * m.P(k));
        st.u[k] = w.per(CH * m.P(k));
        st.zpw[k] = w.per(CH * m.Q(k));
        st.a[k] = w.per(CH * m.Q(k));
    }
    st.gin = w.per(CH * m.P(N_BLOCKS - 1));
    st.gdw = w.per(CH * m.P(N_BLOCKS - 1));
    st.dy4 = w.per(CH);
}

// The largest batch whose workspace stays within WS_LIMIT floats, at most COMPOSED_MAX_CLIPS (grid.z of the pointwise kernel).
int max_batch(int T, int F) {
    const DscnnMap m(T, F);
    BnStages st;
    Carver one(BWD_MAX_GROUPS);  // the fixed part at its largest
    carve(one, m, st);
    if (one.fixed + one.per_clip > WS_LIMIT) return 0;
    return (int)std::min<size_t>((WS_LIMIT - one.fixed) / one.per_clip, COMPOSED_MAX_CLIPS);
}

struct BnCall {
    kws_ctx* c;
    const float* prm;
    BL L;
    DscnnMap m;
    int B, T, F, cpg, G;
    float eps;
    BnStages st;
    hipStream_t s;
    BnCall(kws_ctx* c_, const float* prm_, int C, int B_, int T_, int F_, float eps_)
        : c(c_), prm(prm_), L(C), m(T_, F_), B(B_), T(T_), F(F_), eps(eps_), s(c_->stream) {
        const ClipGroups cg = clip_groups(B, BWD_MAX_GROUPS);
        cpg = cg.cpg, G = cg.G;
    }
    double count(size_t n) const { return (double)B * (double)n; }
    float* coef(int layer) const { return st.coef + (size_t)layer * 2 * CH; }

    // BatchNorm layer `layer` over z [B][64][n] -> y (ReLU where one follows)
    hipError_t norm(int layer, const float* z, size_t n, bool relu_out, float* y, float* d_stats) {
        hipLaunchKernelGGL(kws_bn_stats_kernel, dim3(CH / 4, G), dim3(256), 0, s, z, (int)n, B, cpg, st.part64);
        hipLaunchKernelGGL(kws_bn_finish_kernel, dim3(1), dim3(64 * FIN_SEG), 0, s, st.part64, G, count(n), eps, coef(layer),
                           d_stats ? d_stats + (size_t)layer * 2 * CH : nullptr);
        const size_t total = (size_t)B * CH * n;
        hipLaunchKernelGGL(relu_out ? kws_bn_apply_kernel<true> : kws_bn_apply_kernel<false>, dim3(elementwise_blocks(total)), dim3(256), 0,
                           s, z, coef(layer), prm + L.gamma(layer), prm + L.beta(layer), (int)n, total, y);
        return hipGetLastError();
    }

    // the train-mode forward, every stage kept
    hipError_t forward(const float* feat, float* d_stats) {
        hipLaunchKernelGGL(kws_bn_c1_transpose_kernel, dim3((DL::C1_W + 255) / 256), dim3(256), 0, s, prm, st.c1t);
        hipError_t e = launch_conv1_any(s, feat, B, 1, T, F, st.c1t, prm + DL::C1_W, st.z0, false);
        if (e == hipSuccess) e = norm(0, st.z0, m.P(0), true, st.a0, d_stats);
        for (int k = 0; k < N_BLOCKS && e == hipSuccess; ++k) {
            const float* blk = prm + L.plain.block(k);
            e = launch_dsblock_depthwise(s, k ? st.a[k - 1] : st.a0, B, CH, m.H(k), m.W(k), blk, blk + DL::B_DWB, 3, 1, 1, st.zdw[k]);
            if (e == hipSuccess) e = norm(2 * k + 1, st.zdw[k], m.P(k), false, st.u[k], d_stats);
            if (e == hipSuccess)
                e = launch_dsblock_pointwise(s, st.u[k], B, CH, m.H(k), m.W(k), blk + DL::B_PWW, blk + DL::B_PWB, CH, 1, st.zpw[k], false);
            if (e == hipSuccess) e = norm(2 * k + 2, st.zpw[k], m.Q(k), true, st.a[k], d_stats);
        }
        return e;
    }

    // BatchNorm layer `layer` backwards: dy (and a, where a ReLU follows) -> g_gamma, g_beta, and dz over z
    hipError_t norm_backward(int layer, const float* dy, int dy_plane, int dy_q, const float* a, float* z, size_t n, float* d_grad) {
        const bool relu_out = a != nullptr;
        if (!a) a = z;  // not read
        hipLaunchKernelGGL(relu_out ? kws_bn_bwd_stats_kernel<true> : kws_bn_bwd_stats_kernel<false>, dim3(CH / 4, G), dim3(256), 0, s, dy,
                           dy_plane, dy_q, a, z, coef(layer), (int)n, B, cpg, st.part64);
        hipLaunchKernelGGL(kws_bn_bwd_finish_kernel, dim3(1), dim3(64 * FIN_SEG), 0, s, st.part64, G, count(n), coef(layer),
                           prm + L.gamma(layer), d_grad + L.gamma(layer), d_grad + L.beta(layer), st.bcoef);
        const size_t total = (size_t)B * CH * n;
        hipLaunchKernelGGL(relu_out ? kws_bn_bwd_apply_kernel<true> : kws_bn_bwd_apply_kernel<false>, dim3(elementwise_blocks(total)),
                           dim3(256), 0, s, dy, dy_plane, dy_q, a, z, coef(layer), st.bcoef, (int)n, total, z);
        return hipGetLastError();
    }

    hipError_t backward(const float* feat, const float* d_dlogits, float* d_grad) {
        constexpr int LAST = N_BLOCKS - 1;
        const int C = L.plain.num_classes;
        hipError_t e = launch_bwd_fc(s, st.a[LAST], d_dlogits, prm + L.plain.b_fcw, (int)m.Q(LAST), C, B, cpg, G, st.dy4, st.part);
        if (e == hipSuccess) e = bwd_reduce(s, st.part, G, fc_part(C), d_grad + L.plain.b_fcw);
        for (int k = LAST; k >= 0 && e == hipSuccess; --k) {
            const float* blk = prm + L.plain.block(k);
            float* gk = d_grad + L.plain.block(k);
            const int H = m.H(k), W = m.W(k), Q = (int)m.Q(k), P = (int)m.P(k);
            e = k == LAST ? norm_backward(2 * k + 2, st.dy4, 1, 0, st.a[k], st.zpw[k], Q, d_grad)
                          : norm_backward(2 * k + 2, st.gin, Q, 1, st.a[k], st.zpw[k], Q, d_grad);
            if (e == hipSuccess) e = launch_bwd_pointwise_dz(s, st.zpw[k], st.u[k], blk + DL::B_PWW, H, W, B, cpg, G, st.gdw, st.part);
            if (e == hipSuccess) e = bwd_reduce(s, st.part, G, PW_PART, gk + DL::B_PWW);
            if (e == hipSuccess) e = norm_backward(2 * k + 1, st.gdw, P, 1, nullptr, st.zdw[k], P, d_grad);
            if (e == hipSuccess) e = launch_bwd_depthwise(s, st.zdw[k], k ? st.a[k - 1] : st.a0, blk, H, W, B, cpg, G, st.gin, st.part);
            if (e == hipSuccess) e = bwd_reduce(s, st.part, G, DW_PART, gk);
        }
        const int P0 = (int)m.P(0);
        if (e == hipSuccess) e = norm_backward(0, st.gin, P0, 1, st.a0, st.z0, P0, d_grad);
        if (e == hipSuccess) e = launch_bwd_conv1_dz(s, st.z0, feat, T, F, m.H1, m.W1, B, cpg, G, st.part);
        if (e == hipSuccess) e = bwd_reduce(s, st.part, G, C1_PART, d_grad);
        return e;
    }
};

// What the three entries check, in this order, all on the host before any allocation or launch; then the workspace.
int prepare(kws_ctx* c, const char* fn, const float* d_params, size_t n_floats, int num_classes, const float* d_feat, int B, int T, int F,
            float eps, BnStages& st) {
    if (!d_params) return fail(c, KWS_EINVAL, std::string(fn) + ": d_params is NULL");
    if (num_classes < 1 || num_classes > MAX_CLASSES) return fail(c, KWS_EUNSUPPORTED, std::string(fn) + ": num_classes must be in [1, 64]");
    if (n_floats != BL(num_classes).n_floats)
        return fail(c, KWS_EINVAL, std::string(fn) + ": n_floats must be 25664 + 65 * num_classes + 1152 (one input channel, nine BatchNorm layers)");
    if (!(eps > 0.f) || !std::isfinite(eps)) return fail(c, KWS_EINVAL, std::string(fn) + ": eps must be positive and finite");
    int rc = check_dscnn_map(c, fn, T, F);
    if (rc) return rc;
    const DscnnMap m(T, F);
    if ((size_t)B * m.P(0) < 2)
        return fail(c, KWS_EINVAL, std::string(fn) + ": batch statistics need more than one value per channel (B * H1 * W1 >= 2)");
    if (B > max_batch(T, F))
        return fail(c, KWS_EUNSUPPORTED, std::string(fn) + ": B exceeds kws_host_dscnn_bn_max_batch(T, F): batch statistics are not chunked");
    HIP_TRY(c, hipSetDevice(c->device));
    Carver need(B);
    carve(need, m, st);
    rc = grow_device_buffer(c, c->d_train_ws, need.floats(), fn, "workspace");
    if (rc) return rc;
    Carver ws(B, c->d_train_ws.get());
    carve(ws, m, st);
    return KWS_OK;
}

int train_forward(kws_ctx* c, const char* fn, const float* d_params, size_t n_floats, int num_classes, const float* d_feat, int B, int T,
                  int F, float eps, float* d_logits, int32_t* d_label, float* d_layers, float* d_stats) {
    int rc = check_batch(c, d_feat, B, fn);
    if (rc) return rc;
    if (!d_logits) return fail(c, KWS_EINVAL, std::string(fn) + ": d_logits is NULL");
    BnCall call(c, d_params, std::max(1, std::min(num_classes, MAX_CLASSES)), B, T, F, eps);
    rc = prepare(c, fn, d_params, n_floats, num_classes, d_feat, B, T, F, eps, call.st);
    if (rc) return rc;
    HIP_TRY(c, call.forward(d_feat, d_stats));
    const DscnnMap& m = call.m;
    const BnStages& st = call.st;
    HIP_TRY(c, launch_pool_fc(c->stream, st.a[N_BLOCKS - 1], B, (int)m.Q(N_BLOCKS - 1), d_params + call.L.plain.b_fcw,
                              d_params + call.L.plain.b_fcb, num_classes, d_logits, d_label));
    if (d_layers) {
        size_t off = 0;
        for (int k = -1; k < N_BLOCKS; ++k) {
            const size_t n = (size_t)B * CH * (k < 0 ? m.P(0) : m.Q(k));
            HIP_TRY(c, hipMemcpyAsync(d_layers + off, k < 0 ? st.a0 : st.a[k], n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
            off += n;
        }
    }
    return KWS_OK;
}

}  // namespace
}  // namespace kws

using namespace kws;

#pragma GCC visibility push(default)
extern "C" {

int kws_host_dscnn_bn_max_batch(int T, int F) {
    if (T < 6 || F < 6 || (size_t)(T + 4) * (F + 4) * sizeof(float) > 160 * 1024) return 0;
    return max_batch(T, F);
}

int kws_dscnn_bn_train_forward_f32(kws_ctx* c, const float* d_params, size_t n_floats, int num_classes, const float* d_feat, int B, int T,
                                   int F, float eps, float* d_logits, int32_t* d_label, float* d_stats) {
    KWS_GUARD_BEGIN
    return train_forward(c, "kws_dscnn_bn_train_forward_f32", d_params, n_floats, num_classes, d_feat, B, T, F, eps, d_logits, d_label,
                         nullptr, d_stats);
    KWS_GUARD_END(c, "kws_dscnn_bn_train_forward_f32")
}

int kws_dscnn_bn_train_debug_f32(kws_ctx* c, const float* d_params, size_t n_floats, int num_classes, const float* d_feat, int B, int T,
                                 int F, float eps, float* d_logits, int32_t* d_label, float* d_layers, float* d_stats) {
    KWS_GUARD_BEGIN
    if (c && !d_layers) return fail(c, KWS_EINVAL, "kws_dscnn_bn_train_debug_f32: d_layers is NULL");
    return train_forward(c, "kws_dscnn_bn_train_debug_f32", d_params, n_floats, num_classes, d_feat, B, T, F, eps, d_logits, d_label,
                         d_layers, d_stats);
    KWS_GUARD_END(c, "kws_dscnn_bn_train_debug_f32")
}

int kws_dscnn_bn_backward_f32(kws_ctx* c, const float* d_params, size_t n_floats, int num_classes, const float* d_feat, int B, int T, int F,
                              float eps, const float* d_dlogits, float* d_grad) {
    static const char* fn = "kws_dscnn_bn_backward_f32";
    KWS_GUARD_BEGIN
    int rc = check_backward_args(c, d_feat, B, d_dlogits, d_grad, fn);
    if (rc) return rc;
    BnCall call(c, d_params, std::max(1, std::min(num_classes, MAX_CLASSES)), B, T, F, eps);
    rc = prepare(c, fn, d_params, n_floats, num_classes, d_feat, B, T, F, eps, call.st);
    if (rc) return rc;
    HIP_TRY(c, call.forward(d_feat, nullptr));
    HIP_TRY(c, call.backward(d_feat, d_dlogits, d_grad));
    return KWS_OK;
    KWS_GUARD_END(c, "kws_dscnn_bn_backward_f32")
}

}  // extern "C"
#pragma GCC visibility pop
