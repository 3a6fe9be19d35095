// The scaffold the training back ends share (kws_dscnn_bwd.hip, kws_cnntrad_bwd.hip, kws_dscnn_bn.hip): the conventions of their
// long sums, the clip-group plan behind the deterministic reduction and its reduce body, the f32 MFMA helpers, the DS-CNN's
// backward launches as the BatchNorm path calls them, the workspace carver and the argument check of the backward entries.  The
// state_dict layouts come from kws_pack.h.
#pragma once
#include <algorithm>
#include <string>

#include "kws_ctx.h"
#include "kws_pack.h"

namespace kws {

// Sums over the positions of a map are taken in runs of RUN terms, each started from zero and added to a running total.
// One chain per accumulator over block 4's Q / 4 = 2772 positions per wave at 156 x 252 missed the 4x torch-f32 bound on
// dsconv4.pointwise.bias (2.1x) and, through the pooled mean, on fc.weight (1.1x).
constexpr int RUN = 64;
constexpr int PART_RUN = 32;  // partial rows per run of the reduce kernels

// ---- the f32-input MFMA v_mfma_f32_32x32x2_f32 -------------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ void zero16(f32x16& v) {
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = 0.f;
}
// D layout of the 32x32 MFMAs: register r of a lane in half-wave `half` is row (r & 3) + 8 (r >> 2) + 4 half, column lane & 31
__device__ __forceinline__ int drow(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// ---- clip groups and the deterministic reduction -------------------------------------------------------------------------------
// No float atomics: a chunk of nb clips is split into G contiguous groups of cpg = ceil(nb / cap) clips; the workgroup(s) of group
// g accumulate its clips g * cpg .. group_end - 1 in order and write partial row g ([G][n] floats), and a reduce kernel sums the
// G rows in a fixed order.  G and cpg depend on nb and the cap only.
struct ClipGroups {
    int cpg, G;
};
inline ClipGroups clip_groups(int nb, int cap) {
    const int cpg = (nb + cap - 1) / cap;
    return {cpg, (nb + cpg - 1) / cpg};
}
__device__ __forceinline__ int group_end(int g, int cpg, int nb) { return min(nb, (g + 1) * cpg); }

// The body of a reduce kernel, one thread per column: out[o(i)] (+)= sum over g < G of part[g][i], runs of PART_RUN rows summed in
// order and the run sums added in order (chains of at most 32 + 32 additions at G = 1024).  o(i) = i, except that PERM_C2 with
// perm_c2 set takes the columns below CtLayout::N_C2 as cnn-trad conv2 partials [kk][co][ci] and writes the blob's [co][ci][kk].
template <bool PERM_C2>
__device__ __forceinline__ void reduce_partials(const float* __restrict__ part, int G, int n, int perm_c2, float* __restrict__ out,
                                                int accumulate) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int g0 = 0; g0 < G; g0 += PART_RUN) {
        const int g1 = min(G, g0 + PART_RUN);
        float t = 0.f;
        for (int g = g0; g < g1; ++g) t += part[(size_t)g * n + i];
        s += t;
    }
    if constexpr (PERM_C2) {
        int o = i;
        if (perm_c2 && i < CtLayout::N_C2) o = ((i >> 6) & 63) * (CtLayout::N_C2 / 64) + (i & 63) * 40 + (i >> 12);
        out[o] = accumulate ? out[o] + s : s;
    } else {
        out[i] = accumulate ? out[i] + s : s;
    }
}

// ---- the DS-CNN's backward launches (kws_dscnn_bwd.hip), shared with the train-mode BatchNorm path (kws_dscnn_bn.hip) -----------
constexpr int BWD_MAX_GROUPS = 1024;                                   // partial rows per stage and chunk
constexpr int PW_PART = DscnnLayout::PW_W + DscnnLayout::CO;           // pointwise.weight [co][ci] | pointwise.bias
constexpr int DW_PART = DscnnLayout::DW_W + DscnnLayout::CO;           // depthwise.weight [c][3][3] | depthwise.bias
constexpr int C1_PART = DscnnLayout::C1_W + DscnnLayout::CO;           // conv1.weight [co][10][10] | conv1.bias
constexpr int fc_part(int C) { return C * DscnnLayout::CO + C; }       // fc.weight [C][64] | fc.bias
// Each writes G = clip_groups(nb, BWD_MAX_GROUPS).G partial rows to `part`; bwd_reduce sums them in fixed order into `out`.
// The *_dz launches take a finished dloss/d(pre-activation) where the plain model's kernels mask dloss/d(output) by output > 0.
hipError_t bwd_reduce(hipStream_t s, const float* part, int G, int n, float* out);
hipError_t launch_bwd_fc(hipStream_t s, const float* y4, const float* dl, const float* fc_w, int Q4, int C, int nb, int cpg, int G,
                         float* dy4, float* part);
hipError_t launch_bwd_pointwise_dz(hipStream_t s, const float* dz, const float* xdw, const float* w, int H, int W, int nb, int cpg, int G,
                                   float* dxdw, float* part);
hipError_t launch_bwd_depthwise(hipStream_t s, const float* dxdw, const float* xin, const float* w, int H, int W, int nb, int cpg, int G,
                                float* dxin, float* part);
hipError_t launch_bwd_conv1_dz(hipStream_t s, const float* dz, const float* x, int T, int F, int H1, int W1, int nb, int cpg, int G,
                               float* part);

// ---- host side --------------------------------------------------------------------------------------------------------------
// Hands out consecutive float ranges of a workspace for `clips` clips.  Run the same carving lines twice: without a base they
// only count (per_clip, and floats() to size the buffer), with the base they assign the pointers.
struct Carver {
    size_t clips;
    float* base;
    size_t per_clip = 0, fixed = 0;  // handed out so far: floats per clip, floats that do not scale with the clips
    explicit Carver(size_t clips_, float* base_ = nullptr) : clips(clips_), base(base_) {}
    size_t floats() const { return clips * per_clip + fixed; }
    float* next() const { return base ? base + floats() : nullptr; }
    float* per(size_t n) { float* p = next(); per_clip += n; return p; }  // n floats for every clip
    float* flat(size_t n) { float* p = next(); fixed += n; return p; }    // n floats
};

// What the backward entries check first, in this order.
inline int check_backward_args(kws_ctx* c, const float* d_feat, int B, const float* d_dlogits, const float* d_grad, const char* fn) {
    int rc = check_batch(c, d_feat, B, fn);
    if (rc) return rc;
    if (!d_dlogits) return fail(c, KWS_EINVAL, std::string(fn) + ": d_dlogits is NULL");
    if (!d_grad) return fail(c, KWS_EINVAL, std::string(fn) + ": d_grad is NULL");
    return KWS_OK;
}

}  // namespace kws
