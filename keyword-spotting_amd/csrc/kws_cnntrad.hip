// cnn-trad-fpool3 forward for gfx950 (MI355X) -- a build-defined member of the model zoo (SURVEY.md section 8 f-4;
// the reference only names it, test.py:80).  Sainath & Parada's "cnn-trad-fpool3" on the reference's [1,99,10] MFCC
// map with SAME padding:
//   conv1  1->64, 20 (time) x 8 (freq), pad 9/10 x 3/4, ReLU          -> 64 x 99 x 10
//   max-pool 1 x 3 over frequency, stride 3 (floor)                    -> 64 x 99 x 3
//   conv2  64->64, 10 x 4, pad 4/5 x 1/2, ReLU                          -> 64 x 99 x 3
//   flatten (channel-major, 19 008) -> Linear 32 -> Linear 128 + ReLU -> Linear C ; argmax (first maximum wins)
// 59.4 M multiply-adds per clip, 82 % of them in conv2.
//
// Kernel A (one 512-thread workgroup per clip): both convolutions as implicit GEMMs on the bf16 matrix pipe with
// the exact three-way bf16 split of kws_split_mfma.h (f32-grade results).  conv1 gathers its f32 im2col operand
// from the zero-padded map in LDS and splits it on the fly; its ReLU'd, frequency-pooled output is written to LDS
// ALREADY split, as three bf16 planes [position][input channel], so that conv2's B operand -- eight consecutive
// input channels of one input position -- is a single aligned ds_read_b128 per piece with no VALU work in the
// loop.  Taps that fall into the padding read a zero region.  conv2's pre-split weights (983 KB) stream from L2.
// Kernel B: the dense tail, 16 clips per workgroup; its 19008 -> 32 layer is a GEMM on the same matrix-pipe path.
// Behind the kernels and their launchers: the one conv + dense host sequence, the model's ModelOps and its C entry points.
#include <type_traits>

#include "kws_ctx.h"
#include "kws_split_mfma.h"

namespace kws {
namespace {

constexpr int CT_T = 99, CT_F = 10, CT_FP = 3, CT_P2 = CT_T * CT_FP;  // 297 pooled positions
constexpr int CT_K1H = 20, CT_K1W = 8, CT_K2H = 10, CT_K2W = 4;
constexpr int XP_H = CT_T + CT_K1H - 1, XP_W = CT_F + CT_K1W - 1;      // 118 x 17 zero-padded conv1 input
constexpr int XP_BYTES = 8192;                                          // >= 118*17*4, keeps the planes 16-byte aligned
constexpr int PL_STRIDE = CH * 2 + 16;                                  // bytes per position: 128 of channels + 16 of padding, so
                                                                        // that the 16 lanes of a ds_read_b128 group (consecutive
                                                                        // positions) fall on 16 different 16-byte bank groups
                                                                        // (at 128 they collide eight ways: measured LDS-bound)
// Taps that fall into the padding read zeros.  A single zero row would sit on the banks of one of the valid lanes
// of the same instruction (two-way conflict on three of four taps: 27 % of conv2's LDS cycles by the counters);
// instead every plane ends in a 256-byte-aligned zero region and a padding lane reads it at the offset its natural
// address has modulo 256 -- the bank slot that lane would have used anyway, which no valid lane touches.
constexpr int PL_ZERO_OFF = (CT_P2 * PL_STRIDE + 255) / 256 * 256;      // 43 008
constexpr int PL_ZERO_BYTES = 256 + 3 * 32 + 32;                        // natural offset mod 256, + channel block, + read width
constexpr int PLANE_BYTES = PL_ZERO_OFF + PL_ZERO_BYTES;                // one bf16 piece plane [pos][64 cin + pad] + zero region
constexpr int CT_LDS_BYTES = XP_BYTES + 3 * PLANE_BYTES;                // 138 368
constexpr int WIN_PLANE_BYTES = XP_H * CT_F * 16;                       // 18 880: f16-pair arithmetic, conv1's input windows per piece
constexpr int CT_NW = 8, CT_NT = CT_NW * 64;
constexpr int C1_TILES = CT_T / 3;                                      // 33 tiles of 3 time rows x 10 bins (30 of 32 columns)
constexpr int C2_TILES = (CT_P2 + 31) / 32;                             // 10
static_assert(CT_T % 3 == 0, "conv1 tiles hold whole time rows");
static_assert(C2_TILES == 10 && CT_NW == 8, "conv2 tile groups {3,3,2,2} x 2 channel tiles assume 10 tiles on 8 wavefronts");
static_assert(XP_BYTES % 256 == 0 && PL_STRIDE % 16 == 0, "the zero regions rely on 256-byte bank periodicity");
static_assert(XP_H * XP_W * 4 <= XP_BYTES, "padded input does not fit its LDS slot");

__device__ __forceinline__ float lane_up(float v) { return from_lane_above(v); }

// ---- f16-pair arithmetic (H2 = true, the default; kws_set_cnn_trad_math) ----------------------------------------
// Every f32 GEMM operand v, first scaled by a power of two s into f16's range, is written as hi + lo' * 2^-11 with
// hi = f16(v s) (round to nearest) and lo' = f16((v s - hi) * 2^11): 22 significant bits.  f16 x f16 products are exact in
// the matrix core's f32 accumulate; hi*hi goes to one accumulator, hi*lo' + lo'*hi to a second one that is scaled by
// 2^-11 at the end (the dropped lo*lo term is <= 2^-22 of the product).  THREE v_mfma_f32_32x32x16_f16 per f32 k-block
// instead of the six bf16 ones of the three-way split, two operand pieces to load instead of three -- this model is
// bound by the matrix pipe, so that is the lever -- for logits that differ from float64 by what torch's own f32 forward
// differs by (tests/test_cnntrad_f16_pair_sim.py).  Range: weights are scaled per layer at load time so that max |w| s < 2^15;
// activations per CLIP, from rigorous bounds known before the values exist: M0 = max |feature| of the clip (measured
// while staging), |conv1 out| <= max_c sum|w1[c]| M0 + max|b1|, |conv2 out| <= max_c sum|w2[c]| * that + max|b2|.  The
// bounds are loose by 2^4..2^7 per layer; f16 keeps 11 bits down to 2^-14 and the scaled values top out below 2^15, so a
// value keeps full relative precision down to 2^-29 of its layer's bound and an absolute 2^-40 of it below that: no
// overflow for any input, no precision cliff.  All scalings are by powers of two (exact).
__device__ __forceinline__ void split_pair(float even, float odd, uint32_t& hi, uint32_t& lo) {
    const halfx2 h = {(_Float16)even, (_Float16)odd};
    const halfx2 l = {(_Float16)((even - (float)h[0]) * 2048.f), (_Float16)((odd - (float)h[1]) * 2048.f)};
    hi = __builtin_bit_cast(uint32_t, h);
    lo = __builtin_bit_cast(uint32_t, l);
}
__device__ __forceinline__ void split2(const float (&y)[8], uintx4& hi, uintx4& lo) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t h, l;
        split_pair(y[2 * i], y[2 * i + 1], h, l);
        hi[i] = h;
        lo[i] = l;
    }
}
constexpr float LO_UNSCALE = 1.f / 2048.f;
template <bool H2>
__global__ __launch_bounds__(CT_NT) void kws_cnntrad_conv_kernel(CnnTradWeights w, const float* __restrict__ feat, int B,
                                                                 float* __restrict__ conv_out, float* __restrict__ clip_scale) {
    // clip b of [B][99][10]
#define CT_SOURCE_PROLOGUE      \
    const int clip = blockIdx.x; \
    if (clip >= B) return;
#define CT_FEAT(i) feat[(size_t)clip * (CT_T * CT_F) + i]
#include "kws_cnntrad_conv_body.h"
#undef CT_SOURCE_PROLOGUE
#undef CT_FEAT
}

// Windows of recordings read in place (kws_forward_cnn_trad_windows_f32): workgroup b of a chunk takes window i = sw.first + b --
// window i % wpr of recording i / wpr, 99 consecutive rows of that recording's [F][10] frame array -- and writes slot b of the
// workspace.  The base is wave-uniform and formed in 64 bits from factors that fit 32 (R * F <= 2^28 frames).
template <bool H2>
__global__ __launch_bounds__(CT_NT) void kws_cnntrad_conv_windows_kernel(CnnTradWeights w, const float* __restrict__ frames, CtWindows sw, int n,
                                                                         float* __restrict__ conv_out, float* __restrict__ clip_scale) {
#define CT_SOURCE_PROLOGUE                                                                               \
    const int clip = blockIdx.x;                                                                          \
    if (clip >= n) return;                                                                                \
    const unsigned win_i = sw.first + (unsigned)clip, win_r = win_i / sw.wpr;                             \
    const float* feat = frames + ((size_t)win_r * sw.row_floats + (size_t)(win_i - win_r * sw.wpr) * sw.win_floats);
#define CT_FEAT(i) feat[i]
#include "kws_cnntrad_conv_body.h"
#undef CT_SOURCE_PROLOGUE
#undef CT_FEAT
}

// The streams' windows read from the feature ring behind kws_stream_frame_kernel (kws_stream_push_cnn_trad_i16): stream s of
// [S][99][10]; window row t is ring row (head + t) mod 99, head = ((*hops + 1 - lag) mod 99 + 99) mod 99 -- what
// kws_dscnn_fwd_kernel's two-launch route derives.  Float i of the window is ring float (i + 10 head) mod 990.
template <bool H2>
__global__ __launch_bounds__(CT_NT) void kws_cnntrad_conv_ring_kernel(CnnTradWeights w, const float* __restrict__ ring, const int* __restrict__ hops,
                                                                      int lag, int S, float* __restrict__ conv_out, float* __restrict__ clip_scale) {
#define CT_SOURCE_PROLOGUE                                                       \
    const int clip = blockIdx.x;                                                  \
    if (clip >= S) return;                                                        \
    const int rot = ((((*hops + 1 - lag) % CT_T) + CT_T) % CT_T) * CT_F;          \
    const float* feat = ring + (size_t)clip * (CT_T * CT_F);
#define CT_FEAT(i) feat[(i) + rot < CT_T * CT_F ? (i) + rot : (i) + rot - CT_T * CT_F]
#include "kws_cnntrad_conv_body.h"
#undef CT_SOURCE_PROLOGUE
#undef CT_FEAT
}

// Kernel B: Linear(19008 -> 32) ; Linear(32 -> 128) + ReLU ; Linear(128 -> C) ; argmax.
// The first layer is a [clips x 19008] x [19008 x 32] GEMM: 16 clips per workgroup (in the 32 MFMA rows), D[clip][output] on the bf16
// matrix pipe with the exact split (activations split on the fly, weights pre-split as B operands), K divided
// among the 12 wavefronts of the workgroup (99 k-blocks of 16 each) and the partial sums combined through LDS.
// It reads the 76 KB per clip that kernel A wrote: HBM-bound, so loads run three k-blocks ahead in every wave.
constexpr int CT_FLAT = CH * CT_P2;  // 19008
constexpr int CT_LIN = 32, CT_DNN = 128;
constexpr int DN_WAVES = 12, DN_KB = CT_FLAT / 16 / DN_WAVES;  // 99 k-blocks per wavefront
constexpr int DN_CLIPS = 16;  // clips per workgroup: 4096 clips = 256 workgroups, one per CU (32 leaves half the CUs idle: 2.31 vs 2.27 ms for the model; 8 is slower again, 2.36)
static_assert(DN_KB * DN_WAVES * 16 == CT_FLAT, "K must divide evenly among the wavefronts");
template <bool H2>
__global__ __launch_bounds__(DN_WAVES * 64) void kws_cnntrad_dense_kernel(CnnTradWeights w, const float* __restrict__ conv_out,
                                                                          const float* __restrict__ clip_scale, int B,
                                                                          float* __restrict__ logits, int32_t* __restrict__ label) {
    constexpr int NP = H2 ? 2 : 3;
    __shared__ float part[DN_WAVES][32 * 32];  // partial D of every wavefront, [clip][output]
    __shared__ float h1[32][CT_LIN];
    __shared__ float h2[32][CT_DNN];
    __shared__ float lg[32][MAX_CLASSES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, half = lane >> 5, col = lane & 31;
    const int clip0 = blockIdx.x * DN_CLIPS;
    {
        // A operand: lane (row = clip slot col, half) holds x[clip][16kb + 8half .. +7]
        // the 32 MFMA rows hold DN_CLIPS clips (the upper rows repeat them: same addresses, L1 hits, results unused)
        const int aslot = col % DN_CLIPS;
        const int aclip = clip0 + aslot < B ? clip0 + aslot : B - 1;
        const float4* xa = reinterpret_cast<const float4*>(conv_out + (size_t)aclip * CT_FLAT + (size_t)wv * DN_KB * 16 + 8 * half);
        // B operand: pre-split weights [kb][piece][lane]
        const uintx4* wb = reinterpret_cast<const uintx4*>(H2 ? w.lin_h2 : w.lin_split) + (size_t)wv * DN_KB * NP * 64 + lane;
        floatx16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, accx = acc;
        const float s2 = H2 ? clip_scale[aclip] : 1.f;  // H2: the clip's power-of-two scale into f16's range (written by the conv kernel)
        constexpr int DEPTH = 3;
        float4 xr[DEPTH][2];
        uintx4 wr[DEPTH][NP];
        auto load = [&](int kb, int slot) {
            xr[slot][0] = xa[kb * 4];
            xr[slot][1] = xa[kb * 4 + 1];
#pragma unroll
            for (int pc = 0; pc < NP; ++pc) wr[slot][pc] = wb[(kb * NP + pc) * 64];
        };
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) load(d, d);
        for (int kb0 = 0; kb0 < DN_KB; kb0 += DEPTH) {
#pragma unroll
            for (int d = 0; d < DEPTH; ++d) {
                const int kb = kb0 + d;
                if constexpr (H2) {
                    const float y[8] = {xr[d][0].x * s2, xr[d][0].y * s2, xr[d][0].z * s2, xr[d][0].w * s2,
                                        xr[d][1].x * s2, xr[d][1].y * s2, xr[d][1].z * s2, xr[d][1].w * s2};
                    uintx4 ah, al;
                    split2(y, ah, al);
                    const uintx4 bh = wr[d][0], bl = wr[d][NP - 1];
                    if (kb + DEPTH < DN_KB) load(kb + DEPTH, d);
                    accx = mfma_f16(ah, bl, accx);
                    acc = mfma_f16(ah, bh, acc);
                    accx = mfma_f16(al, bh, accx);
                } else {
                    const float y[8] = {xr[d][0].x, xr[d][0].y, xr[d][0].z, xr[d][0].w, xr[d][1].x, xr[d][1].y, xr[d][1].z, xr[d][1].w};
                    uintx4 ah, am, al;
                    split3(y, ah, am, al);
                    const uintx4 bh = wr[d][0], bm = wr[d][1], bl = wr[d][NP - 1];
                    if (kb + DEPTH < DN_KB) load(kb + DEPTH, d);
                    acc = mfma_bf16(al, bh, acc);
                    acc = mfma_bf16(ah, bl, acc);
                    acc = mfma_bf16(am, bm, acc);
                    acc = mfma_bf16(am, bh, acc);
                    acc = mfma_bf16(ah, bm, acc);
                    acc = mfma_bf16(ah, bh, acc);
                }
            }
        }
        if constexpr (H2) acc += accx * LO_UNSCALE;
#pragma unroll
        for (int r = 0; r < 16; ++r) part[wv][row_of(r, half) * 32 + col] = acc[r];  // D row = clip slot, column = output
    }
    __syncthreads();
    for (int i = tid; i < DN_CLIPS * CT_LIN; i += DN_WAVES * 64) {
        float a = H2 ? 0.f : w.lin_b[i & 31];
#pragma unroll
        for (int k = 0; k < DN_WAVES; ++k) a += part[k][i];
        if constexpr (H2) {  // back to true units: the clip's scale and the layer's weight scale are powers of two
            const int cl = clip0 + (i >> 5) < B ? clip0 + (i >> 5) : B - 1;
            a = a * (w.inv_swl / clip_scale[cl]) + w.lin_b[i & 31];
        }
        h1[i >> 5][i & 31] = a;
    }
    __syncthreads();
    for (int i = tid; i < DN_CLIPS * CT_DNN; i += DN_WAVES * 64) {
        const int s = i / CT_DNN, j = i % CT_DNN;
        float a = w.dnn_b[j];
        for (int k = 0; k < CT_LIN; ++k) a = fmaf(h1[s][k], w.dnn_w[j * CT_LIN + k], a);
        h2[s][j] = a > 0.f ? a : 0.f;
    }
    __syncthreads();
    const int C = w.num_classes;
    for (int i = tid; i < DN_CLIPS * C; i += DN_WAVES * 64) {
        const int s = i / C, c = i % C;
        float a = w.fc_b[c];
        for (int k = 0; k < CT_DNN; ++k) a = fmaf(h2[s][k], w.fc_w[c * CT_DNN + k], a);
        lg[s][c] = a;
        if (clip0 + s < B) logits[(size_t)(clip0 + s) * C + c] = a;
    }
    __syncthreads();
    if (tid < DN_CLIPS && clip0 + tid < B && label) {
        int arg = 0;
        float best = lg[tid][0];
        for (int c = 1; c < C; ++c)
            if (lg[tid][c] > best) {
                best = lg[tid][c];
                arg = c;
            }
        label[clip0 + tid] = arg;
    }
}

}  // namespace

constexpr int CT_LDS_BYTES_H2 = XP_BYTES + 2 * PLANE_BYTES + 2 * WIN_PLANE_BYTES;  // 132 800

hipError_t cnntrad_init_device() {
    const void* const three[] = {reinterpret_cast<const void*>(kws_cnntrad_conv_kernel<false>),
                                 reinterpret_cast<const void*>(kws_cnntrad_conv_windows_kernel<false>),
                                 reinterpret_cast<const void*>(kws_cnntrad_conv_ring_kernel<false>)};
    const void* const pair[] = {reinterpret_cast<const void*>(kws_cnntrad_conv_kernel<true>),
                                reinterpret_cast<const void*>(kws_cnntrad_conv_windows_kernel<true>),
                                reinterpret_cast<const void*>(kws_cnntrad_conv_ring_kernel<true>)};
    for (int k = 0; k < 3; ++k) {
        hipError_t e = hipFuncSetAttribute(three[k], hipFuncAttributeMaxDynamicSharedMemorySize, CT_LDS_BYTES);
        if (e == hipSuccess) e = hipFuncSetAttribute(pair[k], hipFuncAttributeMaxDynamicSharedMemorySize, CT_LDS_BYTES_H2);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// One launch per source kind and arithmetic: the six instantiations cnntrad_init_device has prepared.
template <bool H2>
static void conv_launch(hipStream_t s, const CnnTradWeights& w, const CtSource& src, int n, float* d_conv_ws, float* scale) {
    constexpr int lds = H2 ? CT_LDS_BYTES_H2 : CT_LDS_BYTES;
    const dim3 grid(n), block(CT_NT);
    if (src.kind == CtSource::CLIPS)
        hipLaunchKernelGGL(kws_cnntrad_conv_kernel<H2>, grid, block, lds, s, w, src.maps, n, d_conv_ws, scale);
    else if (src.kind == CtSource::WINDOWS)
        hipLaunchKernelGGL(kws_cnntrad_conv_windows_kernel<H2>, grid, block, lds, s, w, src.maps, src.windows, n, d_conv_ws, scale);
    else
        hipLaunchKernelGGL(kws_cnntrad_conv_ring_kernel<H2>, grid, block, lds, s, w, src.maps, src.hops, src.lag, n, d_conv_ws, scale);
}
hipError_t launch_cnntrad_conv(hipStream_t s, const CnnTradWeights& w, const CtSource& src, int n, float* d_conv_ws, bool f16_pair) {
    float* scale = d_conv_ws + (size_t)n * CT_FLAT;
    if (f16_pair)
        conv_launch<true>(s, w, src, n, d_conv_ws, scale);
    else
        conv_launch<false>(s, w, src, n, d_conv_ws, scale);
    return hipGetLastError();
}

hipError_t launch_cnntrad_dense(hipStream_t s, const CnnTradWeights& w, const float* d_conv_ws, int B, float* d_logits,
                                int32_t* d_label, bool f16_pair) {
    const float* scale = d_conv_ws + (size_t)B * CT_FLAT;
    const dim3 grid((B + DN_CLIPS - 1) / DN_CLIPS), block(DN_WAVES * 64);
    if (f16_pair)
        hipLaunchKernelGGL(kws_cnntrad_dense_kernel<true>, grid, block, 0, s, w, d_conv_ws, scale, B, d_logits, d_label);
    else
        hipLaunchKernelGGL(kws_cnntrad_dense_kernel<false>, grid, block, 0, s, w, d_conv_ws, scale, B, d_logits, d_label);
    return hipGetLastError();
}

}  // namespace kws

using namespace kws;

// ---- behind the C ABI: conv from `src`, then dense, over n slots of the context workspace: n * 19008 floats of conv2 output, then one scale per slot
// (f16-pair arithmetic).  Logits [n][C] and labels [n] (or NULL); fn names the caller in the allocation's refusal.
static int ct_reserve(kws_ctx* c, const char* fn, int n) { return grow_conv_ws(c, (size_t)n * 64 * 297 + (size_t)n, fn); }
static int ct_conv_dense(kws_ctx* c, const char* fn, const CtSource& src, int n, float* d_logits, int32_t* d_label) {
    int rc = ct_reserve(c, fn, n);
    if (rc) return rc;
    const bool pair = c->cnntrad_math == KWS_CT_F16_PAIR;
    {
        ProfScope ps(c, KWS_K_CNNTRAD_CONV);
        HIP_TRY(c, launch_cnntrad_conv(c->stream, c->tw, src, n, c->d_conv_ws.get(), pair));
    }
    {
        ProfScope ps(c, KWS_K_CNNTRAD_DENSE);
        HIP_TRY(c, launch_cnntrad_dense(c->stream, c->tw, c->d_conv_ws.get(), n, d_logits, d_label, pair));
    }
    return KWS_OK;
}

// The model as the host flows see it (ModelOps, kws_ctx.h); the recording flows and the fused clip entries ask the same of it.
static int ct_scan_check(kws_ctx* c, const char* fn) {
    if (!c->fe_ready || !c->cnntrad_ready) return fail(c, KWS_ESTATE, std::string(fn) + ": front end or model not configured (kws_load_cnn_trad)");
    return check_ref_map(c, fn, ": the kernels are built for a 99 x 10 feature map");
}
static int ct_model_check(kws_ctx* c, const char* fn) {
    return c->cnntrad_ready ? KWS_OK : fail(c, KWS_ESTATE, std::string(fn) + ": no model loaded (kws_load_cnn_trad)");
}
static int ct_push_check(kws_ctx* c, const char* fn) {
    if (int rc = ct_model_check(c, fn)) return rc;
    return check_ref_map(c, fn, ": the kernels are built for a 99 x 10 feature map");
}
static int ct_classes(const kws_ctx* c) { return c->tw.num_classes; }

// B contiguous clips: the product entry, its parity aid and the fused clip entries.
static int ct_forward(kws_ctx* c, const float* d_feat, int B, float* d_logits, int32_t* d_label, const char* fn) {
    int rc = check_batch(c, d_feat, B, fn);
    if (rc) return rc;
    if (!d_logits) return fail(c, KWS_EINVAL, std::string(fn) + ": d_logits is NULL");
    if ((rc = ct_model_check(c, fn))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    return ct_conv_dense(c, fn, {CtSource::CLIPS, d_feat, {}, nullptr, 0}, B, d_logits, d_label);
}

// The R * W windows of a frame array [R][F][10], read in place, in chunks of CT_WINDOW_CHUNK: per chunk one conv and one dense launch
// that writes logits and labels at the chunk's offset.  The caller has checked the arguments and the limits (2^28 frames, 2^30 windows).
static int ct_windows(kws_ctx* c, const char* fn, const float* d_frames, int R, int F, int W, int hop_frames, float* d_logits,
                      int32_t* d_label) {
    const long long n = (long long)R * W;
    const int C = c->tw.num_classes;
    for (long long i0 = 0; i0 < n; i0 += CT_WINDOW_CHUNK) {
        const int nb = n - i0 < CT_WINDOW_CHUNK ? (int)(n - i0) : CT_WINDOW_CHUNK;
        const CtWindows sw = {(unsigned)i0, (unsigned)W, (unsigned)F * (unsigned)IN_F, (unsigned)hop_frames * (unsigned)IN_F};
        int rc = ct_conv_dense(c, fn, {CtSource::WINDOWS, d_frames, sw, nullptr, 0}, nb, d_logits + (size_t)i0 * C, d_label ? d_label + i0 : nullptr);
        if (rc) return rc;
    }
    return KWS_OK;
}

// The launches of a push: the frame kernel, then every stream's window of the feature ring, rotated by the hop counter it has
// advanced.  The workspace is there before the frame launch: a push that cannot allocate leaves the set as it was.
static int ct_ring_push(kws_ctx* c, const char* fn, const int16_t* d_hop, float* d_logits, int32_t* d_label) {
    if (int rc = ct_reserve(c, fn, c->n_streams)) return rc;
    HIP_TRY(c, stream_enqueue_frame(c, d_hop, true));
    return ct_conv_dense(c, fn, {CtSource::RING, c->d_feat_ring.get(), {}, c->d_hops.get(), frames_lag(c->fp)}, c->n_streams, d_logits, d_label);
}

static const ModelOps kCnnTradOps = {ct_scan_check, ct_scan_check, ct_push_check, ct_classes, ct_forward, ct_windows, ct_ring_push};
namespace kws {
const ModelOps& model_ops_cnn_trad() { return kCnnTradOps; }
}  // namespace kws

#pragma GCC visibility push(default)
extern "C" {

int kws_forward_cnn_trad_f32(kws_ctx* c, const float* d_feat, int B, float* d_logits, int32_t* d_label) {
    return ct_forward(c, d_feat, B, d_logits, d_label, "kws_forward_cnn_trad_f32");
}

int kws_forward_cnn_trad_debug_f32(kws_ctx* c, const float* d_feat, int B, float* d_logits, int32_t* d_label, float* d_conv2,
                                   float* d_clip_scale) {
    const char* fn = "kws_forward_cnn_trad_debug_f32";
    if (c && !d_conv2) return fail(c, KWS_EINVAL, std::string(fn) + ": d_conv2 is NULL");
    int rc = ct_forward(c, d_feat, B, d_logits, d_label, fn);
    if (rc) return rc;
    const size_t n = (size_t)B * 64 * 297;
    HIP_TRY(c, hipMemcpyAsync(d_conv2, c->d_conv_ws.get(), sizeof(float) * n, hipMemcpyDeviceToDevice, c->stream));
    if (d_clip_scale && c->cnntrad_math == KWS_CT_F16_PAIR)
        HIP_TRY(c, hipMemcpyAsync(d_clip_scale, c->d_conv_ws.get() + n, sizeof(float) * (size_t)B, hipMemcpyDeviceToDevice, c->stream));
    return KWS_OK;
}

int kws_set_cnn_trad_math(kws_ctx* c, int math) {
    if (!c) return KWS_EINVAL;
    if (math != KWS_CT_F16_PAIR && math != KWS_CT_BF16_TRIPLE) return fail(c, KWS_EINVAL, "kws_set_cnn_trad_math: unknown arithmetic");
    c->cnntrad_math = math;
    return KWS_OK;
}

int kws_host_cnn_trad_window_chunk(void) { return CT_WINDOW_CHUNK; }

int kws_forward_cnn_trad_windows_f32(kws_ctx* c, const float* d_frames, int R, int F, int hop_frames, float* d_logits, int32_t* d_label) {
    const char* fn = "kws_forward_cnn_trad_windows_f32";
    if (!c) return KWS_EINVAL;
    if (!d_frames || !d_logits) return fail(c, KWS_EINVAL, std::string(fn) + ": d_frames / d_logits is NULL");
    if (R < 1 || hop_frames < 1) return fail(c, KWS_EINVAL, std::string(fn) + ": R and hop_frames must be positive");
    if (F < IN_T) return fail(c, KWS_EINVAL, std::string(fn) + ": a recording of fewer than 99 frames has no window");
    if (int rc = ct_model_check(c, fn)) return rc;
    const int W = (F - IN_T) / hop_frames + 1;
    if ((unsigned long long)R * F > (1ull << 28) || (unsigned long long)R * W > (1ull << 30))
        return fail(c, KWS_EUNSUPPORTED, std::string(fn) + ": more than 2^28 frames or 2^30 windows in one call");
    HIP_TRY(c, hipSetDevice(c->device));
    return ct_windows(c, fn, d_frames, R, F, W, hop_frames, d_logits, d_label);
}

}  // extern "C"
#pragma GCC visibility pop
