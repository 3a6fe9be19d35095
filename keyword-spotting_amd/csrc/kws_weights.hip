// Model weights: the device images of the DS-CNN and of cnn-trad-fpool3 (layouts: kws_internal.h), built on the host by pure
// functions of the state_dict blob, the upload / install behind the kws_load_* entries, the device-side loaders of both models
// (the same image from a device-resident blob) and the image exports.  Every weight bit comes from kws_pack.h.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "kws_ctx.h"
#include "kws_dscnn_units.h"
#include "kws_pack.h"

using namespace kws;

static float max_abs(const float* w, size_t n) {
    float m = 0.f;
    for (size_t i = 0; i < n; ++i) m = std::max(m, std::fabs(w[i]));
    return m;
}
// The bound terms the per-clip activation scales are derived from: max|b| and max over rows of sum |w| (one float64 chain per
// row), rounded up.
static double max_row_sum(const float* w, int rows, size_t row_len) {
    double best = 0.0;
    for (int r = 0; r < rows; ++r) {
        double a = 0.0;
        for (size_t i = 0; i < row_len; ++i) a += std::fabs((double)w[(size_t)r * row_len + i]);
        best = std::max(best, a);
    }
    return best;
}
static float bound_of_row_sum(double best) { return (float)(best * 1.0000002); }  // rounded up

static int check_dscnn_blob(kws_ctx* c, const char* fn, size_t n_floats, int num_classes, int input_channels) {
    if (num_classes < 1 || num_classes > MAX_CLASSES) return fail(c, KWS_EUNSUPPORTED, std::string(fn) + ": num_classes must be in [1, 64]");
    if (input_channels < 1 || input_channels > 64) return fail(c, KWS_EUNSUPPORTED, std::string(fn) + ": input_channels must be in [1, 64]");
    const size_t expect = DscnnLayout(num_classes, input_channels).n_floats;
    if (n_floats != expect) {
        char msg[200];
        snprintf(msg, sizeof msg, "%s: expected %zu floats for %d classes and %d input channel(s), got %zu", fn, expect, num_classes,
                 input_channels, n_floats);
        return fail(c, KWS_EINVAL, msg);
    }
    return KWS_OK;
}

// The statistics of a DS-CNN blob the members DscnnWeights carries by value derive from; kws_ds_load_stats_kernel writes exactly
// this.  m: max|w| of conv1.weight, max|conv1.bias|, then per block b max|pointwise.weight| [2 + b], max|depthwise.bias| [6 + b],
// max|pointwise.bias| [10 + b].  r: the largest row sum of |w| of conv1 [0], of depthwise b [1 + b], of pointwise b [5 + b].  The
// conv1 entries are 0 for more than one input channel (no fused conv1, no bounds).
struct DscnnStats {
    float m[14];
    double r[9];
};
static_assert(sizeof(DscnnStats) == 14 * sizeof(float) + 9 * sizeof(double), "DscnnStats: the read-back is exactly the statistics");

static DscnnStats dscnn_host_stats(const float* blob, const DscnnLayout& L) {
    DscnnStats st{};
    if (L.in_channels == 1) {
        st.m[0] = max_abs(blob, 6400);
        st.m[1] = max_abs(blob + 6400, 64);
        st.r[0] = max_row_sum(blob, 64, 100);
    }
    for (int b = 0; b < 4; ++b) {
        const float* blk = blob + L.b_blk + b * DscnnLayout::BLK;
        st.m[2 + b] = max_abs(blk + DscnnLayout::B_PWW, 4096);
        st.m[6 + b] = max_abs(blk + DscnnLayout::B_DWB, 64);
        st.m[10 + b] = max_abs(blk + DscnnLayout::B_PWB, 64);
        st.r[1 + b] = max_row_sum(blk, 64, 9);
        st.r[5 + b] = max_row_sum(blk + DscnnLayout::B_PWW, 64, 64);
    }
    return st;
}

static int exponent_of_scale(float sw) {  // sw = 2^(ke - 1)
    int ke;
    (void)std::frexp(sw, &ke);
    return ke - 1;
}

// The members DscnnWeights carries by value (its pointers stay null) and the scales of the f16-pair images, from the statistics:
// for the host and the device loader alike.
static DscnnWeights ds_scalars(const DscnnStats& st, const DscnnLayout& L, DscnnScales& sw) {
    DscnnWeights mw{};
    mw.num_classes = L.num_classes;
    mw.in_channels = L.in_channels;
    sw.c1 = 1.f;
    if (L.in_channels == 1) {
        sw.c1 = pow2_scale_of_max(st.m[0]);
        mw.k_c1 = exponent_of_scale(sw.c1);
        mw.c1_abs = bound_of_row_sum(st.r[0]);
        mw.c1_bmax = st.m[1];
    }
    for (int b = 0; b < 4; ++b) {
        sw.pw[b] = pow2_scale_of_max(st.m[2 + b]);
        mw.k_pw[b] = exponent_of_scale(sw.pw[b]);
        mw.dw_abs[b] = bound_of_row_sum(st.r[1 + b]);
        mw.pw_abs[b] = bound_of_row_sum(st.r[5 + b]);
        mw.dw_bmax[b] = st.m[6 + b];
        mw.pw_bmax[b] = st.m[10 + b];
    }
    return mw;
}

// The 23 scalars of the image exports (kws_host_dscnn_image, kws_dscnn_image_read).
static void dscnn_scalars_out(const DscnnWeights& mw, float* scalars) {
    *scalars++ = (float)mw.k_c1;
    for (int b = 0; b < 4; ++b) *scalars++ = (float)mw.k_pw[b];
    *scalars++ = mw.c1_abs;
    *scalars++ = mw.c1_bmax;
    const float* const bounds[4] = {mw.dw_abs, mw.dw_bmax, mw.pw_abs, mw.pw_bmax};
    for (const float* p : bounds)
        for (int b = 0; b < 4; ++b) *scalars++ = p[b];
}

// The device allocation of a DS-CNN model: the image (L.total words, what the exports return) and behind it the unit descriptor
// table of the persistent forward kernel (kws_dscnn_units.h), which no export returns.
static size_t ds_alloc_words(const DscnnLayout& L) {
    static_assert(DS_UNIT_WORDS % 4 == 0, "whole 16-byte rows");
    return L.total + DS_UNIT_WORDS;  // (L.total is a multiple of four words: the table is 16-byte aligned)
}

// The host image h of a checked blob with the unit table behind it, and the members DscnnWeights carries by value (its pointers
// stay null).
static void build_dscnn_image(const float* blob, const DscnnLayout& L, std::vector<float>& h, DscnnWeights& mw) {
    const int input_channels = L.in_channels;
    DscnnScales sw;
    mw = ds_scalars(dscnn_host_stats(blob, L), L, sw);
    h.assign(ds_alloc_words(L), 0.f);
    const float* src = blob;
    memcpy(&h[L.o_raw], blob, L.n_floats * sizeof(float));  // torch layouts, for the composed any-map path (kws_forward_map_f32)
    // conv1.weight [64][C][10][10] -> [ci][tap][cout] (kws_conv1_general_kernel for C > 1, kws_conv1_any_kernel for any map)
    for (int co = 0; co < 64; ++co)
        for (int ci = 0; ci < input_channels; ++ci)
            for (int k = 0; k < 100; ++k) h[L.o_c1g + ((size_t)ci * 100 + k) * 64 + co] = src[((size_t)co * input_channels + ci) * 100 + k];
    if (input_channels == 1)
        for (int co = 0; co < 64; ++co)  // conv1.weight [64][1][10][10] -> [k][cout]
            for (int k = 0; k < 100; ++k) h[L.o_c1w + (size_t)k * 64 + co] = src[co * 100 + k];
    src += L.c1_floats;
    memcpy(&h[L.o_c1b], src, 64 * sizeof(float));
    src += 64;
    for (int b = 0; b < 4; ++b) {
        const float *dw_w = src, *dw_b = src + DscnnLayout::B_DWB, *pw_w = src + DscnnLayout::B_PWW, *pw_b = src + DscnnLayout::B_PWB;
        for (int ch = 0; ch < 64; ++ch) {  // channel PAIRS interleaved, 24 floats per pair: (tap t of ch, of ch + 1) at 2t, the biases at 18, 19
            float* q = &h[L.o_dw + ((size_t)b * 32 + ch / 2) * 24 + (ch & 1)];
            for (int t = 0; t < 9; ++t) q[2 * t] = dw_w[ch * 9 + t];
            q[18] = dw_b[ch];
        }
        for (int co = 0; co < 64; ++co)  // pointwise.weight [cout][cin][1][1] -> [cin][cout]
            for (int ci = 0; ci < 64; ++ci) h[L.o_pww + (size_t)b * 4096 + (size_t)ci * 64 + co] = pw_w[co * 64 + ci];
        memcpy(&h[L.o_pwb + (size_t)b * 64], pw_b, 64 * sizeof(float));
        src += DscnnLayout::BLK;
    }
    memcpy(&h[L.o_fcw], src, (size_t)L.num_classes * 64 * sizeof(float));
    src += (size_t)L.num_classes * 64;
    memcpy(&h[L.o_fcb], src, (size_t)L.num_classes * sizeof(float));
    // conv1 and the pointwise layers as MFMA A operands, both arithmetics (kws_pack.h)
    uint32_t* const img = reinterpret_cast<uint32_t*>(h.data());
    for (size_t i = 0; i < L.n_frag; ++i) ds_pack_fragment(L, blob, i, sw, img);
    for (size_t i = 0; i < DS_UNIT_WORDS; ++i) img[L.total + i] = ds_unit_word(i);
}

// Point the context at the complete device image in c->d_model (layout L); mw holds the values DscnnWeights carries by value.
static void install_dscnn(kws_ctx* c, const DscnnLayout& L, DscnnWeights mw) {
    float* const d = c->d_model.get();
    c->ds_image_words = L.total;
    mw.c1_w = d + L.o_c1w;
    mw.c1_b = d + L.o_c1b;
    mw.dw_w = d + L.o_dw;
    mw.pw_w = d + L.o_pww;
    mw.pw_b = d + L.o_pwb;
    mw.pw_split = reinterpret_cast<const uint32_t*>(d + L.o_split);
    mw.c1_split = reinterpret_cast<const uint32_t*>(d + L.o_c1s);
    mw.pw_pair = reinterpret_cast<const uint32_t*>(d + L.o_pwp);
    mw.c1_pair = reinterpret_cast<const uint32_t*>(d + L.o_c1p);
    mw.fc_w = d + L.o_fcw;
    mw.fc_b = d + L.o_fcb;
    mw.c1_general = d + L.o_c1g;
    mw.raw = d + L.o_raw;
    mw.units = reinterpret_cast<const uint32_t*>(d + L.total);
    c->mw = mw;
    c->model_ready = true;
}

// ---- kws_load_dscnn_device: the same image built on the device from a device-resident blob ---------------------------------------
// DscnnStats in the host's arithmetic: maxima of |w| (exact in any order; fmaxf drops NaN as std::max does there), the row sums of
// max_row_sum as ONE sequential float64 chain per row, in the host's order.  Workgroup q < 14: the maximum m[q]; workgroup 14 + g:
// the 64 rows behind r[g], one thread each.  (extern "C": profilers show the plain names.)
extern "C" __global__ __launch_bounds__(256) void kws_ds_load_stats_kernel(const float* __restrict__ blob, DscnnLayout L, DscnnStats* __restrict__ st) {
    __shared__ float s_m[256];
    __shared__ double s_r[64];
    const int tid = threadIdx.x, q = blockIdx.x;
    const bool one = L.in_channels == 1;
    if (q < 14) {
        size_t off = 0, len = one ? 6400 : 0;  // q == 0: conv1.weight
        if (q == 1) off = 6400, len = one ? 64 : 0;
        if (q >= 2) {
            const int kind = (q - 2) >> 2;  // 0 pointwise.weight, 1 depthwise.bias, 2 pointwise.bias
            off = L.b_blk + (size_t)((q - 2) & 3) * DscnnLayout::BLK + (kind == 0 ? DscnnLayout::B_PWW : kind == 1 ? DscnnLayout::B_DWB : DscnnLayout::B_PWB);
            len = kind == 0 ? 4096 : 64;
        }
        float m = 0.f;
        for (size_t i = tid; i < len; i += 256) m = fmaxf(m, fabsf(blob[off + i]));
        s_m[tid] = m;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w) s_m[tid] = fmaxf(s_m[tid], s_m[tid + w]);
            __syncthreads();
        }
        if (tid == 0) st->m[q] = s_m[0];
        return;
    }
    const int g = q - 14;  // 0: conv1 [64][100]; 1..4: depthwise [64][9]; 5..8: pointwise [64][64]
    if (tid < 64) {
        const size_t len = g == 0 ? (one ? 100 : 0) : g < 5 ? 9 : 64;
        const size_t base = g == 0 ? 0 : L.b_blk + (size_t)((g - 1) & 3) * DscnnLayout::BLK + (g < 5 ? 0 : DscnnLayout::B_PWW);
        const float* w = blob + base + (size_t)tid * len;
        double a = 0.0;
        for (size_t i = 0; i < len; ++i) a += fabs((double)w[i]);
        s_r[tid] = a;
    }
    __syncthreads();
    if (tid == 0) {
        double best = 0.0;
        for (int r = 0; r < 64; ++r) best = fmax(best, s_r[r]);
        st->r[g] = best;
    }
}

// one thread per 8-value fragment of conv1 and the pointwise layers: the host loader's loop body, compiled for the device
extern "C" __global__ __launch_bounds__(256) void kws_ds_load_pack_kernel(const float* __restrict__ blob, DscnnLayout L, DscnnScales sw,
                                                               uint32_t* __restrict__ img) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < L.n_frag) ds_pack_fragment(L, blob, i, sw, img);
}

// One thread per image word outside the fragment blocks the pack kernel writes: the transposed, interleaved and copied float32
// sections of build_dscnn_image, gathered from the blob, the unit table behind the image, and zero wherever the host image keeps its initial zero -- the depthwise
// pad floats, the alignment padding, and for more than one input channel c1_w and conv1's fragment blocks.
extern "C" __global__ __launch_bounds__(256) void kws_ds_load_fill_kernel(const float* __restrict__ blob, DscnnLayout L, uint32_t* __restrict__ img) {
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= L.total) {  // the unit descriptor table behind the image
        if (w - L.total < DS_UNIT_WORDS) img[w] = ds_unit_word(w - L.total);
        return;
    }
    constexpr size_t ZERO = ~(size_t)0;
    const bool one = L.in_channels == 1;
    const size_t cin = (size_t)L.in_channels;
    size_t src = ZERO;
    if (w < L.o_c1b) {  // conv1.weight [64][1][10][10] -> [k][cout]
        if (one) src = (w & 63) * 100 + (w >> 6);
    } else if (w < L.o_dw) {
        src = L.c1_floats + (w - L.o_c1b);
    } else if (w < L.o_pww) {  // channel pairs interleaved: (tap t of ch, of ch + 1) at 2t, the biases at 18, 19, four pad floats
        const size_t u = w - L.o_dw, blk = L.b_blk + u / 768 * DscnnLayout::BLK, e = u % 24, ch = 2 * (u % 768 / 24) + (e & 1);
        if (e < 18) src = blk + ch * 9 + (e >> 1);
        else if (e < 20) src = blk + DscnnLayout::B_DWB + ch;
    } else if (w < L.o_pwb) {  // pointwise.weight [cout][cin] -> [cin][cout]
        const size_t u = w - L.o_pww;
        src = L.b_blk + (u >> 12) * DscnnLayout::BLK + DscnnLayout::B_PWW + (u & 63) * 64 + ((u >> 6) & 63);
    } else if (w < L.o_fcw) {
        const size_t u = w - L.o_pwb;
        src = L.b_blk + (u >> 6) * DscnnLayout::BLK + DscnnLayout::B_PWB + (u & 63);
    } else if (w < L.o_fcb + (size_t)L.num_classes) {  // fc_w | fc_b: contiguous in both
        src = L.b_fcw + (w - L.o_fcw);
    } else if (w < L.o_split) {  // alignment
    } else if (w < L.o_c1s) {
        return;  // pointwise fragments
    } else if (w < L.o_c1g) {
        if (one) return;  // conv1 fragments
    } else if (w < L.o_raw) {  // conv1.weight [64][C][10][10] -> [ci][tap][cout]
        const size_t u = w - L.o_c1g;
        src = ((u & 63) * cin + u / 6400) * 100 + (u % 6400 >> 6);
    } else if (w < L.o_raw + L.n_floats) {
        src = w - L.o_raw;
    } else if (w < L.o_pwp) {  // alignment
    } else if (w < L.o_c1p || one) {
        return;  // f16-pair fragments
    }
    img[w] = src == ZERO ? 0u : __builtin_bit_cast(uint32_t, blob[src]);
}

static int check_cnntrad_blob(kws_ctx* c, const char* fn, size_t n_floats, int num_classes) {
    if (num_classes < 1 || num_classes > MAX_CLASSES) return fail(c, KWS_EUNSUPPORTED, std::string(fn) + ": num_classes must be in [1, 64]");
    const size_t expect = CtLayout(num_classes).n_floats;
    if (n_floats != expect) {
        char msg[160];
        snprintf(msg, sizeof msg, "%s: expected %zu floats for %d classes, got %zu", fn, expect, num_classes, n_floats);
        return fail(c, KWS_EINVAL, msg);
    }
    return KWS_OK;
}

// The members CnnTradWeights carries by value (its pointers stay null) from the layers' statistics, for the host and the device
// loader alike: the scales, the largest row sums of |w1|, |w2| and max|b1|, max|b2|.
static CnnTradWeights ct_scalars(int num_classes, float sw1, float sw2, float swl, double row1, double row2, float b1_max, float b2_max) {
    CnnTradWeights w{};
    w.num_classes = num_classes;
    w.inv_sw1 = 1.f / sw1;
    w.inv_sw2 = 1.f / sw2;
    w.inv_swl = 1.f / swl;
    w.w1_abs = bound_of_row_sum(row1);
    w.w2_abs = bound_of_row_sum(row2);
    w.b1_max = b1_max;
    w.b2_max = b2_max;
    return w;
}

// The host image h of a checked blob and the members CnnTradWeights carries by value (its pointers stay null).
static void build_cnntrad_image(const float* blob, const CtLayout& L, int num_classes, std::vector<uint32_t>& h, CnnTradWeights& w) {
    h.assign(L.total, 0u);
    const float sw1 = pow2_scale_of_max(max_abs(blob + L.b_w1, L.n_c1)), sw2 = pow2_scale_of_max(max_abs(blob + L.b_w2, L.n_c2)),
                swl = pow2_scale_of_max(max_abs(blob + L.b_wl, L.n_lin));
    for (size_t i = 0; i < CtLayout::N_FRAG; ++i) ct_pack_fragment(L, blob, i, sw1, sw2, swl, h.data());
    auto put = [&](size_t off, size_t src, size_t n) { memcpy(&h[off], blob + src, n * sizeof(float)); };
    put(L.o_c1b, L.b_b1, CtLayout::CO);
    put(L.o_c2b, L.b_b2, CtLayout::CO);
    put(L.o_linb, L.b_bl, 32);
    put(L.o_dnn, L.b_wd, L.n_floats - L.b_wd);  // dnn_w | dnn_b | fc_w | fc_b: contiguous in both
    put(L.o_raw, 0, L.n_floats);
    w = ct_scalars(num_classes, sw1, sw2, swl, max_row_sum(blob + L.b_w1, CtLayout::CO, L.n_c1 / CtLayout::CO),
                   max_row_sum(blob + L.b_w2, CtLayout::CO, L.n_c2 / CtLayout::CO), max_abs(blob + L.b_b1, CtLayout::CO),
                   max_abs(blob + L.b_b2, CtLayout::CO));
}

// Point the context at the complete device image in c->d_cnntrad (layout L); w holds the values CnnTradWeights carries by value.
static void install_cnntrad(kws_ctx* c, const CtLayout& L, const CnnTradWeights& w) {
    uint32_t* const d = c->d_cnntrad.get();
    c->ct_image_words = L.total;
    const float* df = reinterpret_cast<const float*>(d);
    c->tw = w;
    c->tw.c1_split = d + L.o_c1s;
    c->tw.c2_split = d + L.o_c2s;
    c->tw.c1_b = df + L.o_c1b;
    c->tw.c2_b = df + L.o_c2b;
    c->tw.lin_split = d + L.o_lin;
    c->tw.lin_b = df + L.o_linb;
    c->tw.dnn_w = df + L.o_dnn;
    c->tw.dnn_b = df + L.o_dnnb;
    c->tw.fc_w = df + L.o_fc;
    c->tw.fc_b = df + L.o_fcb;
    c->tw.c1_h2 = d + L.o_c1h;
    c->tw.c2_h2 = d + L.o_c2h;
    c->tw.lin_h2 = d + L.o_linh;
    c->ct_raw = df + L.o_raw;
    c->cnntrad_ready = true;
}

// ---- kws_load_cnn_trad_device: the same image built on the device from a device-resident blob ----------------------------------
// Statistics in the host's arithmetic: maxima of |w| (exact in any order; fmaxf drops NaN as std::max does there), the row sums of
// max_row_sum as ONE sequential float64 chain per row, in the host's order.  st: float [5] = max|w1|, max|w2|, max|wl|, max|b1|,
// max|b2|, then (8-byte aligned) double [2] = the largest row sums of w1 and w2.  (extern "C": profilers show the plain names.)
extern "C" __global__ __launch_bounds__(1024) void kws_ct_load_stats_kernel(const float* __restrict__ blob, CtLayout L, float* __restrict__ st) {
    __shared__ float s_m[1024];
    __shared__ double s_r[2 * CtLayout::CO];
    const int tid = threadIdx.x, q = blockIdx.x;
    if (q < 5) {  // one maximum per workgroup
        const size_t off = q == 0 ? L.b_w1 : q == 1 ? L.b_w2 : q == 2 ? L.b_wl : q == 3 ? L.b_b1 : L.b_b2;
        const size_t len = q == 0 ? L.n_c1 : q == 1 ? L.n_c2 : q == 2 ? L.n_lin : CtLayout::CO;
        float m = 0.f;
        for (size_t i = tid; i < len; i += 1024) m = fmaxf(m, fabsf(blob[off + i]));
        s_m[tid] = m;
        __syncthreads();
        for (int w = 512; w > 0; w >>= 1) {
            if (tid < w) s_m[tid] = fmaxf(s_m[tid], s_m[tid + w]);
            __syncthreads();
        }
        if (tid == 0) st[q] = s_m[0];
        return;
    }
    // q == 5: row sums (thread r < CO: w1 row r; CO <= r < 2 CO: w2 row r - CO)
    constexpr int CO = (int)CtLayout::CO;
    if (tid < 2 * CO) {
        const bool c2 = tid >= CO;
        const size_t len = (c2 ? L.n_c2 : L.n_c1) / CO;
        const float* w = blob + (c2 ? L.b_w2 : L.b_w1) + (size_t)(tid % CO) * len;
        double a = 0.0;
        for (size_t i = 0; i < len; ++i) a += fabs((double)w[i]);
        s_r[tid] = a;
    }
    __syncthreads();
    if (tid < 2) {
        double best = 0.0;
        for (int r = 0; r < CO; ++r) best = fmax(best, s_r[tid * CO + r]);
        reinterpret_cast<double*>(st + 6)[tid] = best;
    }
}

// one thread per 8-value fragment of the three GEMM layers: the host loader's loop body, compiled for the device
extern "C" __global__ __launch_bounds__(256) void kws_ct_load_pack_kernel(const float* __restrict__ blob, CtLayout L, float sw1, float sw2, float swl,
                                                               uint32_t* __restrict__ img) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < CtLayout::N_FRAG) ct_pack_fragment(L, blob, i, sw1, sw2, swl, img);
}
// The f32 sections (biases, dnn, fc), the alignment padding (zero) in front of the f16-pair images and behind the blob, and the blob.
extern "C" __global__ __launch_bounds__(256) void kws_ct_load_copy_kernel(const float* __restrict__ blob, CtLayout L, uint32_t* __restrict__ img) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= L.n_floats) return;
    const uint32_t u = __builtin_bit_cast(uint32_t, blob[i]);
    img[L.o_raw + i] = u;
    if (i >= L.b_b1 && i < L.b_w2) img[L.o_c1b + i - L.b_b1] = u;
    if (i >= L.b_b2 && i < L.b_wl) img[L.o_c2b + i - L.b_b2] = u;
    if (i >= L.b_bl && i < L.b_wd) img[L.o_linb + i - L.b_bl] = u;
    if (i >= L.b_wd) img[L.o_dnn + i - L.b_wd] = u;  // dnn_w | dnn_b | fc_w | fc_b: contiguous in both
    const size_t pad1 = L.o_dnn + L.n_floats - L.b_wd, pad2 = L.o_raw + L.n_floats;
    if (i < L.o_c1h - pad1) img[pad1 + i] = 0u;
    if (i < L.total - pad2) img[pad2 + i] = 0u;
}

// Shared tail of the host-only image exports: report the size, and say whether out can take the image.
static int export_room(size_t total, const uint32_t* out_words, size_t cap_words, size_t* need_words) {
    if (need_words) *need_words = total;
    return out_words && cap_words < total ? KWS_EINVAL : KWS_OK;
}

#pragma GCC visibility push(default)
extern "C" {

int kws_load_dscnn(kws_ctx* c, const float* blob, size_t n_floats, int num_classes) {
    return kws_load_dscnn_ex(c, blob, n_floats, num_classes, 1);
}

int kws_load_dscnn_ex(kws_ctx* c, const float* blob, size_t n_floats, int num_classes, int input_channels) {
    KWS_GUARD_BEGIN
    if (!c) return KWS_EINVAL;
    if (!blob) return fail(c, KWS_EINVAL, "kws_load_dscnn: blob is NULL");
    int rc = check_dscnn_blob(c, "kws_load_dscnn", n_floats, num_classes, input_channels);
    if (rc) return rc;
    const DscnnLayout L(num_classes, input_channels);
    std::vector<float> h;
    DscnnWeights mw;  // (a local: the context keeps its old model if the upload below fails)
    build_dscnn_image(blob, L, h, mw);

    HIP_TRY(c, hipSetDevice(c->device));
    static_assert(sizeof(float) == sizeof(uint32_t), "image words");
    if (L.total % 4) return fail(c, KWS_EINVAL, "kws_load_dscnn: image size is not a multiple of 16 bytes");
    rc = replace_device_image(c, c->d_model, h.data(), ds_alloc_words(L) * sizeof(float), "kws_load_dscnn");
    if (rc) return rc;
    drop_stream_graph(c);  // a captured push holds the old weight pointers by value
    install_dscnn(c, L, mw);
    return KWS_OK;
    KWS_GUARD_END(c, "kws_load_dscnn")
}

int kws_load_dscnn_device(kws_ctx* c, const float* d_blob, size_t n_floats, int num_classes, int input_channels) {
    static const char* fn = "kws_load_dscnn_device";
    KWS_GUARD_BEGIN
    if (!c) return KWS_EINVAL;
    if (!d_blob) return fail(c, KWS_EINVAL, std::string(fn) + ": blob is NULL");
    int rc = check_dscnn_blob(c, fn, n_floats, num_classes, input_channels);
    if (rc) return rc;
    const DscnnLayout L(num_classes, input_channels);
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->d_ds_stats && !c->d_ds_stats.alloc(sizeof(DscnnStats)))  // (the words this refusal has always had)
        return fail_hip(c, hipGetLastError(), "hipMalloc(&c->d_ds_stats, sizeof(DscnnStats))");
    hipStream_t s = c->stream;
    {
        ProfScope ps(c, KWS_K_DSCNN_LOAD_STATS);
        hipLaunchKernelGGL(kws_ds_load_stats_kernel, dim3(14 + 9), dim3(256), 0, s, d_blob, L, reinterpret_cast<DscnnStats*>(c->d_ds_stats.get()));
    }
    HIP_TRY(c, hipGetLastError());
    DscnnStats st;
    HIP_TRY(c, hipMemcpyAsync(&st, c->d_ds_stats.get(), sizeof st, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    DscnnScales sw;
    const DscnnWeights mw = ds_scalars(st, L, sw);
    // the stream has drained: rewrite an image of this size where it lies, else build a fresh one beside it and swap after success
    DeviceBuffer<float> fresh;
    const bool in_place = c->d_model && c->ds_image_words == L.total;
    if (!in_place && !fresh.alloc(ds_alloc_words(L))) return fail(c, KWS_ENOMEM, std::string(fn) + ": device allocation failed");
    float* const d = in_place ? c->d_model.get() : fresh.get();
    drop_stream_graph(c);  // a captured push holds the old weight pointers and scalars by value
    uint32_t* img = reinterpret_cast<uint32_t*>(d);
    hipError_t e;
    {
        ProfScope ps(c, KWS_K_DSCNN_LOAD_PACK);
        hipLaunchKernelGGL(kws_ds_load_pack_kernel, dim3((unsigned)((L.n_frag + 255) / 256)), dim3(256), 0, s, d_blob, L, sw, img);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        ProfScope ps(c, KWS_K_DSCNN_LOAD_FILL);
        hipLaunchKernelGGL(kws_ds_load_fill_kernel, dim3((unsigned)((ds_alloc_words(L) + 255) / 256)), dim3(256), 0, s, d_blob, L, img);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {  // no mixed image is served: the context's own image may be half rewritten, a fresh one goes with `fresh`
        if (in_place) c->model_ready = false;
        return fail_hip(c, e, fn);
    }
    if (!in_place) c->d_model = std::move(fresh);  // frees the old image
    install_dscnn(c, L, mw);
    return KWS_OK;
    KWS_GUARD_END(c, "kws_load_dscnn_device")
}

int kws_dscnn_image_read(kws_ctx* c, uint32_t* out_words, size_t cap_words, size_t* need_words, float* scalars) {
    if (need_words) *need_words = 0;
    if (!c) return KWS_EINVAL;
    if (!c->model_ready) return fail(c, KWS_ESTATE, "kws_dscnn_image_read: no model loaded (kws_load_dscnn)");
    int rc = export_room(c->ds_image_words, out_words, cap_words, need_words);
    if (rc) return fail(c, rc, "kws_dscnn_image_read: cap_words is below the image's size");
    if (!out_words) return KWS_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(out_words, c->d_model.get(), c->ds_image_words * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (scalars) dscnn_scalars_out(c->mw, scalars);
    return KWS_OK;
}

int kws_load_cnn_trad(kws_ctx* c, const float* blob, size_t n_floats, int num_classes) {
    KWS_GUARD_BEGIN
    if (!c) return KWS_EINVAL;
    if (!blob) return fail(c, KWS_EINVAL, "kws_load_cnn_trad: blob is NULL");
    int rc = check_cnntrad_blob(c, "kws_load_cnn_trad", n_floats, num_classes);
    if (rc) return rc;
    const CtLayout L(num_classes);
    std::vector<uint32_t> h;
    CnnTradWeights w;
    build_cnntrad_image(blob, L, num_classes, h, w);

    HIP_TRY(c, hipSetDevice(c->device));
    rc = replace_device_image(c, c->d_cnntrad, h.data(), L.total * sizeof(uint32_t), "kws_load_cnn_trad");
    if (rc) return rc;
    install_cnntrad(c, L, w);
    return KWS_OK;
    KWS_GUARD_END(c, "kws_load_cnn_trad")
}

int kws_load_cnn_trad_device(kws_ctx* c, const float* d_blob, size_t n_floats, int num_classes) {
    static const char* fn = "kws_load_cnn_trad_device";
    KWS_GUARD_BEGIN
    if (!c) return KWS_EINVAL;
    if (!d_blob) return fail(c, KWS_EINVAL, std::string(fn) + ": blob is NULL");
    int rc = check_cnntrad_blob(c, fn, n_floats, num_classes);
    if (rc) return rc;
    const CtLayout L(num_classes);
    HIP_TRY(c, hipSetDevice(c->device));
    // same size: write into the live image; else build a fresh one beside it and swap after success (a failure lets it go)
    DeviceBuffer<uint32_t> fresh;
    const bool in_place = c->d_cnntrad && c->ct_image_words == L.total;
    if (!in_place) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (!fresh.alloc(L.total)) return fail(c, KWS_ENOMEM, std::string(fn) + ": device allocation failed");
    }
    uint32_t* const d = in_place ? c->d_cnntrad.get() : fresh.get();
    if (!c->d_ct_stats && !c->d_ct_stats.alloc(16))  // (the words this refusal has always had)
        return fail_hip(c, hipGetLastError(), "hipMalloc(reinterpret_cast<void**>(&c->d_ct_stats), 16 * sizeof(float))");
    hipStream_t s = c->stream;
    hipLaunchKernelGGL(kws_ct_load_stats_kernel, dim3(6), dim3(1024), 0, s, d_blob, L, c->d_ct_stats.get());
    HIP_TRY(c, hipGetLastError());
    float st[10];
    HIP_TRY(c, hipMemcpyAsync(st, c->d_ct_stats.get(), sizeof st, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    double rows[2];
    memcpy(rows, st + 6, sizeof rows);
    const float sw1 = pow2_scale_of_max(st[0]), sw2 = pow2_scale_of_max(st[1]), swl = pow2_scale_of_max(st[2]);
    hipLaunchKernelGGL(kws_ct_load_pack_kernel, dim3((unsigned)((CtLayout::N_FRAG + 255) / 256)), dim3(256), 0, s, d_blob, L, sw1, sw2, swl, d);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(kws_ct_load_copy_kernel, dim3((unsigned)((n_floats + 255) / 256)), dim3(256), 0, s, d_blob, L, d);
    HIP_TRY(c, hipGetLastError());
    if (!in_place) c->d_cnntrad = std::move(fresh);  // frees the old image
    install_cnntrad(c, L, ct_scalars(num_classes, sw1, sw2, swl, rows[0], rows[1], st[3], st[4]));
    return KWS_OK;
    KWS_GUARD_END(c, "kws_load_cnn_trad_device")
}

// ---- host-only image exports ---------------------------------------------------------------------------------------------------
int kws_host_dscnn_image(const float* blob, size_t n_floats, int num_classes, int input_channels, uint32_t* out_words, size_t cap_words,
                         size_t* need_words, float* scalars) {
    KWS_GUARD_BEGIN
    if (!blob) return fail(nullptr, KWS_EINVAL, "kws_host_dscnn_image: blob is NULL");
    int rc = check_dscnn_blob(nullptr, "kws_host_dscnn_image", n_floats, num_classes, input_channels);
    if (rc) return rc;
    const DscnnLayout L(num_classes, input_channels);
    rc = export_room(L.total, out_words, cap_words, need_words);
    if (rc || !out_words) return rc;
    std::vector<float> h;
    DscnnWeights mw;
    build_dscnn_image(blob, L, h, mw);
    memcpy(out_words, h.data(), L.total * sizeof(float));
    if (scalars) dscnn_scalars_out(mw, scalars);
    return KWS_OK;
    KWS_GUARD_END(nullptr, "kws_host_dscnn_image")
}

int kws_host_dscnn_units(uint32_t* out_words, size_t cap_words, size_t* need_words, int* unit_base) {
    KWS_GUARD_BEGIN
    int rc = export_room(DS_UNIT_WORDS, out_words, cap_words, need_words);
    if (unit_base)
        for (int n = 0; n <= 4; ++n) unit_base[n] = ds_unit_base(n);
    if (rc || !out_words) return rc;
    for (size_t i = 0; i < DS_UNIT_WORDS; ++i) out_words[i] = ds_unit_word(i);
    return KWS_OK;
    KWS_GUARD_END(nullptr, "kws_host_dscnn_units")
}

int kws_host_cnn_trad_image(const float* blob, size_t n_floats, int num_classes, uint32_t* out_words, size_t cap_words,
                            size_t* need_words, float* scalars) {
    KWS_GUARD_BEGIN
    if (!blob) return fail(nullptr, KWS_EINVAL, "kws_host_cnn_trad_image: blob is NULL");
    int rc = check_cnntrad_blob(nullptr, "kws_host_cnn_trad_image", n_floats, num_classes);
    if (rc) return rc;
    const CtLayout L(num_classes);
    rc = export_room(L.total, out_words, cap_words, need_words);
    if (rc || !out_words) return rc;
    std::vector<uint32_t> h;
    CnnTradWeights w;
    build_cnntrad_image(blob, L, num_classes, h, w);
    memcpy(out_words, h.data(), L.total * sizeof(uint32_t));
    if (scalars) {
        const float s[7] = {w.inv_sw1, w.inv_sw2, w.inv_swl, w.w1_abs, w.b1_max, w.w2_abs, w.b2_max};
        memcpy(scalars, s, sizeof s);
    }
    return KWS_OK;
    KWS_GUARD_END(nullptr, "kws_host_cnn_trad_image")
}

}  // extern "C"
#pragma GCC visibility pop
