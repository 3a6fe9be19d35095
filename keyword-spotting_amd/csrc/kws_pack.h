// The arithmetic that decides, bit for bit, what the MFMA kernels read as weights -- one copy for the host loaders
// (kws_weights.hip) and for the device loaders' kernels: the two exact splits of eight weights into one lane's operand
// fragment, the power-of-two layer scale, and the blob / image layouts of the DS-CNN and of cnn-trad-fpool3 with their fragment
// orders.
// Compiled with -ffp-contract=off on both sides: the expressions below must stay as they are.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

namespace kws {

// A fragment block is [piece][lane 64][4 words]: the eight values of lane l, piece p, are the words (p * 64 + l) * 4 .. + 3,
// value 2i in the low half of word i and 2i + 1 in the high half.  The packers take the address of piece 0's words.
constexpr size_t FRAG_PIECE = 64 * 4;

// Exact bf16 hi/mid/lo pieces: piece p = the top 16 bits of what pieces 0 .. p-1 left over (kws_split_mfma.h).
__host__ __device__ inline void pack_bf16_triple(const float (&v)[8], uint32_t* dst) {
    uint32_t w[3][4] = {};
    for (int j = 0; j < 8; ++j) {
        float r = v[j];
        for (int p = 0; p < 3; ++p) {
            const uint32_t u = __builtin_bit_cast(uint32_t, r) & 0xffff0000u;
            r -= __builtin_bit_cast(float, u);
            w[p][j >> 1] |= (u >> 16) << (16 * (j & 1));
        }
    }
    for (int p = 0; p < 3; ++p)
        for (int i = 0; i < 4; ++i) dst[p * FRAG_PIECE + i] = w[p][i];
}

// f16-pair pieces of x = v * scale (the layer's power of two): hi = f16(x) (round to nearest), lo = f16((x - hi) * resid).
// resid = 1: the DS-CNN's PLAIN flavour (kws_dscnn_stages.h); resid = 2^11: cnn-trad-fpool3's (kws_cnntrad.hip, split_pair).
__host__ __device__ inline void pack_f16_pair(const float (&v)[8], float scale, float resid, uint32_t* dst) {
    uint32_t w[2][4] = {};
    for (int j = 0; j < 8; ++j) {
        const float x = v[j] * scale;
        const _Float16 h = (_Float16)x;
        const _Float16 l = (_Float16)((x - (float)h) * resid);
        w[0][j >> 1] |= (uint32_t)__builtin_bit_cast(uint16_t, h) << (16 * (j & 1));
        w[1][j >> 1] |= (uint32_t)__builtin_bit_cast(uint16_t, l) << (16 * (j & 1));
    }
    for (int p = 0; p < 2; ++p)
        for (int i = 0; i < 4; ++i) dst[p * FRAG_PIECE + i] = w[p][i];
}

// The power of two s with m * s < 2^15 for m = max|w| of a layer (1 for an all-zero or non-finite layer).
__host__ __device__ inline float pow2_scale_of_max(float m) {
    if (!(m > 0.f) || !std::isfinite(m)) return 1.f;
    int e;
    (void)std::frexp(m, &e);  // m = f * 2^e, f in [0.5, 1): m < 2^e
    return std::ldexp(1.f, std::max(-100, std::min(100, 15 - e)));
}

// DS-CNN.  The blob (b_*: floats) is the 20 state_dict tensors in order: conv1.weight [64][C_in][10][10] | conv1.bias [64] | four
// blocks of BLK floats (depthwise.weight [64][9] | depthwise.bias [64] | pointwise.weight [64][64] | pointwise.bias [64]) | fc.weight
// | fc.bias.  The device image (o_*, total: 32-bit words): c1_w [100][64] | c1_b [64] | dw [4][32][24] | pw_w [4][cin][cout] |
// pw_b [4][64] | fc_w | fc_b | the bf16-triple fragments of the pointwise layers and of conv1 (16-byte aligned) | conv1 as
// [ci][tap][cout] | the blob itself | the f16-pair fragments (16-byte aligned).
struct DscnnLayout {
    // tensor sizes the kernels need at compile time: channels, conv1.weight per input channel, a depthwise and a pointwise weight
    static constexpr int CO = 64, C1_TAPS = 100, C1_W = CO * C1_TAPS, DW_W = CO * 9, PW_W = CO * CO;
    static constexpr size_t B_DWB = DW_W, B_PWW = B_DWB + CO, B_PWB = B_PWW + PW_W, BLK = B_PWB + CO;  // a block and its tensors
    // 8-value fragments: pointwise [b 4][ct 2][m 4][lane], then (one input channel only) conv1 [ct 2][kb 7][lane]
    static constexpr size_t F_PW = 4 * 2 * 4 * 64, F_C1 = 2 * 7 * 64;
    size_t c1_floats, n_floats, b_blk, b_fcw, b_fcb, n_frag;
    size_t o_c1w, o_c1b, o_dw, o_pww, o_pwb, o_fcw, o_fcb, o_split, o_c1s, o_c1g, o_raw, o_pwp, o_c1p, total;
    int num_classes, in_channels;
    __host__ __device__ DscnnLayout(int num_classes_, int input_channels) : num_classes(num_classes_), in_channels(input_channels) {
        c1_floats = (size_t)C1_W * input_channels;
        b_blk = c1_floats + CO, b_fcw = b_blk + 4 * BLK, b_fcb = b_fcw + (size_t)num_classes * 64, n_floats = b_fcb + num_classes;
        n_frag = F_PW + (input_channels == 1 ? F_C1 : 0);
        o_c1w = 0, o_c1b = o_c1w + 6400, o_dw = o_c1b + 64, o_pww = o_dw + 4 * 64 * 12, o_pwb = o_pww + 4 * 4096, o_fcw = o_pwb + 4 * 64,
        o_fcb = o_fcw + (size_t)num_classes * 64, o_split = (o_fcb + num_classes + 3) & ~(size_t)3, o_c1s = o_split + F_PW * 3 * 4,
        o_c1g = o_c1s + F_C1 * 3 * 4, o_raw = o_c1g + c1_floats, o_pwp = (o_raw + n_floats + 3) & ~(size_t)3,
        o_c1p = o_pwp + F_PW * 2 * 4, total = o_c1p + F_C1 * 2 * 4;
    }
    __host__ __device__ size_t block(int k) const { return b_blk + (size_t)k * BLK; }  // blob offset of block k (0-based)
};

// DepthwiseSeparableConvBN's parameters() as one blob (kws_dscnn_bn.hip): the plain model's 20 tensors (DscnnLayout, one input
// channel), then weight [64] | bias [64] of bn_conv1, bn_dw.0 .. 3, bn_pw.0 .. 3.  A BatchNorm LAYER is counted in data-flow order,
// as d_stats is: 0 = conv1, 2k + 1 = the depthwise and 2k + 2 = the pointwise convolution of block k (0-based).
struct DscnnBnLayout {
    static constexpr int N_BN = 9, CO = DscnnLayout::CO, BN_FLOATS = N_BN * 2 * CO;
    DscnnLayout plain;
    size_t b_bn, n_floats;
    __host__ __device__ explicit DscnnBnLayout(int num_classes) : plain(num_classes, 1), b_bn(plain.n_floats), n_floats(plain.n_floats + BN_FLOATS) {}
    // the layer's module in blob order: bn_conv1, the four bn_dw, the four bn_pw
    __host__ __device__ static int module_of(int layer) { return layer == 0 ? 0 : (layer & 1) ? 1 + (layer - 1) / 2 : 5 + (layer - 2) / 2; }
    __host__ __device__ size_t gamma(int layer) const { return b_bn + (size_t)module_of(layer) * 2 * CO; }
    __host__ __device__ size_t beta(int layer) const { return gamma(layer) + CO; }
};

// The layers' power-of-two weight scales of the f16-pair images (pow2_scale_of_max of max|w|): conv1, the four pointwise layers.
struct DscnnScales {
    float c1, pw[4];
};

// Both images of fragment i < L.n_frag of the DS-CNN (MFMA A operands, 32x32x16), from the blob into the image.  Lane l = i & 63
// holds cout = 32ct + (l&31).
//   i < F_PW, block (b, ct, m): cin = 16m + 8(l>>5) + j, j = 0..7, of pointwise layer b.
//   then conv1, block (ct, kb): half-wave l >> 5 takes kernel rows 5(l>>5) .. + 4, i.e. 50 consecutive taps w[0..49], in two K orders:
//     bf16 image: w[8kb + j], zeros from 50 on -- both halves walk the same offsets 10*(kh%5) + kw, so their LDS addresses differ by
//                 a constant
//     f16 image (the pre-split windows, kws_dscnn_stages.h, conv1_unit_pairwin): kb < 5: row kb, taps kw = j; kb = 5: taps
//                 kw = 8 + (j & 1) of row j >> 1; kb = 6: taps kw = 8 + j (j < 2) of row 4, then zeros
__host__ __device__ inline void ds_pack_fragment(const DscnnLayout& L, const float* blob, size_t i, const DscnnScales& sw, uint32_t* img) {
    const size_t l = i & 63, row = l & 31, half = l >> 5;
    size_t f = i >> 6;  // fragment block
    if (i < DscnnLayout::F_PW) {
        const size_t b = f >> 3, ct = (f >> 2) & 1, m = f & 3;
        const float* w = blob + L.b_blk + b * DscnnLayout::BLK + DscnnLayout::B_PWW + (32 * ct + row) * 64 + 16 * m + 8 * half;
        float v[8];
        for (int j = 0; j < 8; ++j) v[j] = w[j];
        pack_bf16_triple(v, img + L.o_split + (f * 3 * 64 + l) * 4);
        pack_f16_pair(v, sw.pw[b], 1.f, img + L.o_pwp + (f * 2 * 64 + l) * 4);
        return;
    }
    f -= DscnnLayout::F_PW / 64;
    const int ct = (int)(f / 7), kb = (int)(f % 7);
    const float* w = blob + (32 * ct + row) * 100 + 50 * half;
    float v3[8], v2[8];
    for (int j = 0; j < 8; ++j) {
        const int t = kb < 5 ? 10 * kb + j : kb == 5 ? 10 * (j >> 1) + 8 + (j & 1) : j < 2 ? 48 + j : -1;
        v3[j] = 8 * kb + j < 50 ? w[8 * kb + j] : 0.f;
        v2[j] = t >= 0 ? w[t] : 0.f;
    }
    pack_bf16_triple(v3, img + L.o_c1s + (f * 3 * 64 + l) * 4);
    pack_f16_pair(v2, sw.c1, 1.f, img + L.o_c1p + (f * 2 * 64 + l) * 4);
}

// cnn-trad-fpool3.  The blob (b_*, n_*: floats) is the ten state_dict tensors in order.  The device image (o_*, total: 32-bit
// words): c1_split | c2_split | c1_b | c2_b | lin_split | lin_b | dnn_w | dnn_b | fc_w | fc_b, the f16-pair images (two pieces,
// 16-byte aligned), then the blob itself as float32 (16-byte aligned; the weights of kws_cnn_trad_backward_f32).
struct CtLayout {
    static constexpr size_t CO = 64, FLAT = 64 * 297;  // conv channels; inputs of the first dense layer
    // tensor sizes the kernels need at compile time: conv1.weight, conv2.weight, outputs of lin and dnn, dnn.weight
    static constexpr int N_C1 = 64 * 160, N_C2 = 64 * 64 * 40, LIN_OUT = 32, DNN_OUT = 128, N_DNN = DNN_OUT * LIN_OUT;
    // 8-value fragments per GEMM layer: conv1 [kb 10][ct 2][lane], conv2 [kk 40][cb 4][ct 2][lane], lin [kb FLAT/16][lane]
    static constexpr size_t F_C1 = 10 * 2 * 64, F_C2 = 40 * 4 * 2 * 64, F_LIN = FLAT / 16 * 64, N_FRAG = F_C1 + F_C2 + F_LIN;
    size_t n_c1, n_c2, n_lin, n_dnn, n_fc, n_floats;
    size_t b_w1, b_b1, b_w2, b_b2, b_wl, b_bl, b_wd, b_bd, b_wf, b_bf;
    size_t o_c1s, o_c2s, o_c1b, o_c2b, o_lin, o_linb, o_dnn, o_dnnb, o_fc, o_fcb, o_c1h, o_c2h, o_linh, o_raw, total;
    __host__ __device__ explicit CtLayout(int num_classes) {
        n_c1 = N_C1, n_c2 = N_C2, n_lin = LIN_OUT * FLAT, n_dnn = N_DNN, n_fc = (size_t)num_classes * DNN_OUT;
        b_w1 = 0, b_b1 = b_w1 + n_c1, b_w2 = b_b1 + CO, b_b2 = b_w2 + n_c2, b_wl = b_b2 + CO, b_bl = b_wl + n_lin, b_wd = b_bl + LIN_OUT,
        b_bd = b_wd + n_dnn, b_wf = b_bd + DNN_OUT, b_bf = b_wf + n_fc, n_floats = b_bf + num_classes;
        o_c1s = 0, o_c2s = o_c1s + F_C1 * 3 * 4, o_c1b = o_c2s + F_C2 * 3 * 4, o_c2b = o_c1b + CO, o_lin = o_c2b + CO,
        o_linb = o_lin + F_LIN * 3 * 4, o_dnn = o_linb + 32, o_dnnb = o_dnn + n_dnn, o_fc = o_dnnb + 128, o_fcb = o_fc + n_fc,
        o_c1h = (o_fcb + num_classes + 3) / 4 * 4, o_c2h = o_c1h + F_C1 * 2 * 4, o_linh = o_c2h + F_C2 * 2 * 4,
        o_raw = o_linh + F_LIN * 2 * 4, total = o_raw + (n_floats + 3) / 4 * 4;
    }
};

// Fragment i < N_FRAG of cnn-trad-fpool3: its eight weights are blob[src + j * step], j = 0..7; its bf16 pieces go to image word
// o3 (+ FRAG_PIECE per piece), its f16 pieces to o2; layer 0 / 1 / 2 = conv1 / conv2 / lin picks the scale.  Lane l = i & 63.
struct CtFrag {
    size_t src, step, o3, o2;
    int layer;
};
__host__ __device__ inline CtFrag ct_frag(const CtLayout& L, size_t i) {
    const size_t l = i & 63, row = l & 31, half = l >> 5;
    size_t f = i >> 6;  // fragment block inside its layer
    if (i < CtLayout::F_C1) {  // (kb, ct): cout = 32ct + (l&31), kernel row 2kb + (l>>5), kernel columns j
        const size_t kb = f >> 1, ct = f & 1;
        return {L.b_w1 + ((32 * ct + row) * 20 + 2 * kb + half) * 8, 1, L.o_c1s + (f * 3 * 64 + l) * 4, L.o_c1h + (f * 2 * 64 + l) * 4, 0};
    }
    f -= CtLayout::F_C1 / 64;
    if (f < CtLayout::F_C2 / 64) {  // (kk = kh*4 + kw, cb, ct): cout = 32ct + (l&31), input channels 16cb + 8(l>>5) + j
        const size_t kk = f >> 3, cb = (f >> 1) & 3, ct = f & 1;
        return {L.b_w2 + (((32 * ct + row) * 64 + 16 * cb + 8 * half) * 10 + (kk >> 2)) * 4 + (kk & 3), 40,
                L.o_c2s + (f * 3 * 64 + l) * 4, L.o_c2h + (f * 2 * 64 + l) * 4, 1};
    }
    f -= CtLayout::F_C2 / 64;  // first dense layer as MFMA B operands, k-block f: output l&31, inputs 16f + 8(l>>5) + j
    return {L.b_wl + row * CtLayout::FLAT + 16 * f + 8 * half, 1, L.o_lin + (f * 3 * 64 + l) * 4, L.o_linh + (f * 2 * 64 + l) * 4, 2};
}

// Both images of fragment i, from the blob into the image (sw1, sw2, swl: the layers' scales).
__host__ __device__ inline void ct_pack_fragment(const CtLayout& L, const float* blob, size_t i, float sw1, float sw2, float swl,
                                                 uint32_t* img) {
    const CtFrag f = ct_frag(L, i);
    float v[8];
    for (int j = 0; j < 8; ++j) v[j] = blob[f.src + j * f.step];
    pack_bf16_triple(v, img + f.o3);
    pack_f16_pair(v, f.layer == 0 ? sw1 : f.layer == 1 ? sw2 : swl, 2048.f, img + f.o2);
}

}  // namespace kws
