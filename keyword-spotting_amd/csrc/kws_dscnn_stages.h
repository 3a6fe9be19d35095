// The stages of the DS-CNN forward kernel (kws_dscnn.hip) as device functions: depthwise stencil, block tables and per-clip
// scales, stage maxima, operand loads, conv1 on the matrix cores, leftover tiles, the depthwise + pointwise block phase.  The
// arithmetic and the MFMA mapping: top of kws_dscnn.hip; the LDS map: kws_dscnn_geom.h.  Anonymous namespace, inlined per unit.
#pragma once
#include <type_traits>

#include "kws_dscnn_geom.h"
#include "kws_dscnn_units.h"
#include "kws_mfcc_dev.h"
#include "kws_split_mfma.h"

namespace kws {
namespace {

// The depthwise table is interleaved in channel PAIRS: a record is ten (channel c, channel c + 1) pairs -- nine taps and the
// bias -- in 96 bytes.  The record is the same for all 32 lanes of a half-wave, and a ds_read_b128 costs its four LDS-array
// cycles whether or not the addresses coincide, so no lane reads the whole record: lane l reads the ONE pair at
// 8 * (l & 15) bytes into it (dw_row_offset), the 16 lanes of a row then hold the record between them, and every tap reaches
// its multiply-add through row_newbcast.  One ds_read_b64 and two registers per step pair where whole records took five
// ds_read_b128 and twenty.  Lanes 10 - 15 of a row read the pad and the head of the next record (the last record: the head of
// the pointwise bias); those values are never selected.  (`tools/experiments/dscnn_unit_ablations.patch`: without the weight
// reloads the kernel runs 9.5 % faster; DESIGN 4.2, "Depthwise weights by row broadcast".)
struct DwPair {
    float2 w;  // in lane l: element l & 15 of (w0 .. w8, b, pad ...), as the (channel c, channel c + 1) pair
};
static_assert((2 * 768 - 24) * 4 + 8 * 15 + 8 <= (OFF_PWB + 2 * 64 - OFF_DWTAB) * 4,
              "a row's read of the last record of the second table buffer ends inside the pointwise biases that follow it");
__device__ __forceinline__ int dw_row_offset(int lane) { return 2 * (lane & 15); }  // in floats
// Depthwise 3x3 (+bias) at this lane's column from its three own-column inputs: nine multiply-adds and two
// fused DPP multiply-adds that pull the neighbouring lanes' column sums across the wavefront (0 shifted in at the
// ends).  w: one channel's element of the row-resident record (DwPair); tap k is row_newbcast:k, the bias row_newbcast:9
// (v_mov_b32_dpp into c, then c = w1 * up + c in one v_fmac: the fused w1 * up + b).  Written as one asm block so that (a) the
// shift or broadcast and the multiply-add are one instruction each (v_fmac_f32_dpp; the compiler emits v_mov_b32_dpp +
// v_fmac), and (b) each DPP source a VALU writes (to_right, to_left) is written three instructions before it is read -- the
// VALU-write -> DPP-read hazard needs two wait states and the hazard recognizer does not look inside inline asm; w comes
// from an LDS read, which the compiler waits for.  All 64 lanes must be active: a source lane that EXEC disables reads as
// invalid.  TO_MFMA: the result is fed straight to a matrix-core instruction (f32 path), which needs two more wait states
// after the last VALU write.
template <bool TO_MFMA = false>
__device__ __forceinline__ float stencil3x3(float w, float up, float mid, float dn, float mask_l, float mask_r) {
    float c, to_right, to_left;
    asm("v_mov_b32_dpp %0, %3 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"        // c = b
        "v_mul_f32_dpp %1, %3, %4 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"    // to_right = w0*up   (what lane+1 needs: its (.., -1) taps)
        "v_mul_f32_dpp %2, %3, %4 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"    // to_left  = w2*up   (what lane-1 needs: its (.., +1) taps)
        "v_fmac_f32_dpp %0, %3, %4 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"   // c = w1*up + b
        "v_fmac_f32_dpp %1, %3, %5 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"   // to_right += w3*mid
        "v_fmac_f32_dpp %2, %3, %5 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"   // to_left  += w5*mid
        "v_fmac_f32_dpp %0, %3, %5 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"   // c += w4*mid
        "v_fmac_f32_dpp %1, %3, %6 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"   // to_right += w6*dn
        "v_fmac_f32_dpp %2, %3, %6 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"   // to_left  += w8*dn
        "v_fmac_f32_dpp %0, %3, %6 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"   // c += w7*dn
        "v_fmac_f32_dpp %0, %1, %7 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"   // c += to_right[lane-1]*mask_l
        "v_fmac_f32_dpp %0, %2, %8 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"        // c += to_left[lane+1]*mask_r
        : "=&v"(c), "=&v"(to_right), "=&v"(to_left)
        : "v"(w), "v"(up), "v"(mid), "v"(dn), "v"(mask_l), "v"(mask_r));
    if constexpr (TO_MFMA) asm volatile("s_nop 1" : "+v"(c));
    return c;
}
template <bool TO_MFMA, int E>  // E: which channel of the pair
__device__ __forceinline__ float stencil3x3_of_pair(const DwPair& w, float up, float mid, float dn, float mask_l, float mask_r) {
    return stencil3x3<TO_MFMA>(E == 0 ? w.w.x : w.w.y, up, mid, dn, mask_l, mask_r);
}
// Sum over each 32-lane half of the wavefront without touching LDS: inclusive scan inside the 16-lane rows
// (row_shr 1,2,4,8), then row 0 -> row 1 and row 2 -> row 3 (row_bcast:15).  Lanes 31 and 63 hold the totals.
// (dpp_shift_add<CTRL, ROW_MASK>: kws_mfcc_dev.h)
__device__ __forceinline__ float half_wave_sum_to_last_lane(float v) {
    v = dpp_shift_add<0x111, 0xf>(v);  // row_shr:1
    v = dpp_shift_add<0x112, 0xf>(v);  // row_shr:2
    v = dpp_shift_add<0x114, 0xf>(v);  // row_shr:4
    v = dpp_shift_add<0x118, 0xf>(v);  // row_shr:8
    v = dpp_shift_add<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
    return v;
}

// Depthwise table [32 channel pairs][24] and pointwise bias [64] of block n (1..4) go to LDS buffer (n-1)&1 in two
// halves so the global-memory latency hides under a whole phase: fetch() issues the loads into three
// registers at the start of the previous phase, store() writes them to LDS after that phase's units.
struct BlockTables {
    float d0, d1, b;
};
__device__ __forceinline__ void fetch_block_tables(const DscnnWeights& w, int n, int tid, BlockTables& r) {
    const float* src = w.dw_w + (n - 1) * CH * 12;
    r.d0 = tid < CH * 12 ? src[tid] : 0.f;
    r.d1 = NT + tid < CH * 12 ? src[NT + tid] : 0.f;
    r.b = tid < CH ? w.pw_b[(n - 1) * CH + tid] : 0.f;
}
// s_dww / s_dwb / s_pwb (f16-pair arithmetic; 1 otherwise): the block's activations are kept in LDS scaled by per-clip powers
// of two and its depthwise OUTPUT is wanted in the operand units 2^ky of the matrix instructions (below 2^15): the depthwise
// weights carry the factor 2^(ky - input units), the depthwise bias 2^ky, so the stencil's result needs no scaling before it is
// split (powers of two: the same bits as scaling afterwards); the pointwise bias (= accumulator seed and ring value) is stored
// in the units of the block's output.
__device__ __forceinline__ void store_block_tables(float* lds, int n, int tid, const BlockTables& r, float s_dwb = 1.f, float s_pwb = 1.f,
                                                   float s_dww = 1.f) {
    float* dwtab = lds + OFF_DWTAB + ((n - 1) & 1) * 768;
    if (tid < CH * 12) dwtab[tid] = r.d0 * ((tid % 24) >> 1 == 9 ? s_dwb : s_dww);  // (pair-interleaved rows of 24: the biases at 18, 19)
    if (NT + tid < CH * 12) dwtab[NT + tid] = r.d1 * (((NT + tid) % 24) >> 1 == 9 ? s_dwb : s_dww);
    if (tid < CH) lds[OFF_PWB + ((n - 1) & 1) * 64 + tid] = r.b * s_pwb;
}
// f16-pair arithmetic: what a stage needs to know about the clip's scales (all powers of two)
struct PairCtx {
    float s_dww = 1.f;      // next block's depthwise weight factor = its operand scale over this block's output units
    float s_dwb = 1.f;      // next block's depthwise bias factor = its operand scale
    float s_pwb = 1.f;      // next block's pointwise bias factor = the next block's output units
    float inv_out = 1.f;    // block 4: pooled sums back to true units
};
// Units of a stage: its operand exponent ky (operand * 2^ky < 2^15) plus the layer's weight exponent.  The stage's stored
// output -- bias included, which the operand bound knows nothing about -- must stay a finite float in those units, and every
// factor derived from them a normal one: 2^sg * bz < 2^100 (bz: bound on the stage's output in true units) and sg <= 120,
// enforced by LOWERING the operand scale (always safe; it binds only for bias-dominated or vanishing stages).
__device__ __forceinline__ void cap_units(int& ky, int& sg, int k_w, float bz) {
    sg = ky + k_w;
    const int eb = (int)((__builtin_bit_cast(uint32_t, bz) >> 23) & 0xffu) - 126;  // bz < 2^eb
    int limit = 100 - eb;
    limit = limit > 120 ? 120 : limit;
    if (sg > limit) {
        ky -= sg - limit;
        sg = limit;
    }
}
// wavefront maximum of non-negative values -> per-wavefront slot (read by everyone after the stage's barrier).  DPP row
// scans, no LDS round trips: six dependent ds_bpermute exchanges sat at the end of every wavefront's stage, in front of the barrier.
__device__ __forceinline__ void publish_wave_max(float* lds, int set, int wv, int lane, float mx) {
    auto step = [](float m, auto ctrl, auto row_mask) {
        return fmaxf(m, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, m), __builtin_bit_cast(int, m), decltype(ctrl)::value,
                                                                              decltype(row_mask)::value, 0xf, false)));
    };
    mx = step(mx, std::integral_constant<int, 0x111>{}, std::integral_constant<int, 0xf>{});  // row_shr:1
    mx = step(mx, std::integral_constant<int, 0x112>{}, std::integral_constant<int, 0xf>{});  // row_shr:2
    mx = step(mx, std::integral_constant<int, 0x114>{}, std::integral_constant<int, 0xf>{});  // row_shr:4
    mx = step(mx, std::integral_constant<int, 0x118>{}, std::integral_constant<int, 0xf>{});  // row_shr:8
    mx = step(mx, std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xa>{});  // row_bcast:15 into rows 1, 3
    mx = step(mx, std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xc>{});  // row_bcast:31 into rows 2, 3
    if (lane == 63) lds[OFF_WMAX + set * NW + wv] = mx;
}
// the maximum over n_sets consecutive sets (NW values each): two 16-byte reads per set
__device__ __forceinline__ float read_stage_max(const float* lds, int set0, int n_sets) {
    static_assert(NW % 4 == 0 && OFF_WMAX % 4 == 0, "the stage maxima are read as float4s");
    float m = 0.f;
    const float4* q = reinterpret_cast<const float4*>(lds + OFF_WMAX + set0 * NW);
    for (int i = 0; i < (NW / 4) * n_sets; ++i) {
        const float4 v = q[i];
        m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    }
    return m;
}

// Pointwise weights of the running block as MFMA A operands.
//   f32 path   (32x32x2 f32):   wa[ct][s] = W[cout = ct*32 + (l&31)][cin = 16(s>>3) + 8(l>>5) + (s&7)], held for the
//     whole block (the K order of the f32 MFMA steps is free; this one is the lane -> channel walk of the split
//     path, so every variant shares the depthwise stage).
//   split path (32x32x16 bf16): piece p (0 hi, 1 mid, 2 lo) of W[cout = ct*32 + (l&31)][cin = 16m + 8(l>>5) + j],
//     j = 0..7 -- eight bf16 per lane and (ct, m, p), pre-split on the host (exactly: hi + mid + lo == W).  Only
//     two k-blocks m are in registers at a time: ring[m & 1] is fetched one k-block ahead from global memory
//     (L1/L2-resident; the same bytes per block as the f32 path loads), which frees 48 registers.
// NP pieces per operand: 3 = bf16 hi/mid/lo (modes 4, 6), 2 = f16 pair (mode 5)
template <int NP>
struct PwRing {
    uintx4 ring[2][2][NP];  // [ring slot][channel tile][piece] of one k-block
};
struct PwRegsF32 {
    float wa[2][32];
};
template <int MODE>
using PwOperands = std::conditional_t<(MODE >= 4), PwRing<(MODE == 5 ? 2 : 3)>, PwRegsF32>;
__device__ __forceinline__ void load_pointwise(const DscnnWeights& w, int n, int lane, PwRegsF32& o) {
    const float* pw = w.pw_w + (n - 1) * CH * CH + 8 * (lane >> 5) * CH + (lane & 31);
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int s = 0; s < 32; ++s) o.wa[ct][s] = pw[(16 * (s >> 3) + (s & 7)) * CH + ct * 32];
}
template <int NP>
__device__ __forceinline__ void load_afrag(const DscnnWeights& w, int n, int m, int lane, uintx4 (&f)[2][NP]) {
    const uintx4* src = reinterpret_cast<const uintx4*>(NP == 2 ? w.pw_pair : w.pw_split) + (size_t)(n - 1) * (2 * 4 * NP * 64) + lane;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int p = 0; p < NP; ++p) f[ct][p] = src[((ct * 4 + m) * NP + p) * 64];
}
// first operands of block n: the whole block (f32) or its k-block 0 (split)
__device__ __forceinline__ void load_block_head(const DscnnWeights& w, int n, int lane, PwRegsF32& o) { load_pointwise(w, n, lane, o); }
template <int NP>
__device__ __forceinline__ void load_block_head(const DscnnWeights& w, int n, int lane, PwRing<NP>& o) { load_afrag(w, n, 0, lane, o.ring[0]); }

// The descriptor of a block-phase unit as its lane holds it (kws_dscnn_units.h): requested where the unit's first A operands
// are requested -- a unit ahead -- so it returns in order with them, and read at the unit's head in place of the geometry
// arithmetic.  The persistent batched f16-pair kernels only (UT); every other route computes its geometry.
struct UnitDesc {
    uintx4 a;  // tlo[0..2], valid
    uint2 m;   // mask_l, mask_r
};
__device__ __forceinline__ void load_unit_desc(const DscnnWeights& w, int n, int tile, int lane, UnitDesc& d) {
    const uint32_t* src = w.units + ((size_t)(ds_unit_base(n - 1) + tile) * 2 * 64 + lane) * 4;
    d.a = *reinterpret_cast<const uintx4*>(src);
    d.m = *reinterpret_cast<const uint2*>(src + 64 * 4);
}

// ------------------------------------------------------------------------------------------------
// conv1: D[cout][pos] = sum_k W[cout][k] * im2col[k][pos], k = kh*10 + kw, as 50 MFMA k-steps.
template <bool MFMA>
__device__ __forceinline__ void conv1_phase(const DscnnWeights& w, float* lds, int tid, const float (&a)[50]) {
    const float* featp = lds + OFF_FEAT;
    float* z0 = lds + OFF_Z0;
    if constexpr (MFMA) {
        const int lane = tid & 63, wv = tid >> 6, half = lane >> 5, col = lane & 31;
        const int ct = wv & 1;  // units u = wv, wv + NW share the output-channel tile (NW is even)
        for (int u = wv; u < 10; u += NW) {
            const int pt = u >> 1;
            const int pos = pt * 32 + col;
            const int posc = pos < P0 ? pos : P0 - 1;
            const int oh = posc / C1_W, ow = posc % C1_W;
            const float* base = featp + (2 * oh) * FEAT_W + 2 * ow + half;
            floatx16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < 50; ++s) {
                const float b = base[((2 * s) / 10) * FEAT_W + (2 * s) % 10];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b, acc, 0, 0, 0);
            }
            if (pos < P0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = ct * 32 + row_of(r, half);
                    z0[pidx(co, pos, P0 + 2)] = relu(acc[r] + w.c1_b[co]);
                }
            }
        }
    } else {
        for (int idx = tid; idx < CH * P0; idx += NT) {
            const int co = idx / P0, pos = idx % P0;
            const int oh = pos / C1_W, ow = pos % C1_W;
            float acc = w.c1_b[co];
            for (int kh = 0; kh < C1_K; ++kh)
                for (int kw = 0; kw < C1_K; ++kw)
                    acc = fmaf(w.c1_w[(kh * C1_K + kw) * CH + co], featp[(2 * oh + kh) * FEAT_W + 2 * ow + kw], acc);
            z0[pidx(co, pos, P0 + 2)] = relu(acc);
        }
    }
    if (tid < CH) {  // extra slots of the conv1 planes: no ring in block 1, slot P+1 is the zero pad
        z0[pidx(tid, P0, P0 + 2)] = 0.f;
        z0[pidx(tid, P0 + 1, P0 + 2)] = 0.f;
    }
}

// conv1 on the bf16 matrix pipe (split path).  K order: the half-wave h takes kernel rows 5h..5h+4, so both
// halves walk the same 56 offsets f = 8kb + j -> (kh%5 = f/10, kw = f%10) (f >= 50: zero weights) and lane
// (col, h) of k-block kb supplies im2col values feat[2oh + 5h + f/10][2ow + f%10], j = 0..7, split into three bf16
// pieces like the pointwise operands.  c1f: the channel tile wv & 1, [kb][piece], loaded at kernel start.
//
// Work split: 141 positions = 5 tiles of 32, two channel tiles each.  As ten (tile, channel tile) units on eight
// wavefronts two wavefronts run two units back to back and every unit gathers and splits its tile's im2col values
// again.  Instead wavefronts 0-3 take tiles 0-3 for BOTH channel tiles (one gather + split feeds twelve MFMAs per
// k-block; the other tile's A fragments stream from L2 through a two-deep ring), wavefronts 4 and 5 take tile 4 for
// one channel tile each, 6 and 7 have no conv1 work: one round, and the busiest SIMD (a dual and a single unit)
// carries the matrix work of three single units but two split streams instead of three.
// p_lo / p_hi: the positions this workgroup computes (the whole map, or the rows of one time tile: see PosRange).
// NP = 3: bf16 hi/mid/lo, six products per k-block.  NP = 2: f16 pairs, three (kws_split_mfma.h); the features are multiplied
// by the clip's scale sx inside the split, the accumulators are in units sig0 = sx * (the layer's weight scale), the bias is
// added in those units and the output is STORED in them (block 1's depthwise bias is scaled to match); mx collects the
// largest stored value of this wavefront.
template <bool DUAL, int NP>
__device__ __forceinline__ void conv1_unit_split(const DscnnWeights& w, const float* featp, float* z0, int ptile, int ct, int lane,
                                                 const uintx4 (&c1f)[7][NP], int p_lo, int p_hi, float sx, float sig0, float& mx) {
    constexpr bool PAIR = NP == 2;
    const int half = lane >> 5, col = lane & 31;
    const int pos = p_lo + ptile * 32 + col;
    const int posc = pos < p_hi ? pos : p_hi - 1;
    const int oh = posc / C1_W, ow = posc % C1_W;
    const float* base = featp + (2 * oh + 5 * half) * FEAT_W + 2 * ow;
    const floatx16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    floatx16 acc = zero, acc2 = zero;  // two chains per channel tile keep the matrix pipe fed
    floatx16 occ = zero, occ2 = zero;  // the other channel tile (DUAL)
    const uintx4* osrc = reinterpret_cast<const uintx4*>(PAIR ? w.c1_pair : w.c1_split) + (size_t)(ct ^ 1) * (7 * NP * 64) + lane;
    uintx4 of[2][NP];                  // its A fragments: k-block kb in of[kb & 1], requested two k-blocks ahead
    auto load_other = [&](int kb) {
#pragma unroll
        for (int pc = 0; pc < NP; ++pc) of[kb & 1][pc] = osrc[(kb * NP + pc) * 64];
    };
    if (DUAL) {
        load_other(0);
        load_other(1);
    }
    float y[2][8];
    auto gather = [&](int kb, float (&dst)[8]) {  // offsets f, f+1 (f even) are neighbours in one row: 8-byte reads
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
            const float2 v = *reinterpret_cast<const float2*>(base + ((8 * kb + j) / 10) * FEAT_W + (8 * kb + j) % 10);
            dst[j] = v.x;
            dst[j + 1] = v.y;
        }
    };
    uintx4 bf[2][NP];  // [buffer][piece] B operands: k-block kb multiplies while kb+1 is being split
    gather(0, y[0]);
    gather(1, y[1]);
    if constexpr (PAIR)
        split_pair8(y[0], sx, bf[0][0], bf[0][1]);
    else
        split3(y[0], bf[0][0], bf[0][1], bf[0][NP - 1]);
    gather(2, y[0]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kb = 0; kb < 7; ++kb) {
        const int cur = kb & 1, nxt = cur ^ 1;
        // the piece products of this k-block (per channel tile), smallest first, spread over the next k-block's split
        auto product = [&](int q) {
            // triple: (lo,hi) (hi,lo) (mid,mid) (mid,hi) (hi,mid) (hi,hi); pair: (hi,lo) (lo,hi) (hi,hi)
            const int pa = PAIR ? (q == 1 ? 1 : 0) : (q == 0 ? 2 : (q == 2 || q == 3) ? 1 : 0);
            const int pb = PAIR ? (q == 0 ? 1 : 0) : ((q == 0 || q == 3 || q == 5) ? 0 : (q == 1 ? 2 : 1));
            auto mm = [&](const uintx4& a, const uintx4& b, floatx16 c) {
                if constexpr (PAIR)
                    return mfma_f16(a, b, c);
                else
                    return mfma_bf16(a, b, c);
            };
            if (q & 1)
                acc2 = mm(c1f[kb][pa], bf[cur][pb], acc2);
            else
                acc = mm(c1f[kb][pa], bf[cur][pb], acc);
            __builtin_amdgcn_sched_barrier(0);
            if (DUAL) {
                if (q & 1)
                    occ2 = mm(of[cur][pa], bf[cur][pb], occ2);
                else
                    occ = mm(of[cur][pa], bf[cur][pb], occ);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        if constexpr (PAIR) {
            product(0);
            if (kb + 1 < 7) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    uint32_t h, l;
                    split_pair2(y[nxt][2 * i], y[nxt][2 * i + 1], sx, h, l);
                    bf[nxt][0][i] = h;
                    bf[nxt][1][i] = l;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            product(1);
            if (kb + 1 < 7) {
#pragma unroll
                for (int i = 2; i < 4; ++i) {
                    uint32_t h, l;
                    split_pair2(y[nxt][2 * i], y[nxt][2 * i + 1], sx, h, l);
                    bf[nxt][0][i] = h;
                    bf[nxt][1][i] = l;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (kb + 3 < 7) gather(kb + 3, y[nxt]);
            __builtin_amdgcn_sched_barrier(0);
            product(2);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                product(i);
                if (kb + 1 < 7) {
                    const float a0 = y[nxt][2 * i], a1 = y[nxt][2 * i + 1];
                    const float r0 = a0 - top16(a0), r1 = a1 - top16(a1);
                    bf[nxt][0][i] = pack_top16(a0, a1);
                    bf[nxt][1][i] = pack_top16(r0, r1);
                    bf[nxt][NP - 1][i] = pack_top16(r0 - top16(r0), r1 - top16(r1));
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            product(4);
            if (kb + 3 < 7) gather(kb + 3, y[nxt]);
            __builtin_amdgcn_sched_barrier(0);
            product(5);
        }
        if (DUAL && kb + 2 < 7) {
            load_other(kb + 2);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    acc += acc2;
    occ += occ2;
    if (pos < p_hi) {
#pragma unroll
        for (int r = 0; r < 16; r += 2) {  // accumulator rows r, r+1 are adjacent output channels: one 8-byte store
            const int co = ct * 32 + row_of(r, half);
            const float v0 = relu(fmaf(w.c1_b[co], sig0, acc[r])), v1 = relu(fmaf(w.c1_b[co + 1], sig0, acc[r + 1]));
            *reinterpret_cast<float2*>(z0 + pidx(co, pos, P0 + 2)) = make_float2(v0, v1);
            if constexpr (PAIR) mx = fmaxf(mx, fmaxf(v0, v1));
            if (DUAL) {
                const int oo = (ct ^ 1) * 32 + row_of(r, half);
                const float u0 = relu(fmaf(w.c1_b[oo], sig0, occ[r])), u1 = relu(fmaf(w.c1_b[oo + 1], sig0, occ[r + 1]));
                *reinterpret_cast<float2*>(z0 + pidx(oo, pos, P0 + 2)) = make_float2(u0, u1);
                if constexpr (PAIR) mx = fmaxf(mx, fmaxf(u0, u1));
            }
        }
    }
}

// ---- conv1 on f16 pairs from PRE-SPLIT WINDOWS (PAIR only) ---------------------------------------------------------------
// Gathered and split per unit, conv1's B operand cost four 8-byte LDS reads and twelve VALU instructions per k-block in front
// of every three (six) MFMAs, and the phase ran at the latency of that chain.  Instead the scaled, zero-padded feature map is
// split ONCE per clip into LDS (the region block 1's output takes later):
//   W8[piece][row 0..102][s 0..2]  16 bytes: the eight features (row, 2s .. 2s + 7) as f16
//   P2[piece][row][s]               4 bytes: the two features (row, 2s + 8), (row, 2s + 9)
// and K is ordered to match: half-wave h takes kernel rows 5h .. 5h + 4; k-block kb < 5 = kernel row 5h + kb, taps kw 0..7 --
// one aligned ds_read_b128 per piece; k-block 5 = taps kw 8, 9 of kernel rows 5h .. 5h + 3 (four dwords per piece), k-block 6 =
// taps kw 8, 9 of kernel row 5h + 4 and six zeros.  (c1_pair is laid out in this order by kws_load_dscnn.)
constexpr int C1W_ROWS = FEAT_H;                                   // 103 padded feature rows
constexpr int OFF_C1W8 = OFF_Z1;                                   // floats; [2][103][3][4 dwords]
constexpr int OFF_C1P2 = OFF_C1W8 + 2 * C1W_ROWS * 3 * 4;          // [2][103][3] dwords
static_assert(OFF_C1P2 + 2 * C1W_ROWS * 3 <= OFF_Z0, "conv1's operand windows live where block 1's output goes later");
static_assert(2 * (C1_W - 1) + 9 < FEAT_W && 2 * (C1_H - 1) + 9 < FEAT_H, "window reach inside the padded map");

__device__ __forceinline__ void conv1_build_windows(float* lds, int tid, float sx, int off_feat = OFF_FEAT) {
    const float* featp = lds + off_feat;
    uint32_t* w8 = reinterpret_cast<uint32_t*>(lds + OFF_C1W8);
    uint32_t* p2 = reinterpret_cast<uint32_t*>(lds + OFF_C1P2);
    for (int i = tid; i < C1W_ROWS * 3; i += NT) {
        const float* src = featp + (i / 3) * FEAT_W + 2 * (i % 3);
        const float y[8] = {src[0], src[1], src[2], src[3], src[4], src[5], src[6], src[7]};
        uintx4 hi, lo;
        split_pair8(y, sx, hi, lo);
        *reinterpret_cast<uintx4*>(w8 + i * 4) = hi;
        *reinterpret_cast<uintx4*>(w8 + (C1W_ROWS * 3 + i) * 4) = lo;
        uint32_t h, l;
        split_pair2(src[8], src[9], sx, h, l);
        p2[i] = h;
        p2[C1W_ROWS * 3 + i] = l;
    }
}

template <bool DUAL>
__device__ __forceinline__ void conv1_unit_pairwin(const DscnnWeights& w, const float* lds, float* z0, int ptile, int ct, int lane,
                                                   const uintx4 (&c1f)[7][2], int p_lo, int p_hi, float sig0, float& mx) {
    const int half = lane >> 5, col = lane & 31;
    const int pos = p_lo + ptile * 32 + col;
    const int posc = pos < p_hi ? pos : p_hi - 1;
    const int oh = posc / C1_W, ow = posc % C1_W;
    const int wi = (2 * oh + 5 * half) * 3 + ow;  // window of kernel row 5h at this position; kernel row 5h + i: + 3i
    const uintx4* w8 = reinterpret_cast<const uintx4*>(lds + OFF_C1W8) + wi;
    const uint32_t* p2 = reinterpret_cast<const uint32_t*>(lds + OFF_C1P2) + wi;
    const floatx16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    floatx16 acc = zero, acc2 = zero, occ = zero, occ2 = zero;  // two chains per channel tile; occ*: the other channel tile (DUAL)
    const uintx4* osrc = reinterpret_cast<const uintx4*>(w.c1_pair) + (size_t)(ct ^ 1) * (7 * 2 * 64) + lane;
    // the other tile's A fragments, all seven k-blocks requested up front (L2 hits, but ~600 cycles away: with the operand split
    // gone a k-block is too short to hide them two k-blocks ahead; the registers are free in this phase)
    uintx4 of[DUAL ? 7 : 1][2];
    if (DUAL) {
#pragma unroll
        for (int kb = 0; kb < 7; ++kb) {
            of[kb][0] = osrc[(kb * 2 + 0) * 64];
            of[kb][1] = osrc[(kb * 2 + 1) * 64];
        }
    }
    // the biases of this lane's accumulator rows (rows 4q .. 4q+3 = channels 8q + 4 half + 0..3: one float4 each), requested
    // now: read in the epilogue they were an L2 round trip at the end of every unit
    float4 cb[4], ob[DUAL ? 4 : 1];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        cb[q] = *reinterpret_cast<const float4*>(w.c1_b + ct * 32 + 8 * q + 4 * half);
        if (DUAL) ob[DUAL ? q : 0] = *reinterpret_cast<const float4*>(w.c1_b + (ct ^ 1) * 32 + 8 * q + 4 * half);
    }
    uintx4 bq[3][2];  // [k-block mod 3][piece], fetched two k-blocks ahead
    auto b_load = [&](int kb, uintx4 (&d)[2]) {
        if (kb < 5) {
            d[0] = w8[kb * 3];
            d[1] = w8[kb * 3 + C1W_ROWS * 3];
        } else if (kb == 5) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                d[0][i] = p2[i * 3];
                d[1][i] = p2[i * 3 + C1W_ROWS * 3];
            }
        } else {
            d[0] = uintx4{p2[4 * 3], 0u, 0u, 0u};
            d[1] = uintx4{p2[4 * 3 + C1W_ROWS * 3], 0u, 0u, 0u};
        }
    };
    b_load(0, bq[0]);
    b_load(1, bq[1]);
#pragma unroll
    for (int kb = 0; kb < 7; ++kb) {
        if (kb + 2 < 7) b_load(kb + 2, bq[(kb + 2) % 3]);
        const uintx4 &bh = bq[kb % 3][0], &bl = bq[kb % 3][1];
        // (hi, lo) (lo, hi) (hi, hi), the two channel tiles interleaved
        acc2 = mfma_f16(c1f[kb][0], bl, acc2);
        if (DUAL) occ2 = mfma_f16(of[DUAL ? kb : 0][0], bl, occ2);
        acc = mfma_f16(c1f[kb][1], bh, acc);
        if (DUAL) occ = mfma_f16(of[DUAL ? kb : 0][1], bh, occ);
        acc2 = mfma_f16(c1f[kb][0], bh, acc2);
        if (DUAL) occ2 = mfma_f16(of[DUAL ? kb : 0][0], bh, occ2);
    }
    acc += acc2;
    occ += occ2;
    if (pos < p_hi) {
#pragma unroll
        for (int r = 0; r < 16; r += 2) {  // accumulator rows r, r+1 are adjacent output channels: one 8-byte store
            const int co = ct * 32 + row_of(r, half);
            const float4 b4 = cb[r >> 2];
            const float b0 = (r & 2) ? b4.z : b4.x, b1 = (r & 2) ? b4.w : b4.y;
            const float v0 = relu(fmaf(b0, sig0, acc[r])), v1 = relu(fmaf(b1, sig0, acc[r + 1]));
            *reinterpret_cast<float2*>(z0 + pidx(co, pos, P0 + 2)) = make_float2(v0, v1);
            mx = fmaxf(mx, fmaxf(v0, v1));
            if (DUAL) {
                const int oo = (ct ^ 1) * 32 + row_of(r, half);
                const float4 o4 = ob[DUAL ? (r >> 2) : 0];
                const float c0 = (r & 2) ? o4.z : o4.x, c1 = (r & 2) ? o4.w : o4.y;
                const float u0 = relu(fmaf(c0, sig0, occ[r])), u1 = relu(fmaf(c1, sig0, occ[r + 1]));
                *reinterpret_cast<float2*>(z0 + pidx(oo, pos, P0 + 2)) = make_float2(u0, u1);
                mx = fmaxf(mx, fmaxf(u0, u1));
            }
        }
    }
}

// Rows [lo, hi) of a map, as flattened positions [lo * W, hi * W): what one workgroup of a time-tile cluster computes of a
// stage (the streaming push at few streams, see kws_dscnn_fwd_kernel).  The full map when the workgroup owns the clip.
struct PosRange {
    int lo, hi;
};

template <bool RANGED, int NP>
__device__ __forceinline__ void conv1_phase_split(const DscnnWeights& w, float* lds, int tid, const uintx4 (&c1f)[7][NP],
                                                  PosRange rg, float sx = 1.f, float sig0 = 1.f, int off_feat = OFF_FEAT) {
    static_assert(P0 > 4 * 32 && P0 <= 5 * 32 && NW >= 6, "conv1 work split: four dual tiles + one tile in two halves");
    const float* featp = lds + off_feat;
    float* z0 = lds + OFF_Z0;
    const int lane = tid & 63, wv = tid >> 6;
    float mx = 0.f;
    if constexpr (NP == 2) {  // f16 pairs: operands from the pre-split windows (built by the caller, behind a barrier)
        if constexpr (RANGED) {
            const int n_pt = (rg.hi - rg.lo + 31) / 32;
            for (int u = wv; u < 2 * n_pt; u += NW) conv1_unit_pairwin<false>(w, lds, z0, u >> 1, u & 1, lane, c1f, rg.lo, rg.hi, sig0, mx);
        } else if (wv < 4)
            conv1_unit_pairwin<true>(w, lds, z0, wv, wv & 1, lane, c1f, 0, P0, sig0, mx);
        else if (wv < 6)
            conv1_unit_pairwin<false>(w, lds, z0, 4, wv & 1, lane, c1f, 0, P0, sig0, mx);
    } else if constexpr (RANGED) {
        // a time tile holds at most 4 position tiles of 32: one (tile, channel tile) unit per wavefront, one round -- the
        // shortest critical path (a dual unit carries twice the matrix work); c1f holds channel tile wv & 1
        const int n_pt = (rg.hi - rg.lo + 31) / 32;
        for (int u = wv; u < 2 * n_pt; u += NW) conv1_unit_split<false, NP>(w, featp, z0, u >> 1, u & 1, lane, c1f, rg.lo, rg.hi, sx, sig0, mx);
    } else if (wv < 4)
        conv1_unit_split<true, NP>(w, featp, z0, wv, wv & 1, lane, c1f, 0, P0, sx, sig0, mx);
    else if (wv < 6)
        conv1_unit_split<false, NP>(w, featp, z0, 4, wv & 1, lane, c1f, 0, P0, sx, sig0, mx);
    if constexpr (NP == 2) publish_wave_max(lds, 1, wv, lane, mx);
    if (tid < CH) {  // extra slots of the conv1 planes: no ring in block 1, slot P+1 is the zero pad
        z0[pidx(tid, P0, P0 + 2)] = 0.f;
        z0[pidx(tid, P0 + 1, P0 + 2)] = 0.f;
    }
}

// ------------------------------------------------------------------------------------------------
// A quarter of the leftover tile of block N (see Leftover): k-block M (input channels 16M .. 16M+15) of tile Leftover<N>::TILE
// for both output-channel tiles.  Eight stencil steps, one split, twelve MFMAs, the raw partial sums (no bias, no ReLU) of the
// tile's valid columns to part[M][position in tile][cout] (Leftover<N>::CSTRIDE floats per position).  af: the pre-split weights of k-block M (requested long before).
// UT: the tile's geometry from its unit descriptor ud (else ud is not read).
template <int N, int NP, bool UT = false>
__device__ __forceinline__ void leftover_partial_unit(float* lds, int lane, int M, const uintx4 (&af)[2][NP], const UnitDesc& ud) {
    using G = Blk<N>;
    using L = Leftover<N>;
    const int half = lane >> 5, col = lane & 31;
    const float* dwtab = lds + OFF_DWTAB + G::BUF * 768;
    const float* dwrow = dwtab + half * 96 + dw_row_offset(lane);  // (channel pair 4 * half; this lane's element of a record)
    bool valid;
    float mask_l, mask_r;
    int ta[3];  // own-column tap addresses (rows h-1, h, h+1) of channel pair 8 * half, as float indices into lds
    if constexpr (UT) {
        valid = ud.a[3] != 0u;
        mask_l = __builtin_bit_cast(float, ud.m.x), mask_r = __builtin_bit_cast(float, ud.m.y);
#pragma unroll
        for (int i = 0; i < 3; ++i) ta[i] = (int)ud.a[i];
    } else {
        const int pos = L::P0T - 1 + col;
        valid = col >= 1 && col <= TW && pos < G::POUT;
        const int posc = pos < G::POUT ? pos : G::POUT - 1;  // (pos >= P0T - 1 >= 0)
        const int h = posc / G::W, x = posc % G::W;
        mask_l = x > 0 ? 1.f : 0.f, mask_r = x < G::W - 1 ? 1.f : 0.f;
#pragma unroll
        for (int dh = -1; dh <= 1; ++dh) {
            const int o = G::RING ? 1 : 0;
            const int hh = h + dh - o, xx = x - o;
            const bool inside = (unsigned)hh < (unsigned)G::HI && (unsigned)xx < (unsigned)G::WI;
            const bool in_map = (unsigned)(h + dh) < (unsigned)G::H;
            const int a = inside ? hh * G::WI + xx : ((G::RING && in_map) ? G::PIN : G::PIN + 1);
            ta[dh + 1] = G::OFF_IN + pidx(half * 8, a, G::SIN);
        }
    }
    float y[8];
#pragma unroll
    for (int j = 0; j < 8; j += 2) {  // channels (cs, cs + 1) = 16M + j, + 1 (+ 8 * half through the addresses)
        const int cs = 16 * M + j;
        const int o = cs * G::SIN;    // pair-interleaved planes: channel pair cs / 2 starts at (cs / 2) * 2 * SIN
        const float2 up = *reinterpret_cast<const float2*>(lds + ta[0] + o);
        const float2 mid = *reinterpret_cast<const float2*>(lds + ta[1] + o);
        const float2 dn = *reinterpret_cast<const float2*>(lds + ta[2] + o);
        DwPair wp;
        wp.w = *reinterpret_cast<const float2*>(dwrow + (cs >> 1) * 24);
        y[j] = stencil3x3_of_pair<false, 0>(wp, up.x, mid.x, dn.x, mask_l, mask_r);
        y[j + 1] = stencil3x3_of_pair<false, 1>(wp, up.y, mid.y, dn.y, mask_l, mask_r);
    }
    floatx16 acc0 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, acc1 = acc0;
    if constexpr (NP == 2) {  // f16 pair: (hi,lo) (lo,hi) (hi,hi)
        uintx4 bh, bl;
        split_pair8_scaled(y, bh, bl);  // (ends with the two wait states a matrix operand needs)
        acc0 = mfma_f16(af[0][0], bl, acc0);
        acc1 = mfma_f16(af[1][0], bl, acc1);
        acc0 = mfma_f16(af[0][1], bh, acc0);
        acc1 = mfma_f16(af[1][1], bh, acc1);
        acc0 = mfma_f16(af[0][0], bh, acc0);
        acc1 = mfma_f16(af[1][0], bh, acc1);
    } else {
        uintx4 bh, bm, bl;
        split3(y, bh, bm, bl);
#pragma unroll
        for (int q = 0; q < 6; ++q) {  // the six piece products, smallest first
            const int pa = q == 0 ? 2 : (q == 2 || q == 3) ? 1 : 0;
            const uintx4& b = (q == 0 || q == 3 || q == 5) ? bh : (q == 1 ? bl : bm);
            acc0 = mfma_bf16(af[0][pa], b, acc0);
            acc1 = mfma_bf16(af[1][pa], b, acc1);
        }
    }
    // accumulator registers 4q .. 4q+3 are output channels 8q + 4 * half + (0..3) (row_of): one 16-byte store each
    if (valid) {  // (plain stores of the accumulators: the compiler waits out the matrix-core write itself)
        float4* part4 = reinterpret_cast<float4*>(lds + L::OFF_PART + M * L::PART + (col - 1) * L::CSTRIDE) + half;  // (valid: 1 <= col <= NP)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            part4[2 * q] = make_float4(acc0[4 * q], acc0[4 * q + 1], acc0[4 * q + 2], acc0[4 * q + 3]);
            part4[8 + 2 * q] = make_float4(acc1[4 * q], acc1[4 * q + 1], acc1[4 * q + 2], acc1[4 * q + 3]);
        }
    }
}

// Wavefront priority in the block phases (PRIO: the persistent batched kernels).  A SIMD carries two wavefronts, w and w + 4;
// VALU issue between them goes by priority, then age, so at equal priority the older one (0-3) runs a unit at its lone speed and
// the younger gets the leftover slots -- and whenever one of the two runs out of work first the SIMD spends the rest of the
// block with one busy wavefront, at about two thirds of its throughput ("Wavefront priority per block").  s_setprio
// moves issue slots and nothing else: the results are the same bits.  It changes only at a wavefront's own unit boundaries and
// is 0 again in front of every barrier.
//   block 1 (f16 pairs): whichever of the quarter wavefronts 4-7 combines the leftover tile does so at 1 -- the combine was the
//            block's tail, done in the slots the tile of 0-3 left over
//   block 2: 0-3 at 2 for their tile and at 0 for their quarter, 4-7 at 1 throughout: both halves end together
//   block 4: 4-7 at 1 for their first unit and at 0 for their second: 0-3 still finish first and stage the next clip, but
//            under a shorter lone tail of 4-7
// Blocks 3 and conv1 are balanced as they are.  KWS_DSCNN_PRIO_BLOCKS: bit n - 1 set = block n runs its schedule (A/B builds).
// s_setprio is a scalar instruction and ignores EXEC: every raise sits under a condition formed through readfirstlane, so that
// it lowers to a scalar branch and not to an exec mask around an unconditional s_setprio, which would raise every wavefront
// and change nothing (tests/test_dscnn_priority_isa.py holds the device assembly to that).
#ifndef KWS_DSCNN_PRIO_BLOCKS
#define KWS_DSCNN_PRIO_BLOCKS 0xb
#endif
template <int N>
constexpr bool kPrioBlock = ((KWS_DSCNN_PRIO_BLOCKS >> (N - 1)) & 1) != 0;
__device__ __forceinline__ void set_wave_priority(int p) {  // p: a compile-time constant at every call
    __builtin_amdgcn_sched_barrier(0);
    if (p == 0)
        __builtin_amdgcn_s_setprio(0);
    else if (p == 1)
        __builtin_amdgcn_s_setprio(1);
    else
        __builtin_amdgcn_s_setprio(2);
    __builtin_amdgcn_sched_barrier(0);
}

// A quarter wavefront of block N's leftover tile, behind leftover_partial_unit: it counts itself in at OFF_ARRIVE, and the one of
// the four that counts in last (it reads 3) combines the tile alone, 64 lanes striding over it four channels at a time: output = relu(bias + the four
// k-block partials, added in a fixed order).  Nobody waits for another wavefront.  The LDS instructions of a wavefront execute in
// order, so a wavefront's partial stores are done when its count is, and whoever reads 3 reads finished partials.  The waits are
// on lgkmcnt alone: the requests for the next block's operands, issued by the caller, stay in flight.  The combining wavefront
// leaves the counter at zero, for block 2 and for the next clip.  Returns the largest value stored (zero on the other three).
template <int N, int RAISE = 0>  // RAISE: the priority the combining wavefront takes for the combine (0: it keeps its own)
__device__ __forceinline__ float leftover_arrive(float* lds, int lane) {
    using G = Blk<N>;
    using L = Leftover<N>;
    int* arrived = reinterpret_cast<int*>(lds + OFF_ARRIVE);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wavefront's partial stores
    int before = 0;
    if (lane == 0) before = __hip_atomic_fetch_add(arrived, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    before = __builtin_amdgcn_readfirstlane(before);
    asm volatile("" ::: "memory");  // (no partial is read ahead of the count)
    float mx = 0.f;
    if (before == 3) {
        if constexpr (RAISE != 0) set_wave_priority(RAISE);
        // An item is four consecutive output channels of one position: four 16-byte reads (one per k-block), two 8-byte stores
        // (the planes are interleaved in channel pairs).  Lane l takes the channels 4 (l & 15) .. + 3 of position (l >> 4) + 4 r
        // in round r; RB rounds' reads are in flight before the first of their stores.
        const float4* part4 = reinterpret_cast<const float4*>(lds + L::OFF_PART);
        float* zout = lds + G::OFF_OUT;
        const int cq = lane & 15;
        const float4 b = reinterpret_cast<const float4*>(lds + OFF_PWB + G::BUF * 64)[cq];  // (pwb is stored in the accumulators' units)
        constexpr int ROUNDS = (L::NP + 3) / 4, RB = 2;
        static_assert(ROUNDS % RB == 0, "whole batches");
        auto comb = [&](float p0, float p1, float p2, float p3, float bias) { return relu(((p0 + p1) + (p2 + p3)) + bias); };
#pragma unroll 1
        for (int r0 = 0; r0 < ROUNDS; r0 += RB) {
            float4 p[RB][4];
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int j = (lane >> 4) + 4 * (r0 + r);
                const int jc = j < L::NP ? j : L::NP - 1;  // (a lane past the tile reads its last position and stores nothing)
#pragma unroll
                for (int m = 0; m < 4; ++m) p[r][m] = part4[(m * L::PART + jc * L::CSTRIDE) / 4 + cq];
            }
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int j = (lane >> 4) + 4 * (r0 + r);
                const float4(&q)[4] = p[r];
                const float v0 = comb(q[0].x, q[1].x, q[2].x, q[3].x, b.x), v1 = comb(q[0].y, q[1].y, q[2].y, q[3].y, b.y);
                const float v2 = comb(q[0].z, q[1].z, q[2].z, q[3].z, b.z), v3 = comb(q[0].w, q[1].w, q[2].w, q[3].w, b.w);
                if (j < L::NP) {
                    *reinterpret_cast<float2*>(zout + pidx(4 * cq, L::P0T + j, G::SOUT)) = make_float2(v0, v1);
                    *reinterpret_cast<float2*>(zout + pidx(4 * cq + 2, L::P0T + j, G::SOUT)) = make_float2(v2, v3);
                    mx = fmaxf(mx, fmaxf(fmaxf(v0, v1), fmaxf(v2, v3)));
                }
            }
        }
        if (lane == 0) *arrived = 0;
    }
    return mx;
}

// ------------------------------------------------------------------------------------------------
// One depthwise-separable block.  pwo: pointwise operands of THIS block on entry (f32: all of them; split:
// k-block 0 in ring[0]); on exit (N < 4) the loads of the next block's have been issued into it, so they fly
// across the barrier.
// MODE: 0 = pointwise GEMM on the VALU (cross-check of the MFMA operand mappings), 1 = f32 MFMA,
// 4 = split-bf16 MFMA (product path), 2 / 3 = timing ablations of mode 1 (matrix core only / stencil only;
// wrong results by construction).
// act4 (diagnostics instantiation only, block 4): global [64][53*9] that receives the block's output, which the product
// path never stores (it is pooled in registers).
// RANGED: only the positions rg.lo .. rg.hi - 1 (whole rows) are computed -- one time tile of a workgroup cluster.
// UT (persistent batched kernel, whole maps): a unit's geometry comes from its descriptor.  ud: on entry the descriptor of this
// wavefront's FIRST unit of this block (a tile, or its quarter of block 1's leftover tile), requested by the caller or by the
// previous block; on exit (N < 4) the request for its first unit of the next block.  Every later unit's descriptor is
// requested beside the A operands of that unit, in front of them.  Not read or written without UT.
// PRIO (persistent batched kernel, whole maps): the block's wavefront-priority schedule, see above.
template <int N, int MODE, bool RANGED = false, bool UT = false, bool PRIO = false>
__device__ __forceinline__ void block_phase(const DscnnWeights& w, float* lds, int tid, PwOperands<MODE>& pwo, UnitDesc& ud,
                                            float* __restrict__ act4 = nullptr, PosRange rg = PosRange{0, 0}, PairCtx pc = PairCtx{},
                                            int off_poolbuf = OFF_POOLBUF) {
    static_assert(!UT || ((MODE == 4 || MODE == 5) && !RANGED && Leftover<1>::HAS), "unit descriptors: product paths on whole maps");
    using G = Blk<N>;
    constexpr bool PAIR = MODE == 5;          // f16 pairs: three products per k-block, activations in per-clip scaled units
    constexpr int NP = PAIR ? 2 : 3;
    constexpr int NPROD = PAIR ? 3 : 6;
    // the leftover tile of blocks 1 / 2 is K-split over four wavefronts (product paths on whole maps only)
    constexpr bool KSL = Leftover<N>::HAS && (MODE == 4 || MODE == 5) && !RANGED;
    const int p_lo = RANGED ? rg.lo : 0, p_hi = RANGED ? rg.hi : G::POUT;
#ifdef KWS_X_DSCNN_SKIP_LEFTOVER  // timing experiment (wrong results): block 2 without its ninth tile, the upper bound of what
                                  // spreading that tile over idle wavefronts could win
    const int n_tiles = RANGED ? (p_hi - p_lo + TW - 1) / TW : (N == 2 ? 8 : G::TILES);
#else
    const int n_tiles = RANGED ? (p_hi - p_lo + TW - 1) / TW : (KSL ? Leftover<N>::TILE : G::TILES);
#endif
    constexpr bool MFMA = MODE != 0;
    constexpr bool SPLIT = MODE >= 4;  // input channel of step s: 16(s>>3) + 8*half + (s&7) instead of 2s + half
    // timing ablation of the split path (wrong results by construction): 6 = split + matrix core without the stencil
    constexpr bool NO_STENCIL = MODE == 6;
    const int lane = tid & 63, wv = tid >> 6, half = lane >> 5, col = lane & 31;
    float* zout = lds + G::OFF_OUT;
    const float* dwtab = lds + OFF_DWTAB + G::BUF * 768;
    const float* pwb = lds + OFF_PWB + G::BUF * 64;
    float* poolbuf = lds + off_poolbuf;  // block 4's pool partials (PERSIST: OFF_POOLBUF_P)
    static_assert(!PRIO || ((MODE == 4 || MODE == 5) && !RANGED && NW == 8), "priority schedules: product paths on whole maps, two wavefronts per SIMD");
    constexpr bool PR = PRIO && kPrioBlock<N> && (N == 2 || N == 4);                 // the block's units run under a schedule
    constexpr int COMBINE_AT = (PRIO && kPrioBlock<N> && N == 1 && MODE == 5) ? 1 : 0;  // the leftover tile's combine is raised
    // the wavefront index as a scalar the compiler knows to be one: the conditions around s_setprio must be scalar branches
    const int wv_s = PR ? __builtin_amdgcn_readfirstlane(wv) : 0;
    if constexpr (PR) {
        if constexpr (N == 2) {
            if (wv_s < 4) set_wave_priority(2);
        }
        if (wv_s >= 4) set_wave_priority(1);
    }

    // The other table buffer is idle during this block: the next block's tables are fetched now and
    // stored after the units.  Ring and zero slots of the output planes.  No barrier needed before the
    // units: everything they read was staged during the previous phase.
    BlockTables next_tables;
    if constexpr (N < 4) {
        fetch_block_tables(w, N + 1, tid, next_tables);
        if (tid < CH) {
            zout[pidx(tid, G::POUT, G::SOUT)] = relu(pwb[tid]);
            zout[pidx(tid, G::POUT + 1, G::SOUT)] = 0.f;
        }
    } else if (!MFMA) {
        poolbuf[wv * CH + lane] = 0.f;  // the VALU path accumulates into its wave's scratch row
    }

    // accumulator rows 4q..4q+3 of tile ct are output channels ct*32 + 8q + 4*half + (0..3): one float4
    const float4* bias4 = reinterpret_cast<const float4*>(pwb) + half;
    // lane (column, half) walks the input channels 16m + 8*half + j (m = 0..3, j = 0..7) in 32 steps s = 8m + j
    const float* dwrow = dwtab + half * 96 + dw_row_offset(lane);  // (channel pair 4 * half; this lane's element of a record of 24 floats)
    float psum[2][16];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) psum[ct][r] = 0.f;
    float stage_max = 0.f;  // PAIR, blocks 1 and 2: this wavefront's largest stored output

    for (int t = wv; t < n_tiles; t += NW) {
        // column j of the tile is output position p_lo + t*TW - 1 + j: columns 0 and 31 are halo.  A halo column past the
        // range's ends is clamped into it: a range ends on a row end, where the neighbour's contribution is masked anyway,
        // and the clamp keeps the lane's own reads on rows this workgroup has computed.
        const int pos = p_lo + t * TW - 1 + col;
        bool valid;
        uint32_t keep;  // valid as all ones / all zeros
        float mask_l, mask_r;
        // own-column tap addresses (rows h-1, h, h+1), as float indices into lds, for channel pairs
        // 0..15 (lo) and 16..31 (hi): two bases keep every ds_read inside the 64 KiB immediate window;
        // the empty asm stops the compiler from re-deriving one base register per step.
        int tlo[3], thi[3];
        if constexpr (UT) {
            keep = ud.a[3];
            valid = keep != 0u;
            mask_l = __builtin_bit_cast(float, ud.m.x), mask_r = __builtin_bit_cast(float, ud.m.y);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                tlo[i] = (int)ud.a[i];
                thi[i] = tlo[i] + 32 * G::SIN;
                asm volatile("" : "+v"(tlo[i]));
                asm volatile("" : "+v"(thi[i]));
            }
        } else {
            valid = col >= 1 && col <= TW && pos < p_hi;
            keep = valid ? 0xffffffffu : 0u;
            const int posc = pos < p_lo ? p_lo : (pos < p_hi ? pos : p_hi - 1);
            const int h = posc / G::W, x = posc % G::W;
            mask_l = x > 0 ? 1.f : 0.f, mask_r = x < G::W - 1 ? 1.f : 0.f;
#pragma unroll
            for (int dh = -1; dh <= 1; ++dh) {
                const int o = G::RING ? 1 : 0;
                const int hh = h + dh - o, xx = x - o;
                const bool inside = (unsigned)hh < (unsigned)G::HI && (unsigned)xx < (unsigned)G::WI;
                const bool in_map = (unsigned)(h + dh) < (unsigned)G::H;
                const int a = inside ? hh * G::WI + xx : ((G::RING && in_map) ? G::PIN : G::PIN + 1);
                tlo[dh + 1] = G::OFF_IN + pidx(half * 8, a, G::SIN);
                thi[dh + 1] = tlo[dh + 1] + 32 * G::SIN;
                asm volatile("" : "+v"(tlo[dh + 1]));
                asm volatile("" : "+v"(thi[dh + 1]));
            }
        }
        UnitDesc ud_next = ud;  // UT: the descriptor this wavefront reads next, requested in the last k-block

        auto cs_of = [](int s) { return 16 * (s >> 3) + (s & 7); };  // channel of step s minus the half's offset 8*half
        // the own-column inputs of channels (cs, cs+1), cs even, in three 8-byte reads (pair-interleaved planes)
        struct TapPair {
            float2 up, mid, dn;
        };
        auto tap_pair_load = [&](int sp, TapPair& tp) {  // sp: pair of steps (2sp, 2sp+1)
            const int cs = cs_of(2 * sp);
            const int* ta = cs < 32 ? tlo : thi;
            const int o = (cs & 31) * G::SIN;
            if constexpr (!NO_STENCIL) {
                tp.up = *reinterpret_cast<const float2*>(lds + ta[0] + o);
                tp.dn = *reinterpret_cast<const float2*>(lds + ta[2] + o);
            }
            tp.mid = *reinterpret_cast<const float2*>(lds + ta[1] + o);
        };
        // the depthwise weights of the step pair's two channels: one 8-byte read, a row of lanes holds the record (DwPair)
        auto wts_pair_load = [&](int sp, DwPair& wp) {
            const int cs = cs_of(2 * sp);
            wp.w = *reinterpret_cast<const float2*>(dwrow + (cs >> 1) * 24);
        };
        // depthwise 3x3 (+bias) of step 2sp + odd at this lane's column -> one MFMA B operand element
        auto dw_eval = [&](const DwPair& wp, const TapPair& tq, auto odd) -> float {
            constexpr int E = decltype(odd)::value;
            return stencil3x3_of_pair<(MFMA && !SPLIT), E>(wp, E ? tq.up.y : tq.up.x, E ? tq.mid.y : tq.mid.x, E ? tq.dn.y : tq.dn.x, mask_l, mask_r);
        };

        if constexpr (MFMA) {
            floatx16 acc0, acc1;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 b0 = bias4[2 * q], b1 = bias4[8 + 2 * q];
                acc0[4 * q + 0] = b0.x; acc0[4 * q + 1] = b0.y; acc0[4 * q + 2] = b0.z; acc0[4 * q + 3] = b0.w;
                acc1[4 * q + 0] = b1.x; acc1[4 * q + 1] = b1.y; acc1[4 * q + 2] = b1.z; acc1[4 * q + 3] = b1.w;
            }
            // software pipeline, two steps deep: reads of step s+2 are issued before step s is evaluated
            DwPair wq0, wq1;   // depthwise weights of step pairs, two pairs in flight
            TapPair tq0, tq1;  // inputs of step pairs, two pairs in flight
            if constexpr (!NO_STENCIL) {
                wts_pair_load(0, wq0);
                wts_pair_load(1, wq1);
            }
            tap_pair_load(0, tq0);
            tap_pair_load(1, tq1);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (SPLIT) {
                // eight depthwise outputs fill one k-block of 16 input channels (8 per half-wave); they are split
                // into three bf16 pieces and multiplied with the pre-split weights: 6 products x 2 channel tiles.
                // The bf16 matrix pipe runs beside the VALU, so the stencil of the next k-block overlaps them.
                // The 12 MFMAs of k-block m are issued one per half step while the VALU evaluates the stencil of
                // k-block m+1 (sched_barrier pins that interleave; left alone, the compiler issues them back to back
                // and the wavefront sits behind the busy matrix pipe).  Smallest products first.
                float y[8];
                uintx4 bh, bm, bl;
                auto product = [&](int ct, int m, int q) {  // q-th of the piece products of k-block m, channel tile ct
                    // triple: (lo,hi) (hi,lo) (mid,mid) (mid,hi) (hi,mid) (hi,hi); pair: (hi,lo) (lo,hi) (hi,hi)
                    const int pa = PAIR ? (q == 1 ? 1 : 0) : (q == 0 ? 2 : (q == 2 || q == 3) ? 1 : 0);
                    const uintx4& b = PAIR ? (q == 0 ? bl : bh) : ((q == 0 || q == 3 || q == 5) ? bh : (q == 1 ? bl : bm));
                    if constexpr (PAIR) {
                        if (ct == 0)
                            acc0 = mfma_f16(pwo.ring[m & 1][0][pa], b, acc0);
                        else
                            acc1 = mfma_f16(pwo.ring[m & 1][1][pa], b, acc1);
                    } else {
                        if (ct == 0)
                            acc0 = mfma_bf16(pwo.ring[m & 1][0][pa], b, acc0);
                        else
                            acc1 = mfma_bf16(pwo.ring[m & 1][1][pa], b, acc1);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                };
#pragma unroll
                for (int s = 0; s < 32; ++s) {
                    const int m = s >> 3, j = s & 7;
                    DwPair& wp = (s & 2) ? wq1 : wq0;
                    TapPair& tq = (s & 2) ? tq1 : tq0;  // step pair s >> 1
                    const bool feed = m > 0 && j < NPROD;
                    if (feed) product(0, m - 1, j);
                    if constexpr (NO_STENCIL)
                        y[j] = (s & 1) ? tq.mid.y : tq.mid.x;
                    else
                        y[j] = (s & 1) ? dw_eval(wp, tq, std::integral_constant<int, 1>{}) : dw_eval(wp, tq, std::integral_constant<int, 0>{});
                    __builtin_amdgcn_sched_barrier(0);
                    if (feed) product(1, m - 1, j);
                    if ((s & 1) && s + 3 < 32) {  // both steps of the pair are done: its registers take the pair after the next
                        if constexpr (!NO_STENCIL) wts_pair_load((s >> 1) + 2, wp);
                        tap_pair_load((s >> 1) + 2, tq);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if (j == 6) {
                        // the products of k-block m-1 are done: its ring slot takes k-block m+1, or k-block 0 of
                        // this wave's next unit / of the next block (UT: that unit's descriptor in front of it -- the tap
                        // addresses of this unit were last read four steps ago)
                        if (m < 3) {
                            load_afrag(w, N, m + 1, lane, pwo.ring[(m + 1) & 1]);
                        } else if (t + NW < n_tiles) {
                            if constexpr (UT) load_unit_desc(w, N, t + NW, lane, ud_next);
                            load_afrag(w, N, 0, lane, pwo.ring[0]);
                        } else if (KSL && N == 2 && wv < 4) {
                            if constexpr (UT) load_unit_desc(w, N, Leftover<N>::TILE, lane, ud_next);
                            load_afrag(w, N, wv, lane, pwo.ring[0]);  // this wavefront's quarter of the leftover tile comes next
                        } else if (N < 4) {
                            // (blocks 2 - 4 have a tile for every wavefront: its first unit there is tile wv)
                            if constexpr (UT) load_unit_desc(w, N < 4 ? N + 1 : N, wv, lane, ud_next);
                            load_afrag(w, N < 4 ? N + 1 : N, 0, lane, pwo.ring[0]);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if (j == 7) {
                        if constexpr (PAIR) {
                            split_pair8_scaled(y, bh, bl);  // (the next product reads bl a stencil evaluation later; the operand
                                                            // scale sits in the depthwise table: store_block_tables)
                        } else {
                            split3(y, bh, bm, bl);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
#pragma unroll
                for (int q = 0; q < NPROD; ++q) {
                    product(0, 3, q);
                    product(1, 3, q);
                }
            } else {
                auto& wa = pwo.wa;
#pragma unroll
                for (int s = 0; s < 32; s += 2) {  // one pair of k-steps per iteration
                    TapPair& tq = (s & 2) ? tq1 : tq0;
                    DwPair& wp = (s & 2) ? wq1 : wq0;
                    float y0, y1;
                    if constexpr (MODE == 2) {  // timing ablation: matrix core only (results are wrong)
                        y0 = tq.mid.x;
                        y1 = tq.mid.y;
                    } else {
                        y0 = dw_eval(wp, tq, std::integral_constant<int, 0>{});
                        y1 = dw_eval(wp, tq, std::integral_constant<int, 1>{});
                        if (s + 4 < 32) {
                            wts_pair_load((s >> 1) + 2, wp);
                            tap_pair_load((s >> 1) + 2, tq);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if constexpr (MODE == 3) {  // timing ablation: stencil only (results are wrong)
                        acc0[0] += y0 * wa[0][s];
                        acc1[0] += y1 * wa[1][s + 1];
                    } else {
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[0][s], y0, acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[1][s], y0, acc1, 0, 0, 0);
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[0][s + 1], y1, acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[1][s + 1], y1, acc1, 0, 0, 0);
                    }
                }
            }
            auto epilogue = [&]() {
                // relu() is inline asm: the compiler's hazard recognizer does not see that it reads MFMA results, and the
                // hardware does not interlock a VALU read behind a matrix-core write (XDL write -> VALU read: up to 18 wait
                // states for a 16-pass MFMA).  The wait is spelled out here; the +v ties pin it after the last MFMA.
                // (Round 1's `valid ? relu(x) : 0` happened to put an exec-mask branch in between; a branch-free select
                // read stale accumulators: nondeterministic sums.)
#ifndef KWS_X_NO_MFMA_EPILOGUE_NOP  // (the switch exists for tests/test_isa_hazards.py: without the wait the lint must fail)
                asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc0), "+v"(acc1));
#endif
                if constexpr (N < 4) {
                    if constexpr (PAIR && N <= 2) {
                        // the largest stored value (halo columns hold outputs of real positions too): the scale of the block
                        // after the next is derived from it.  One exec-masked region for the stores, none for the maximum.
                        float o0[16], o1[16];
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            o0[r] = relu(acc0[r]);
                            o1[r] = relu(acc1[r]);
                        }
#pragma unroll
                        for (int r = 0; r < 16; r += 2) stage_max = fmaxf(stage_max, fmaxf(fmaxf(o0[r], o0[r + 1]), fmaxf(o1[r], o1[r + 1])));
                        if (valid) {
#pragma unroll
                            for (int r = 0; r < 16; r += 2) {
                                *reinterpret_cast<float2*>(zout + pidx(row_of(r, half), pos, G::SOUT)) = make_float2(o0[r], o0[r + 1]);
                                *reinterpret_cast<float2*>(zout + pidx(32 + row_of(r, half), pos, G::SOUT)) = make_float2(o1[r], o1[r + 1]);
                            }
                        }
                    } else if (valid) {
#pragma unroll
                        for (int r = 0; r < 16; r += 2) {  // rows r, r+1 are adjacent output channels: one 8-byte store
                            *reinterpret_cast<float2*>(zout + pidx(row_of(r, half), pos, G::SOUT)) =
                                make_float2(relu(acc0[r]), relu(acc0[r + 1]));
                            *reinterpret_cast<float2*>(zout + pidx(32 + row_of(r, half), pos, G::SOUT)) =
                                make_float2(relu(acc1[r]), relu(acc1[r + 1]));
                        }
                    }
                } else {
                    // relu is an asm statement: written as `valid ? relu(x) : 0` every element became its own exec-masked
                    // branch region (16 per unit).  An AND with an all-ones / all-zeros mask selects without a branch -- and,
                    // unlike a 0/1 factor, also if a halo lane ever held a NaN.
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        psum[0][r] += __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, relu(acc0[r])) & keep);
                        psum[1][r] += __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, relu(acc1[r])) & keep);
                    }
                    if (act4 && valid) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            act4[row_of(r, half) * G::POUT + pos] = relu(acc0[r]) * pc.inv_out;
                            act4[(32 + row_of(r, half)) * G::POUT + pos] = relu(acc1[r]) * pc.inv_out;
                        }
                    }
                }
            };
            // this wave's last unit: the A operands are dead, so the next block's are fetched now and the
            // loads fly under the epilogue, the barrier and the next prologue
            if constexpr (!SPLIT) {
                if (N < 4 && t + NW >= n_tiles) {
                    __builtin_amdgcn_sched_barrier(0);  // not before the last MFMA has read the old operands
                    if constexpr (N < 4) load_pointwise(w, N + 1, lane, pwo);
                    __builtin_amdgcn_sched_barrier(0);
                    epilogue();
                    break;
                }
            }
            epilogue();
            if constexpr (UT) ud = ud_next;
#ifndef KWS_X_DSCNN_PRIO_STATIC4  // diagnostics builds: wavefronts 4-7 keep priority 1 for the whole of block 4 (the test that the
                                  // hardware honours it: the halves swap roles)
            if constexpr (PR && N == 4) set_wave_priority(0);  // a unit boundary: the second unit of 4-7 runs at 0, behind the older partner
#endif
        } else {
            // VALU cross-check of the pointwise GEMM: each half sums its 32 input channels, halves are
            // combined with a lane exchange.
            const float* pw_w = w.pw_w + (N - 1) * CH * CH;
            float y[32];
#pragma unroll
            for (int s = 0; s < 32; s += 2) {
                TapPair tq;
                tap_pair_load(s >> 1, tq);
                DwPair wp;
                wts_pair_load(s >> 1, wp);
                y[s] = dw_eval(wp, tq, std::integral_constant<int, 0>{});
                y[s + 1] = dw_eval(wp, tq, std::integral_constant<int, 1>{});
            }
#pragma unroll 1
            for (int co = 0; co < CH; ++co) {
                float part = 0.f;
#pragma unroll
                for (int s = 0; s < 32; ++s) part = fmaf(pw_w[(16 * (s >> 3) + 8 * half + (s & 7)) * CH + co], y[s], part);
                const float tot = relu(part + __shfl_xor(part, 32, 64) + pwb[co]);
                if constexpr (N < 4) {
                    if (valid && half == 0) zout[pidx(co, pos, G::SOUT)] = tot;
                } else {
                    // pool: sum this tile's positions and accumulate into the wave's own scratch row
                    if (act4 && valid && half == 0) act4[co * G::POUT + pos] = tot;
                    float sum = (valid && half == 0) ? tot : 0.f;
#pragma unroll
                    for (int o = 16; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
                    if (lane == 0) poolbuf[wv * CH + co] += sum;
                }
            }
        }
    }

    if constexpr (KSL) {
        using L = Leftover<N>;
        if (wv >= L::WAVE0 && wv < L::WAVE0 + 4) {
            if constexpr (PR && N == 2) set_wave_priority(0);  // the quarter of 0-3 runs behind the tile of 4-7 (still at 1)
            leftover_partial_unit<N, NP, UT>(lds, lane, wv - L::WAVE0, pwo.ring[0], ud);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (UT) load_unit_desc(w, N + 1, wv, lane, ud);  // (block 2 has a tile for every wavefront, block 3 too)
            load_afrag(w, N + 1, 0, lane, pwo.ring[0]);  // the next block's first operands fly across the barrier
            __builtin_amdgcn_sched_barrier(0);
            // the last of the four to get here combines the tile; its maximum joins this wavefront's (a maximum is exact in any order)
            stage_max = fmaxf(stage_max, leftover_arrive<N, COMBINE_AT>(lds, lane));
        }
    }
    if constexpr (PR || COMBINE_AT != 0) set_wave_priority(0);  // the units are done: everyone is at 0 again in front of the block's barrier
    if constexpr (N < 4) store_block_tables(lds, N + 1, tid, next_tables, pc.s_dwb, pc.s_pwb, pc.s_dww);
    if constexpr (PAIR && N <= 2) publish_wave_max(lds, N == 1 ? 2 : 0, wv, lane, stage_max);
    if constexpr (MFMA) {
        if constexpr (N < 4) {
            if (wv >= n_tiles && !(KSL && N == 1)) load_block_head(w, N + 1, lane, pwo);  // waves without a unit in this block
        } else {
            // reduce the pool partials over the positions held by each half-wave (DPP, no LDS round trips).  Step-major:
            // all 32 sums take a shift step before any takes the next, so a value is read by DPP well after it was written and
            // the VALU -> DPP wait states cost no s_nop (register-major the compiler padded every add: 132 s_nop per clip
            // and wavefront; as builtins it splits every add into v_mov_b32_dpp + v_add_f32).
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                float (&q)[16] = psum[ct];
                // sixteen sums per block, step-major and fused (v_add_f32_dpp reads its own destination shifted): a register is
                // read by DPP sixteen instructions after it was written, so no wait states are owed
                asm volatile("s_nop 4\n\t"  // also covers an EXEC write just before the block (5 wait states before DPP)
                    "v_add_f32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %1, %1, %1 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %2, %2, %2 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %3, %3, %3 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %4, %4, %4 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %5, %5, %5 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %6, %6, %6 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %7, %7, %7 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %8, %8, %8 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %9, %9, %9 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %10, %10, %10 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %11, %11, %11 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %12, %12, %12 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %13, %13, %13 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %14, %14, %14 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %15, %15, %15 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %1, %1, %1 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %2, %2, %2 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %3, %3, %3 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %4, %4, %4 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %5, %5, %5 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %6, %6, %6 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %7, %7, %7 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %8, %8, %8 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %9, %9, %9 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %10, %10, %10 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %11, %11, %11 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %12, %12, %12 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %13, %13, %13 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %14, %14, %14 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %15, %15, %15 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %1, %1, %1 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %2, %2, %2 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %3, %3, %3 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %4, %4, %4 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %5, %5, %5 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %6, %6, %6 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %7, %7, %7 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %8, %8, %8 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %9, %9, %9 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %10, %10, %10 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %11, %11, %11 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %12, %12, %12 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %13, %13, %13 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %14, %14, %14 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %15, %15, %15 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %1, %1, %1 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %2, %2, %2 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %3, %3, %3 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %4, %4, %4 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %5, %5, %5 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %6, %6, %6 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %7, %7, %7 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %8, %8, %8 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %9, %9, %9 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %10, %10, %10 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %11, %11, %11 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %12, %12, %12 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %13, %13, %13 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %14, %14, %14 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %15, %15, %15 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                    "v_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                    "v_add_f32_dpp %1, %1, %1 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                    "v_add_f32_dpp %2, %2, %2 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                    "v_add_f32_dpp %3, %3, %3 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                    "v_add_f32_dpp %4, %4, %4 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                    "v_add_f32_dpp %5, %5, %5 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                    "v_add_f32_dpp %6, %6, %6 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                    "v_add_f32_dpp %7, %7, %7 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                    "v_add_f32_dpp %8, %8, %8 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                    "v_add_f32_dpp %9, %9, %9 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                    "v_add_f32_dpp %10, %10, %10 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                    "v_add_f32_dpp %11, %11, %11 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                    "v_add_f32_dpp %12, %12, %12 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                    "v_add_f32_dpp %13, %13, %13 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                    "v_add_f32_dpp %14, %14, %14 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                    "v_add_f32_dpp %15, %15, %15 row_bcast:15 row_mask:0xa bank_mask:0xf"
                    : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]), "+v"(q[4]), "+v"(q[5]), "+v"(q[6]), "+v"(q[7]), "+v"(q[8]), "+v"(q[9]), "+v"(q[10]), "+v"(q[11]), "+v"(q[12]), "+v"(q[13]), "+v"(q[14]), "+v"(q[15]));
            }
            if (col == 31) {
#pragma unroll
                for (int k = 0; k < 32; ++k) poolbuf[wv * CH + (k >> 4) * 32 + row_of(k & 15, half)] = psum[k >> 4][k & 15] * pc.inv_out;
            }
        }
    }
    (void)bias4;
}

// conv1's pre-split A operands of channel tile wv & 1, all seven k-blocks (split paths)
template <int NP>
__device__ __forceinline__ void load_conv1_frags(const DscnnWeights& w, int wv, int lane, uintx4 (&c1f)[7][NP]) {
    const uintx4* src = reinterpret_cast<const uintx4*>(NP == 2 ? w.c1_pair : w.c1_split) + (size_t)(wv & 1) * (7 * NP * 64) + lane;
#pragma unroll
    for (int kb = 0; kb < 7; ++kb)
#pragma unroll
        for (int p = 0; p < NP; ++p) c1f[kb][p] = src[(kb * NP + p) * 64];
}

// Argmax over lanes 0 .. C-1 of a wavefront, first maximum wins: wave maximum by DPP (no LDS round trips; six dependent
// __shfl_xor rounds through ds_bpermute were 1.4 k of the 2.6 k cycles the classifier tail took), then the lowest lane that
// holds it.  v = -inf in lanes >= C.
__device__ __forceinline__ int wave_argmax_first(float v, int lane, int C) {
    float m = v;
    m = fmaxf(m, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, m), __builtin_bit_cast(int, m), 0x111, 0xf, 0xf, false)));
    m = fmaxf(m, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, m), __builtin_bit_cast(int, m), 0x112, 0xf, 0xf, false)));
    m = fmaxf(m, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, m), __builtin_bit_cast(int, m), 0x114, 0xf, 0xf, false)));
    m = fmaxf(m, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, m), __builtin_bit_cast(int, m), 0x118, 0xf, 0xf, false)));
    m = fmaxf(m, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, m), __builtin_bit_cast(int, m), 0x142, 0xa, 0xf, false)));
    m = fmaxf(m, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, m), __builtin_bit_cast(int, m), 0x143, 0xc, 0xf, false)));
    const float vmax = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, m), 63));
    const unsigned long long holders = __ballot(lane < C && v == vmax);
    return holders ? __ffsll(holders) - 1 : 0;  // all-NaN logits: label 0
}

}  // namespace
}  // namespace kws
