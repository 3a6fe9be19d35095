// Geometry of the LDS-resident DS-CNN forward kernel (kws_dscnn.hip): workgroup shape, LDS map, per-block planes, leftover tiles
// and the persistent launch's offsets, with the assertions that hold them together.  Also read by kws_conv1_general_kernel
// (kws_dsblock.hip).  Anonymous namespace: one copy per translation unit.
//
// LDS map (floats): planes hold P+2 floats and are interleaved in channel pairs (see pidx)
//   Z3 (block3 out, 51x7)  @ 0      .. 22976     Z2 (block2 out, 49x5) @ 22976 .. 38784
//   Z1 (block1 out, 47x3)  @ 0      .. 9152      Z0 (conv1 out, 47x3)  @ 9152  .. 18304
//   padded MFCC 103x14     @ 18304  .. 19746     (conv1 phase only)
//   conv1 operand windows  @ 0      .. 3090      (f16 pairs, conv1 phase only: where Z1 goes afterwards; conv1_build_windows)
//   misc                   @ 38784  .. 40960     2 x depthwise table, 2 x pointwise bias, pooled, per-wavefront stage maxima (f16 pairs)
#pragma once
#include "kws_internal.h"

namespace kws {
namespace {

#ifndef KWS_DSCNN_WAVES
#define KWS_DSCNN_WAVES 8
#endif
constexpr int NW = KWS_DSCNN_WAVES;  // wavefronts per workgroup (8 = 2 per SIMD; 12 = 3 per SIMD measured slower)
constexpr int NT = NW * 64;
constexpr int TW = 30;               // output positions per tile (32 MFMA columns - 2 halo columns)

constexpr int P0 = C1_H * C1_W;                  // 141
constexpr int FEAT_H = 103, FEAT_W = 14;         // MFCC zero-padded by 2 (top/left) and up to the conv1 reach
constexpr int OFF_Z3 = 0, OFF_Z2 = 22976, OFF_Z1 = 0, OFF_Z0 = 9152, OFF_FEAT = 18304;
constexpr int OFF_DWTAB = 38784;                 // [2][64][12]  double-buffered per block
constexpr int OFF_PWB = OFF_DWTAB + 2 * 768;     // [2][64]      pointwise bias, double-buffered
constexpr int OFF_POOLED = OFF_PWB + 2 * 64;     // [64]
constexpr int OFF_POOLBUF = OFF_DWTAB;           // [NW][64] aliases depthwise buffer 0 (idle during block 4)
constexpr int OFF_WMAX = OFF_POOLED + 64 + 8;    // [3][NW] f16-pair arithmetic: per-wavefront maxima of a stage's stored output.  Sets: features 0,
                                                 // conv1 1, block 1 2, block 2 0 (a leftover tile's maximum is folded into the slot of the
                                                 // wavefront that combined it): a set is rewritten two barriers after its last reader at the earliest
constexpr int OFF_ARRIVE = OFF_WMAX + 3 * NW;    // one dword: how many quarter wavefronts of the running block's K-split leftover tile have
                                                 // stored their partial sums (leftover_arrive); zero outside blocks 1 and 2
constexpr int LDS_FLOATS = 40960;                // 160 KiB
static_assert(OFF_ARRIVE + 1 <= LDS_FLOATS, "LDS overflow");
static_assert(NW * 64 <= 768, "pool scratch must fit one depthwise buffer");
static_assert(OFF_FEAT + FEAT_H * FEAT_W <= OFF_Z2, "feature pad overlaps Z2");
static_assert(CH * 12 <= 2 * NT, "table staging assumes at most two elements per thread");

// Activation planes in LDS are stored as channel PAIRS interleaved per position: element (c, p) of a map whose
// planes hold S floats lives at (c >> 1) * 2S + 2p + (c & 1).  One ds_read_b64 then fetches a column's value for
// two consecutive channels (the split path walks channels two at a time) and the epilogue stores two output
// channels with one ds_write_b64: half the tap reads and stores, at twice the bytes per LDS cycle.
__host__ __device__ __forceinline__ constexpr int pidx(int c, int p, int S) { return (c >> 1) * 2 * S + 2 * p + (c & 1); }

// Geometry of block N (1..4): output plane H x W (all of it is the next block's interior).
template <int N>
struct Blk {
    static constexpr int H = 45 + 2 * N, W = 1 + 2 * N;           // 47x3, 49x5, 51x7, 53x9
    static constexpr bool RING = N > 1;                            // block 1 reads conv1's output: no ring
    static constexpr int HI = RING ? H - 2 : H, WI = RING ? W - 2 : W;  // stored input plane
    static constexpr int PIN = HI * WI, SIN = PIN + 2;
    static constexpr int POUT = H * W, SOUT = POUT + 2;
    static constexpr int OFF_IN = N == 1 ? OFF_Z0 : N == 2 ? OFF_Z1 : N == 3 ? OFF_Z2 : OFF_Z3;
    static constexpr int OFF_OUT = N == 1 ? OFF_Z1 : N == 2 ? OFF_Z2 : OFF_Z3;  // block 4 stores nothing
    static constexpr int TILES = (POUT + TW - 1) / TW;
    static constexpr int BUF = (N - 1) & 1;                       // which depthwise / bias buffer it reads
};

// Leftover tiles (round 3).  Block 1 has 5 tiles and block 2 has 9 for 8 wavefronts: the fifth / ninth tile costs a whole
// extra unit on one wavefront while others idle (block 2: 12.5 k cycles for 9 tiles, block 3: 13 k for 12).  With
// KWS_DSCNN_KSPLIT_LEFTOVER that tile is cut along K instead: four wavefronts take one k-block (16 input channels, 8 steps)
// each and write their 64 x positions partial sums to a dead region of LDS; the one of the four that stores its partials last
// (an arrival counter at OFF_ARRIVE, nobody waits) adds the four partials in a fixed order, adds the bias, applies ReLU and
// stores, ahead of the block's one barrier (leftover_arrive).  Block 1: tiles 0-3 on wavefronts 0-3, the leftover on 4-7 (one
// per SIMD); block 2: tiles 0-7 on all eight, the leftover as a second, quarter-size unit of the older wavefronts 0-3.
#ifndef KWS_DSCNN_KSPLIT_LEFTOVER
#define KWS_DSCNN_KSPLIT_LEFTOVER 1
#endif
template <int N>
struct Leftover {
    static constexpr bool HAS = KWS_DSCNN_KSPLIT_LEFTOVER && (N == 1 || N == 2);
    static constexpr int TILE = N == 1 ? 4 : 8;                     // the tile that is K-split
    static constexpr int P0T = TILE * TW;                           // its first position
    static constexpr int NP = HAS ? Blk<N>::POUT - P0T : 1;         // its positions: 21 (block 1), 5 (block 2)
    static constexpr int WAVE0 = N == 1 ? 4 : 0;                    // wavefronts WAVE0 .. WAVE0 + 3 take k-blocks 0 .. 3
    static constexpr int OFF_PART = N == 1 ? OFF_Z2 : OFF_Z0;       // [4][NP][CSTRIDE] partial sums, in a plane that is dead during block N
    static constexpr int CSTRIDE = CH + 4;                          // floats per position: the 64 channels as float4s, padded so that the
                                                                    // 16-byte stores of neighbouring columns fall into different banks
    static constexpr int PART = NP * CSTRIDE;                       // floats per k-block
};
static_assert(Blk<1>::TILES == 5 && Blk<2>::TILES == 9, "the leftover tiles are the fifth of block 1 and the ninth of block 2");
static_assert(4 * Leftover<1>::PART <= 38784 - OFF_Z2 && OFF_Z0 + 4 * Leftover<2>::PART <= OFF_FEAT, "partial sums fit their dead planes");
static_assert(Leftover<1>::OFF_PART % 4 == 0 && Leftover<2>::OFF_PART % 4 == 0 && Leftover<1>::CSTRIDE % 4 == 0, "partial sums move as float4s");

// Persistent batched launch (PERSIST, kws_dscnn_fwd_kernel): a workgroup carries clips g, g + grid, ... one after another and
// the next clip is staged in block 4's tail.  Block 4 reads only Z3 and the odd table buffer, so the Z2 plane is dead from
// block 3's barrier until block 2 of the next clip: the next clip's padded features and this clip's pool partials go there.
// Both are dead again before block 1 writes its leftover partials over them (Leftover<1>::OFF_PART = OFF_Z2): the features
// after conv1, the pool partials once the pool / fc wavefront has read them, which it does before conv1's barrier.
constexpr int OFF_FEAT_P = OFF_Z2;                            // [103][14] features of the NEXT clip
constexpr int OFF_POOLBUF_P = OFF_FEAT_P + 1456;              // [NW][64]  block 4's pool partials of THIS clip
constexpr int STAGE_WAVES = 4;                                // wavefronts 0-3 stage the next clip (they finish block 4 first)
static_assert(OFF_FEAT_P >= OFF_Z3 + Blk<3>::SOUT * CH, "the next clip's features must not overlap block 4's input");
static_assert(OFF_FEAT_P + FEAT_H * FEAT_W <= OFF_POOLBUF_P && OFF_POOLBUF_P % 4 == 0, "features and pool partials are disjoint");
static_assert(OFF_POOLBUF_P + NW * CH <= OFF_Z2 + Blk<2>::SOUT * CH && OFF_Z2 + Blk<2>::SOUT * CH <= OFF_DWTAB,
              "pool partials stay inside the Z2 plane, clear of the table buffers the next clip's block 1 rewrites");

}  // namespace
}  // namespace kws
