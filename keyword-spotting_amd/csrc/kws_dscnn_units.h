// Unit descriptors of the DS-CNN forward kernel's block phases (kws_dscnn_stages.h, block_phase / leftover_partial_unit): what a
// lane of a (block, tile) unit derives from its thread index and the tile for a WHOLE map -- the three own-column tap
// offsets, the two neighbour masks and the store mask.  They depend on the map geometry alone (kws_dscnn_geom.h), so the
// persistent batched kernel reads them from a table instead of recomputing them for every clip and unit.  One packer for the
// host image (build_dscnn_image), the device loader (kws_ds_load_fill_kernel) and the export (kws_host_dscnn_units); the table
// follows the weight image in the same allocation (DscnnLayout::total words in, 16-byte aligned).
//
// Layout (32-bit words): [unit 42][part 2][lane 64][4].  Unit = ds_unit_base(block - 1) + tile, every tile of blocks 1..4, the
// K-split leftover tiles (the fifth of block 1, the ninth of block 2) included: their geometry is the tile's.
//   part 0: tlo[0], tlo[1], tlo[2] (float indices into LDS of rows h-1, h, h+1, channel pair 8 * half; thi = tlo + 32 * SIN),
//           valid (all ones / all zeros: the word block 4's epilogue selects with)
//   part 1: mask_l, mask_r (1.0f / 0.0f), two zero words
// A lane fetches part 0 with one 16-byte load and the masks with one 8-byte load; 64 lanes read 1 KiB + 1 KiB, L2-resident.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "kws_dscnn_geom.h"

namespace kws {
namespace {

// first unit of block n + 1 (n = 0..3); n = 4: the number of units
__host__ __device__ constexpr int ds_unit_base(int n) {
    return (n > 0 ? Blk<1>::TILES : 0) + (n > 1 ? Blk<2>::TILES : 0) + (n > 2 ? Blk<3>::TILES : 0) + (n > 3 ? Blk<4>::TILES : 0);
}
constexpr int DS_UNITS = ds_unit_base(4);                       // 5 + 9 + 12 + 16 = 42
constexpr size_t DS_UNIT_LANE_WORDS = 8;                        // per lane: two parts of four words
constexpr size_t DS_UNIT_WORDS = (size_t)DS_UNITS * 2 * 64 * 4;  // 21504 words = 84 KiB
static_assert(DS_UNITS == 42, "unit table: every tile of the four blocks");

// Word k (0..7: part 0 then part 1) of lane `lane` of tile t of block N: block_phase's arithmetic for a whole map (p_lo = 0,
// p_hi = POUT), expression for expression.
template <int N>
__host__ __device__ inline uint32_t ds_unit_word_of(int t, int lane, int k) {
    using G = Blk<N>;
    const int half = lane >> 5, col = lane & 31;
    const int pos = t * TW - 1 + col;
    const bool valid = col >= 1 && col <= TW && pos < G::POUT;
    const int posc = pos < 0 ? 0 : (pos < G::POUT ? pos : G::POUT - 1);
    const int h = posc / G::W, x = posc % G::W;
    if (k == 3) return valid ? 0xffffffffu : 0u;
    if (k == 4) return __builtin_bit_cast(uint32_t, x > 0 ? 1.f : 0.f);
    if (k == 5) return __builtin_bit_cast(uint32_t, x < G::W - 1 ? 1.f : 0.f);
    if (k > 5) return 0u;
    const int dh = k - 1;
    const int o = G::RING ? 1 : 0;
    const int hh = h + dh - o, xx = x - o;
    const bool inside = (unsigned)hh < (unsigned)G::HI && (unsigned)xx < (unsigned)G::WI;
    const bool in_map = (unsigned)(h + dh) < (unsigned)G::H;
    const int a = inside ? hh * G::WI + xx : ((G::RING && in_map) ? G::PIN : G::PIN + 1);
    return (uint32_t)(G::OFF_IN + pidx(half * 8, a, G::SIN));
}

// Word i < DS_UNIT_WORDS of the table.
__host__ __device__ inline uint32_t ds_unit_word(size_t i) {
    const int k4 = (int)(i & 3), lane = (int)((i >> 2) & 63), part = (int)((i >> 8) & 1), unit = (int)(i >> 9);
    const int k = part * 4 + k4;
    if (unit < ds_unit_base(1)) return ds_unit_word_of<1>(unit, lane, k);
    if (unit < ds_unit_base(2)) return ds_unit_word_of<2>(unit - ds_unit_base(1), lane, k);
    if (unit < ds_unit_base(3)) return ds_unit_word_of<3>(unit - ds_unit_base(2), lane, k);
    return ds_unit_word_of<4>(unit - ds_unit_base(3), lane, k);
}

}  // namespace
}  // namespace kws
