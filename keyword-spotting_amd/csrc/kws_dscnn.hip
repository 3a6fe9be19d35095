// DS-CNN forward for gfx950 (MI355X): one 512-thread workgroup per clip, every activation resident in the
// CU's 160 KiB LDS; conv1 and the pointwise 1x1 convolutions on the matrix cores, depthwise 3x3 on the VALU
// straight into the MFMA B-operand registers.
//
// Replaces DepthwiseSeparableConv.forward (reference kws/libs/models.py:160-183; rows a9-a15 of
// SURVEY.md section 8) for the [1,99,10] MFCC map:
//   conv1  1->64, 10x10, stride 2, pad 2, ReLU                      -> 64 x 47 x 3
//   4 x { depthwise 3x3 pad 1 ; pointwise 1x1 *padding=1* ; ReLU }  -> 64 x (49x5, 51x7, 53x9, 55x11)
//   global average pool, Linear(64 -> C), argmax (first maximum wins)
//
// Three arithmetic routes for the GEMMs, same f32-grade results (include/kws_hip.h, kws_set_pointwise_math):
//   f16 pairs (product, MODE 5): every f32 operand, scaled by a per-clip power of two, = hi + lo, two f16 pieces (22 bits);
//     three piece products on v_mfma_f32_32x32x16_f16 into one f32 accumulator.  The activations live in LDS in per-clip
//     power-of-two units; their exponents are decided two layers ahead from measured maxima and weight-derived bounds, so no
//     input overflows f16 (PairCtx, kws_dscnn_fwd_kernel).
//   split-bf16 (MODE 4, the product path of rounds 1-2): every f32 operand = hi + mid + lo, three bf16 pieces that reproduce it
//     exactly; the six piece products of combined order <= 2 on v_mfma_f32_32x32x16_bf16 (f32 accumulate) give the f32 product
//     to 2^-24.  16x the f32 MFMA rate, and the 16-bit matrix pipe runs beside the VALU (the f32 MFMA shares its datapath).
//   f32: v_mfma_f32_32x32x2_f32.
// A third variant runs the GEMMs on the VALU: an independent check of the operand mappings (tests only).
//
// The relu(bias) ring.  The reference's 1x1 convolution with padding=1 surrounds each block's output
// with a ring equal to relu(bias) (models.py:104-106).  The ring is never stored: each channel plane in
// LDS holds only the "interior" H x W values followed by two extra slots, [P] = relu(bias[c]) and
// [P+1] = 0.  A depthwise tap that falls on the ring reads slot P, one that falls outside the padded
// map reads slot P+1, so a stencil tap is an unconditional LDS read at a per-lane precomputed address.
//
// MFMA mapping, split path (32x32x16, D[i][j] += A[i][k] * B[k][j]): i = output channel, j = position, k = input
// channel.  Lane l supplies B[k = 8(l>>5) + e][j = l&31], e = 0..7: it computes the depthwise output of column j
// for input channels 16m + 8(l>>5) + e itself (m = k-block), splits the eight values into bf16 pieces and feeds
// them to the matrix core without touching LDS; A = pre-split weights from a two-k-block register ring.
// (f32 path, 32x32x2: lane l supplies A[i = l&31][k = l>>5] and B[k = l>>5][j = l&31]; its 32 k-steps walk the
// same channels in the same order.)
// D: column = lane&31 (position), row = (r&3) + 8*(r>>2) + 4*(lane>>5) (output channel).
//
// Stencil with 3 LDS reads instead of 9.  The 32 MFMA columns of a tile are 30 consecutive output
// positions plus one halo column on each side.  A lane reads only its own column (rows h-1, h, h+1);
// because the depthwise weights are the same in all 32 lanes of a half-wave, each lane forms the two
// 3-tap column sums its right and left neighbours need, and the neighbours' sums arrive through one fused DPP
// multiply-add each.  A neighbour that belongs to another row (x == 0 or x == W-1) is outside the zero-padded
// map, so its contribution is multiplied by a per-lane 0/1 mask.  The reads of step s+2 are in flight while
// step s is evaluated and the matrix core works through the MFMAs of the previous k-block.
//
//
// The LDS map and the per-block geometry: kws_dscnn_geom.h.  The stages (stencil, tables, operand loads, conv1, leftover tiles,
// block phase): kws_dscnn_stages.h.  Here: the kernel-argument mirrors, the kernel, the table of its instantiations, the launchers.
#include <array>
#include <utility>

#include "kws_dscnn_stages.h"

namespace kws {
namespace {

#ifndef KWS_X_DSCNN_STAMP_TID   // diagnostics builds (tools/build_variant.sh): which thread writes the phase stamps
#define KWS_X_DSCNN_STAMP_TID 0
#endif

// PERSIST: the kernel's weight argument read again for every clip, through a kernel-argument pointer the compiler cannot see
// through.  Every weight load of the body is clip-invariant: hoisted out of the clip loop, the loads (and the ~50 argument
// dwords) would stay live for the workgroup's whole life and spill.  The argument is the kernel's first: offset 0.
__device__ __forceinline__ DscnnWeights weights_for_this_clip() {
#if defined(__HIP_DEVICE_COMPILE__)
    using KArg = const __attribute__((address_space(4))) DscnnWeights*;
    KArg p = (KArg)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *p;
#else
    return DscnnWeights{};
#endif
}

// The arguments of kws_dscnn_fwd_kernel as they lie in the kernel-argument segment (each at its natural alignment), for reads
// that must not be hoisted (weights_for_this_clip, scan_windows_now).  FwdKernelFn is the kernel's type with the same members
// in the same order; a static_assert below the kernel holds its signature to it, so the two cannot drift apart unnoticed.
using FwdKernelFn = void (*)(DscnnWeights, const float*, int, float*, int32_t*, float*, unsigned long long*, const int*, StreamPush);
struct FwdKernelArgs {
    DscnnWeights w;
    const float* feat;
    int B;
    float* logits;
    int32_t* label;
    float* act;
    unsigned long long* stamps;
    const int* ring_hops;
    StreamPush sp;
};

// PERSIST + SCAN: the window strides read again where a clip is staged, as weights_for_this_clip reads the weights: kept in
// scalar registers across the clip loop they push others out into vector registers, and block 4's tail has none to spare.
__device__ __forceinline__ ScanWindows scan_windows_now() {
#if defined(__HIP_DEVICE_COMPILE__)
    using KArg = const __attribute__((address_space(4))) FwdKernelArgs*;
    KArg p = (KArg)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p->sp.scan;
#else
    return ScanWindows{};
#endif
}

// Where the 99 x 10 floats of `clip` start: consecutive clips, or (SCAN) the strided windows of a scan (ScanWindows).
template <bool SCAN>
__device__ __forceinline__ const float* clip_features(const float* __restrict__ feat, int clip, const ScanWindows& sw) {
    if constexpr (SCAN) {
        // mulhi(i, floor(2^32 / d)) lies in (i / d - 1, i / d]: the quotient or one less
        unsigned rec = __umulhi((unsigned)clip, sw.wpr_recip), win = (unsigned)clip - rec * sw.wpr;
        if (win >= sw.wpr) {
            win -= sw.wpr;
            ++rec;
        }
        return feat + (size_t)rec * sw.row_floats + (size_t)win * sw.win_floats;
    } else {
        return feat + (size_t)clip * (IN_T * IN_F);
    }
}

// PERSIST, block 4's tail: wavefronts 0 .. STAGE_WAVES-1 stage the padded feature map of `clip` at OFF_FEAT_P (the loads,
// the zero pad, the scatter) and, for f16 pairs, publish its largest |feature| to stage-maxima set 0 -- the slots of the other
// wavefronts are zeroed, so read_stage_max sees this clip alone (set 0 was last read before block 3).
template <bool PAIR, bool SCAN = false>
__device__ __forceinline__ void stage_features_persist(float* lds, const float* __restrict__ feat, int clip, int tid,
                                                       const ScanWindows& sw = ScanWindows{}) {
    constexpr int ST = STAGE_WAVES * 64;
    constexpr int FV = (IN_T * IN_F + ST - 1) / ST;
    static_assert(2 * STAGE_WAVES == NW, "each staging wavefront zeroes the maximum slot of one other wavefront");
    const int lane = tid & 63, wv = tid >> 6;
    const float* f = clip_features<SCAN>(feat, clip, sw);
    float fv[FV];
#pragma unroll
    for (int k = 0; k < FV; ++k) {
        const int i = tid + k * ST;
        fv[k] = i < IN_T * IN_F ? f[i] : 0.f;
    }
    float* featp = lds + OFF_FEAT_P;
    for (int i = tid; i < FEAT_H * FEAT_W; i += ST) {  // the zero fill touches only the padding, the scatter only the interior
        const int r = i / FEAT_W - 2, c = i % FEAT_W - 2;
        if (!((unsigned)r < (unsigned)IN_T && (unsigned)c < (unsigned)IN_F)) featp[i] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < FV; ++k) {
        const int i = tid + k * ST;
        if (i < IN_T * IN_F) featp[(i / IN_F + 2) * FEAT_W + (i % IN_F) + 2] = fv[k];
    }
    if constexpr (PAIR) {
        float m = 0.f;
#pragma unroll
        for (int k = 0; k < FV; ++k) m = fmaxf(m, fabsf(fv[k]));
        publish_wave_max(lds, 0, wv, lane, m);
        if (lane == 63) lds[OFF_WMAX + wv + STAGE_WAVES] = 0.f;
    }
}

// PERSIST: global average pool + Linear(64 -> C) + argmax of a finished clip on ONE wavefront (NW - 1, which has no conv1 unit),
// while the others run the next clip's conv1.  Same sums in the same order as the one-clip tail of kws_dscnn_fwd_kernel: lane c
// adds the NW partials of channel c, then the ring term; the classifier row of lane j takes the 64 pooled values in channel
// order, broadcast from their lanes (v_readlane) instead of through LDS.
__device__ __forceinline__ void pool_fc_wave(const DscnnWeights& w, const float* lds, int lane, int clip, float* __restrict__ logits,
                                             int32_t* __restrict__ label, float* __restrict__ a_pool) {
    const int C = w.num_classes;
    float4 fcw[CH / 4];
    float fcb = 0.f;
    const float4* wr = reinterpret_cast<const float4*>(w.fc_w + (lane < C ? lane : 0) * CH);
#pragma unroll
    for (int c = 0; c < CH / 4; ++c) fcw[c] = wr[c];
    if (lane < C) fcb = w.fc_b[lane];
    const float ring_b = w.pw_b[3 * CH + lane];
    constexpr float RING_N = 55.f * 11.f - 53.f * 9.f;  // 128
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NW; ++k) s += lds[OFF_POOLBUF_P + k * CH + lane];
    s = fmaf(RING_N, relu(ring_b), s) * (1.0f / (55.f * 11.f));
    if (a_pool) a_pool[lane] = s;
    float acc = fcb;  // every lane runs the chain (rows >= C are row 0 again): the broadcasts stay outside divergent code
#pragma unroll
    for (int c = 0; c < CH / 4; ++c) {
        const float4 a4 = fcw[c];
        acc = fmaf(a4.x, __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, s), 4 * c + 0)), acc);
        acc = fmaf(a4.y, __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, s), 4 * c + 1)), acc);
        acc = fmaf(a4.z, __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, s), 4 * c + 2)), acc);
        acc = fmaf(a4.w, __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, s), 4 * c + 3)), acc);
    }
    if (lane < C) logits[(size_t)clip * C + lane] = acc;
    const int idx = wave_argmax_first(lane < C ? acc : -INFINITY, lane, C);
    if (label && lane == 0) label[clip] = idx;
}

// DIAG = false: the product instantiation -- no activation dump, no stamps (their pointers and loops cost
// registers and 5 KB of code even when unused).
// PRECONV: `feat` is not the MFCC map but conv1's output [B][64][47*3] (ReLU applied), computed by kws_conv1_general_kernel
// for a model with input_channels > 1 (models.py:125,135); the kernel then starts at block 1.
// STREAM: the streaming push in one launch (launch_dscnn_stream).  `feat` is the feature ring (its newest row is written
// here, through a pointer derived from `feat`, and never read), wavefront 0 computes the stream's new frame straight into the LDS feature map while the other
// wavefronts fetch the 98 older rows, and the hop counter sp.hops advances when the last workgroup is done.
// CLUSTER (with STREAM): sp.cluster workgroups share one stream's network by TIME TILES -- at 64 streams one workgroup per
// stream leaves three quarters of the CUs idle and the push latency is one clip's serial path through the kernel.  Workgroup
// (stream, tile) computes the rows of block 4's output that belong to its tile and, of every earlier stage, the rows those
// depend on (one more row per side and stage: ~4 conv1 rows of halo per side, recomputed, no exchange between workgroups);
// everything stays LDS-resident per tile.  Only the LAST tile needs the window's newest row, so only its wavefront 0 runs
// the one-frame front end.  The tiles' pooled partial sums meet in global memory; the workgroup that arrives last (a
// counter per stream) adds them in tile order, adds the ring term and runs fc + argmax.
// PERSIST (batched product paths, launch_dscnn with B above the CU count): grid = CU count, workgroup g carries clips g,
// g + grid, ... and overlaps consecutive ones.  Wavefronts 0-3, which finish block 4 first, stage the next clip's features
// (OFF_FEAT_P) while 4-7 finish their units; one barrier closes both.  The pool + fc + argmax of the finished clip then runs
// on wavefront NW - 1 beside the next clip's conv1, in which it has no unit.  Same units, orders and sums as one clip per
// workgroup: the results are bit-identical.  Its block phases run under a per-block wavefront-priority schedule (s_setprio at
// unit boundaries, kws_dscnn_stages.h "Wavefront priority"), which moves issue slots between the two wavefronts of a SIMD
// and nothing else.
// SCAN (kws_scan_i16, launch_dscnn_scan): "clip" i is a window of a long recording's frame array -- only the address its
// features are fetched from changes (clip_features); logits and labels stay indexed by i.
// ACTIVE (with STREAM; a set with deactivated streams, kws_stream_active.hip): the grid holds the ACTIVE streams' workgroups only and
// workgroup slot i serves stream ring_hops[i] -- the set's device list of active streams, ascending, in the argument the fused push
// does not otherwise read, so that the kernel-argument segment of every instantiation stays as it was.  Everything else, the
// finishers count among it (gridDim.x / cluster), is the body below: rings, partial sums, results and labels are addressed by `clip`.
// The parameter list is mirrored by FwdKernelArgs / FwdKernelFn (the persistent kernels read arguments from the segment).
template <int MODE, bool DIAG = true, bool PRECONV = false, bool STREAM = false, bool CLUSTER = false, bool PERSIST = false,
          bool SCAN = false, bool ACTIVE = false>
__global__ __launch_bounds__(NT) void kws_dscnn_fwd_kernel(DscnnWeights w_arg, const float* __restrict__ feat, int B,
                                                           float* __restrict__ logits, int32_t* __restrict__ label,
                                                           float* __restrict__ act_arg,
                                                           unsigned long long* __restrict__ stamps_arg,
                                                           const int* __restrict__ ring_hops, StreamPush sp) {
    static_assert(!STREAM || (MODE >= 4 && !DIAG && !PRECONV), "the fused push exists for the product paths only");
    static_assert(!PERSIST || ((MODE == 4 || MODE == 5) && !PRECONV && !STREAM), "persistent workgroups: batched product paths only");
    static_assert(!SCAN || ((MODE == 4 || MODE == 5) && !DIAG && !PRECONV && !STREAM && !CLUSTER), "strided windows: batched product paths only");
    constexpr bool PAIR = MODE == 5;   // f16-pair arithmetic (kws_split_mfma.h): activations live in LDS in per-clip scaled units
    constexpr int NP = PAIR ? 2 : 3;
    BlockTables t1_pre{};              // PRECONV: block 1's tables between their fetch and their (PAIR: scaled) store
    static_assert(!CLUSTER || STREAM, "time-tile clusters exist for the streaming push only");
    static_assert(!ACTIVE || STREAM, "a list of active streams exists for the streaming push only");
    float* const act = DIAG ? act_arg : nullptr;
    unsigned long long* const stamps = DIAG ? stamps_arg : nullptr;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr bool MFMA = MODE != 0;
    const int tid_k = threadIdx.x;
    const int lane_k = tid_k & 63, wv_k = tid_k >> 6;

    // One clip per workgroup, or (PERSIST) one workgroup per CU that loops over its clips: the loop body sees the weights and
    // the thread index through opaque values once per clip, so nothing clip-invariant is hoisted into registers.
    const int cl_n = CLUSTER ? sp.cluster : 1;
    int clip = CLUSTER ? (int)blockIdx.x / cl_n : (int)blockIdx.x;  // PERSIST: the running clip
    const int cl_tile = CLUSTER ? (int)blockIdx.x - clip * cl_n : 0;
    if constexpr (ACTIVE) clip = ring_hops[clip];  // workgroup-uniform: slot -> stream
    if (clip >= B) return;
    // Rows of each stage this workgroup computes (CLUSTER; otherwise everything).  Block 4's output rows [j0, j1) need block
    // 3's rows [j0 - 2, j1) (a 3-row stencil, and block 3's stored plane is block 4's input without its ring: row index - 1),
    // those need block 2's [j0 - 4, j1), block 1's [j0 - 6, j1), and block 1 reads conv1's rows [j0 - 7, j1 + 1) (no ring there).
    const int j0 = Blk<4>::H * cl_tile / cl_n, j1 = Blk<4>::H * (cl_tile + 1) / cl_n;
    auto rows = [&](int lo, int hi, int H, int W) { return PosRange{(lo < 0 ? 0 : lo) * W, (hi > H ? H : hi) * W}; };
    const PosRange rg4 = rows(j0, j1, Blk<4>::H, Blk<4>::W), rg3 = rows(j0 - 2, j1, Blk<3>::H, Blk<3>::W),
                   rg2 = rows(j0 - 4, j1, Blk<2>::H, Blk<2>::W), rg1 = rows(j0 - 6, j1, Blk<1>::H, Blk<1>::W),
                   rg0 = rows(j0 - 7, j1 + 1, C1_H, C1_W);
    // diagnostics only (stamps == nullptr in every product call): shader-clock stamps of thread 0 at the
    // phase boundaries, KWS_DSCNN_STAMPS per clip; [14] and [15] carry the 100 MHz real-time counter
    int n_stamp = 0;
    auto stamp = [&]() {
        if (stamps && tid_k == KWS_X_DSCNN_STAMP_TID) stamps[(size_t)clip * KWS_DSCNN_STAMPS + n_stamp] = __builtin_amdgcn_s_memtime();
        ++n_stamp;
    };

    constexpr bool SPLIT = MODE >= 4;
    // unit descriptors (block_phase, UT): the persistent f16-pair kernels.  The bf16 triple, three pieces per operand, has no
    // registers for a descriptor in flight (it spilled more and ran 0.9 % slower) and keeps computing its geometry.
    constexpr bool UT = PERSIST && PAIR;
    // PERSIST: block 1's tables are the same for every clip (3 registers for the whole loop); conv1's operands are reloaded in
    // every block-4 tail, after the pool sums have left the registers.  The first clip is staged here.
    BlockTables t1p{};
    uintx4 c1p[PERSIST ? 7 : 1][NP];
    int prev_clip = -1;         // PERSIST: the clip whose pool + fc is still to run (on wavefront NW - 1)
    float* a_prev = nullptr;    // its pooled-means slot in the activation dump (diagnostics)
    // the arrival counter of the K-split leftover tiles: zeroed once per workgroup (conv1's barrier, at the latest, lies between
    // this store and block 1); whoever combines a tile leaves it at zero again (leftover_arrive)
    if ((MODE == 4 || MODE == 5) && !CLUSTER && tid_k == 0) lds[OFF_ARRIVE] = 0.f;
    if constexpr (PERSIST) {
        fetch_block_tables(w_arg, 1, tid_k, t1p);
        if (wv_k < STAGE_WAVES) stage_features_persist<PAIR, SCAN>(lds, feat, clip, tid_k, sp.scan);
        load_conv1_frags(w_arg, wv_k, lane_k, c1p);
        __syncthreads();
    }
    for (;;) {  // one pass unless PERSIST (the body keeps its one-clip indentation)
    // PERSIST: every weight load of the body is clip-invariant; hoisted out of the loop they would pin hundreds of registers
    // for the workgroup's whole life (spills).  Opaque weight pointers per clip keep each load where it is.
    // The same per PHASE: one copy for the whole clip keeps every pointer and bound of DscnnWeights live in scalar registers from
    // the clip's head to block 4 (they spill into vector lanes); each phase reads what it uses again, ahead of the barrier it
    // starts behind.
    auto weights_now = [&]() -> DscnnWeights { return PERSIST ? weights_for_this_clip() : w_arg; };
    const DscnnWeights w = weights_now();
    int tid = tid_k;
    if constexpr (PERSIST) {
        // the same for the thread index: every LDS address and mask is derived from it, and hoisted they spill.  The wavefront
        // index stays a wave-uniform scalar: tid = 64 wv + lane with wv from a readfirstlane and lane < 64 visible.
        int wv_l = __builtin_amdgcn_readfirstlane(wv_k), lane_l = lane_k;
        asm volatile("" : "+s"(wv_l), "+v"(lane_l));
        tid = (wv_l << 6) | (lane_l & 63);
    }
    const int lane = tid & 63, wv = tid >> 6;
    if constexpr (PERSIST) n_stamp = 0;
    if (stamps && tid == KWS_X_DSCNN_STAMP_TID) stamps[(size_t)clip * KWS_DSCNN_STAMPS + KWS_DSCNN_STAMPS - 2] = __builtin_amdgcn_s_memrealtime();
    stamp();  // 0: start (PERSIST: features already staged)

    PwOperands<MODE> wa;            // pointwise operands of the running block
    UnitDesc ud{};                  // PERSIST: the descriptor of this wavefront's next block-phase unit (block_phase, UT)
    int hops_before = 0;            // STREAM: pushes before this one
    // PAIR: exponents of the clip's scales.  kx: features; ky[n]: block n's depthwise output (true units) * 2^ky[n] < 2^15;
    // sg[n]: the units stage n's accumulators and stored output are in (sg[0]: conv1), = ky[n] + the layer's weight exponent
    int kx = 0, ky[5] = {0, 0, 0, 0, 0}, sg[5] = {0, 0, 0, 0, 0};
    if constexpr (PERSIST) {
        // the features were staged behind the previous barrier (block 4's tail of the previous clip, or the prologue)
        if constexpr (PAIR) {  // scales of conv1 and block 1 exactly as below
            const float mxf = read_stage_max(lds, 0, 1);
            kx = pow2_exp_for(mxf);
            const float bz0 = (w.c1_abs * mxf + w.c1_bmax) * 1.001f;
            cap_units(kx, sg[0], w.k_c1, bz0);
            const float by1 = (w.dw_abs[0] * bz0 + w.dw_bmax[0]) * 1.001f;
            ky[1] = pow2_exp_for(by1);
            cap_units(ky[1], sg[1], w.k_pw[0], (w.pw_abs[0] * by1 + w.pw_bmax[0]) * 1.001f);
            store_block_tables(lds, 1, tid, t1p, pow2f(ky[1]), pow2f(sg[1]), pow2f(ky[1] - sg[0]));
            conv1_build_windows(lds, tid, pow2f(kx), OFF_FEAT_P);
            __syncthreads();
        } else {
            store_block_tables(lds, 1, tid, t1p);  // (read in block 1, behind conv1's barrier)
        }
        stamp();  // 1: scales and conv1 windows ready
        conv1_phase_split<false, NP>(w, lds, tid, c1p, rg0, pow2f(kx), pow2f(sg[0]), OFF_FEAT_P);
        if (wv == NW - 1 && prev_clip >= 0) {
            pool_fc_wave(w, lds, lane, prev_clip, logits, label, a_prev);
            if (stamps && lane == 0) stamps[(size_t)prev_clip * KWS_DSCNN_STAMPS + 13] = __builtin_amdgcn_s_memtime();
        }
        // block 1's first unit: tile wv, or (wavefronts 4-7) a quarter of the leftover tile
        if constexpr (UT) load_unit_desc(w, 1, wv < Leftover<1>::TILE ? wv : Leftover<1>::TILE, lane, ud);
        load_afrag(w, 1, wv >= 4 ? wv - 4 : 0, lane, wa.ring[0]);  // wavefronts 4-7: their k-block of block 1's leftover tile
    } else if constexpr (PRECONV) {
        static_assert(!PRECONV || MODE >= 4, "the pre-convolved entry exists for the product (split) path only");
        const float* z = feat + (size_t)clip * (CH * P0);
        fetch_block_tables(w, 1, tid, t1_pre);
        float zmax = 0.f;
        for (int i = tid; i < CH * P0; i += NT) {
            const float v = z[i];
            lds[OFF_Z0 + pidx(i / P0, i % P0, P0 + 2)] = v;
            zmax = fmaxf(zmax, v);
        }
        if (tid < CH) {
            lds[OFF_Z0 + pidx(tid, P0, P0 + 2)] = 0.f;
            lds[OFF_Z0 + pidx(tid, P0 + 1, P0 + 2)] = 0.f;
        }
        // PAIR: conv1's output arrives in true units (sg[0] = 0) and nothing bounds it in advance: its largest value is measured
        // here, block 1's scale and tables follow behind the barrier below (one more barrier than the single-channel path)
        if constexpr (PAIR)
            publish_wave_max(lds, 1, wv, lane, zmax);
        else
            store_block_tables(lds, 1, tid, t1_pre);
        if constexpr (Leftover<1>::HAS && (MODE == 4 || MODE == 5) && !CLUSTER)
            load_afrag(w, 1, wv >= 4 ? wv - 4 : 0, lane, wa.ring[0]);  // wavefronts 4-7: their k-block of block 1's leftover tile
        else
            load_block_head(w, 1, lane, wa);
        stamp();  // 1
    } else {
    // ---- phase 0: MFCC map -> zero-padded [103][14] in LDS, weight loads in flight --------------------
    // The feature map and block 1's tables are on the critical path of this phase: their loads are issued first
    // (vector memory returns in order), the conv1 operands behind them.
    float* featp = lds + OFF_FEAT;
    const float* f = clip_features<SCAN>(feat, clip, sp.scan);
    constexpr int FV = (IN_T * IN_F + NT - 1) / NT;
    float fv[FV];
    // streaming: the feature map is a ring of IN_T frames; after `hops` pushes the newest frame sits in row
    // (hops - K) mod IN_T, K = ceil(frame_len / frame_step) hops per frame, and the window starts one row after it
    int row_new = -1;  // STREAM: window row the new frame takes (-1: none yet)
    int head;
    if constexpr (STREAM) {
        hops_before = *sp.hops;
        // K = hops a frame spans = ceil(frame_len / frame_step) (3 for 400 / 160): after h pushes the newest frame is h - K
        // and the window starts one row after it; here h = hops_before + 1
        const int K = frames_lag(sp.p);
        head = (((hops_before + 2 - K) % IN_T) + IN_T) % IN_T;  // what the two-launch path derives from the advanced counter
        const int step = sp.p.frame_step;
        const long f_start = (long)step * hops_before + step - (long)K * step;
        if (f_start >= 0) row_new = (int)((((f_start / step) - head) % IN_T + IN_T) % IN_T);
    } else {
        head = ring_hops ? (((*ring_hops + 1 - sp.frames_lag) % IN_T) + IN_T) % IN_T : 0;
    }
#pragma unroll
    for (int k = 0; k < FV; ++k) {
        const int i = tid + k * NT;
        fv[k] = (i < IN_T * IN_F && i / IN_F != row_new) ? f[((i / IN_F + head) % IN_T) * IN_F + i % IN_F] : 0.f;
    }
    BlockTables t1;
    fetch_block_tables(w, 1, tid, t1);
    __builtin_amdgcn_sched_barrier(0);
    float a1[SPLIT ? 1 : 50];       // conv1 weights of this wave's output-channel tile (f32 MFMA A operands)
    uintx4 c1f[SPLIT ? 7 : 1][NP];  // the same as bf16 pieces / f16 pairs (split paths)
    if constexpr (SPLIT) {
        load_conv1_frags(w, wv, lane, c1f);
    } else if constexpr (MFMA) {
        const int half = lane >> 5, col = lane & 31, ct = wv & 1;
#pragma unroll
        for (int s = 0; s < 50; ++s) a1[s] = w.c1_w[(2 * s + half) * CH + ct * 32 + col];
        load_pointwise(w, 1, lane, wa);
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (PAIR) {  // the clip's largest |feature| (the row the streaming front end adds is looked at after the barrier)
        float m = 0.f;
#pragma unroll
        for (int k = 0; k < FV; ++k) m = fmaxf(m, fabsf(fv[k]));
        publish_wave_max(lds, 0, wv, lane, m);
    }
    if constexpr (STREAM) {
        // One barrier: the zero fill touches only the padding, the scatter only the interior, and the new frame's row is
        // written by wavefront 0 alone, straight from the cepstrum registers of its one-frame front end (scratch and tables
        // in the region block 2 will overwrite much later).
#ifdef KWS_X_STREAM_NO_FRAME  // timing experiment (wrong results): the push without the one-frame front end on any tile's path
        if (false)
#else
        if (wv == 0 && cl_tile == cl_n - 1)  // first: its sample and table loads join the feature loads already in flight
#endif
            stream_frame_wave(sp.p, sp.t, sp.hop, clip, clip, false, sp.pcm_ring, sp.ring_len, const_cast<float*>(feat), hops_before,
                              reinterpret_cast<unsigned char*>(lds + OFF_Z2), lane,
                              row_new >= 0 ? featp + (row_new + 2) * FEAT_W + 2 : nullptr, sp.refine_ctr);
        for (int i = tid; i < FEAT_H * FEAT_W; i += NT) {
            const int r = i / FEAT_W - 2, c = i % FEAT_W - 2;
            if (!((unsigned)r < (unsigned)IN_T && (unsigned)c < (unsigned)IN_F)) featp[i] = 0.f;
        }
        if constexpr (!PAIR) store_block_tables(lds, 1, tid, t1);
#pragma unroll
        for (int k = 0; k < FV; ++k) {
            const int i = tid + k * NT;
            if (i < IN_T * IN_F && i / IN_F != row_new) featp[(i / IN_F + 2) * FEAT_W + (i % IN_F) + 2] = fv[k];
        }
        __syncthreads();
    } else {
    // one barrier: the zero fill touches only the padding cells, the scatter only the interior
    for (int i = tid; i < FEAT_H * FEAT_W; i += NT) {
        const int r = i / FEAT_W - 2, c = i % FEAT_W - 2;
        if (!((unsigned)r < (unsigned)IN_T && (unsigned)c < (unsigned)IN_F)) featp[i] = 0.f;
    }
    if constexpr (!PAIR) store_block_tables(lds, 1, tid, t1);
#pragma unroll
    for (int k = 0; k < FV; ++k) {
        const int i = tid + k * NT;
        if (i < IN_T * IN_F) featp[(i / IN_F + 2) * FEAT_W + (i % IN_F) + 2] = fv[k];
    }
    __syncthreads();
    }
    if constexpr (PAIR) {
        // Scales of conv1 and block 1, from the clip's largest |feature| Mx and bounds that hold for any input (kws_internal.h):
        // features * 2^kx < 2^15; conv1's accumulators and stored output are in units 2^sg0; block 1's depthwise output
        // (true units) is below dw_abs (c1_abs Mx + c1_bmax) + dw_bmax, which fixes its operand scale 2^ky1 and its units.
        float mxf = read_stage_max(lds, 0, 1);
        if constexpr (STREAM) {
            // the window's newest row exists only in the workgroup whose wavefront 0 computed it (the last time tile); in the
            // others its cells are never written (their ranges stop short of it)
            if (row_new >= 0 && cl_tile == cl_n - 1)
                for (int c = 0; c < IN_F; ++c) mxf = fmaxf(mxf, fabsf(featp[(row_new + 2) * FEAT_W + 2 + c]));
        }
        kx = pow2_exp_for(mxf);
        const float bz0 = (w.c1_abs * mxf + w.c1_bmax) * 1.001f;
        cap_units(kx, sg[0], w.k_c1, bz0);
        const float by1 = (w.dw_abs[0] * bz0 + w.dw_bmax[0]) * 1.001f;
        ky[1] = pow2_exp_for(by1);
        cap_units(ky[1], sg[1], w.k_pw[0], (w.pw_abs[0] * by1 + w.pw_bmax[0]) * 1.001f);
        store_block_tables(lds, 1, tid, t1, pow2f(ky[1]), pow2f(sg[1]), pow2f(ky[1] - sg[0]));  // (read in block 1, behind conv1's barrier)
        conv1_build_windows(lds, tid, pow2f(kx));                          // conv1's operands, split once
        __syncthreads();
    }
    stamp();  // 1: features staged

    if constexpr (SPLIT) {
        conv1_phase_split<CLUSTER, NP>(w, lds, tid, c1f, rg0, pow2f(kx), pow2f(sg[0]));
        // the conv1 operands are dead: block 1's first fly across the barrier (wavefronts 4-7: their k-block of the leftover tile)
        if constexpr (Leftover<1>::HAS && (MODE == 4 || MODE == 5) && !CLUSTER)
            load_afrag(w, 1, wv >= 4 ? wv - 4 : 0, lane, wa.ring[0]);
        else
            load_block_head(w, 1, lane, wa);
    } else {
        conv1_phase<MFMA>(w, lds, tid, a1);
    }
    }
    stamp();  // 2: conv1 units of wave 0 done
    const DscnnWeights w1 = weights_now();
    __syncthreads();
    stamp();  // 3: conv1 barrier
    float* a = act ? act + (size_t)clip * KWS_ACT_FLOATS_PER_CLIP : nullptr;
    // PAIR: the planes hold activations * 2^sg[n]; the dumps (diagnostics) go out in true units
    if (a) {
        const float u = PAIR ? pow2f(-sg[0]) : 1.f;
        for (int i = tid; i < CH * P0; i += NT) a[i] = lds[OFF_Z0 + pidx(i / P0, i % P0, P0 + 2)] * u;
        a += CH * P0;
    }
    PairCtx pc;
    if constexpr (PAIR && PRECONV) {
        const float mz0 = read_stage_max(lds, 1, 1);  // true units
        const float by1 = (w1.dw_abs[0] * mz0 + w1.dw_bmax[0]) * 1.001f;
        ky[1] = pow2_exp_for(by1);
        cap_units(ky[1], sg[1], w1.k_pw[0], (w1.pw_abs[0] * by1 + w1.pw_bmax[0]) * 1.001f);
        store_block_tables(lds, 1, tid, t1_pre, pow2f(ky[1]), pow2f(sg[1]), pow2f(ky[1]));
        __syncthreads();
    }
    if constexpr (PAIR) {
        // conv1's largest output is known now: it bounds block 1's output, which fixes block 2's operand scale and units --
        // two layers ahead, so that block 2's tables can be stored (scaled) while block 1 runs
        const float mz = read_stage_max(lds, 1, 1) * pow2f(-sg[0]);
        const float bz = (w1.pw_abs[0] * ((w1.dw_abs[0] * mz + w1.dw_bmax[0]) * 1.001f) + w1.pw_bmax[0]) * 1.001f;
        const float by = (w1.dw_abs[1] * bz + w1.dw_bmax[1]) * 1.001f;
        ky[2] = pow2_exp_for(by);
        cap_units(ky[2], sg[2], w1.k_pw[1], (w1.pw_abs[1] * by + w1.pw_bmax[1]) * 1.001f);
        pc.s_dww = pow2f(ky[2] - sg[1]);
        pc.s_dwb = pow2f(ky[2]);
        pc.s_pwb = pow2f(sg[2]);
    }
    block_phase<1, MODE, CLUSTER, UT, PERSIST>(w1, lds, tid, wa, ud, nullptr, rg1, pc);
    stamp();  // 4: block 1 units of wave 0 done
    const DscnnWeights w2 = weights_now();
    __syncthreads();  // (the K-split leftover tile was combined ahead of it: leftover_arrive)
    stamp();  // 5: block 1 barrier
    if (a) {
        const float u = PAIR ? pow2f(-sg[1]) : 1.f;
        for (int i = tid; i < CH * Blk<1>::POUT; i += NT)
            a[i] = lds[OFF_Z1 + pidx(i / Blk<1>::POUT, i % Blk<1>::POUT, Blk<1>::SOUT)] * u;
        a += CH * Blk<1>::POUT;
    }
    if constexpr (PAIR) {
        // block 2 reads block 1's interior and its ring (relu(bias) <= pw_bmax)
        const float mz = fmaxf(read_stage_max(lds, 2, 1) * pow2f(-sg[1]), w2.pw_bmax[0]);
        const float bz = (w2.pw_abs[1] * ((w2.dw_abs[1] * mz + w2.dw_bmax[1]) * 1.001f) + w2.pw_bmax[1]) * 1.001f;
        const float by = (w2.dw_abs[2] * bz + w2.dw_bmax[2]) * 1.001f;
        ky[3] = pow2_exp_for(by);
        cap_units(ky[3], sg[3], w2.k_pw[2], (w2.pw_abs[2] * by + w2.pw_bmax[2]) * 1.001f);
        pc.s_dww = pow2f(ky[3] - sg[2]);
        pc.s_dwb = pow2f(ky[3]);
        pc.s_pwb = pow2f(sg[3]);
    }
    block_phase<2, MODE, CLUSTER, UT, PERSIST>(w2, lds, tid, wa, ud, nullptr, rg2, pc);
    stamp();  // 6
    const DscnnWeights w3 = weights_now();
    __syncthreads();
    stamp();  // 7
    if (a) {
        const float u = PAIR ? pow2f(-sg[2]) : 1.f;
        for (int i = tid; i < CH * Blk<2>::POUT; i += NT)
            a[i] = lds[OFF_Z2 + pidx(i / Blk<2>::POUT, i % Blk<2>::POUT, Blk<2>::SOUT)] * u;
        a += CH * Blk<2>::POUT;
    }
    if constexpr (PAIR) {
        const float mz = fmaxf(read_stage_max(lds, 0, 1) * pow2f(-sg[2]), w3.pw_bmax[1]);
        const float bz = (w3.pw_abs[2] * ((w3.dw_abs[2] * mz + w3.dw_bmax[2]) * 1.001f) + w3.pw_bmax[2]) * 1.001f;
        const float by = (w3.dw_abs[3] * bz + w3.dw_bmax[3]) * 1.001f;
        ky[4] = pow2_exp_for(by);
        cap_units(ky[4], sg[4], w3.k_pw[3], (w3.pw_abs[3] * by + w3.pw_bmax[3]) * 1.001f);
        pc.s_dww = pow2f(ky[4] - sg[3]);
        pc.s_dwb = pow2f(ky[4]);
        pc.s_pwb = pow2f(sg[4]);
    }
    block_phase<3, MODE, CLUSTER, UT, PERSIST>(w3, lds, tid, wa, ud, nullptr, rg3, pc);
    stamp();  // 8
    const DscnnWeights w4 = weights_now();
    __syncthreads();
    stamp();  // 9
    if (a) {
        const float u = PAIR ? pow2f(-sg[3]) : 1.f;
        for (int i = tid; i < CH * Blk<3>::POUT; i += NT)
            a[i] = lds[OFF_Z3 + pidx(i / Blk<3>::POUT, i % Blk<3>::POUT, Blk<3>::SOUT)] * u;
        a += CH * Blk<3>::POUT;
    }
    if constexpr (PAIR) {
        pc.inv_out = pow2f(-sg[4]);
    }
    block_phase<4, MODE, CLUSTER, UT, PERSIST>(w4, lds, tid, wa, ud, a ? a + CH : nullptr, rg4, pc,  // block 4's output follows the pooled means
                                      PERSIST ? OFF_POOLBUF_P : OFF_POOLBUF);
    stamp();  // 10
    if constexpr (PERSIST) {
        // block 4's tail: the pool partials are stored; wavefronts 0-3 stage the next clip while 4-7 finish their units, and
        // everyone requests conv1's operands (the pool sums have left the registers).  One barrier closes block 4 of this clip
        // and the staging of the next; this clip's pool + fc runs behind it, beside the next clip's conv1.
        const int next = clip + (int)gridDim.x;
        __builtin_amdgcn_sched_barrier(0);
        const ScanWindows sw_next = SCAN ? scan_windows_now() : ScanWindows{};  // (outside the branch: a uniform scalar read)
        if (wv < STAGE_WAVES && next < B) stage_features_persist<PAIR, SCAN>(lds, feat, next, tid, sw_next);
        stamp();  // 11: next clip staged (wavefront 0)
        load_conv1_frags(w4, wv, lane, c1p);  // (unconditional: a conditional reload keeps the old copy live through the whole loop)
        __syncthreads();
        stamp();  // 12: block 4 barrier
        if (stamps && tid == KWS_X_DSCNN_STAMP_TID) stamps[(size_t)clip * KWS_DSCNN_STAMPS + KWS_DSCNN_STAMPS - 1] = __builtin_amdgcn_s_memrealtime();
        prev_clip = clip;
        a_prev = a;
        clip = next;
        if (clip >= B) break;
        continue;
    }
    // The classifier row of lane c (wavefront 0) and the ring bias of channel tid are requested BEFORE the barrier:
    // their L2 round trips pass while the workgroup waits for its slowest wavefront, instead of sitting exposed at
    // the very end of the clip (the CU cannot take its next clip before this wavefront is done).
    const int C = w4.num_classes;
    float4 fcw[CH / 4];
    float fcb = 0.f, ring_b = 0.f;
    if (wv == 0 && lane < C) {
        const float4* wr = reinterpret_cast<const float4*>(w4.fc_w + lane * CH);
#pragma unroll
        for (int c = 0; c < CH / 4; ++c) fcw[c] = wr[c];
        fcb = w4.fc_b[lane];
    }
    if (tid < CH) ring_b = w4.pw_b[3 * CH + tid];
    __syncthreads();
    stamp();  // 11

    // ---- global average pool over 55 x 11 = 477 interior + 128 ring positions ---------------------
    float* pooled = lds + OFF_POOLED;
    constexpr float RING_N = 55.f * 11.f - 53.f * 9.f;  // 128
    bool run_fc = true;  // workgroup-uniform
    if constexpr (CLUSTER) {
        // this tile's partial sums go to global memory (agent-scope stores: the other tiles' workgroups sit on other XCDs, whose
        // L2s are not coherent with this one); the workgroup of the stream that arrives last combines them in tile order
        float* part = sp.cl_part + ((size_t)clip * cl_n + cl_tile) * CH;
        if (tid < CH) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < NW; ++k) s += lds[OFF_POOLBUF + k * CH + tid];
            __hip_atomic_store(part + tid, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // No fence: an agent-scope release writes the XCD's whole L2 back -- measured 0.33 us per workgroup, serialised
        // across the chip (256 workgroups: 88 us).  The partial sums are agent-scope atomic stores (write-through to the
        // coherence point); once they are acknowledged (vmcnt 0) any XCD's agent-scope load sees them, and the counter is
        // bumped only after the whole workgroup has passed that wait.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int* last_flag = reinterpret_cast<int*>(lds + OFF_POOLED + CH);
        if (tid == 0) {
            const int arrived = atomicAdd(&sp.cl_count[clip], 1);
            *last_flag = arrived == cl_n - 1;
            if (arrived == cl_n - 1) sp.cl_count[clip] = 0;  // for the next push (published by the kernel boundary)
        }
        __syncthreads();
        run_fc = *last_flag != 0;
        if (run_fc) {
            if (tid < CH) {  // agent-scope loads: never served from this XCD's (non-coherent) L2
                float s = 0.f;
                for (int t = 0; t < cl_n; ++t)
                    s += __hip_atomic_load(sp.cl_part + ((size_t)clip * cl_n + t) * CH + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                pooled[tid] = fmaf(RING_N, relu(ring_b), s) * (1.0f / (55.f * 11.f));
            }
        }
        __syncthreads();
    } else {
    if (tid < CH) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NW; ++k) s += lds[OFF_POOLBUF + k * CH + tid];
        s = fmaf(RING_N, relu(ring_b), s) * (1.0f / (55.f * 11.f));
        pooled[tid] = s;
        if (a) a[tid] = s;
    }
    __syncthreads();
    }

    // ---- Linear(64 -> C) + argmax (first maximum wins) on wavefront 0 ------------------------------
    if (run_fc && wv == 0) {
        float v = -INFINITY;
        if (lane < C) {
            float acc = fcb;
            const float4* pl = reinterpret_cast<const float4*>(pooled);
#pragma unroll
            for (int c = 0; c < CH / 4; ++c) {
                const float4 a4 = fcw[c], p4 = pl[c];
                acc = fmaf(a4.x, p4.x, acc);
                acc = fmaf(a4.y, p4.y, acc);
                acc = fmaf(a4.z, p4.z, acc);
                acc = fmaf(a4.w, p4.w, acc);
            }
            logits[(size_t)clip * C + lane] = acc;
            if constexpr (STREAM) {  // zero-copy delivery: the host's pinned copy, written through (system scope), see below
                if (sp.h_logits) __hip_atomic_store(sp.h_logits + (size_t)clip * C + lane, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            v = acc;
        }
        const int idx = wave_argmax_first(v, lane, C);
        if (label && lane == 0) label[clip] = idx;
        if constexpr (STREAM) {
            if (sp.h_label && lane == 0) __hip_atomic_store(sp.h_label + clip, idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    if constexpr (STREAM) {
        // hop counter: every workgroup read sp.hops[0] in its prologue; the one that finishes last advances it
        // (sp.hops[1] counts finished workgroups).  The kernel boundary publishes it to the next push.
        // Zero-copy result delivery (kws_stream_host_results): logits and labels also went to pinned host memory as
        // system-scope stores; a workgroup bumps the counter only after its own have been acknowledged (vmcnt 0: they are
        // on their way over PCIe, in order), and the last one raises the host's flag behind them -- posted writes of one
        // device keep their order, so the host that sees the flag sees every stream's results.  No fence (they write whole
        // L2s back on this part).
        // Only the workgroup that ran a stream's fc takes part (with time tiles it is the last of the stream's workgroups to
        // arrive, so every tile of the stream is past its reads of the counter): one add per STREAM to this one address, not
        // one per workgroup -- adds from eight XCDs to one address queue up at the coherence point.
        int finishers = (int)gridDim.x;
        if constexpr (CLUSTER) finishers /= cl_n;
        if (sp.h_flag) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (run_fc && tid == 0 && atomicAdd(&sp.hops[1], 1) == finishers - 1) {
            sp.hops[1] = 0;
            sp.hops[0] = hops_before + 1;
            if (sp.h_flag) __hip_atomic_store(sp.h_flag, hops_before + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    stamp();  // 12: pool + fc + argmax done
    if (stamps && tid == KWS_X_DSCNN_STAMP_TID) stamps[(size_t)clip * KWS_DSCNN_STAMPS + KWS_DSCNN_STAMPS - 1] = __builtin_amdgcn_s_memrealtime();
    break;
    }
    if constexpr (PERSIST) {  // the last clip's pool + fc (its partials are behind the loop's last barrier)
        if (wv_k == NW - 1) {
            pool_fc_wave(w_arg, lds, lane_k, prev_clip, logits, label, a_prev);
            if (stamps && lane_k == 0) stamps[(size_t)prev_clip * KWS_DSCNN_STAMPS + 13] = __builtin_amdgcn_s_memtime();
        }
    }
}

// The instantiations of kws_dscnn_fwd_kernel the host can launch.  This table is the one place that names them:
// dscnn_init_device walks it, launch_variant looks a launch up in it.
enum : unsigned { F_DIAG = 1, F_PRECONV = 2, F_STREAM = 4, F_CLUSTER = 8, F_PERSIST = 16, F_SCAN = 32, F_ACTIVE = 64 };
struct FwdVariant {
    int mode;
    unsigned flags;  // the seven template booleans below as one word: what launch_variant is asked for
    bool diag, preconv, stream, cluster, persist, scan, active;
    constexpr FwdVariant(int m, unsigned f)
        : mode(m), flags(f), diag(f & F_DIAG), preconv(f & F_PRECONV), stream(f & F_STREAM), cluster(f & F_CLUSTER), persist(f & F_PERSIST), scan(f & F_SCAN),
          active(f & F_ACTIVE) {}
};
// The ACTIVE instantiations are compiled in a unit of their own (kws_dscnn_active.hip, which includes this file with
// KWS_DSCNN_ACTIVE_UNIT defined): instantiated beside the others they gave the stages' templates a second caller each, and the
// compiler then laid out the two cluster kernels differently.
constexpr FwdVariant kFwdVariants[] = {
#ifdef KWS_DSCNN_ACTIVE_UNIT
    {4, F_STREAM | F_ACTIVE},              // launch_dscnn_stream_active: split-bf16, one workgroup per active stream
    {4, F_STREAM | F_CLUSTER | F_ACTIVE},  // ... sp.cluster > 1 workgroups per active stream
    {5, F_STREAM | F_ACTIVE},              // launch_dscnn_stream_active: f16 pairs, one workgroup per active stream
    {5, F_STREAM | F_CLUSTER | F_ACTIVE},  // ... sp.cluster > 1 workgroups per active stream
#else
    {0, F_DIAG},                       // launch_dscnn: VALU cross-check of the GEMMs (diagnostics entry)
    {1, F_DIAG},                       // launch_dscnn: f32 MFMA, and every mode number without a case of its own
    {2, F_DIAG},                       // launch_dscnn: timing ablation, matrix core only
    {3, F_DIAG},                       // launch_dscnn: timing ablation, stencil only
    {4, F_DIAG},                       // launch_dscnn: split-bf16 with an activation dump or stamps
    {6, F_DIAG},                       // launch_dscnn: timing ablation, split-bf16 without the stencil
    {4, 0},                            // launch_dscnn: split-bf16 product, one clip per workgroup
    {4, F_PRECONV},                    // launch_dscnn: multi-channel model, every mode but 5
    {4, F_STREAM},                     // launch_dscnn_stream: split-bf16, one workgroup per stream
    {4, F_STREAM | F_CLUSTER},         // launch_dscnn_stream: split-bf16, sp.cluster > 1 workgroups per stream
    {5, F_DIAG},                       // launch_dscnn: f16 pairs with an activation dump or stamps
    {5, 0},                            // launch_dscnn: f16-pair product, one clip per workgroup
    {5, F_PRECONV},                    // launch_dscnn: multi-channel model, f16 pairs
    {5, F_STREAM},                     // launch_dscnn_stream: f16 pairs, one workgroup per stream
    {5, F_STREAM | F_CLUSTER},         // launch_dscnn_stream: f16 pairs, sp.cluster > 1 workgroups per stream
    {4, F_DIAG | F_PERSIST},           // launch_dscnn: split-bf16, B > n_cu, with an activation dump or stamps
    {4, F_PERSIST},                    // launch_dscnn: split-bf16 product, B > n_cu
    {5, F_DIAG | F_PERSIST},           // launch_dscnn: f16 pairs, B > n_cu, with an activation dump or stamps
    {5, F_PERSIST},                    // launch_dscnn: f16-pair product, B > n_cu (the flagship batch)
    {4, F_SCAN},                       // launch_dscnn_scan: split-bf16, one window per workgroup
    {4, F_PERSIST | F_SCAN},           // launch_dscnn_scan: split-bf16, B > n_cu
    {5, F_SCAN},                       // launch_dscnn_scan: f16 pairs, one window per workgroup
    {5, F_PERSIST | F_SCAN},           // launch_dscnn_scan: f16 pairs, B > n_cu
#endif
};
constexpr size_t N_FWD_VARIANTS = sizeof(kFwdVariants) / sizeof(kFwdVariants[0]);

template <size_t I>
constexpr auto kFwdKernel = &kws_dscnn_fwd_kernel<kFwdVariants[I].mode, kFwdVariants[I].diag, kFwdVariants[I].preconv, kFwdVariants[I].stream,
                                                  kFwdVariants[I].cluster, kFwdVariants[I].persist, kFwdVariants[I].scan, kFwdVariants[I].active>;
template <size_t... I>
constexpr std::array<FwdKernelFn, sizeof...(I)> fwd_kernel_table(std::index_sequence<I...>) {
    return {{kFwdKernel<I>...}};
}
constexpr auto kFwdKernels = fwd_kernel_table(std::make_index_sequence<N_FWD_VARIANTS>{});

// weights_for_this_clip and scan_windows_now read the arguments through FwdKernelArgs: a new or moved argument goes there too
static_assert(std::is_same_v<decltype(kFwdKernel<0>), const FwdKernelFn>,
              "kws_dscnn_fwd_kernel's parameters and FwdKernelArgs / FwdKernelFn must change together");

// One launch of the instantiation (mode, flags) on `grid` workgroups; the remaining arguments are the kernel's.  A variant that
// is not in the table is refused before any launch: it would have no dynamic-LDS attribute (dscnn_init_device).
hipError_t launch_variant(int mode, unsigned flags, int grid, hipStream_t s, const DscnnWeights& w, const float* d_feat, int B, float* d_logits,
                          int32_t* d_label, float* d_act, unsigned long long* d_stamps, const int* d_ring_hops, const StreamPush& sp) {
    for (size_t i = 0; i < N_FWD_VARIANTS; ++i) {
        if (kFwdVariants[i].mode != mode || kFwdVariants[i].flags != flags) continue;
        hipLaunchKernelGGL(kFwdKernels[i], dim3(grid), dim3(NT), LDS_FLOATS * sizeof(float), s, w, d_feat, B, d_logits, d_label, d_act, d_stamps,
                           d_ring_hops, sp);
        return hipGetLastError();
    }
    return hipErrorInvalidValue;
}

// The kernel needs the CU's whole 160 KiB of LDS as dynamic shared memory: opt in once per device.
hipError_t init_variants() {
    for (FwdKernelFn k : kFwdKernels) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_FLOATS * (int)sizeof(float));
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

#ifdef KWS_DSCNN_ACTIVE_UNIT
hipError_t dscnn_active_init_device() { return init_variants(); }

hipError_t launch_dscnn_stream_active(hipStream_t s, const DscnnWeights& w, const StreamPush& sp, float* d_feat_ring, int n_streams, float* d_logits,
                                      int32_t* d_label, bool pair, const int32_t* d_active, int n_active) {
    const bool tiles = sp.cluster > 1;  // time tiles: sp.cluster workgroups per active stream
    return launch_variant(pair ? 5 : 4, (tiles ? F_STREAM | F_CLUSTER : F_STREAM) | F_ACTIVE, tiles ? n_active * sp.cluster : n_active, s, w, d_feat_ring,
                          n_streams, d_logits, d_label, nullptr, nullptr, d_active, sp);
}
#else
hipError_t dscnn_init_device() {
    const hipError_t e = init_variants();
    return e == hipSuccess ? dscnn_active_init_device() : e;
}

hipError_t launch_dscnn_stream(hipStream_t s, const DscnnWeights& w, const StreamPush& sp, float* d_feat_ring, int n_streams,
                               float* d_logits, int32_t* d_label, bool pair) {
    static_assert(sizeof(float) * (size_t)(LDS_FLOATS - OFF_Z2) >= 16 * 1024 + STREAM_F64_BYTES, "room for the one-frame front end's tables and scratch");
    const bool tiles = sp.cluster > 1;  // time tiles: sp.cluster workgroups per stream
    return launch_variant(pair ? 5 : 4, tiles ? F_STREAM | F_CLUSTER : F_STREAM, tiles ? n_streams * sp.cluster : n_streams, s, w, d_feat_ring,
                          n_streams, d_logits, d_label, nullptr, nullptr, nullptr, sp);
}

hipError_t launch_dscnn(hipStream_t s, const DscnnWeights& w, const float* d_feat, int B, float* d_logits,
                        int32_t* d_label, float* d_act, int mode, unsigned long long* d_stamps, const int* d_ring_hops,
                        bool preconv, int frames_lag, int n_cu) {
    StreamPush lag{};  // the two-launch streaming route: only the hops-per-frame count travels (the window's first row)
    lag.frames_lag = frames_lag;
    const bool product = mode == 4 || mode == 5;
    const unsigned diag = (d_act || d_stamps) ? F_DIAG : 0u;  // without either, the product modes run their DIAG = false instantiation
    // More clips than CUs on a product path: persistent workgroups, one per CU, each carrying its clips one after another
    // (kws_dscnn_fwd_kernel, PERSIST).  The streaming route (d_ring_hops) and the pre-convolved entry keep one clip per workgroup.
    if (n_cu > 0 && B > n_cu && !preconv && !d_ring_hops && product)
        return launch_variant(mode, F_PERSIST | diag, n_cu, s, w, d_feat, B, d_logits, d_label, d_act, d_stamps, nullptr, lag);
    // d_feat = conv1 output of a multi-channel model (kws_conv1_general_kernel): product paths only
    if (preconv) return launch_variant(mode == 5 ? 5 : 4, F_PRECONV, B, s, w, d_feat, B, d_logits, d_label, nullptr, nullptr, nullptr, StreamPush{});
    // mode: 0 = VALU cross-check of the GEMMs, 1 = f32 MFMA (and any number not listed here), 2 / 3 = timing ablations (matrix
    // core only / stencil only; wrong results by construction, reachable only through the diagnostics entry point), 4 / 5 = the
    // product paths, 6 = split-bf16 without the stencil.  One clip per workgroup; one workgroup per CU (160 KiB LDS).
    const bool listed = mode == 0 || (mode >= 2 && mode <= 6);
    return launch_variant(listed ? mode : 1, product ? diag : F_DIAG, B, s, w, d_feat, B, d_logits, d_label, d_act, d_stamps, d_ring_hops, lag);
}

hipError_t launch_dscnn_scan(hipStream_t s, const DscnnWeights& w, const float* d_feat, int B, float* d_logits, int32_t* d_label,
                             int mode, int n_cu, const ScanWindows& sw) {
    if (mode != 4 && mode != 5) return hipErrorInvalidValue;  // refused by kws_scan_i16 before it gets here
    StreamPush sp{};
    sp.scan = sw;
    const bool persist = n_cu > 0 && B > n_cu;  // persistent workgroups above the CU count, as launch_dscnn
    return launch_variant(mode, persist ? F_PERSIST | F_SCAN : F_SCAN, persist ? n_cu : B, s, w, d_feat, B, d_logits, d_label, nullptr, nullptr,
                          nullptr, sp);
}
#endif  // KWS_DSCNN_ACTIVE_UNIT

}  // namespace kws
