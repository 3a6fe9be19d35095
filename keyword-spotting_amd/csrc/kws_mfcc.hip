// Batched MFCC front end for gfx950 (MI355X), replacing per-clip psf.mfcc calls
// (reference call site kws/libs/audio_processor.py:270-278; stages a1-a8 of SURVEY.md section 8).
//
// Work decomposition
//   grid = (ceil(num_frames / 24), B); a workgroup is MFCC_WAVES (4) wavefronts and owns 24 frames
//   (12 frame pairs, three per wavefront; shape chosen by A/B timing on MI355X).  Together
//   the waves stage the PCM span of those frames (4080 samples for 400/160) from HBM with 16-byte loads,
//   convert to float32, apply pre-emphasis once
//   and keep the span in LDS, next to the tables every wave needs (DCT x lifter, sparse-mel weights,
//   second-pass twiddles).  After one barrier the waves never synchronise again: each has a private
//   5 KiB scratch and LDS instructions of one wavefront execute in order.
//
//   Two real frames are packed into one 512-point complex FFT (z = a + i*b): lane l holds
//   z[64*n1 + l], n1 = 0..7, and the transform is three radix-8 passes in registers with two LDS
//   exchanges (8 x 8 x 8).  The spectra of the two frames are separated with the conjugate-symmetry
//   identity, |X|^2/512 goes to LDS once, and the 26 triangular mel filters are evaluated sparsely:
//   the bins [edge_s, edge_s+1) between two mel edges are cut into chunks of <= 8 bins, one chunk per
//   lane, each lane accumulating the rising weights (filter s) and falling weights (filter s-1) of its
//   bins; a filter is the sum of <= a few chunk partials.  log, then a [numcep x nfilt] DCT-II(ortho)
//   x lifter table from LDS; coefficient 0 is log(frame energy) (psf appendEnergy).
//
// Numerics: PCM/32768 and pre-emphasis are bit-exact float32 as in the reference pipeline (separate
// multiply and subtract roundings); everything after is float32 here vs float64 in psf
// (tolerance 1e-4 on MFCC, see tests/test_gpu_parity.py).
#include <cstdlib>

#include "kws_augment_dev.h"
#include "kws_internal.h"
#include "kws_mfcc_dev.h"

namespace kws {
namespace {

// ------------------------------------------------------------------------------------------------
// TAIL6: frame_len in (384, 448] (the reference's 400): sample blocks n1 < 6 lie wholly inside the frame, block 6 is cut
// by a lane bound and block 7 is zero -- no loads or selects for it, and the zeros fold through the first butterflies.
template <typename T, bool TAIL6>
__device__ __forceinline__ void mfcc_body(const FrontendParams& p, const FrontendTables& t, const T* __restrict__ wav,
                                          float* __restrict__ out, const RefineList& rl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // workgroup-shared part (every offset a multiple of 16 bytes)
    const int nfp = (p.nfilt + 3) & ~3;                        // DCT rows padded to float4
    float* dctb = reinterpret_cast<float*>(smem);              // [numcep][nfp]
    cf* tw2 = reinterpret_cast<cf*>(dctb + ((p.numcep * nfp + 3) & ~3));  // [8][8]
    float* ybuf = reinterpret_cast<float*>(tw2 + 64);          // chunk_samples floats (padded to 8)
    unsigned char* scr0 = reinterpret_cast<unsigned char*>(ybuf + ((p.chunk_samples + 7) & ~7));

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int clip = blockIdx.y;
    const int f0 = blockIdx.x * MFCC_FRAMES_PER_WG;
    const T* __restrict__ x = wav + (size_t)clip * p.n_samples;

    // ---- stage PCM span -> float32, pre-emphasised, in LDS; shared tables -------------------------
    const int s0 = f0 * p.frame_step;
    const float c = p.preemph;
    // the clip's last workgroup owns fewer frames (3 of 24 for 99 frames): it stages only the span they cover
    const int my_frames = min(MFCC_FRAMES_PER_WG, p.num_frames - f0);
    const int my_samples = (my_frames - 1) * p.frame_step + p.frame_len;
    for (int g = tid; g * 8 < my_samples; g += MFCC_THREADS) {
        const int n = s0 + g * 8;
        float y[8];
        if (sizeof(T) == 2 && p.vec_ok && n + 8 <= p.n_samples) {
            // every 8-sample group is 16-byte aligned here
            const uint4 raw = *reinterpret_cast<const uint4*>(x + n);
            float prev = (n > 0) ? to_unit(x[n - 1]) : 0.f;
            const uint32_t wd[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int16_t s = (int16_t)((wd[i >> 1] >> (16 * (i & 1))) & 0xffffu);
                const float cur = to_unit(s);
                y[i] = (n + i > 0) ? __fsub_rn(cur, __fmul_rn(c, prev)) : cur;
                prev = cur;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int m = n + i;
                float v = 0.f;
                if (m < p.n_samples) {
                    const float cur = to_unit(x[m]);
                    v = (m > 0) ? __fsub_rn(cur, __fmul_rn(c, to_unit(x[m - 1]))) : cur;
                }
                y[i] = v;
            }
        }
        float4* dst = reinterpret_cast<float4*>(ybuf + g * 8);
        dst[0] = make_float4(y[0], y[1], y[2], y[3]);
        dst[1] = make_float4(y[4], y[5], y[6], y[7]);
    }
    for (int i = tid; i < (p.numcep * nfp + 3) / 4; i += MFCC_THREADS)  // the host keeps the padded LDS image
        reinterpret_cast<float4*>(dctb)[i] = reinterpret_cast<const float4*>(t.dct_pad)[i];
    fill_tw2(t.twiddle, tw2, tid);

    // ---- per-lane constants -----------------------------------------------------------------------
    cf t1[8];
    load_twiddles(t.twiddle, lane, t1);
    MelLane ml;
    load_mel_lane(t, lane, ml);
    unsigned char* scr = scr0 + wv * SCR_BYTES;
    zero_scratch(scr, lane);
    __syncthreads();  // the only workgroup barrier: staged samples and tables are visible to all waves

    const PairScratch sc = {reinterpret_cast<cf*>(scr + SCR_XBUF), reinterpret_cast<float2*>(scr + SCR_PBUF),
                            reinterpret_cast<float*>(scr + SCR_LBUF),
                            dctb, tw2, nfp};

    for (int pr = wv; pr < MFCC_FRAMES_PER_WG / 2; pr += MFCC_WAVES) {
        const int fa = f0 + 2 * pr;
        if (fa >= p.num_frames) break;  // wave-uniform
        const bool has_b = (fa + 1) < p.num_frames;
        const float* ya = ybuf + (2 * pr) * p.frame_step;
        const float* yb = ya + p.frame_step;

        // The loads are unconditional and the frame bound is applied by a select: a read past the frame (at most
        // 511 floats past the staged span) lands in the wavefronts' scratch behind ybuf -- allocated LDS, any bits --
        // and is discarded; conditional loads compile to one branch per load.  The all-zero test ORs the bit
        // patterns (sign bit dropped: -0.0 counts as zero, like the float comparison).
        cf v[8];
        uint32_t ora = 0u, orb = 0u;
        if constexpr (TAIL6) {
#pragma unroll
            for (int n1 = 0; n1 < 7; ++n1) {
                const int i = 64 * n1 + lane;
                float a = ya[i], b = yb[i];
                if (n1 == 6) {
                    const bool in = i < p.frame_len;
                    a = in ? a : 0.f, b = in ? b : 0.f;
                }
                v[n1] = cf{a, b};
                ora |= __builtin_bit_cast(uint32_t, a);
                orb |= __builtin_bit_cast(uint32_t, b);
            }
            v[7] = cf{0.f, 0.f};
            if (!has_b) {  // wave-uniform, the clip's last pair only: frame b is past the clip
#pragma unroll
                for (int n1 = 0; n1 < 7; ++n1) v[n1].y = 0.f;
                orb = 0u;
            }
        } else {
#pragma unroll
            for (int n1 = 0; n1 < 8; ++n1) {
                const int i = 64 * n1 + lane;
                const bool in = i < p.frame_len;
                const float la = ya[i], lb = yb[i];  // loaded whether or not they are used (see above)
                const float a = in ? la : 0.f, b = (in && has_b) ? lb : 0.f;
                v[n1] = cf{a, b};
                ora |= __builtin_bit_cast(uint32_t, a);  // (bit_cast of a vector ELEMENT reads element 0 with this clang:
                orb |= __builtin_bit_cast(uint32_t, b);  //  cast the scalars)
            }
        }
        const bool nza = __any((ora << 1) != 0u);
        const bool nzb = __any((orb << 1) != 0u);
        const uint32_t flags = mfcc_pair(v, nza, nzb, has_b, p, sc, t1, ml, lane,
                                         out + ((size_t)clip * p.num_frames + fa) * p.numcep,
                                         out + ((size_t)clip * p.num_frames + fa + 1) * p.numcep);
        // a frame the float32 arithmetic cannot hold to 1e-4 (rare; wave-uniform): the pair goes onto the refinement
        // kernel's worklist with the mask of its flagged frames
        // (one 64-bit atomic: entries in the low word -- its old value is the slot --, flagged frames in the high word)
        if (flags && rl.ctr && lane == 0) {
            const unsigned long long old = atomicAdd(reinterpret_cast<unsigned long long*>(rl.ctr), 1ull | ((unsigned long long)__builtin_popcount(flags) << 32));
            const int at = (int)(unsigned)old;
            if (at < rl.cap) rl.list[at] = (int)((((unsigned)(rl.clip0 + clip) * (unsigned)((p.num_frames + 1) / 2) + (unsigned)(fa >> 1)) << 2) | flags);
        }
        wave_lds_order();
    }
}

#ifndef KWS_MFCC_EU
#define KWS_MFCC_EU 4
#endif
// amdgpu_waves_per_eu(4, 4): 128 registers, so that the four 4-wave workgroups the LDS admits per CU (16
// wavefronts, 4 per SIMD) all become resident; the kernel is latency-bound on LDS round trips.
// kws_mfcc_i16_tile_kernel / kws_mfcc_f32_kernel: frame lengths in (384, 448] (the reference's 400 samples), see TAIL6; the
// *_any_kernel pair takes every other frame length up to 512 (one kernel with both bodies spills registers).  int16 input
// at a geometry the wavefront-resident kernel below covers goes there instead (kws_mfcc_i16_kernel, the product path).
__global__ __launch_bounds__(MFCC_THREADS) __attribute__((amdgpu_waves_per_eu(KWS_MFCC_EU, KWS_MFCC_EU))) void kws_mfcc_i16_tile_kernel(FrontendParams p, FrontendTables t,
                                                                    const int16_t* __restrict__ wav,
                                                                    float* __restrict__ out, RefineList rl) {
    mfcc_body<int16_t, true>(p, t, wav, out, rl);
}
__global__ __launch_bounds__(MFCC_THREADS) __attribute__((amdgpu_waves_per_eu(KWS_MFCC_EU, KWS_MFCC_EU))) void kws_mfcc_f32_kernel(FrontendParams p, FrontendTables t,
                                                                    const float* __restrict__ wav,
                                                                    float* __restrict__ out, RefineList rl) {
    mfcc_body<float, true>(p, t, wav, out, rl);
}
__global__ __launch_bounds__(MFCC_THREADS) __attribute__((amdgpu_waves_per_eu(KWS_MFCC_EU, KWS_MFCC_EU))) void kws_mfcc_i16_any_kernel(FrontendParams p, FrontendTables t,
                                                                    const int16_t* __restrict__ wav,
                                                                    float* __restrict__ out, RefineList rl) {
    mfcc_body<int16_t, false>(p, t, wav, out, rl);
}
__global__ __launch_bounds__(MFCC_THREADS) __attribute__((amdgpu_waves_per_eu(KWS_MFCC_EU, KWS_MFCC_EU))) void kws_mfcc_f32_any_kernel(FrontendParams p, FrontendTables t,
                                                                    const float* __restrict__ wav,
                                                                    float* __restrict__ out, RefineList rl) {
    mfcc_body<float, false>(p, t, wav, out, rl);
}

// ------------------------------------------------------------------------------------------------
// The product kernel for int16 PCM at the reference geometry (round 3): WAVEFRONT-RESIDENT runs of a clip.
//
// The tile kernel above pays, for every 12 frame pairs, a workgroup launch, ~40 table loads per lane, a scratch clear, the
// global-memory latency of its PCM span and a workgroup barrier, and its four wavefronts march in step.  Here a wavefront
// owns a run of a clip's chunks (five by default: 20 frames) for its whole lifetime: tables and per-lane constants are
// loaded once, then it walks its run in chunks of four frames (two packed pairs).  A chunk's PCM span (3 steps + one frame
// = 880 samples) arrives as two 16-byte loads per lane, is converted and pre-emphasised in registers (the sample before a
// lane's vector comes from its neighbour by DPP) and lands in the wavefront's own 4 KB of LDS.  No wavefront ever waits for
// another: the one __syncthreads publishes the shared DCT and twiddle tables at the start.  Consecutive spans overlap by
// 240 samples; the re-read is an L2 hit issued by the same wavefront a few microseconds earlier.  Same arithmetic, same
// bits as the tile kernel (PCM scaling and pre-emphasis are the same two float32 roundings; mfcc_pair is shared).
// Measured on 4096 clips, same box and call: tile kernel 0.208 ms, this kernel 0.183 ms.  (Issuing the next chunk's loads
// before this chunk's transforms -- a register prefetch -- was measured and dropped: the eight vector registers it keeps
// alive spill under the 128-register cap, 0.201 ms; the other three wavefronts of the SIMD cover the latency.)
constexpr int WR_PAIRS = 2, WR_FRAMES = 2 * WR_PAIRS;   // frames per chunk
constexpr int WR_SPAN = 1024;                            // floats of LDS per wavefront for the chunk's span (two uint4 of PCM per lane)
constexpr int WR_WAVE_BYTES = WR_SPAN * 4 + SCR_BYTES;
static_assert(WR_FRAMES == MFCC_WR_FRAMES, "the host's plan of a ragged batch counts chunks of WR_FRAMES frames");

// One 16-byte vector of a recording of a ragged batch (n0 a multiple of 8, x + n0 16-byte aligned): the vector itself when it lies
// inside the recording, zeros when it lies past it, and the one vector that straddles len sample by sample -- what follows the
// recording in the buffer (the next recording, or the buffer's end) is never read.
__device__ __forceinline__ uint4 ragged_vec8(const int16_t* __restrict__ x, int n0, int len) {
    if (n0 + 8 <= len) return *reinterpret_cast<const uint4*>(x + n0);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (n0 < len) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (n0 + i < len) w[i >> 1] |= (uint32_t)(uint16_t)x[n0 + i] << (16 * (i & 1));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// The same for float32 samples: a vector of 8 samples is two 16-byte loads (n0 a multiple of 8, x + n0 16-byte aligned), zeros past
// len, and the one vector that straddles len sample by sample.  len = the clip's length for an equal-length batch, where
// n_samples % 8 == 0 and no vector straddles.
template <bool RAGGED>
__device__ __forceinline__ void f32_vec8(const float* __restrict__ x, int n0, int len, float (&a)[8]) {
    if (n0 + 8 <= len) {
        const float4 lo = *reinterpret_cast<const float4*>(x + n0), hi = *reinterpret_cast<const float4*>(x + n0 + 4);
        a[0] = lo.x, a[1] = lo.y, a[2] = lo.z, a[3] = lo.w, a[4] = hi.x, a[5] = hi.y, a[6] = hi.z, a[7] = hi.w;
        return;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = 0.f;
    if constexpr (RAGGED) {
        if (n0 < len) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (n0 + i < len) a[i] = x[n0 + i];
        }
    }
}

// Eight consecutive augmented samples n0 .. n0 + 7 (n0 a multiple of 8) of a clip of the resident split, the values aug_sample
// gives one by one.  The source run starts at j0 = n0 - shift, aligned to 2 bytes only: the two ALIGNED 16-byte vectors that
// hold it are read -- each lies wholly inside the clip's own row or is replaced by zeros (n_samples % 8 == 0), so nothing
// outside the row is touched and positions outside [0, n) contribute zeros -- and funnelled by j0 mod 8 half-words.  That
// amount is wave-uniform (every n0 of a wavefront is a multiple of 8), so the word selects take scalar conditions.  The
// background term is a float32 stream at 4-byte alignment: two 16-byte loads when the eight samples lie inside the pool.
typedef float float4_a4 __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ void aug_vec8(const AugClip& c, int n0, int n, float (&a)[8]) {
    if (n0 + 8 > n) {  // past the clip: the caller zeroes the pre-emphasised samples
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = 0.f;
        return;
    }
    const int r = uniform_i(-c.shift & 7);  // = (n0 - shift) mod 8
    const int base = n0 - c.shift - r;      // a multiple of 8, possibly negative
    uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
    if (!c.silence) {
        if (base >= 0 && base + 8 <= n) lo = *reinterpret_cast<const uint4*>(c.x + base);
        if (base + 8 >= 0 && base + 16 <= n) hi = *reinterpret_cast<const uint4*>(c.x + base + 8);
    }
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    // word shift by r / 2 as two levels of bit selects under scalar masks (ternaries on the words turn into one dynamically
    // indexed array in private memory with this compiler)
    const uint32_t m2 = (r & 4) ? ~0u : 0u, m1 = (r & 2) ? ~0u : 0u;
    uint32_t u[6], v[5];
#pragma unroll
    for (int k = 0; k < 6; ++k) u[k] = (w[k + 2] & m2) | (w[k] & ~m2);
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = (u[k + 1] & m1) | (u[k] & ~m1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t wd = (r & 1) ? __builtin_amdgcn_alignbyte(v[k + 1], v[k], 2) : v[k];
        a[2 * k] = pcm_unit((int16_t)(wd & 0xffffu));
        a[2 * k + 1] = pcm_unit((int16_t)(wd >> 16));
    }
    if (c.bg) {
        const int k0 = c.off + n0;
        float g[8];
        if (k0 >= 0 && k0 + 8 <= c.bg_len) {
            const float4_a4 g0 = *reinterpret_cast<const float4_a4*>(c.bg + k0);
            const float4_a4 g1 = *reinterpret_cast<const float4_a4*>(c.bg + k0 + 4);
            g[0] = g0.x, g[1] = g0.y, g[2] = g0.z, g[3] = g0.w, g[4] = g1.x, g[5] = g1.y, g[6] = g1.z, g[7] = g1.w;
        } else {  // an offset that leaves the pool (never one of kws_augment_draw's): zeros outside it, as kws_augment_i16 reads them
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int k = c.off + n0 + i;
                g[i] = (k >= 0 && k < c.bg_len) ? c.bg[k] : 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = __fadd_rn(a[i], __fmul_rn(g[i], c.vol));
    }
}

__host__ __device__ inline size_t mfcc_wr_lds_bytes(const FrontendParams& p) {
    const int nfp = (p.nfilt + 3) & ~3;
    return sizeof(float) * (size_t)(((p.numcep * nfp + 3) & ~3) + 2 * 64) + (size_t)MFCC_WAVES * WR_WAVE_BYTES;
}

// The body of the wavefront-resident kernels.  AUG (kws_mfcc_augment_i16_kernel, the resident training loader): the same run of
// chunks, LDS map and mfcc_pair; only the way a chunk's samples reach the registers differs -- see aug_vec8 above.  Every AUG
// branch is an if constexpr: the plain instantiation keeps the instruction sequence kws_mfcc_i16_kernel had as a kernel of
// its own (register names apart).
// G (kws_mfcc_dev.h): GeomAny reads the geometry from p, as every wavefront-resident kernel did before the type existed; GeomRef
// is the reference configuration at compile time (kws_mfcc_i16_ref_kernel): the row pointer and the frames' LDS addresses
// advance by constants, the frame bound is a lane mask, and the worklist code exists only in the instantiation that flags.
// RAGGED (kws_mfcc_i16_ragged_kernel): the clips are the recordings of rg, each with its own length, frame count, first row and
// share of the launch's wavefronts; a wavefront finds its recording once, by a scalar binary search over the records' first
// wavefronts, and from there on p.n_samples / p.num_frames are that recording's.  Every RAGGED branch is an if constexpr.
// T (kws_mfcc_f32_wr_kernel, kws_mfcc_f32_ragged_kernel): float32 samples, taken as they are.  A chunk's span is then four
// 16-byte loads per lane, taken one half-span (two loads) at a time: load, pre-emphasise, store, and only then the other half --
// both halves in registers at once would be the eight extra registers the dropped prefetch could not afford.  Every float branch
// is an if constexpr: the int16 instantiations compile to the instructions they had.
template <bool AUG, class G = GeomAny, bool RAGGED = false, typename T = int16_t>
__device__ __forceinline__ void mfcc_wr_body(FrontendParams p, FrontendTables t, const T* __restrict__ wav,
                                             float* __restrict__ out, RefineList rl, int B, int chunks_per_wave,
                                             AugmentArgs aug, RaggedArgs rg = RaggedArgs{}) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool F32 = sizeof(T) == 4;
    static_assert(!F32 || (!AUG && !G::REF), "float32 samples take the generic geometry and no augmentation");
    static_assert(!(AUG && G::REF), "the fused loader keeps the generic geometry");
    static_assert(!RAGGED || (!AUG && !G::REF), "the ragged kernel reads PCM at the generic geometry");
    const int nfp = (G::nfilt(p) + 3) & ~3;
    const int numcep = G::numcep(p), frame_step = G::frame_step(p);
    float* dctb = reinterpret_cast<float*>(smem);
    cf* tw2 = reinterpret_cast<cf*>(dctb + ((numcep * nfp + 3) & ~3));
    // (GeomRef: the wavefront's number as a scalar -- the compiler cannot see that threadIdx.x >> 6 is wave-uniform; with a vector
    // number the chunk and pair loops are exec-masked vector loops whose counters, pointers and LDS bases take vector registers)
    const int tid = threadIdx.x, lane = tid & 63, wv = G::REF ? uniform_i(tid >> 6) : tid >> 6;
    unsigned char* mine = reinterpret_cast<unsigned char*>(tw2 + 64) + wv * WR_WAVE_BYTES;
    float* ybuf = reinterpret_cast<float*>(mine);
    unsigned char* scr = mine + WR_SPAN * 4;

    for (int i = tid; i < (numcep * nfp + 3) / 4; i += MFCC_THREADS)
        reinterpret_cast<float4*>(dctb)[i] = reinterpret_cast<const float4*>(t.dct_pad)[i];
    fill_tw2(t.twiddle, tw2, tid);
    cf t1[8];
    load_twiddles(t.twiddle, lane, t1);
    MelLane ml;
    load_mel_lane(t, lane, ml);
    zero_scratch(scr, lane);

    // this wavefront's share: chunks [c, c_end) of clip `clip`
    int n_chunks, clip, c, c_end_of, pair_base = 0, pad_floats = 0;
    bool active_of;
    size_t x_first;
    if constexpr (RAGGED) {
        const int gw = uniform_i(blockIdx.x * MFCC_WAVES + wv);
        active_of = gw < B;  // B: the launch's wavefronts
        int lo = 0, hi = rg.R;  // rec[lo].wave_off <= gw < rec[hi].wave_off (record R closes the table)
        if (active_of)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (rg.rec[mid].wave_off <= gw) lo = mid;
                else hi = mid;
            }
        const RaggedRec rr = rg.rec[lo];
        p.n_samples = uniform_i(rr.len);
        p.num_frames = uniform_i(rr.frames);
        n_chunks = (p.num_frames + WR_FRAMES - 1) / WR_FRAMES;
        const int cpw = uniform_i(rr.cpw);
        c = (gw - uniform_i(rr.wave_off)) * cpw;
        c_end_of = min(n_chunks, c + cpw);
        active_of = active_of && c < c_end_of;
        clip = 0;  // rows and worklist entries count from the recording's own first row and pair
        x_first = (size_t)rr.start;
        out += (size_t)uniform_i(rr.frame_off) * numcep;
        pair_base = uniform_i(rr.pair_off);
        pad_floats = (uniform_i(rg.rec[lo + 1].frame_off) - uniform_i(rr.frame_off) - p.num_frames) * numcep;
    } else {
        n_chunks = (p.num_frames + WR_FRAMES - 1) / WR_FRAMES;
        const int waves_per_clip = (n_chunks + chunks_per_wave - 1) / chunks_per_wave;
        const int gw = blockIdx.x * MFCC_WAVES + wv;
        clip = gw / waves_per_clip;
        const int part = gw - clip * waves_per_clip;
        c = part * chunks_per_wave;
        c_end_of = min(n_chunks, c + chunks_per_wave);
        active_of = clip < B && c < c_end_of;  // wave-uniform
        x_first = (size_t)(active_of ? clip : 0) * p.n_samples;
    }
    const int c_end = c_end_of;
    const bool active = active_of;
    const T* __restrict__ x = AUG ? nullptr : wav + x_first;
    AugClip ac{};
    if constexpr (AUG) ac = aug_clip(aug, active ? clip : 0, p.n_samples);  // wave-uniform: scalar registers
    const int chunk_step = WR_FRAMES * frame_step;  // samples from one chunk's span to the next (a multiple of 8: checked by the launcher)

    // two 16-byte vectors of PCM per lane cover the span; a vector is inside the clip or past its end (n_samples % 8 == 0)
    uint4 v0 = make_uint4(0, 0, 0, 0), v1 = v0;
    int16_t before = 0;
    auto fetch = [&](int cc, int lane) {
        if constexpr (!F32) {
            const int s0 = cc * chunk_step;
            const int n0 = s0 + 8 * lane, n1 = n0 + 512;
            if constexpr (RAGGED) {
                v0 = ragged_vec8(x, n0, p.n_samples);
                v1 = ragged_vec8(x, n1, p.n_samples);
            } else {
                v0 = n0 + 8 <= p.n_samples ? *reinterpret_cast<const uint4*>(x + n0) : make_uint4(0, 0, 0, 0);
                v1 = n1 + 8 <= p.n_samples ? *reinterpret_cast<const uint4*>(x + n1) : make_uint4(0, 0, 0, 0);
            }
            before = s0 > 0 ? x[s0 - 1] : (int16_t)0;
        }
    };
    __syncthreads();  // the only workgroup barrier: the shared tables are in place
    if (!active) return;

    const PairScratch sc = {reinterpret_cast<cf*>(scr + SCR_XBUF), reinterpret_cast<float2*>(scr + SCR_PBUF),
                            reinterpret_cast<float*>(scr + SCR_LBUF), dctb, tw2, nfp};
    const float pre = p.preemph;
    // The wavefront's flagged pairs go to the worklist together: two flag bits per pair collect in one scalar mask (pair k of the
    // wavefront at bits 2k, 2k+1; a register per entry would spill under the 128-register cap), and when the wavefront is done --
    // or 16 pairs are in -- lane k rebuilds pair k's entry from the mask, ONE 64-bit atomic reserves the slots (entries in the low
    // word: its old value is the first slot; flagged frames in the high word) and the lanes store side by side.  An atomic per
    // flagged pair queued up at the counter's L2 line when flags are dense (speech-like clips, 5 % of the frames: 0.194 -> 0.262 ms).
    uint32_t fmask = 0u;
    int pair0 = 2 * c;  // pair index (within the clip) of mask position 0
    // GeomRef: the row of the run's first frame, advanced by two rows per pair (wave-uniform: scalar registers)
    float* orow = G::REF ? out + ((size_t)clip * p.num_frames + WR_FRAMES * c) * REF_NUMCEP : nullptr;
#define KWS_FLUSH_FLAGS()                                                                                                          \
    if (fmask && (G::REF || rl.ctr)) {                                                                                              \
        const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); /* (recomputed: the loop's copy would have to be kept in scratch) */ \
        const uint32_t fk = lane < 16 ? (fmask >> (2 * lane)) & 3u : 0u;                                                            \
        const uint32_t has = (uint32_t)__ballot(fk != 0u);                                                                          \
        unsigned long long old = 0ull;                                                                                              \
        if (lane == 0)                                                                                                              \
            old = atomicAdd(reinterpret_cast<unsigned long long*>(rl.ctr),                                                          \
                            (unsigned long long)__builtin_popcount(has) | ((unsigned long long)__builtin_popcount(fmask) << 32));   \
        const int at = __builtin_amdgcn_readfirstlane((int)(unsigned)old) + __builtin_popcount(has & ((1u << (lane & 31)) - 1u));   \
        if (fk != 0u && at < rl.cap)                                                                                                \
            rl.list[at] = (int)((((RAGGED ? (unsigned)pair_base : (unsigned)(rl.clip0 + clip) * (unsigned)((p.num_frames + 1) / 2)) + (unsigned)(pair0 + lane)) << 2) | fk); \
    }
    for (; c < c_end; ++c) {
        if constexpr (!AUG && !F32) fetch(c, lane);
        // ---- registers -> float32, pre-emphasised, into this wavefront's span buffer -----------------------
        if constexpr (AUG) {
            const int s0 = c * chunk_step;
            float a0[8], a1[8];
            aug_vec8(ac, s0 + 8 * lane, p.n_samples, a0);
            aug_vec8(ac, s0 + 512 + 8 * lane, p.n_samples, a1);
            // the sample before a lane's vector is an AUGMENTED sample too: the neighbouring lane's last one (wave_shr:1), lane 63's
            // first vector for lane 0's second, the clip's sample s0 - 1 for lane 0's first
            const float w0 = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a0[7]), 0x138, 0xf, 0xf, false));
            const float w1 = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a1[7]), 0x138, 0xf, 0xf, false));
            const float last0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a0[7]), 63));
            const float before_a = s0 > 0 ? aug_sample(ac, s0 - 1, p.n_samples) : 0.f;
            auto emphasise = [&](const float (&a)[8], float prev, int n, float* dst) {
                float y[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    y[i] = __fsub_rn(a[i], __fmul_rn(pre, prev));
                    prev = a[i];
                }
                if (n == 0) y[0] = a[0];       // the clip's first sample is not pre-emphasised
                if (n + 8 > p.n_samples) {     // past the clip: psf pads the PRE-EMPHASISED signal with zeros
#pragma unroll
                    for (int i = 0; i < 8; ++i) y[i] = 0.f;
                }
                reinterpret_cast<float4*>(dst)[0] = make_float4(y[0], y[1], y[2], y[3]);
                reinterpret_cast<float4*>(dst)[1] = make_float4(y[4], y[5], y[6], y[7]);
            };
            emphasise(a0, lane == 0 ? before_a : w0, s0 + 8 * lane, ybuf + 8 * lane);
            emphasise(a1, lane == 0 ? last0 : w1, s0 + 512 + 8 * lane, ybuf + 512 + 8 * lane);
        } else if constexpr (F32) {
            const int s0 = c * chunk_step;
            // one half-span at a time (see T above).  The sample before a lane's vector: the neighbouring lane's last one
            // (wave_shr:1), lane 63's last of the first half for lane 0's second, the clip's sample s0 - 1 for lane 0's first
            float carry = s0 > 0 ? x[s0 - 1] : 0.f;  // wave-uniform
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int n = s0 + 512 * h + 8 * lane;
                float a[8], y[8];
                f32_vec8<RAGGED>(x, n, p.n_samples, a);
                const float w = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a[7]), 0x138, 0xf, 0xf, false));
                float prev = lane == 0 ? carry : w;
                if (h == 0) carry = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a[7]), 63));
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    y[i] = __fsub_rn(a[i], __fmul_rn(pre, prev));
                    prev = a[i];
                }
                if (n == 0) y[0] = a[0];  // the clip's first sample is not pre-emphasised
                if (n + 8 > p.n_samples) {  // past the end the PRE-EMPHASISED signal is zero, also inside a vector that straddles it
#pragma unroll
                    for (int i = 0; i < 8; ++i) y[i] = (RAGGED && n + i < p.n_samples) ? y[i] : 0.f;
                }
                float* dst = ybuf + 512 * h + 8 * lane;
                reinterpret_cast<float4*>(dst)[0] = make_float4(y[0], y[1], y[2], y[3]);
                reinterpret_cast<float4*>(dst)[1] = make_float4(y[4], y[5], y[6], y[7]);
                if (h == 0) asm volatile("" ::: "memory");  // the second half's loads stay behind the first half's stores
            }
        } else {
            const int s0 = c * chunk_step;
            // the sample before a lane's vector: the last half-word of the neighbouring lane's vector (wave_shr:1), of lane 63's
            // first vector for lane 0's second, of the clip for lane 0's first
            const uint32_t w0 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v0.w, 0x138, 0xf, 0xf, false);
            const uint32_t w1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v1.w, 0x138, 0xf, 0xf, false);
            const uint32_t last0 = (uint32_t)__builtin_amdgcn_readlane((int)v0.w, 63);
            float prev0 = lane == 0 ? to_unit(before) : to_unit((int16_t)(w0 >> 16));
            float prev1 = lane == 0 ? to_unit((int16_t)(last0 >> 16)) : to_unit((int16_t)(w1 >> 16));
            auto convert = [&](const uint4& raw, float prev, int n, float* dst) {
                const uint32_t wd[4] = {raw.x, raw.y, raw.z, raw.w};
                float y[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float cur = to_unit((int16_t)((wd[i >> 1] >> (16 * (i & 1))) & 0xffffu));
                    y[i] = __fsub_rn(cur, __fmul_rn(pre, prev));
                    prev = cur;
                }
#ifdef KWS_X_MFCC_NO_BOOKKEEPING  // timing build, wrong results (see mfcc_pair)
                if constexpr (!G::REF)
#endif
                {
                    if (n == 0) y[0] = to_unit((int16_t)(wd[0] & 0xffffu));  // the clip's first sample is not pre-emphasised
                    if constexpr (G::REF) {
                        // past the clip the vector itself is zeros (fetch), so samples 1..7 are 0 - 0.97 * 0 = +0 already: one select, not eight
                        if (n + 8 > p.n_samples) y[0] = 0.f;
                    } else if constexpr (RAGGED) {
                        // a recording ends at any sample: the pre-emphasised signal is zero from len[r] on, also inside the vector
                        // that straddles it (its first padded sample would otherwise be -preemph * x[len - 1])
                        if (n + 8 > p.n_samples) {
#pragma unroll
                            for (int i = 0; i < 8; ++i) y[i] = n + i < p.n_samples ? y[i] : 0.f;
                        }
                    } else if (n + 8 > p.n_samples) {  // past the clip: psf pads the PRE-EMPHASISED signal with zeros
#pragma unroll
                        for (int i = 0; i < 8; ++i) y[i] = 0.f;
                    }
                }
                reinterpret_cast<float4*>(dst)[0] = make_float4(y[0], y[1], y[2], y[3]);
                reinterpret_cast<float4*>(dst)[1] = make_float4(y[4], y[5], y[6], y[7]);
            };
            convert(v0, prev0, s0 + 8 * lane, ybuf + 8 * lane);
            convert(v1, prev1, s0 + 512 + 8 * lane, ybuf + 512 + 8 * lane);
        }
        wave_lds_order();
        if constexpr (G::REF) {
            const float* ya = ybuf;  // frame a of the pair; frame b lies REF_FRAME_STEP floats on: an immediate offset of its loads
#pragma unroll 1
            for (int pr = 0; pr < WR_PAIRS; ++pr, ya += 2 * REF_FRAME_STEP, orow += 2 * REF_NUMCEP) {
                const int fa = WR_FRAMES * c + 2 * pr;
                if (fa >= p.num_frames) break;  // wave-uniform
                const bool has_b = fa + 1 < p.num_frames;
                [[maybe_unused]] const float* yb = ya + REF_FRAME_STEP;
                cf v[8];
#ifdef KWS_X_MFCC_NO_BOOKKEEPING
#pragma unroll
                for (int n1 = 0; n1 < 7; ++n1) v[n1] = cf{ya[64 * n1 + lane], yb[64 * n1 + lane]};
                v[7] = cf{0.f, 0.f};
                const bool nza = true, nzb = true;
#else
                // sample i of frame a and of frame b, one hop on, as ONE ds_read2_b32: the complex value (a, b) arrives in its
                // register pair (the compiler pairs the loads along a frame instead and regroups with a move per value); the
                // offsets are in floats and end at 255, hence a base per two blocks
                static_assert(REF_FRAME_STEP == 160 && REF_FRAME_LEN > 384 && REF_FRAME_LEN <= 448, "the offsets below");
                {
                    const uint32_t a0 = lds_addr(ya + lane);
                    asm volatile(
                        "ds_read2_b32 %0, %7 offset1:160\n\t"
                        "ds_read2_b32 %1, %7 offset0:64 offset1:224\n\t"
                        "ds_read2_b32 %2, %8 offset1:160\n\t"
                        "ds_read2_b32 %3, %8 offset0:64 offset1:224\n\t"
                        "ds_read2_b32 %4, %9 offset1:160\n\t"
                        "ds_read2_b32 %5, %9 offset0:64 offset1:224\n\t"
                        "ds_read2_b32 %6, %10 offset1:160\n\t"
                        "s_waitcnt lgkmcnt(0)"
                        : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6])
                        : "v"(a0), "v"(a0 + 512u), "v"(a0 + 1024u), "v"(a0 + 1536u)
                        : "memory");
                }
                const bool in6 = lane < REF_FRAME_LEN - 384;  // block 6 holds the frame's last 16 samples, block 7 none
                v[6] = cf{in6 ? v[6].x : 0.f, in6 ? v[6].y : 0.f};
                v[7] = cf{0.f, 0.f};
                if (!has_b) {  // the clip's last pair only: frame b is past the clip (wave-uniform: a real branch)
                    asm volatile("" ::: "memory");
#pragma unroll
                    for (int n1 = 0; n1 < 7; ++n1) v[n1].y = 0.f;
                }
                const bool nza = true, nzb = true;  // mfcc_pair<GeomRef> reads them off the frame energies
#endif
                const uint32_t flags = mfcc_pair<G>(v, nza, nzb, has_b, p, sc, t1, ml, lane, orow, orow + REF_NUMCEP, nullptr, t.mel_seg);
                if constexpr (G::FLAGS) fmask |= flags << (2 * ((fa >> 1) - pair0));  // wave-uniform
                wave_lds_order();
            }
        } else {
#pragma unroll 1
            for (int pr = 0; pr < WR_PAIRS; ++pr) {
                const int fa = WR_FRAMES * c + 2 * pr;
                if (fa >= p.num_frames) break;  // wave-uniform
                const bool has_b = fa + 1 < p.num_frames;
                const float* ya = ybuf + (2 * pr) * p.frame_step;
                const float* yb = ya + p.frame_step;
                cf v[8];
                uint32_t ora = 0u, orb = 0u;
#pragma unroll
                for (int n1 = 0; n1 < 7; ++n1) {  // frame_len in (384, 448]: block 6 is cut by a lane bound, block 7 is zero
                    const int i = 64 * n1 + lane;
                    float a = ya[i], b = yb[i];
                    if (n1 == 6) {
                        const bool in = i < p.frame_len;
                        a = in ? a : 0.f, b = in ? b : 0.f;
                    }
                    v[n1] = cf{a, b};
                    ora |= __builtin_bit_cast(uint32_t, a);
                    orb |= __builtin_bit_cast(uint32_t, b);
                }
                v[7] = cf{0.f, 0.f};
                if (!has_b) {  // the clip's last pair only: frame b is past the clip
#pragma unroll
                    for (int n1 = 0; n1 < 7; ++n1) v[n1].y = 0.f;
                    orb = 0u;
                }
                const bool nza = __any((ora << 1) != 0u);
                const bool nzb = __any((orb << 1) != 0u);
                const uint32_t flags = mfcc_pair(v, nza, nzb, has_b, p, sc, t1, ml, lane,
                                                 out + ((size_t)clip * p.num_frames + fa) * p.numcep,
                                                 out + ((size_t)clip * p.num_frames + fa + 1) * p.numcep);
                fmask |= flags << (2 * ((fa >> 1) - pair0));  // wave-uniform
                wave_lds_order();
            }
        }
        if constexpr (G::FLAGS)
            if (2 * (c + 1) - pair0 >= 16) {  // the mask is full (more than 8 chunks per wavefront: tuning runs only)
                KWS_FLUSH_FLAGS()
                fmask = 0u;
                pair0 = 2 * (c + 1);
            }
    }
    if constexpr (G::FLAGS) KWS_FLUSH_FLAGS()
#undef KWS_FLUSH_FLAGS
    if constexpr (RAGGED) {
        // the wavefront that owns the recording's last chunk writes the zero rows that round its row count up
        if (c_end == n_chunks) {
            const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            float* pad = out + (size_t)p.num_frames * numcep;
            for (int i = lane; i < pad_floats; i += 64) pad[i] = 0.f;
        }
    }
}

__global__ __launch_bounds__(MFCC_THREADS) __attribute__((amdgpu_waves_per_eu(KWS_MFCC_EU, KWS_MFCC_EU))) void kws_mfcc_i16_kernel(
    FrontendParams p, FrontendTables t, const int16_t* __restrict__ wav, float* __restrict__ out, RefineList rl, int B, int chunks_per_wave) {
    mfcc_wr_body<false>(p, t, wav, out, rl, B, chunks_per_wave, AugmentArgs{});
}
// The same kernel at the reference geometry (GeomRef), which every shipped configuration uses: with the precision flag and the
// worklist, and without both for a context whose refinement is off.  Kernels of their own: both bodies in one kernel spill.
__global__ __launch_bounds__(MFCC_THREADS) __attribute__((amdgpu_waves_per_eu(KWS_MFCC_EU, KWS_MFCC_EU))) void kws_mfcc_i16_ref_kernel(
    FrontendParams p, FrontendTables t, const int16_t* __restrict__ wav, float* __restrict__ out, RefineList rl, int B, int chunks_per_wave) {
    mfcc_wr_body<false, GeomRef<true>>(p, t, wav, out, rl, B, chunks_per_wave, AugmentArgs{});
}
__global__ __launch_bounds__(MFCC_THREADS) __attribute__((amdgpu_waves_per_eu(KWS_MFCC_EU, KWS_MFCC_EU))) void kws_mfcc_i16_ref_noflag_kernel(
    FrontendParams p, FrontendTables t, const int16_t* __restrict__ wav, float* __restrict__ out, RefineList rl, int B, int chunks_per_wave) {
    mfcc_wr_body<false, GeomRef<false>>(p, t, wav, out, rl, B, chunks_per_wave, AugmentArgs{});
}
// The generic kernel over the recordings of a ragged batch (kws_frames_ragged_i16); B: the launch's wavefronts.
__global__ __launch_bounds__(MFCC_THREADS) __attribute__((amdgpu_waves_per_eu(KWS_MFCC_EU, KWS_MFCC_EU))) void kws_mfcc_i16_ragged_kernel(
    FrontendParams p, FrontendTables t, const int16_t* __restrict__ pcm, float* __restrict__ out, RefineList rl, RaggedArgs rg, int n_waves) {
    mfcc_wr_body<false, GeomAny, true>(p, t, pcm, out, rl, n_waves, 0, AugmentArgs{}, rg);
}
// float32 samples (kws_frames_f32, kws_scan_f32 and their ragged twins): the generic kernel and its ragged form, no GeomRef.
__global__ __launch_bounds__(MFCC_THREADS) __attribute__((amdgpu_waves_per_eu(KWS_MFCC_EU, KWS_MFCC_EU))) void kws_mfcc_f32_wr_kernel(
    FrontendParams p, FrontendTables t, const float* __restrict__ wav, float* __restrict__ out, RefineList rl, int B, int chunks_per_wave) {
    mfcc_wr_body<false, GeomAny, false, float>(p, t, wav, out, rl, B, chunks_per_wave, AugmentArgs{});
}
__global__ __launch_bounds__(MFCC_THREADS) __attribute__((amdgpu_waves_per_eu(KWS_MFCC_EU, KWS_MFCC_EU))) void kws_mfcc_f32_ragged_kernel(
    FrontendParams p, FrontendTables t, const float* __restrict__ wav, float* __restrict__ out, RefineList rl, RaggedArgs rg, int n_waves) {
    mfcc_wr_body<false, GeomAny, true, float>(p, t, wav, out, rl, n_waves, 0, AugmentArgs{}, rg);
}
#ifndef KWS_MFCC_AUG_EU
#define KWS_MFCC_AUG_EU 4
#endif
__global__ __launch_bounds__(MFCC_THREADS) __attribute__((amdgpu_waves_per_eu(KWS_MFCC_AUG_EU, KWS_MFCC_AUG_EU))) void kws_mfcc_augment_i16_kernel(
    FrontendParams p, FrontendTables t, AugmentArgs aug, float* __restrict__ out, RefineList rl, int B, int chunks_per_wave) {
    mfcc_wr_body<true>(p, t, static_cast<const int16_t*>(nullptr), out, rl, B, chunks_per_wave, aug);
}

// ------------------------------------------------------------------------------------------------
// sigproc operator (kws/libs/speech_features/sigproc.py), float32 device version; the others are in kws_sigproc.hip.
// magspec / powspec with NFFT = 512: one wavefront per pair of frames.
__global__ __launch_bounds__(64) void kws_spec512_f32_kernel(FrontendTables t, const float* __restrict__ frames,
                                                             int num_frames, int frame_len, int power,
                                                             float* __restrict__ spec) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[SCR_BYTES + 512];  // scratch + tw2
    cf* xbuf = reinterpret_cast<cf*>(smem + SCR_XBUF);
    float2* pbuf = reinterpret_cast<float2*>(smem + SCR_PBUF);
    cf* tw2 = reinterpret_cast<cf*>(smem + SCR_BYTES);
    const int lane = threadIdx.x;
    const int fa = 2 * blockIdx.x;
    const bool has_b = fa + 1 < num_frames;
    cf t1[8];
    load_twiddles(t.twiddle, lane, t1);
    fill_tw2(t.twiddle, tw2, lane);
    wave_lds_order();
    const float* ya = frames + (size_t)fa * frame_len;
    const float* yb = ya + frame_len;
    cf v[8];
    bool nza = false, nzb = false;
#pragma unroll
    for (int n1 = 0; n1 < 8; ++n1) {
        const int i = 64 * n1 + lane;
        const bool in = i < frame_len;  // frames longer than NFFT are truncated (sigproc.py:65-66)
        v[n1].x = in ? ya[i] : 0.f;
        v[n1].y = (in && has_b) ? yb[i] : 0.f;
        nza |= v[n1].x != 0.f;
        nzb |= v[n1].y != 0.f;
    }
    nza = __any(nza);
    nzb = __any(nzb);
    const PairLevel lv = equalise_levels(v);
    fft512(v, xbuf, t1, tw2, lane);
    float ea, eb;
    const int ident[4] = {lane, lane + 64, lane + 128, lane + 192};
    split_power(v, xbuf, pbuf, lane, power, nza, nzb, ident, 256, lv, ea, eb);
    for (int k = lane; k < NBINS; k += 64) {
        const float2 pw = pbuf[k];
        spec[(size_t)fa * NBINS + k] = pw.x;
        if (has_b) spec[(size_t)(fa + 1) * NBINS + k] = pw.y;
    }
}

// ------------------------------------------------------------------------------------------------
// Streaming front end as a kernel of its own (pushes that ask for features only, and models other than the fused
// DS-CNN): one wavefront per pair of streams, see stream_frame_wave.
__global__ __launch_bounds__(64) void kws_stream_frame_kernel(FrontendParams p, FrontendTables t,
                                                              const int16_t* __restrict__ hop, int n_streams,
                                                              int16_t* __restrict__ pcm_ring, int ring_len,
                                                              float* __restrict__ feat_ring,
                                                              int* __restrict__ hops_ptr, int* refine_ctr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const int sa = 2 * blockIdx.x, sb = sa + 1;
    const int hops = *hops_ptr;
    stream_frame_wave(p, t, hop, sa, sb, sb < n_streams, pcm_ring, ring_len, feat_ring, hops, smem, lane, nullptr, refine_ctr);
    // hop counter: every workgroup read hops_ptr[0] at its start (its value fed every address above, so that load is
    // long complete); the workgroup that finishes last advances it (hops_ptr[1] counts finished workgroups).  No fence:
    // the counter orders nothing inside this launch, and the kernel boundary publishes it to the next one.
    if (lane == 0) {
        if (atomicAdd(&hops_ptr[1], 1) == (int)gridDim.x - 1) {
            hops_ptr[1] = 0;
            hops_ptr[0] = hops + 1;
        }
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// dynamic LDS of a tile-kernel workgroup: tables, the staged span of its 24 frames, the wavefronts' scratch
size_t mfcc_tile_lds_bytes(const FrontendParams& p) {
    const int nfp = (p.nfilt + 3) & ~3;
    return sizeof(float) * (size_t)(((p.numcep * nfp + 3) & ~3) + 2 * 64 + ((p.chunk_samples + 7) & ~7)) +
           (size_t)MFCC_WAVES * SCR_BYTES;
}

template <typename T, typename K>
static hipError_t launch_mfcc_t(K kernel, hipStream_t s, const FrontendParams& p, const FrontendTables& t, const T* d_wav,
                                int B, float* d_out, RefineList rl) {
    dim3 grid((p.num_frames + MFCC_FRAMES_PER_WG - 1) / MFCC_FRAMES_PER_WG, B);
    const size_t lds = mfcc_tile_lds_bytes(p);
    hipError_t e = raise_lds_limit(kernel, lds);  // geometries (or experiment shapes) beyond the default dynamic-LDS limit opt in per kernel
    if (e != hipSuccess) return e;
    // grid.y is limited to 65535: split very large batches
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const int nb = (B - b0 < 65535) ? (B - b0) : 65535;
        grid.y = nb;
        rl.clip0 = b0;
        hipLaunchKernelGGL(kernel, grid, dim3(MFCC_THREADS), lds, s, p, t, d_wav + (size_t)b0 * p.n_samples,
                           d_out + (size_t)b0 * p.num_frames * p.numcep, rl);
    }
    return hipGetLastError();
}

// frame lengths of the TAIL6 kernels (see mfcc_body)
static bool mfcc_tail6(const FrontendParams& p) { return p.frame_len > 384 && p.frame_len <= 448; }

// the wavefront-resident kernel: 16-byte PCM vectors (aligned clips and chunk starts), a chunk's span within two vectors per lane
bool mfcc_wave_resident_ok(const FrontendParams& p) {
    return mfcc_tail6(p) && p.vec_ok && (WR_FRAMES * p.frame_step) % 8 == 0 && (WR_FRAMES - 1) * p.frame_step + 448 <= WR_SPAN;
}

// the geometry kws_mfcc_i16_ref_kernel is compiled for (GeomRef, kws_mfcc_dev.h); kws_set_frontend asks once per configuration
bool mfcc_reference_geometry(const FrontendParams& p) {
    return p.frame_len == REF_FRAME_LEN && p.frame_step == REF_FRAME_STEP && p.nfilt == REF_NFILT && p.numcep == REF_NUMCEP &&
           p.append_energy != 0;
}

// Chunks per wavefront of the wavefront-resident kernels for a launch of total_chunks chunks (nb clips of n_chunks each, or the
// recordings of a ragged batch together) and a clip of n_chunks.
// ~5 chunks (20 frames) per wavefront, split evenly (99 frames = 25 chunks = 5 x 5): measured on 4096 clips, 1 / 5 / 25
// chunks per wavefront take 0.219 / 0.183 / 0.201 ms -- short-lived wavefronts keep the CUs' phases mixed and the tail
// short, an uneven split (6 + 6 + 6 + 6 + 1: 0.209 ms) wastes a wavefront's set-up on one chunk.  Small batches spread
// a clip over more wavefronts, down to one chunk each, so that even one clip uses 25 wavefronts.
int mfcc_wr_chunks_per_wave(long total_chunks, int n_chunks) {
    int wpc = (n_chunks + 2) / 5;
    wpc = wpc < 1 ? 1 : wpc;
    int cpw = (n_chunks + wpc - 1) / wpc;
    const int fill = (int)((total_chunks + 4095) / 4096);  // chunks per wavefront that still fill 256 CUs x 16 wavefronts
    cpw = cpw > fill ? (fill < 1 ? 1 : fill) : cpw;
    static const int cpw_env = [] {  // experiment hook, read once (profiles/r03_mfcc_ab.txt: the chunks-per-wavefront scan)
        const char* e = getenv("KWS_X_MFCC_CPW");
        return e ? atoi(e) : 0;
    }();
    if (cpw_env > 0) cpw = cpw_env > 16 ? 16 : cpw_env;
    return cpw;
}

// A launch's source from its first clip b0 on: the PCM pointer moves by whole clips, the fused loader's per-clip arrays by b0.
static const int16_t* clips_from(const int16_t* d_wav, int b0, const FrontendParams& p) { return d_wav + (size_t)b0 * p.n_samples; }
static const float* clips_from(const float* d_wav, int b0, const FrontendParams& p) { return d_wav + (size_t)b0 * p.n_samples; }
static AugmentArgs clips_from(AugmentArgs a, int b0, const FrontendParams&) {
    a.index += b0;
    if (a.shift) a.shift += b0;
    if (a.bg_off) a.bg_off += b0;
    if (a.bg_vol) a.bg_vol += b0;
    if (a.silence) a.silence += b0;
    return a;
}

// The launches of a wavefront-resident kernel (kws_mfcc_i16_kernel, or the fused loader kernel: the same launch shape).
template <typename K, typename Src>
static hipError_t launch_mfcc_wr(K kernel, hipStream_t s, const FrontendParams& p, const FrontendTables& t, const Src& src, int B,
                                 float* d_out, RefineList rl) {
    const size_t lds = mfcc_wr_lds_bytes(p);
    const int n_chunks = (p.num_frames + WR_FRAMES - 1) / WR_FRAMES;
    for (int b0 = 0; b0 < B; b0 += (1 << 20)) {  // (grid.x limit: 2^31 workgroups; a million clips per launch keeps indices in 32 bits)
        const int nb = B - b0 < (1 << 20) ? B - b0 : (1 << 20);
        const int cpw = mfcc_wr_chunks_per_wave((long)nb * n_chunks, n_chunks);
        const int waves_per_clip = (n_chunks + cpw - 1) / cpw;
        const long waves = (long)nb * waves_per_clip;
        rl.clip0 = b0;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((waves + MFCC_WAVES - 1) / MFCC_WAVES)), dim3(MFCC_THREADS), lds, s, p, t,
                           clips_from(src, b0, p), d_out + (size_t)b0 * p.num_frames * p.numcep, rl, nb, cpw);
    }
    return hipGetLastError();
}

hipError_t launch_mfcc(hipStream_t s, const FrontendParams& p, const FrontendTables& t, const int16_t* d_wav, int B, float* d_out,
                       const RefineList& rl, bool ref_route) {
#ifndef KWS_X_MFCC_TILE_KERNEL  // (A/B switch: the round-2 tile kernel for every geometry)
    if (mfcc_wave_resident_ok(p)) {
        if (ref_route && mfcc_reference_geometry(p))  // (the caller's p may be a copy with another clip length: asked again, five compares)
            return launch_mfcc_wr(rl.ctr && p.refine_span > 0.f ? kws_mfcc_i16_ref_kernel : kws_mfcc_i16_ref_noflag_kernel, s, p, t,
                                  d_wav, B, d_out, rl);
        return launch_mfcc_wr(kws_mfcc_i16_kernel, s, p, t, d_wav, B, d_out, rl);
    }
#endif
    return launch_mfcc_t(mfcc_tail6(p) ? kws_mfcc_i16_tile_kernel : kws_mfcc_i16_any_kernel, s, p, t, d_wav, B, d_out, rl);
}
hipError_t launch_mfcc_ragged(hipStream_t s, const FrontendParams& p, const FrontendTables& t, const int16_t* d_pcm, const RaggedArgs& rg,
                              int n_waves, float* d_out, const RefineList& rl) {
    if (!mfcc_wave_resident_ok(p)) return hipErrorInvalidValue;  // refused by kws_frames_ragged_i16 before it gets here
    hipLaunchKernelGGL(kws_mfcc_i16_ragged_kernel, dim3((unsigned)((n_waves + MFCC_WAVES - 1) / MFCC_WAVES)), dim3(MFCC_THREADS),
                       mfcc_wr_lds_bytes(p), s, p, t, d_pcm, d_out, rl, rg, n_waves);
    return hipGetLastError();
}
hipError_t launch_mfcc_ragged(hipStream_t s, const FrontendParams& p, const FrontendTables& t, const float* d_wav, const RaggedArgs& rg,
                              int n_waves, float* d_out, const RefineList& rl) {
    if (!mfcc_wave_resident_ok(p)) return hipErrorInvalidValue;  // refused by kws_frames_ragged_f32 before it gets here
    hipLaunchKernelGGL(kws_mfcc_f32_ragged_kernel, dim3((unsigned)((n_waves + MFCC_WAVES - 1) / MFCC_WAVES)), dim3(MFCC_THREADS),
                       mfcc_wr_lds_bytes(p), s, p, t, d_wav, d_out, rl, rg, n_waves);
    return hipGetLastError();
}
// wr_route: the recording entries (kws_frames_f32, kws_scan_f32) ask for the wavefront-resident kernel where the recording's length
// and pointer allow it; kws_mfcc_f32 / kws_infer_f32 do not ask and stay on the tile kernels.
hipError_t launch_mfcc(hipStream_t s, const FrontendParams& p, const FrontendTables& t, const float* d_wav, int B, float* d_out,
                       const RefineList& rl, bool wr_route) {
#ifndef KWS_X_MFCC_TILE_KERNEL
    if (wr_route && mfcc_wave_resident_ok(p)) return launch_mfcc_wr(kws_mfcc_f32_wr_kernel, s, p, t, d_wav, B, d_out, rl);
#endif
    return launch_mfcc_t(mfcc_tail6(p) ? kws_mfcc_f32_kernel : kws_mfcc_f32_any_kernel, s, p, t, d_wav, B, d_out, rl);
}
hipError_t launch_mfcc(hipStream_t s, const FrontendParams& p, const FrontendTables& t, const AugmentArgs& a, int B, float* d_out,
                       const RefineList& rl, bool) {
    if (!mfcc_wave_resident_ok(p)) return hipErrorInvalidValue;  // refused by kws_mfcc_augment_i16 before it gets here
    return launch_mfcc_wr(kws_mfcc_augment_i16_kernel, s, p, t, a, B, d_out, rl);
}

hipError_t launch_stream_frame(hipStream_t s, const FrontendParams& p, const FrontendTables& t, const int16_t* d_hop,
                               int n_streams, int16_t* d_pcm_ring, int ring_len, float* d_feat_ring, int* d_hops, int* d_refine_ctr) {
    const size_t lds = stream_frame_lds_bytes(p);
    hipLaunchKernelGGL(kws_stream_frame_kernel, dim3((n_streams + 1) / 2), dim3(64), lds, s, p, t, d_hop, n_streams,
                       d_pcm_ring, ring_len, d_feat_ring, d_hops, d_refine_ctr);
    return hipGetLastError();
}

hipError_t launch_spec512(hipStream_t s, const FrontendTables& t, const float* d_frames, int num_frames, int frame_len,
                          int power, float* d_spec) {
    hipLaunchKernelGGL(kws_spec512_f32_kernel, dim3((num_frames + 1) / 2), dim3(64), 0, s, t, d_frames, num_frames,
                       frame_len, power, d_spec);
    return hipGetLastError();
}

}  // namespace kws
