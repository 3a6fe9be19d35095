// Internal declarations shared by the translation units of the C ABI (kws_ctx.h lists them) and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "kws_hip.h"

namespace kws {

// ------------------------------------------------------------------------------------------------
// Front end (MFCC) -- a workgroup of MFCC_WAVES wavefronts handles MFCC_FRAMES_PER_WG frames; each wavefront
// transforms frame pairs (2 real frames are packed into one 512-point complex FFT).
constexpr int NFFT = 512;
constexpr int NBINS = NFFT / 2 + 1;       // 257
constexpr int MEL_CHUNK = 8;              // bins per lane in the sparse mel stage
constexpr int MEL_STRIDE = 10;            // power-buffer slots (float2) from one lane's chunk to the next: 80 bytes, so the sixteen
                                          // lanes of a ds_read_b128 group start on sixteen different 16-byte bank groups (with 64
                                          // bytes every fourth lane collided: 48 of the mel stage's LDS cycles per frame pair)
#ifndef KWS_MFCC_WAVES
#define KWS_MFCC_WAVES 4
#endif
#ifndef KWS_MFCC_PAIRS_PER_WAVE
#define KWS_MFCC_PAIRS_PER_WAVE 3
#endif
constexpr int MFCC_WAVES = KWS_MFCC_WAVES;             // wavefronts per workgroup
constexpr int MFCC_THREADS = MFCC_WAVES * 64;
constexpr int MFCC_FRAMES_PER_WG = 2 * KWS_MFCC_PAIRS_PER_WAVE * MFCC_WAVES;
constexpr int MAX_NFILT = 64;
constexpr int MAX_NUMCEP = 32;

struct FrontendParams {
    int n_samples;
    int frame_len;
    int frame_step;
    int num_frames;
    int nfilt;
    int numcep;
    int append_energy;
    float preemph;
    int chunk_samples;     // samples staged per workgroup = (MFCC_FRAMES_PER_WG-1)*frame_step + frame_len
    int vec_ok;            // 1 -> every workgroup's first sample is 16-byte aligned (vector PCM loads legal)
    int nfft;              // transform length (the float32 kernel is built for 512; the float64 kernel takes any)
    int log2_nfft;         // log2(nfft) when nfft is a power of two, else 0 (float64 kernel: FFT vs direct DFT)
    float refine_span;     // float32 kernels: a frame whose weakest mel band lies more than this (log power) below its largest bin is redone in float64 (0: never)
};
// Hops a frame spans, ceil(frame_len / frame_step) (3 for 400 / 160): after h pushes the newest complete frame is h - frames_lag.
__host__ __device__ inline int frames_lag(int frame_len, int frame_step) { return (frame_len + frame_step - 1) / frame_step; }
__host__ __device__ inline int frames_lag(const FrontendParams& p) { return frames_lag(p.frame_len, p.frame_step); }

// Worklist of the selective float64 refinement: the float32 MFCC kernel appends, per frame pair with a
// flagged frame, (global pair index << 2 | mask of flagged frames), global pair index = clip * ceil(num_frames / 2) +
// frame / 2; the refinement kernel consumes the list and clears the counters.
// ctr: int[8], 8-byte aligned = {entries listed by the running call, frames flagged by it (the two are bumped by ONE 64-bit
// atomic), rows rewritten in total (low, high 32 bits), rows rewritten by the last completed call, frames redone in float64
// by streaming pushes, finished refinement workgroups, 0}.
struct RefineList {
    int* ctr;
    int* list;
    int cap;       // entries list can hold (frame pairs of the largest batch reserved); 0 with ctr == nullptr: flagging off
    int clip0;     // index of the launch's first clip inside the call's batch (batches beyond 65535 clips are split)
};

// Device tables of the front end (all float32 unless noted), built on the host in double.
struct FrontendTables {
    const float2* twiddle;     // [512]      (cos, -sin)(2*pi*k/512)
    const int* mel_k0;         // [64]       first bin of lane's chunk (or NBINS-1 for idle lanes)
    const float* mel_rw;       // [8][64]    rising-edge weights of the chunk's bins (0 beyond its length)
    const float* mel_fw;       // [8][64]    falling-edge weights
    const uint32_t* mel_gather;// [64]       per filter: r0 | nr<<8 | f0<<16 | nf<<24  (chunk ranges)
    const int* mel_slot;       // [256]      power-buffer slot of bin k = MEL_STRIDE*chunk(k) + (k - first bin of the chunk)
    const int* mel_seg;        // [64]       per chunk: bit d (0..2) = chunk + 2^d is in the same segment; bit 6 = no segment straddles a 16-lane row; bit 7 = deep
    const float* dct;          // [numcep][nfilt]  DCT-II ortho x lifter
    const float* dct_pad;      // [numcep][nfp]    the same, rows zero-padded to nfp = (nfilt+3)&~3 floats (the LDS image, copied as float4)
    // float64 kernel (kws_mfcc_f64.hip)
    const double* tw64;        // [nfft][2]  (cos, -sin)(2*pi*k/nfft)
    const int* mel_edges;      // [nfilt+2]  psf's bin edges
    const double* mel_w64;     // [2][nfft/2+1]  per bin: its weight on the rising edge of its filter / on the falling edge of the one below
    const double* dct64;       // [numcep][nfilt]  DCT-II ortho x lifter
};

// Opt a kernel in to more than the default 64 KiB of dynamic LDS.
template <typename K>
inline hipError_t raise_lds_limit(K kernel, size_t lds) {
    if (lds <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

struct AugmentArgs;
// The float32 MFCC of B clips read from int16 PCM, float32 samples, or the augmented view of a resident split (gather +
// augment + MFCC in one launch, wavefront-resident geometry only).  Frames over p.refine_span are appended to rl; an empty rl
// (ctr == nullptr) means no flagging.  ref_route: int16 PCM at the reference geometry takes the kernel compiled for it
// (kws_mfcc_i16_ref_kernel: the same bits); the augmented source has one route and ignores it.  wr_route: float32 samples take
// the wavefront-resident kernel where mfcc_wave_resident_ok holds (the recording entries ask; kws_mfcc_f32 / kws_infer_f32 do
// not and stay on the tile kernels: the same bits either way).
hipError_t launch_mfcc(hipStream_t s, const FrontendParams& p, const FrontendTables& t, const int16_t* d_wav, int B, float* d_out,
                       const RefineList& rl, bool ref_route);
hipError_t launch_mfcc(hipStream_t s, const FrontendParams& p, const FrontendTables& t, const float* d_wav, int B, float* d_out,
                       const RefineList& rl, bool wr_route);
hipError_t launch_mfcc(hipStream_t s, const FrontendParams& p, const FrontendTables& t, const AugmentArgs& a, int B, float* d_out,
                       const RefineList& rl, bool ref_route);
// Float64 recomputation of the listed frames, in place in d_out (same source / d_out as the float32 launch before it).
hipError_t launch_mfcc_refine(hipStream_t s, const FrontendParams& p, const FrontendTables& t, const int16_t* d_wav, float* d_out,
                              const RefineList& rl, int B);
hipError_t launch_mfcc_refine(hipStream_t s, const FrontendParams& p, const FrontendTables& t, const float* d_wav, float* d_out,
                              const RefineList& rl, int B);
hipError_t launch_mfcc_refine(hipStream_t s, const FrontendParams& p, const FrontendTables& t, const AugmentArgs& a, float* d_out,
                              const RefineList& rl, int B);
// Ragged batches (kws_frames_ragged_i16; the entries are in kws_ragged.hip): one record per recording and a closing record R
// that holds the totals, derived on the host and uploaded into context scratch.  Recording r is samples [start, start + len) of
// the one PCM buffer, rows [frame_off, frame_off + frames) of the packed frame array and frame pairs [pair_off, ...) of the
// refinement worklist's numbering; wavefronts [wave_off, next record's wave_off) of the front-end launch walk its chunks, cpw each.
struct RaggedRec {
    long long start;
    int len, frames;
    int frame_off;     // record R: F_pack (the rows between a recording's last frame and the next record's first are written as zeros)
    int pair_off;      // record R: the number of pairs
    int wave_off;      // record R: the number of wavefronts
    int cpw;
};
struct RaggedArgs {
    const RaggedRec* rec;  // [R + 1]
    int R;
};
// The float32 wavefront-resident kernel (generic geometry) over the recordings of rg, and the float64 redo of the frames it listed.
hipError_t launch_mfcc_ragged(hipStream_t s, const FrontendParams& p, const FrontendTables& t, const int16_t* d_pcm, const RaggedArgs& rg,
                              int n_waves, float* d_out, const RefineList& rl);
hipError_t launch_mfcc_refine_ragged(hipStream_t s, const FrontendParams& p, const FrontendTables& t, const int16_t* d_pcm,
                                     const RaggedArgs& rg, float* d_out, const RefineList& rl, int B);
// The same pair over float32 samples (kws_frames_ragged_f32): start % 8 == 0 and a 16-byte aligned buffer, as for int16.
hipError_t launch_mfcc_ragged(hipStream_t s, const FrontendParams& p, const FrontendTables& t, const float* d_wav, const RaggedArgs& rg,
                              int n_waves, float* d_out, const RefineList& rl);
hipError_t launch_mfcc_refine_ragged(hipStream_t s, const FrontendParams& p, const FrontendTables& t, const float* d_wav,
                                     const RaggedArgs& rg, float* d_out, const RefineList& rl, int B);
// Chunks per wavefront of a wavefront-resident launch of total_chunks chunks in all, for a clip of n_chunks of them (host).
int mfcc_wr_chunks_per_wave(long total_chunks, int n_chunks);
constexpr int MFCC_WR_FRAMES = 4;  // frames per chunk of the wavefront-resident kernels
// The float64 front end: any nfft (power of two up to 4096: FFT; otherwise up to 2048: direct DFT), any frame length.
hipError_t launch_mfcc_f64(hipStream_t s, const FrontendParams& p, const FrontendTables& t, const int16_t* d_wav, int B, float* d_out);
hipError_t launch_mfcc_f64(hipStream_t s, const FrontendParams& p, const FrontendTables& t, const float* d_wav, int B, float* d_out);
hipError_t launch_spec_f64(hipStream_t s, const double* d_tw64, const float* d_frames, int num_frames, int frame_len, int nfft,
                           int log2n, int power, float* d_spec);
// Streaming: one hop of frame_step new samples per stream -> one new MFCC frame per stream in the feature ring.
// d_hops: int[2] = {hops pushed so far, finished-workgroup counter}; the kernel advances the hop count itself.
hipError_t launch_stream_frame(hipStream_t s, const FrontendParams& p, const FrontendTables& t, const int16_t* d_hop,
                               int n_streams, int16_t* d_pcm_ring, int ring_len, float* d_feat_ring, int* d_hops, int* d_refine_ctr);
// Training-time augmentation on the device (time shift, silence, background mix).
hipError_t launch_augment(hipStream_t s, const int16_t* d_wav, int B, int n, const int32_t* d_shift, const float* d_bg,
                          int bg_len, const int32_t* d_bg_off, const float* d_bg_vol, const uint8_t* d_silence,
                          float* d_out);
// The resident training loader (kws_augment_draw, kws_mfcc_augment_i16): batch row b is clip index[b] of the split,
// augmented with the b-th draws -- the arguments of launch_augment, gathered.
struct AugmentArgs {
    const int16_t* pcm;       // [n_rows][n_samples]  the resident split
    const int32_t* index;     // [B]  dataset indices
    int n_rows;
    const int32_t* shift;     // [B] or nullptr
    const float* bg;          // [bg_len] background pool or nullptr
    int bg_len;
    const int32_t* bg_off;    // [B]
    const float* bg_vol;      // [B]
    const uint8_t* silence;   // [B] or nullptr
};
struct DrawArgs {
    unsigned long long seed;
    unsigned epoch;
    const int32_t* index;     // [B]
    const int32_t* label;     // [n_rows] or nullptr
    int n_rows, time_shift;
    const int32_t* bg_start;  // [n_files]
    const int32_t* bg_len;    // [n_files]
    int n_files;
    float bg_volume, bg_frequency;
    int use_background, n_samples;
    int32_t* shift;           // [B]
    int32_t* bg_off;          // [B]
    float* bg_vol;            // [B]
    uint8_t* silence;         // [B]
};
hipError_t launch_augment_draw(hipStream_t s, const DrawArgs& d, int B);
// true: launch_mfcc picks the wavefront-resident kernel for int16 PCM at this geometry (the fused kernel is a variant of it)
bool mfcc_wave_resident_ok(const FrontendParams& p);
// true: frame length, hop, filters, cepstra and energy row are the reference's, the constants kws_mfcc_i16_ref_kernel is built for
bool mfcc_reference_geometry(const FrontendParams& p);
// dynamic LDS a tile kernel asks for at this geometry (23 hops + one frame of float32 samples): beyond MFCC_TILE_LDS_MAX the
// float32 kernels cannot be launched and kws_set_frontend routes the geometry to the float64 kernel
size_t mfcc_tile_lds_bytes(const FrontendParams& p);
constexpr size_t MFCC_TILE_LDS_MAX = 160 * 1024;  // the CU's LDS on gfx950
hipError_t launch_preemphasis(hipStream_t s, const float* d_in, int n, float coeff, float* d_out);
hipError_t launch_framesig(hipStream_t s, const float* d_in, int n, int frame_len, int frame_step,
                           int num_frames, const float* d_window, float* d_frames);
hipError_t launch_spec512(hipStream_t s, const FrontendTables& t, const float* d_frames, int num_frames,
                          int frame_len, int power, float* d_spec);

// ------------------------------------------------------------------------------------------------
// DS-CNN (kws/libs/models.py:122-183) for the [1,99,10] feature map.
constexpr int CH = 64;
constexpr int IN_T = 99, IN_F = 10;
constexpr int C1_K = 10, C1_H = 47, C1_W = 3;             // conv1 output 64 x 47 x 3
constexpr int N_BLOCKS = 4;
constexpr int MAX_CLASSES = 64;

// Device weights, repacked by the host for the kernel's access patterns.
struct DscnnWeights {
    const float* c1_w;     // [100][64]   conv1 weight transposed: [kh*10+kw][cout]
    const float* c1_b;     // [64]
    const float* dw_w;     // [4][32][24] depthwise 3x3, channel pairs interleaved: (tap t of channel 2p, of 2p + 1) at 2t, t = 0..8; the biases at 18, 19; 4 pad
    const float* pw_w;     // [4][64][64] pointwise transposed: [cin][cout]
    const float* pw_b;     // [4][64]
    const uint32_t* pw_split;  // [4][ct 2][m 4][piece 3][lane 64][4]  pointwise weights as bf16 hi/mid/lo MFMA A operands
    const uint32_t* c1_split;  // [ct 2][kb 7][piece 3][lane 64][4]    conv1 weights, same format (K order: see kws_dscnn_stages.h)
    const float* fc_w;     // [C][64]
    const float* fc_b;     // [C]
    int num_classes;
    int in_channels;           // 1: the fused kernel computes conv1 itself; > 1: kws_conv1_general_kernel + the PRECONV entry
    const float* c1_general;   // [ci][100][64]  conv1 weights as [ci][tap][cout] (multi-channel models and the composed any-map path)
    const float* raw;          // the state_dict blob as loaded (torch layouts): the composed path's depthwise / pointwise operands
    // f16-pair arithmetic (KWS_PW_PAIR_F16, kws_dscnn.hip): every weight scaled by its layer's power of two 2^k (max |w| 2^k <
    // 2^15) as hi = f16(w 2^k), lo = f16(w 2^k - hi); same fragment orders as the bf16 images with two pieces
    const uint32_t* pw_pair;   // [4][ct 2][m 4][piece 2][lane 64][4]
    const uint32_t* c1_pair;   // [ct 2][kb 7][piece 2][lane 64][4]
    int k_c1, k_pw[4];         // the layers' weight-scale exponents
    // bounds the per-clip activation scales are derived from: |conv1 out| <= c1_abs max|x| + c1_bmax; per block
    // |depthwise out| <= dw_abs max|in| + dw_bmax, |pointwise out| <= pw_abs max|depthwise out| + pw_bmax (row sums of |w|,
    // maximised over output channels, rounded up)
    float c1_abs, c1_bmax, dw_abs[4], dw_bmax[4], pw_abs[4], pw_bmax[4];
    const uint32_t* units;     // [unit 42][part 2][lane 64][4]  unit descriptors of the block phases (kws_dscnn_units.h; persistent launch)
};

hipError_t dscnn_init_device();
// Strided windows of a scan (kws_scan_i16; kws_dscnn_fwd_kernel, SCAN): "clip" i of the launch is window i % wpr of recording
// i / wpr, and its 99 x 10 floats start at feat + (i / wpr) * row_floats + (i % wpr) * win_floats -- 99 consecutive rows of the
// recording's [F_total][10] frame array.  The kernel forms the offset in 64 bits; each factor fits 32 (R * F_total <= 2^28).
struct ScanWindows {
    unsigned wpr;          // windows per recording
    unsigned wpr_recip;    // floor(2^32 / wpr), 2^32 - 1 for wpr == 1: i / wpr = mulhi(i, wpr_recip), or one more (all scalar, no
                           // division in the persistent kernel's block-4 tail, where every register is taken)
    unsigned row_floats;   // one recording's frames: F_total * 10
    unsigned win_floats;   // from one window to the next: hop_frames * 10
};
// The streaming push as ONE launch: every stream's workgroup of the DS-CNN kernel computes that stream's new MFCC frame in
// its prologue (kws_mfcc_dev.h: stream_frame_wave), appends the hop to the PCM ring, and the last workgroup to finish
// advances the hop counter.  d_feat_ring: [n_streams][num_frames][numcep]; d_hops: {pushes so far, finished workgroups}.
struct StreamPush {
    union {
        FrontendParams p;
        ScanWindows scan;    // SCAN only (launch_dscnn_scan): where a window's features start; nothing else of this struct is read then.
                             // Shares p's bytes: the kernel-argument segment of every other instantiation stays as it was
    };
    FrontendTables t;
    const int16_t* hop;      // [n_streams][frame_step]
    int16_t* pcm_ring;       // [n_streams][ring_len]
    int ring_len;
    int* hops;
    int* refine_ctr;         // counters of the selective refinement (RefineList::ctr; [5] counts frames redone by pushes) or NULL
    int frames_lag;          // two-launch route only: hops a frame spans, ceil(frame_len / frame_step) (the fused push derives it from p)
    int cluster;             // workgroups per stream of the fused push (time tiles; 1 = one workgroup owns the stream's network)
    float* cl_part;          // [n_streams][cluster][64] pooled partial sums of the tiles
    int* cl_count;           // [n_streams] tiles that have delivered theirs (the last one runs fc + argmax and clears it)
    float* h_logits;         // zero-copy delivery (kws_stream_host_results): pinned host [n_streams][C], or NULL
    int32_t* h_label;        // pinned host [n_streams], or NULL
    int* h_flag;             // pinned host: the push count whose results are complete in h_logits / h_label
};
hipError_t launch_dscnn_stream(hipStream_t s, const DscnnWeights& w, const StreamPush& sp, float* d_feat_ring, int n_streams,
                               float* d_logits, int32_t* d_label, bool pair);
// The same for a set with deactivated streams (kws_dscnn_active.hip): d_active is the device list of the n_active >= 1 active
// streams, ascending; the grid holds their workgroups alone and no other stream's state or result row is touched.
hipError_t launch_dscnn_stream_active(hipStream_t s, const DscnnWeights& w, const StreamPush& sp, float* d_feat_ring, int n_streams, float* d_logits,
                                      int32_t* d_label, bool pair, const int32_t* d_active, int n_active);
hipError_t dscnn_active_init_device();  // called by dscnn_init_device
hipError_t launch_dscnn(hipStream_t s, const DscnnWeights& w, const float* d_feat, int B, float* d_logits,
                        int32_t* d_label, float* d_act, int mode, unsigned long long* d_stamps = nullptr,
                        const int* d_ring_hops = nullptr, bool preconv = false, int frames_lag = 3, int n_cu = 0);
// The batched product kernels over the strided windows of a scan: B = R * sw.wpr windows, logits [B][C] and labels [B] in window
// order; mode 4 or 5 only.  One window per workgroup, or persistent workgroups above n_cu windows, exactly as launch_dscnn chooses.
hipError_t launch_dscnn_scan(hipStream_t s, const DscnnWeights& w, const float* d_feat, int B, float* d_logits, int32_t* d_label,
                             int mode, int n_cu, const ScanWindows& sw);
// conv1 of a model with input_channels > 1 (kws_dsblock.hip): x [B][C_in][99][10] -> relu(conv1) [B][64][141]; d_wt = weights as [ci][tap][co]
hipError_t launch_conv1_general(hipStream_t s, const float* d_x, int B, int C_in, const float* d_wt, const float* d_bias, float* d_out);

// ------------------------------------------------------------------------------------------------
// cnn-trad-fpool3 (build-defined model-zoo member, kws_cnntrad.hip)
struct CnnTradWeights {
    const uint32_t* c1_split;  // [kb 10][ct 2][piece 3][lane 64][4]    conv1 20x8 as bf16 hi/mid/lo MFMA A operands
    const float* c1_b;         // [64]
    const uint32_t* c2_split;  // [kk 40][cb 4][ct 2][piece 3][lane 64][4]  conv2 10x4x64
    const float* c2_b;         // [64]
    const uint32_t* lin_split; // [kb 1188][piece 3][lane 64][4]  first dense layer as bf16 hi/mid/lo MFMA B operands
    const float* lin_b;        // [32]
    const float* dnn_w;        // [128][32]
    const float* dnn_b;        // [128]
    const float* fc_w;         // [C][128]
    const float* fc_b;         // [C]
    int num_classes;
    // f16-pair arithmetic (kws_cnntrad.hip): every weight scaled by the layer's power of two sw (max |w| sw < 2^15) and written
    // as hi = f16(w sw), lo' = f16((w sw - hi) 2^11); same fragment orders as above with two pieces
    const uint32_t* c1_h2;     // [kb 10][ct 2][piece 2][lane 64][4]
    const uint32_t* c2_h2;     // [kk 40][cb 4][ct 2][piece 2][lane 64][4]
    const uint32_t* lin_h2;    // [kb 1188][piece 2][lane 64][4]
    float inv_sw1, inv_sw2, inv_swl;   // 1 / sw per layer
    float w1_abs, b1_max;      // max over output channels of sum |w1[c]|, max |b1|: |conv1 out| <= w1_abs * max|x| + b1_max
    float w2_abs, b2_max;      // the same for conv2
};
hipError_t cnntrad_init_device();
hipError_t launch_cnntrad_dense(hipStream_t s, const CnnTradWeights& w, const float* d_conv_ws, int B, float* d_logits,
                                int32_t* d_label, bool f16_pair);
// Windows of recordings read in place (kws_cnntrad_conv_windows_kernel): window i of the call is window i % wpr of recording
// i / wpr, 99 consecutive rows of the recording's [F][10] frame array from row (i % wpr) * hop_frames on.  A launch takes the n
// windows from `first` on and writes workspace slots 0 .. n - 1, which the dense launch reads as n clips.
struct CtWindows {
    unsigned first;        // the chunk's first window
    unsigned wpr;          // windows per recording
    unsigned row_floats;   // one recording's frames: F * 10
    unsigned win_floats;   // from one window to the next: hop_frames * 10
};
constexpr int CT_WINDOW_CHUNK = 4096;  // windows per launch pair: the workspace of kws_forward_cnn_trad_f32 at the bench batch (311 MB)
// Where the conv kernel finds the n maps of a launch: n contiguous clips [n][99][10] (kws_cnntrad_conv_kernel), n windows of a frame
// array [R][F][10] from windows.first on (kws_cnntrad_conv_windows_kernel), or the n streams' windows of the feature ring
// [n][99][10] (kws_cnntrad_conv_ring_kernel): stream s's window is the ring's 99 rows from ((*hops + 1 - lag) mod 99 + 99) mod 99 on.
struct CtSource {
    enum Kind { CLIPS, WINDOWS, RING } kind;
    const float* maps;
    CtWindows windows;  // WINDOWS
    const int* hops; int lag;  // RING: the hop counter the frame kernel has advanced, and frames_lag
};
// conv1 + pool + conv2 of n maps -> slots 0 .. n - 1 of d_conv_ws (n * 19008 floats, then n per-clip scales: f16-pair arithmetic only)
hipError_t launch_cnntrad_conv(hipStream_t s, const CnnTradWeights& w, const CtSource& src, int n, float* d_conv_ws, bool f16_pair);

// Standalone depthwise-separable block on an arbitrary [B, C_in, H, W] map (kws_dsblock.hip); d_ws: B*C_in*Ho*Wo floats.
hipError_t launch_dsblock(hipStream_t s, const float* d_x, int B, int C_in, int H, int W, const float* d_dw_w, const float* d_dw_b,
                          const float* d_pw_w, const float* d_pw_b, int C_out, int k, int stride, int pad, float* d_ws,
                          float* d_out);
// Its two kernels on their own: the depthwise convolution + bias -> [B][C_in][Ho][Wo], and the pointwise one on such a map ->
// [B][C_out][Ho + 2 pad][Wo + 2 pad] with ReLU, or (relu_out = false) as the pre-activation whose ring is the bias.
hipError_t launch_dsblock_depthwise(hipStream_t s, const float* d_x, int B, int C_in, int H, int W, const float* d_dw_w,
                                    const float* d_dw_b, int k, int stride, int pad, float* d_out);
hipError_t launch_dsblock_pointwise(hipStream_t s, const float* d_dw, int B, int C_in, int Ho, int Wo, const float* d_pw_w,
                                    const float* d_pw_b, int C_out, int pad, float* d_out, bool relu_out);

// DS-CNN on a feature map other than 99 x 10 (composed, HBM-resident): conv1 for any [B][C_in][T][F] (d_wt: [ci][tap][co]) and
// global average pool + fc + argmax over [B][64][HW].
// relu_out = false (the train-mode BatchNorm path, kws_dscnn_bn.hip): the pre-activation conv1 + bias.
hipError_t launch_conv1_any(hipStream_t s, const float* d_x, int B, int C_in, int T, int F, const float* d_wt, const float* d_bias,
                            float* d_out, bool relu_out = true);
hipError_t launch_pool_fc(hipStream_t s, const float* d_x, int B, int HW, const float* d_fc_w, const float* d_fc_b, int C,
                          float* d_logits, int32_t* d_label);
// The composed path's geometry on a T x F map: conv1's output is H1 x W1; block k (0-based) takes H(k) x W(k) = P(k) positions,
// its depthwise output has as many, its pointwise output (the relu(bias) ring included) is the next block's input.
struct DscnnMap {
    int H1, W1;
    DscnnMap(int T, int F) : H1((T - 6) / 2 + 1), W1((F - 6) / 2 + 1) {}
    int H(int k) const { return H1 + 2 * k; }
    int W(int k) const { return W1 + 2 * k; }
    size_t P(int k) const { return (size_t)H(k) * W(k); }
    size_t Q(int k) const { return P(k + 1); }  // block k's output positions
};
// The maps the composed path accepts (forward and backward alike); the error is set on c and returned, KWS_OK otherwise.
int check_dscnn_map(kws_ctx* c, const char* fn, int T, int F);
// Where the stages of nb clips go, each [nb][64][positions]: conv1's output, and per block its depthwise and its pointwise output.
// Stages may share memory as far as the data flow allows (a0 -> dw[0] -> y[0] -> dw[1] -> ...).
struct DscnnStages {
    float* a0;
    float* dw[N_BLOCKS];
    float* y[N_BLOCKS];
};
// conv1 + the four depthwise-separable blocks of nb <= 16384 clips (grid.z of the pointwise kernel), at the weights of the blob w.raw.
hipError_t launch_dscnn_composed(hipStream_t s, const DscnnWeights& w, const float* d_feat, int nb, int T, int F, const DscnnStages& st);
constexpr int COMPOSED_MAX_CLIPS = 16384;

// The decision layer (kws_decide.hip): posteriors and their moving average per stream.
hipError_t launch_softmax(hipStream_t s, const float* d_logits, int B, int C, float* d_prob);
hipError_t launch_smooth_posteriors(hipStream_t s, const float* d_logits, int S, int C, int window, float* d_ring,
                                    float* d_sum, int* d_count, float* d_smoothed, int32_t* d_label);
// Decisions over a scan's logits (kws_scan_detect_f32, kws_scan_score_f32 and their ragged twins): kws_ctx.h, WindowBatch and
// scan_posteriors -- they take the context, whose scratch they carve.

extern const char* const kKernelNames[KWS_K_COUNT];

}  // namespace kws
