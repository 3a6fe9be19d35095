/*
 * kws_hip.h -- C ABI of libkws_hip.so, the MI355X (gfx950) keyword-spotting hot path:
 *
 *     int16 PCM [B, n_samples]  ->  MFCC float32 [B,1,frames,numcep]  ->  DS-CNN  ->  logits [B,C], label [B]
 *
 * The reference (z430/keyword-spotting) is pure Python and has no FFI/plugin layer; its boundary for
 * this path is a handful of Python callables.  Each entry point below names the reference interface
 * it replaces (paths relative to the reference repo).  The reference-side binding is a ctypes stub,
 * shown in INTEGRATION.md; the build's own host mirror of the reference classes lives in
 * keyword-spotting_amd/kws/.
 *
 * Conventions
 *   - every function returns KWS_OK (0) or a negative KWS_E* code; no exception crosses the ABI;
 *     kws_last_error() gives the message of the last failure on that context.
 *   - pointers named d_* are DEVICE pointers owned by the caller (e.g. torch-ROCm tensor.data_ptr());
 *     the library never frees or retains them after the call's work has drained (kws_sync).
 *   - all work is enqueued asynchronously on the context's HIP stream.
 *   - a context belongs to one GPU and is not thread-safe; contexts are independent (one per GPU,
 *     no collectives: utterances are independent end to end).
 *   - there is NO CPU fallback: without a usable HIP device kws_create fails with KWS_EHIP.
 */
#ifndef KWS_HIP_H
#define KWS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kws_ctx kws_ctx;

enum {
    KWS_OK = 0,
    KWS_EINVAL = -1,       /* bad argument (null pointer, non-positive size, ...) */
    KWS_ENOMEM = -2,       /* host or device allocation failed */
    KWS_EHIP = -3,         /* a HIP runtime call failed (message in kws_last_error) */
    KWS_ESTATE = -4,       /* front end / model not configured yet */
    KWS_EUNSUPPORTED = -5  /* configuration outside what the gfx950 kernels implement */
};

/* ABI version of this header; kws_abi_version() returns the library's. */
#define KWS_ABI_VERSION 1
int kws_abi_version(void);

/* ---- context ------------------------------------------------------------------------------- */

/* Create a context on GPU `device_id` with its own non-blocking HIP stream and the default front
 * end (kws_set_frontend defaults).  Replaces the implicit device selection of
 * kws/libs/models.py:67 and kws/libs/data_loader.py:63 (`torch.device("cuda" ...)`). */
int kws_create(kws_ctx** out, int device_id);
void kws_destroy(kws_ctx* ctx);

/* external != 0: enqueue on the caller's stream `hip_stream` (a hipStream_t, e.g.
 * torch.cuda.current_stream().cuda_stream; NULL is the device's default stream, which is what torch
 * uses unless told otherwise).  external == 0: return to the context's own stream. */
int kws_set_stream(kws_ctx* ctx, void* hip_stream, int external);

/* Block the host until everything enqueued on the context's stream has finished. */
int kws_sync(kws_ctx* ctx);

/* Message of the last failure on this context ("" if none).  ctx == NULL: message of the last
 * failed kws_create on this thread. */
const char* kws_last_error(kws_ctx* ctx);

/* ---- front end: AudioProcessor.extract_features (kws/libs/audio_processor.py:235-278) ------- */

/* Parameters of psf.mfcc as the reference calls it.  Defaults (also set by kws_create):
 *   sample_rate 16000, n_samples 16000, frame_len 400, frame_step 160, nfft 512, nfilt 26,
 *   numcep 10, preemph 0.97, ceplifter 22                     (AudioConfig, audio_processor.py:37-46;
 *   psf.mfcc defaults for preemph / ceplifter / lowfreq 0 / highfreq sr/2 / appendEnergy True /
 *   rectangular window).  frame_len and frame_step are in samples (winlen*sr, winstep*sr rounded
 *   half up, as psf does).  Two kernels serve it:
 *     the float32 kernel (the hot path) for nfft == 512, frame_len <= 512, a filterbank that spans bins 0..256 in at most
 *     64 chunks of 8 bins (no stretch between two mel edges longer than 64 bins), and a hop whose 24-frame span fits a
 *     workgroup's LDS: 4 * (23 * frame_step + frame_len) bytes + 21 KB + the DCT table (4 * numcep * nfilt) <= 160 KB, i.e.
 *     frame_step up to ~1500 samples;
 *     the float64 kernel for every other geometry: nfft a power of two in [64, 4096] or any value in [2, 2048] (the
 *     reference derives nfft = max(fft_size, int(winlen*samplerate)), audio_processor.py:268 -- e.g. 640 for a 40 ms
 *     window), any frame_len (frames longer than nfft are truncated, as numpy.fft.rfft does).
 *     A geometry the float32 kernel does not cover is no error: kws_set_frontend returns KWS_OK, kws_frontend_math reports
 *     KWS_FE_F64 and every kws_mfcc_* / kws_scan_i16 call computes it in float64; kws_mfcc_augment_i16 and kws_stream_open
 *     (float32 only) return KWS_EUNSUPPORTED for it.  No geometry kws_set_frontend accepts fails at call time.
 *   Limits of both: nfilt <= 64, numcep <= min(nfilt, 32); anything else returns KWS_EUNSUPPORTED. */
int kws_set_frontend(kws_ctx* ctx, int sample_rate, int n_samples, int frame_len, int frame_step,
                     int nfft, int nfilt, int numcep, float preemph, int ceplifter);

/* Arithmetic of the front end -- replaces nothing in the reference (psf computes in float64 after a float32
 * pre-emphasis); PCM scaling and pre-emphasis are bit-exact float32 in both.
 *   KWS_FE_F32 (default): transform, mel sums, log and DCT in float32 -- the fast kernel.  Its rounding noise sits ~138 dB
 *     below a frame's strongest spectral component: cepstra within 1e-4 of the reference for frames whose mel bands span
 *     less than ~50 dB (noise, speech-like spectra), up to ~6e-4 on a clean tone over a quiet floor; logits within 1e-4.
 *   KWS_FE_F64: everything after framing in float64, as psf does -- cepstra within the float32 rounding of the output
 *     (~4e-6) on every input, at 4-5 times the kernel time (0.96 vs 0.21 ms per 4096 clips).  Geometries the float32 kernel is not built for run in
 *     float64 whatever this setting is; kws_frontend_math returns the arithmetic actually in use.  The streaming frame
 *     kernel (kws_stream_push_i16) is float32 only. */
#define KWS_FE_F32 0
#define KWS_FE_F64 1
int kws_set_frontend_math(kws_ctx* ctx, int math);
int kws_frontend_math(kws_ctx* ctx);

/* Diagnostics: which float32 kernel int16 PCM at the reference geometry (frames of 400 samples every 160, 26 filters, 10
 * cepstra) takes.  Both compute the same bits, flags included.
 *   KWS_FE_ROUTE_AUTO (default): the wavefront-resident kernel compiled for that geometry.
 *   KWS_FE_ROUTE_GENERIC: the wavefront-resident kernel that reads the geometry at run time, as every other geometry it covers
 *     does -- for A/B timing and bit comparison inside one process.
 * Any other value: KWS_EINVAL.  Takes effect from the next call; other geometries, sources and KWS_FE_F64 are unaffected. */
#define KWS_FE_ROUTE_AUTO 0
#define KWS_FE_ROUTE_GENERIC 1
int kws_set_frontend_route(kws_ctx* ctx, int route);

/* Selective float64 refinement of KWS_FE_F32 -- what makes the default front end meet psf's float64 arithmetic
 * (kws/libs/audio_processor.py:270-278) to 1e-4 on every frame.  A float32 transform leaves rounding noise a fixed distance
 * below the frame's strongest spectral component, so the float32 kernel measures, per frame, how far its weakest mel band
 * lies below its largest spectral bin: r = log(max bin power) - min log(mel energy) (natural-log units of power).  A frame
 * with r over `log_ratio` (default 10.2 = 44 dB) goes onto a device worklist and a second launch recomputes exactly those
 * rows in float64 (no host read-back; a batch with nothing listed pays one empty launch).  Frames under the threshold keep
 * the float32 kernel's bits.  Measured against the float64 oracle on 10.7 M frames of noise, tones, chirps, gated bursts,
 * mixtures and speech-like clips (tools/fe_precision_audit.py, profiles/r03_precision_audit.txt): no frame over 1e-4, the
 * worst of a seed's 297 000 frames 6.6e-5 .. 8.4e-5 (two seeds of 36: 9.3e-5 and 9.4e-5).  White noise lists ~0.3 % of its frames,
 * speech-like clips ~5 %, a clean tone over a quiet floor all of them.  (Until late in round 3 the flag was the span max - min
 * of the log-mel values with a threshold of 11.5: it cannot tell white noise, whose peak bin lies well below its strongest
 * band, from a tone, and left four frames of 2.4 M at 1.2-1.5e-4.)  The streaming push redoes a flagged frame in float64
 * inside the same launch.  log_ratio <= 0 switches the refinement off (the float32 kernel alone: up to 2e-3 on such
 * frames).  Takes effect from the next call; KWS_FE_F64 (always float64) is unaffected.  The macro keeps its round-3 name. */
#define KWS_FE_REFINE_SPAN_DEFAULT 10.2f
int kws_set_frontend_refine(kws_ctx* ctx, float log_ratio);
/* Frames that went through the float32 front end since kws_create (*frames_total), how many of them the refinement
 * recomputed in float64 (*frames_refined), and the number the last completed batched call listed (*last_call_refined).
 * Synchronises the context's stream.  Any pointer may be NULL. */
int kws_frontend_stats(kws_ctx* ctx, uint64_t* frames_total, uint64_t* frames_refined, int* last_call_refined);

/* Frames per clip (1 + ceil((n_samples - frame_len)/frame_step), sigproc.py:31-35) and numcep. */
int kws_frontend_shape(kws_ctx* ctx, int* num_frames, int* numcep);

/* Batched MFCC.  d_wav: int16 [B, n_samples] (PCM as stored in a 16-bit WAV; the kernel applies the
 * x/32768 scaling librosa.load applies, audio_processor.py:145).  d_out: float32
 * [B, 1, num_frames, numcep] -- the collated batch of SpeechCommandsDataLoader.__getitem__
 * (kws/libs/data_loader.py:96-105: float32 cast + channel axis) stacked by torch default_collate. */
int kws_mfcc_i16(kws_ctx* ctx, const int16_t* d_wav, int B, float* d_out);

/* Same, for a float32 signal in [-1, 1] that the caller has already decoded and possibly augmented
 * (time shift / background noise, audio_processor.py:154-159): d_wav float32 [B, n_samples].  This is
 * the exact input type of AudioProcessor.extract_features(signal) (audio_processor.py:235). */
int kws_mfcc_f32(kws_ctx* ctx, const float* d_wav, int B, float* d_out);

/* ---- model: DepthwiseSeparableConv (kws/libs/models.py:122-183) ----------------------------- */

/* Load weights: `blob` is a HOST pointer to the 20 state_dict tensors concatenated in state_dict
 * order (conv1.weight, conv1.bias, dsconv{1..4}.{depthwise,pointwise}.{weight,bias}, fc.weight,
 * fc.bias), float32; n_floats must be 25664 + 65*num_classes.  Copied to the device; the caller
 * keeps ownership.  Replaces KeywordSpottingModel.load (models.py:55-72). */
int kws_load_dscnn(kws_ctx* ctx, const float* blob, size_t n_floats, int num_classes);
/* The same for DepthwiseSeparableConv(num_classes, input_channels) with input_channels > 1 (models.py:125,135):
 * conv1.weight is then [64, input_channels, 10, 10], n_floats = 6400*input_channels + 19264 + 65*num_classes, and
 * kws_forward_f32 takes d_feat float32 [B, input_channels, 99, 10]: conv1 runs in a general kernel and the fused kernel
 * starts at block 1.  The wav -> label entry points need input_channels == 1 (an MFCC map has one channel). */
int kws_load_dscnn_ex(kws_ctx* ctx, const float* blob, size_t n_floats, int num_classes, int input_channels);
/* kws_load_dscnn_ex from a DEVICE-resident blob (d_blob: float32 [n_floats] on the context's device, same layout, same argument
 * checks and codes) -- the weight refresh of a training step (the reference re-reads its parameters after every optimizer.step(),
 * train.py:49) without a device-to-host copy: the image is built by kernels on the context stream (the fragment gather is the host
 * loader's source, kws_pack.h), the weight statistics are computed on the device in the host's arithmetic and order, and the 128
 * bytes of them are read back for the scalars the forward kernels take as launch arguments (the call waits for the context
 * stream).  For a finite blob every word of the image and all 23 scalars equal kws_host_dscnn_image of the same values, so every
 * forward is bit-identical to one after kws_load_dscnn_ex.  An image of the same size (same num_classes and input_channels) is
 * rewritten in place, without allocation; a captured streaming push is retired as by the host load.  If a launch fails after the
 * context's own image has been touched, the context has no model until the next successful load (KWS_ESTATE). */
int kws_load_dscnn_device(kws_ctx* ctx, const float* d_blob, size_t n_floats, int num_classes, int input_channels);
/* The context's current DS-CNN image and the 23 scalars, copied to the host, with the size protocol and the scalar order of
 * kws_host_dscnn_image: *need_words (may be NULL) is always set (0 when there is no model), out_words == NULL only asks for the
 * size, a cap_words below it is KWS_EINVAL.  No model loaded: KWS_ESTATE.  Waits for the context stream. */
int kws_dscnn_image_read(kws_ctx* ctx, uint32_t* out_words, size_t cap_words, size_t* need_words, float* scalars);

/* Forward on precomputed features.  d_feat: float32 [B,1,99,10]; d_logits: float32
 * [B,num_classes]; d_label: int32 [B] = argmax (first maximum wins, torch.max semantics,
 * kws/libs/training.py:371) or NULL.  Replaces DepthwiseSeparableConv.forward (models.py:160-183). */
int kws_forward_f32(kws_ctx* ctx, const float* d_feat, int B, float* d_logits, int32_t* d_label);

/* The same forward for a feature map of ANY size: d_feat float32 [B, input_channels, T, F] -- DepthwiseSeparableConv.forward
 * takes any [B,C,T,F] (models.py:160-183; the global average pool is adaptive) and AudioConfig.clip_duration_ms /
 * num_cepstral_coeffs change T and F (audio_processor.py:37-46).  T x F == 99 x 10 runs the fused LDS-resident kernel;
 * any other map runs composed through HBM: conv1 (10x10, stride 2, padding 2) -> four depthwise-separable blocks (each
 * adds its relu(bias) ring) -> global average pool + fc + argmax.  Needs T >= 6, F >= 6 and (T+4)*(F+4) <= 40960.
 * kws_infer_i16 / kws_infer_f32 / kws_infer_host_i16 follow kws_frontend_shape through this entry. */
int kws_forward_map_f32(kws_ctx* ctx, const float* d_feat, int B, int T, int F, float* d_logits, int32_t* d_label);
/* Parity aid for the composed path: also stores every stage's output to d_layers, stage after stage, each stage as
 * [B][64][H][W] -- conv1 (H1 x W1, H1 = (T-6)/2+1, W1 = (F-6)/2+1), then blocks 1..4 WITH their rings ((H1+2k) x (W1+2k)).
 * A 99 x 10 map takes the composed path here too (an independent check of the fused kernel). */
int kws_forward_map_debug_f32(kws_ctx* ctx, const float* d_feat, int B, int T, int F, float* d_logits, int32_t* d_label,
                              float* d_layers);

/* ---- training ------------------------------------------------------------------------------ */

/* Training: gradient of a scalar loss through DepthwiseSeparableConv.forward (models.py:160-183) for the model loaded by
 * kws_load_dscnn, given d_dlogits = dloss/dlogits float32 [B, num_classes].  d_feat float32 [B, C, T, F] as for
 * kws_forward_map_f32.  d_grad: float32 [n_floats] in the kws_load_dscnn blob layout (state_dict order), overwritten.
 * Replaces loss.backward() of train.py:48 / kws/libs/training.py:296 for this model.
 * The forward activations are recomputed by the composed fp32 path of kws_forward_map_f32 (nothing is saved by the
 * forward); the arithmetic is fp32, the two 64 x 64 GEMMs of each pointwise layer on the f32-input matrix cores.  The
 * gradients are deterministic: per-workgroup partials over a fixed clip ownership and a fixed-order reduction, so the same
 * inputs and B give bit-identical d_grad.  The ReLU convention is torch's (no gradient where an output is exactly 0).
 * Any B >= 1 (the workspace is bounded in chunks of at most 16384 clips), any map kws_forward_map_f32 accepts.
 * input_channels must be 1 (KWS_EUNSUPPORTED otherwise); no model loaded: KWS_ESTATE.  Asynchronous on the context
 * stream; the context keeps a workspace of about 1 MB per clip of the largest chunk (99 x 10). */
int kws_dscnn_backward_f32(kws_ctx* ctx, const float* d_feat, int B, int T, int F, const float* d_dlogits, float* d_grad);

/* Training: gradient of a scalar loss through cnn-trad-fpool3's forward (kws_forward_cnn_trad_f32) for the model loaded by
 * kws_load_cnn_trad or kws_load_cnn_trad_device, given d_dlogits = dloss/dlogits float32 [B, num_classes] and the features
 * d_feat float32 [B, 1, 99, 10].  d_grad: float32 [786720 + 129 num_classes] in the kws_load_cnn_trad blob layout (the ten
 * state_dict tensors in order), overwritten.  Replaces loss.backward() of train.py:48 / kws/libs/training.py:296 for this model.
 * The activations are recomputed by the call's own f32 forward (conv2 and lin on the f32-input matrix cores), so the gradients do
 * not depend on kws_set_cnn_trad_math; the pool routes each gradient to the first maximum of its window (torch's max_pool2d), and
 * the ReLU convention is torch's (no gradient where an output is exactly 0).  Deterministic: per-workgroup partials over a fixed
 * clip ownership and fixed-order reductions, no float atomics, so the same inputs and B give bit-identical d_grad.  Any B >= 1:
 * batches are cut into chunks of at most 8192 clips whose results add onto d_grad in chunk order; the context keeps a workspace of
 * about 324 KB per clip of the largest chunk.  No model loaded: KWS_ESTATE; a NULL pointer or B <= 0: KWS_EINVAL.  Asynchronous on
 * the context stream.  The gradient with respect to the features is not computed. */
int kws_cnn_trad_backward_f32(kws_ctx* ctx, const float* d_feat, int B, const float* d_dlogits, float* d_grad);

/* Parity aid of kws_cnn_trad_backward_f32: runs exactly its recompute launches on d_feat float32 [B, 1, 99, 10] and writes their
 * stages (device pointers): d_conv1 float32 [B, 64, 99, 10] (conv1 after ReLU), d_winner int32 [B, 64, 99, 3] (the pool's
 * winner 0..2 within each window of three bins), d_conv2 float32 [B, 64, 99, 3] (conv2 after ReLU), d_hidden float32 [B, 160]
 * (h = lin(.) [32], then d = relu(dnn(h)) [128]).  Tests pin the float64 oracle's ReLU and max-pool decisions to these (the role
 * kws_forward_map_debug_f32 plays for the DS-CNN).  Errors as kws_cnn_trad_backward_f32. */
int kws_cnn_trad_train_debug_f32(kws_ctx* ctx, const float* d_feat, int B, float* d_conv1, int32_t* d_winner, float* d_conv2,
                                 float* d_hidden);

/* Training the BatchNorm DS-CNN (DepthwiseSeparableConvBN, kws/libs/models.py: conv -> BatchNorm2d -> ReLU after conv1 and after
 * every pointwise convolution, conv -> BatchNorm2d after every depthwise one).  The three entries below take the parameters as a
 * DEVICE blob d_params float32 [n_floats] in DepthwiseSeparableConvBN.parameters() order -- the 20 tensors of kws_load_dscnn (one
 * input channel), then weight [64] | bias [64] of bn_conv1, bn_dw.0 .. 3, bn_pw.0 .. 3: n_floats = 25664 + 65*num_classes + 1152 --
 * and neither need nor touch the context's loaded model.  d_feat float32 [B, 1, T, F], any map kws_forward_map_f32 accepts.
 *
 * Train-mode forward: every BatchNorm normalises with the mean and the biased variance of its input over the batch and all
 * positions, y = gamma (z - mean) / sqrt(var + eps) + beta; the ring a padded pointwise convolution puts around its output equals
 * its bias and counts in that layer's statistics.  d_logits float32 [B, num_classes]; d_label int32 [B] or NULL; d_stats float32
 * [9][2][64] or NULL: batch mean and UNBIASED batch variance (var N / (N - 1), what nn.BatchNorm2d's running_var takes) per layer,
 * in the order conv1, dw1, pw1, dw2, pw2, dw3, pw3, dw4, pw4.  The sums are taken in float64 over per-workgroup partials reduced in
 * a fixed order (no float atomics): logits and statistics are bit-identical from call to call.
 * Statistics span the batch, so the batch is not chunked: B above kws_host_dscnn_bn_max_batch(T, F) is KWS_EUNSUPPORTED, refused
 * on the host before any allocation or launch.  B * H1 * W1 < 2 (one value per channel in the first layer; torch raises there too),
 * a NULL pointer, B <= 0, an n_floats other than the layout's, eps not positive and finite: KWS_EINVAL.  num_classes outside
 * [1, 64]: KWS_EUNSUPPORTED.  Map limits as kws_forward_map_f32.  Asynchronous on the context stream; the context keeps a workspace
 * of about 1.8 MB per clip (99 x 10). */
int kws_dscnn_bn_train_forward_f32(kws_ctx* ctx, const float* d_params, size_t n_floats, int num_classes, const float* d_feat, int B,
                                   int T, int F, float eps, float* d_logits, int32_t* d_label, float* d_stats);
/* Gradient of a scalar loss through that forward, given d_dlogits = dloss/dlogits float32 [B, num_classes]: d_grad float32
 * [n_floats] in the layout of d_params, overwritten.  Recompute, not save: the call redoes the train-mode forward into the
 * context's training workspace (it is deterministic, so the backward sees the bits the forward call produced), then per BatchNorm
 * layer S1 = sum dy^ and S2 = sum dy^ x^ in float64 (dy^: the incoming gradient, masked by output > 0 where a ReLU follows),
 * g_beta = S1, g_gamma = S2, dz = gamma / sigma (dy^ - S1 / N - x^ S2 / N), and dz through the convolution's backward of
 * kws_dscnn_backward_f32.  Deterministic as that entry.  Arguments, limits and errors as kws_dscnn_bn_train_forward_f32; the
 * gradient with respect to the features is not computed. */
int kws_dscnn_bn_backward_f32(kws_ctx* ctx, const float* d_params, size_t n_floats, int num_classes, const float* d_feat, int B, int T,
                              int F, float eps, const float* d_dlogits, float* d_grad);
/* Parity aid: kws_dscnn_bn_train_forward_f32 that also stores the five post-ReLU activations a0 .. a4 to d_layers, in the layout
 * of kws_forward_map_debug_f32 (conv1, then blocks 1..4 with their rings, each [B][64][H][W]).  Tests pin their references' ReLU
 * decisions to these. */
int kws_dscnn_bn_train_debug_f32(kws_ctx* ctx, const float* d_params, size_t n_floats, int num_classes, const float* d_feat, int B, int T,
                                 int F, float eps, float* d_logits, int32_t* d_label, float* d_layers, float* d_stats);
/* Host only: the largest B the three entries above take on a T x F map -- what fits 2^31 floats of workspace, at most 16384; 0 for
 * a map they refuse.  4747 at 99 x 10. */
int kws_host_dscnn_bn_max_batch(int T, int F);

/* One depthwise-separable block on an arbitrary map -- replaces DepthwiseSeparableConvBlock.forward
 * (kws/libs/models.py:108-119) used on its own: depthwise Conv2d(C_in, C_in, kernel_size, stride, padding, groups=C_in)
 * + bias, then pointwise Conv2d(C_in, C_out, 1, padding=padding) + bias, then ReLU.  d_x float32 [B,C_in,H,W]; d_dw_w
 * [C_in,1,k,k], d_dw_b [C_in], d_pw_w [C_out,C_in,1,1], d_pw_b [C_out] (device pointers, the module's parameters as torch
 * stores them); d_out float32 [B, C_out, Ho + 2*padding, Wo + 2*padding] with Ho = (H + 2*padding - k)/stride + 1: the
 * pointwise padding adds a ring equal to relu(bias), as in the reference.  The four blocks of the DS-CNN do NOT go
 * through this entry point: they run fused inside kws_forward_f32. */
int kws_dsblock_forward_f32(kws_ctx* ctx, const float* d_x, int B, int C_in, int H, int W, const float* d_dw_w,
                            const float* d_dw_b, const float* d_pw_w, const float* d_pw_b, int C_out, int kernel_size,
                            int stride, int padding, float* d_out);

/* Fused wav -> label: kws_mfcc_i16 into an internal workspace, then kws_forward_f32.  This is the
 * shape of inference(wav) -> label (kws/inference/inference_local.py:67-81), batched. */
int kws_infer_i16(kws_ctx* ctx, const int16_t* d_wav, int B, float* d_logits, int32_t* d_label);

/* The same for float32 signals in [-1, 1] (d_wav float32 [B, n_samples]): what librosa.load hands the reference for files
 * that are not 16-bit PCM (24-bit, float, stereo mixed down in float: audio_processor.py:145). */
int kws_infer_f32(kws_ctx* ctx, const float* d_wav, int B, float* d_logits, int32_t* d_label);

/* The same from HOST memory to HOST memory -- what the reference does between the decoded audio and the model input:
 * DataLoader workers collate batches into pinned memory and the trainer calls inputs.to(device)
 * (kws/libs/data_loader.py:96-105, train.py:108-121, kws/libs/training.py:286).  h_wav: int16 [B, n_samples] in host
 * memory (pageable or pinned), h_logits: float32 [B, C], h_label: int32 [B] or NULL, both host.  The batch is cut into
 * chunks; a pool of host threads packs chunk k+1 into pinned staging while chunk k travels over PCIe on a copy stream,
 * chunk k-1 runs MFCC + DS-CNN and the results of chunk k-2 return on a second copy stream.  Synchronous: the results
 * are complete on return.  A pinned h_wav (hipHostMalloc / hipHostRegister / torch pin_memory) is read by the DMA
 * directly, without the pack stage. */
int kws_infer_host_i16(kws_ctx* ctx, const int16_t* h_wav, int B, float* h_logits, int32_t* h_label);
/* The same in two halves, so that a caller with MANY batches keeps the pipeline full across them (kws_infer_host_i16 alone
 * fills and drains it inside every call): submit enqueues every chunk of the batch and returns -- the caller's pageable h_wav
 * has been packed into pinned staging by then and may be reused; a PINNED h_wav, h_logits and h_label must stay valid until
 * the wait -- and hands back a ticket; kws_infer_host_wait(ctx, ticket) blocks until every batch up to that ticket has its
 * results in its h_logits / h_label (ticket 0: everything in flight).  Submitting batch k+1 before waiting for batch k lets
 * k+1's pack and H2D run under k's kernels.  Results of older batches are also delivered whenever a later submit needs
 * their staging slot.  kws_infer_host_i16 == submit + wait.
 * A submit that is REFUSED -- KWS_EINVAL (B <= 0, a NULL or a device pointer) or KWS_ESTATE (no front end or model; the class
 * count or n_samples changed while batches are in flight) -- has enqueued nothing and leaves the ring, its slots and every
 * ticket in flight exactly as they were: their results still arrive (it may use up a ticket NUMBER, never one handed out).
 * A submit that FAILS after enqueuing chunks of its own (a HIP error mid-batch) first delivers the chunks of every older
 * ticket, then drops its own chunks only, and writes its ticket number to *ticket.  kws_infer_host_wait never returns KWS_OK
 * over rows nobody filled: a wait that covers a dropped ticket (its number, a later one, or 0) -- dropped by such a submit or
 * because its results failed to return -- delivers what it can of the OTHER tickets, returns the code of the failure and
 * names the dropped ticket(s) in kws_last_error, once. */
int kws_infer_host_submit_i16(kws_ctx* ctx, const int16_t* h_wav, int B, float* h_logits, int32_t* h_label, uint64_t* ticket);
int kws_infer_host_wait(kws_ctx* ctx, uint64_t ticket);
/* Pipeline shape of kws_infer_host_i16: clips per chunk (default 1024), staging slots in flight (default 3, 2..16), host
 * threads of the pack stage (default min(16, cores/2); negative = pack on the calling thread).  0 keeps a default.  A batch
 * smaller than chunk x slots is cut into `slots` chunks (not below 128 clips), so that its stages overlap too. */
int kws_ingest_config(kws_ctx* ctx, int chunk_clips, int n_slots, int pack_threads);

/* Pre-size the internal workspaces for batches up to max_batch (otherwise grown on demand, which
 * allocates and must not happen inside stream capture). */
int kws_reserve(kws_ctx* ctx, int max_batch);

/* Arithmetic of conv1 and the 1x1 (pointwise) convolutions on the matrix cores -- replaces nothing in the reference
 * (torch's f32 conv2d, kws/libs/models.py:104-106); every setting keeps the logits within 1e-4 of it.
 *   KWS_PW_PAIR_F16 (default): every f32 operand, after an exact power-of-two scaling into f16's range, as an f16 pair
 *     hi + lo (22 significant bits); three v_mfma_f32_32x32x16_f16 per k-block, f32 accumulate.  Weights are scaled per
 *     layer at load time, activations per CLIP: the kernel keeps them in LDS in power-of-two units whose exponents it derives,
 *     two layers ahead, from the measured maximum of an earlier stage and bounds that hold for any input -- nothing can
 *     overflow, and logits differ from a float64 evaluation by what a plain f32 evaluation differs by.
 *   KWS_PW_SPLIT_BF16: every f32 operand is split exactly into three bf16 pieces (hi + mid + lo == x)
 *     and the six piece products of combined order <= 2 are accumulated in f32 by v_mfma_f32_32x32x16_bf16;
 *     each bf16 x bf16 product is exact, the dropped terms are <= 2^-24 relative -- the size of one f32
 *     rounding.  Twice the matrix instructions of the pair.
 *   KWS_PW_F32: v_mfma_f32_32x32x2_f32 (shares the FP32 datapath with the VALU; slower).
 * Changing it invalidates a captured streaming graph (re-captured on the next push). */
#define KWS_PW_F32 1
#define KWS_PW_SPLIT_BF16 4
#define KWS_PW_PAIR_F16 5
int kws_set_pointwise_math(kws_ctx* ctx, int math);

/* Debug/parity aid: run the DS-CNN and also store every stored activation per clip to d_act
 * (float32 [B, KWS_ACT_FLOATS_PER_CLIP]): conv1 out [64][47*3], block1 out interior [64][47*3],
 * block2 out interior [64][49*5], block3 out interior [64][51*7], pooled mean [64], block4 out interior
 * [64][53*9] (never stored by the product kernel: it is pooled in registers).  "Interior" =
 * the pointwise output without the relu(bias) ring its padding=1 adds (models.py:104-106).
 * use_mfma: KWS_PW_SPLIT_BF16 (4) / KWS_PW_F32 (1) = the two matrix-core kernels, 0 = a variant whose
 * pointwise / conv1 GEMMs run on the VALU (an independent check of the matrix-core operand mappings). */
#define KWS_ACT_FLOATS_PER_CLIP (64 * (141 + 141 + 245 + 357) + 64 + 64 * 477)
int kws_forward_debug_f32(kws_ctx* ctx, const float* d_feat, int B, float* d_logits, int32_t* d_label,
                          float* d_act, int use_mfma);

/* ---- streaming: 10 ms hops over concurrent streams (BASELINE.json config 5) ------------------------ */

/* The reference's streaming use case is VAD-segmented capture followed by one whole-clip inference
 * (kws/inference/inference_local.py:114-192).  Here every push of frame_step (160) new samples per stream
 * completes one MFCC frame per stream (frames of the continuous signal: frame f = samples
 * [160 f, 160 f + 400)), appends it to a ring of num_frames (99) frames, and classifies the last 99 frames
 * (one second) of every stream.  Until a stream has produced 99 frames the missing rows are zeros. */
int kws_stream_open(kws_ctx* ctx, int n_streams);
int kws_stream_close(kws_ctx* ctx);
/* d_hop: int16 [n_streams, frame_step] new samples; d_logits float32 [n_streams, C] (NULL: features only);
 * d_label int32 [n_streams] or NULL.  With logits and the default pointwise math a push is ONE launch: each stream's
 * workgroup of the DS-CNN kernel computes the stream's new frame in its prologue and the last workgroup advances the hop
 * counter.  Features-only pushes, and pushes under KWS_PW_F32 / the VALU check, are the frame kernel (which then advances
 * the counter) followed by the DS-CNN kernel.  use_graph != 0 replays a MULTI-launch push as a hipGraph (built on first use
 * for the given pointer triple); the one-launch push is always launched directly -- a one-node graph replay is 8 us slower
 * than the plain launch on this stack (tools/graph_overhead.hip). */
int kws_stream_push_i16(kws_ctx* ctx, const int16_t* d_hop, float* d_logits, int32_t* d_label, int use_graph);
/* Shape of the one-launch push: workgroups per stream.  1: one workgroup owns a stream's whole DS-CNN (the layout of the
 * batched kernel).  2 / 4: the stream's network is cut into that many TIME TILES, one workgroup each -- every stage's rows
 * a tile's share of block 4's output depends on are recomputed inside the tile (about four rows of halo per side), nothing
 * is exchanged between the workgroups but 64 pooled partial sums per tile at the very end, where the last workgroup to
 * arrive adds them in tile order and runs fc + argmax.  At 64 streams one workgroup per stream leaves three quarters of the
 * CUs idle and the push latency is one clip's serial path; four tiles bring the kernel from 37.6 to ~17 us.  0 (default):
 * 4 up to 64 streams, 2 up to 128, else 1.  Logits of different shapes agree to the float32 rounding of the pooled sums
 * (their order of addition differs); a given shape is deterministic. */
int kws_stream_cluster(kws_ctx* ctx, int workgroups_per_stream);
/* Zero-copy result delivery for the one-launch push (the latency path of BASELINE config 5).  enable != 0: the context
 * allocates pinned, device-mapped host arrays; from then on every push that asks for logits ALSO writes its logits
 * [n_streams, C] and labels [n_streams] there with system-scope stores, and the workgroup that finishes last raises a flag in
 * host memory.  kws_stream_wait_host spins on that flag (falling back to the stream after ~2 ms) and returns the host
 * arrays (owned by the context, overwritten by the next push): the caller has the results in hand without a
 * hipStreamSynchronize round trip and without a device-to-host copy.  d_logits / d_label of kws_stream_push_i16 are still
 * written.  Call after kws_stream_open and kws_load_dscnn; kws_stream_open / kws_stream_close / enable == 0 release it.
 *   The arrays hold n_streams x C floats for the C LOADED AT THIS CALL, and kws_load_dscnn / kws_load_dscnn_device leave them
 *   alone.  After a load with another class count they are stale: kws_stream_push_i16 still takes the hop and writes the caller's
 *   d_logits / d_label (sized by the caller for the new C), delivers NOTHING to the host arrays, and kws_stream_wait_host returns
 *   KWS_ESTATE with a message that names the class-count change until kws_stream_host_results(ctx, 1) is called again.
 *   kws_stream_push_host_i16 and kws_stream_push_host_rate_i16 own their outputs, so they make the arrays again by themselves
 *   (one stream synchronise, as this call) and deliver the new model's results; the hop counter runs on.  No entry hands a
 *   kernel an output array made for another class count. */
int kws_stream_host_results(kws_ctx* ctx, int enable);
int kws_stream_wait_host(kws_ctx* ctx, const float** h_logits, const int32_t** h_label);
/* The whole hop from host memory to host memory in one call: h_hop int16 [n_streams, frame_step] (pageable is fine) is copied
 * into pinned device-mapped memory, the one-launch push reads it from there (no H2D submission), and the call returns when
 * the kernel has delivered logits [n_streams, C] and labels [n_streams] to the context's host arrays (see above; valid until
 * the next push).  Enables kws_stream_host_results by itself.  The reference's live path hands a captured utterance to the
 * model from host memory (kws/inference/inference_local.py:168-192); this is its per-hop counterpart. */
int kws_stream_push_host_i16(kws_ctx* ctx, const int16_t* h_hop, const float** h_logits, const int32_t** h_label);
/* Synchronises and returns the feature ring (float32 [n_streams, num_frames, numcep], device memory owned
 * by the context) and the number of pushes so far; the newest frame is row (hops - K) mod num_frames, K = ceil(frame_len / frame_step)
 * hops per frame (3 for the reference's 400 / 160). */
int kws_stream_state(kws_ctx* ctx, const float** d_feat_ring, int* hops);
/* Copy the raw feature ring (float32 [n_streams, num_frames, numcep], ring order) into caller memory. */
int kws_stream_copy_features(kws_ctx* ctx, float* d_out);

/* Energy endpointer for the streams opened with kws_stream_open (build-defined: it stands in for
 * the webrtcvad endpointing of the reference's live loop, kws/inference/inference_local.py:131-166, with the same
 * hysteresis at hop granularity).  Call after kws_stream_push_i16.  The hop is voiced when the newest frame's log
 * energy (cepstrum 0) exceeds the threshold; an utterance opens when more than 80 % of the last on_window hops are
 * voiced (:151), closes when more than 90 % of the last off_window hops are unvoiced (:161); 400 ms / 800 ms in the
 * reference = 40 / 80 hops of 10 ms.  d_state int32 [n_streams]: bit 0 = inside an utterance, bits 1-2 = event at
 * this hop (1 opened, 2 closed).  The history lives in the context; kws_stream_open or a change of windows resets it. */
int kws_stream_vad_f32(kws_ctx* ctx, float log_energy_threshold, int on_window, int off_window, int32_t* d_state);

/* ---- cnn-trad-fpool3 (build-defined: the reference only names the model, test.py:80) ----
 * Sainath & Parada's cnn-trad-fpool3 on the [1,99,10] MFCC map with SAME padding: conv 64 x (20x8) + ReLU,
 * max-pool 1x3 over frequency, conv 64 x (10x4) + ReLU, flatten, Linear 32, Linear 128 + ReLU, Linear C.
 * blob = the ten state_dict tensors in order, float32: conv1.weight [64,1,20,8], conv1.bias [64], conv2.weight
 * [64,64,10,4], conv2.bias [64], lin.weight [32,19008], lin.bias [32], dnn.weight [128,32], dnn.bias [128],
 * fc.weight [C,128], fc.bias [C] (host pointer, copied). */
int kws_load_cnn_trad(kws_ctx* ctx, const float* blob, size_t n_floats, int num_classes);
/* kws_load_cnn_trad from a DEVICE-resident blob (same layout, same argument checks) -- the weight refresh of a training step
 * (the reference re-reads its parameters after every optimizer.step(), train.py:49): the pre-split images are packed by a kernel
 * and the weight statistics computed on the device in the host's order, and the handful of floats the model carries by value is
 * read back (the call waits for the context stream).  The resulting forward is bit-identical to a kws_load_cnn_trad of the same
 * values.  The image is rebuilt in place when the class count is unchanged. */
int kws_load_cnn_trad_device(kws_ctx* ctx, const float* d_blob, size_t n_floats, int num_classes);
/* float32 [B,1,99,10] features -> logits float32 [B,C] and labels int32 [B] (d_label may be NULL).  The
 * convolution output (76 KB per clip) goes through a context workspace that grows on demand. */
int kws_forward_cnn_trad_f32(kws_ctx* ctx, const float* d_feat, int B, float* d_logits, int32_t* d_label);
/* Arithmetic of cnn-trad-fpool3's three GEMM layers on the matrix cores.  KWS_CT_F16_PAIR (default): every f32 operand as an
 * f16 pair hi + lo' 2^-11 (22 bits) after an exact power-of-two scaling into f16's range -- per layer for the weights, per clip
 * for the activations from rigorous bounds, so no input can overflow -- three f16 MFMAs per k-block; logits differ from a
 * float64 evaluation by what a plain f32 evaluation differs by.  KWS_CT_BF16_TRIPLE: the exact three-way bf16 split the DS-CNN
 * uses (six MFMAs per k-block, twice the matrix time). */
#define KWS_CT_F16_PAIR 0
#define KWS_CT_BF16_TRIPLE 1
int kws_set_cnn_trad_math(kws_ctx* ctx, int math);
/* Parity aid of kws_forward_cnn_trad_f32: runs exactly its two launches (same code path, under the context's current
 * kws_set_cnn_trad_math) and then copies what sits in the context workspace between them, device to device on the context's
 * stream: d_conv2 float32 [B,64,99,3] = conv2 after ReLU, channel-major as the convolution kernel writes it (the dense kernel's
 * input), and d_clip_scale float32 [B] = the clip's power-of-two scale into f16's range.  d_clip_scale may be NULL; it is
 * written only under KWS_CT_F16_PAIR and left untouched under KWS_CT_BF16_TRIPLE (that arithmetic has no such scale).  Errors as
 * kws_forward_cnn_trad_f32, plus KWS_EINVAL for a NULL d_conv2.  (The role kws_forward_debug_f32 plays for the DS-CNN.) */
int kws_forward_cnn_trad_debug_f32(kws_ctx* ctx, const float* d_feat, int B, float* d_logits, int32_t* d_label, float* d_conv2,
                                   float* d_clip_scale);

/* Fused wav -> label for this model (BASELINE.json configs[2]): kws_mfcc_i16 into the context workspace, then
 * kws_forward_cnn_trad_f32, on the context's stream.  Same arguments and errors as kws_infer_i16. */
int kws_infer_cnn_trad_i16(kws_ctx* ctx, const int16_t* d_wav, int B, float* d_logits, int32_t* d_label);
/* The float32 twin: kws_mfcc_f32 into the context workspace, then kws_forward_cnn_trad_f32.  Same arguments and errors as
 * kws_infer_f32; samples of int16 PCM / 32768 give the bits of kws_infer_cnn_trad_i16. */
int kws_infer_cnn_trad_f32(kws_ctx* ctx, const float* d_wav, int B, float* d_logits, int32_t* d_label);

/* ---- cnn-trad-fpool3 on recordings and streams: windows read in place ----
 * Windows per launch pair of kws_forward_cnn_trad_windows_f32 (host only): a positive multiple of 16, the clips the dense kernel
 * takes per workgroup.  The context workspace holds one chunk's convolution output (76 KB per window). */
int kws_host_cnn_trad_window_chunk(void);
/* The model over the strided 99-frame windows of R recordings' frame arrays, read where they lie: d_frames float32 [R][F][10]
 * (kws_frames_i16 / kws_frames_f32 write it), W = (F - 99) / hop_frames + 1 windows per recording, window w of recording r =
 * rows [w * hop_frames, w * hop_frames + 99) -> d_logits float32 [R][W][C] and d_label int32 [R][W] (may be NULL).  Every window's
 * result is bit-identical to kws_forward_cnn_trad_f32 on the same 99 rows handed over as a contiguous clip, under either
 * arithmetic (the f16 pair's scales are per window).  Runs in chunks of kws_host_cnn_trad_window_chunk() windows, one convolution
 * and one dense launch each, on the context's stream.  Needs a loaded model (kws_load_cnn_trad) and nothing of the front end.
 * KWS_EINVAL: NULL d_frames / d_logits, R < 1, hop_frames < 1, F < 99.  KWS_ESTATE: no model loaded.  KWS_EUNSUPPORTED: more than
 * 2^28 frames or 2^30 windows in one call (the limits of kws_scan_i16). */
int kws_forward_cnn_trad_windows_f32(kws_ctx* ctx, const float* d_frames, int R, int F, int hop_frames, float* d_logits,
                                     int32_t* d_label);
/* kws_scan_i16 / kws_scan_f32 for this model: one MFCC pass per recording, then kws_forward_cnn_trad_windows_f32 over the frame
 * array.  Same arguments, shapes and limits; KWS_ESTATE without a front end or a cnn-trad-fpool3 model, KWS_EUNSUPPORTED for a
 * front end whose clip is not 99 x 10. */
int kws_scan_cnn_trad_i16(kws_ctx* ctx, const int16_t* d_pcm, int R, int n_total, int hop_frames, float* d_logits, int32_t* d_label,
                          float* d_feat_out);
int kws_scan_cnn_trad_f32(kws_ctx* ctx, const float* d_wav, int R, int n_total, int hop_frames, float* d_logits, int32_t* d_label,
                          float* d_feat_out);
/* kws_scan_ragged_i16 / kws_scan_ragged_f32 for this model: the ragged front end, then the packed frame array scanned as ONE
 * recording.  Same arguments, plan (kws_host_ragged_plan) and limits; the model's errors as for kws_scan_cnn_trad_i16. */
int kws_scan_ragged_cnn_trad_i16(kws_ctx* ctx, const int16_t* d_pcm, int n_pcm, const int64_t* start, const int32_t* len, int R,
                                 int hop_frames, float* d_logits, int32_t* d_label, float* d_feat_out);
int kws_scan_ragged_cnn_trad_f32(kws_ctx* ctx, const float* d_wav, int n_wav, const int64_t* start, const int32_t* len, int R,
                                 int hop_frames, float* d_logits, int32_t* d_label, float* d_feat_out);
/* kws_stream_push_i16 for this model: d_hop int16 [n_streams][frame_step] -> one new frame per stream in the rings, then every
 * stream's current window classified from the feature ring in place -> d_logits float32 [n_streams][C] (required) and d_label
 * int32 [n_streams] (may be NULL).  Three launches on the context's stream (frame, convolution, dense); a context armed with
 * kws_stream_utt_open / kws_stream_detect_open runs its step behind them, and the detection set's class count must be this
 * model's.  There is no graph replay, no one-launch push and no zero-copy delivery for this model: read the device arrays
 * after kws_sync.  KWS_ESTATE: no open stream set or no model loaded; KWS_EINVAL: NULL d_hop / d_logits; KWS_EUNSUPPORTED: a
 * front end whose clip is not 99 x 10. */
int kws_stream_push_cnn_trad_i16(kws_ctx* ctx, const int16_t* d_hop, float* d_logits, int32_t* d_label);

/* ---- posteriors (build-defined: the reference's scripts stop at argmax of the logits,
 * kws/libs/training.py:371) ------------------------------------------------------------------------------ */

/* Softmax over the C logits of every row: float32 [B,C] -> float32 [B,C] (device pointers, C <= 64). */
int kws_softmax_f32(kws_ctx* ctx, const float* d_logits, int B, int C, float* d_prob);

/* Streaming posterior smoothing for the streams opened with kws_stream_open: softmax of this hop's logits
 * [n_streams, C], then the mean over the last `window` hops per stream (fewer while the history is shorter),
 * written to d_smoothed [n_streams, C]; d_label (may be NULL) = argmax of the smoothed vector, first maximum
 * wins.  The history lives in the context and is reset by kws_stream_open / a change of window or C. */
int kws_stream_smooth_f32(kws_ctx* ctx, const float* d_logits, int C, int window, float* d_smoothed, int32_t* d_label);

/* ---- scanning recordings longer than a clip (build-defined: the reference has no such mode; its nearest code is the
 * record-then-classify loop of kws/inference/inference_local.py:114-192) ------------------------------------------- */

/* Classify every window of R recordings of equal length: ONE MFCC pass over each recording, then the DS-CNN over strided
 * windows of the frame array -- no window of PCM or of features is ever materialised.
 *   d_pcm: int16 [R, n_total] (device).  Frames: each recording is ONE clip of n_total samples under the context's own front
 *   end (kws_set_frontend except its n_samples, kws_set_frontend_math, kws_set_frontend_refine): F_total =
 *   1 + ceil((n_total - frame_len) / frame_step) frames (1 when n_total <= frame_len), the last one zero-padded as psf does;
 *   bit-identical, refinement included, to kws_mfcc_i16 with B = R on a context configured with n_samples = n_total, and
 *   counted by kws_frontend_stats as that call counts them (R * F_total frames through the float32 front end).  The context's
 *   own n_samples is neither used nor changed.
 *   Windows: T = the context's num_frames (the model's clip length, kws_frontend_shape).  Window w of recording r is frames
 *   [w * hop_frames, w * hop_frames + T); W = (F_total - T) / hop_frames + 1, rounded down (kws_host_scan_shape gives both
 *   counts).  Window w covers samples [w * hop_frames * frame_step, w * hop_frames * frame_step + (T - 1) * frame_step +
 *   frame_len), clipped to n_total.
 *   d_logits: float32 [R, W, C].  d_label: int32 [R, W] or NULL, first maximum wins.  d_feat_out: float32 [R, F_total, numcep]
 *   or NULL; NULL keeps the frames in a context workspace that grows on demand, so the call allocates and is not for stream
 *   capture.
 *   A recording of exactly n_samples samples gives W = 1 and the logits and label of kws_infer_i16 on it, bit for bit.  Any
 *   other window differs from clip-wise inference on the same samples in two places, exactly as the streaming ring does: the
 *   first sample of its first frame (pre-emphasis continues across the window start) and its last frame (which sees real
 *   samples where a clip is zero-padded).  Given the frames, a window's logits are bit-identical to kws_forward_f32 on those
 *   99 rows, wherever the window sits.
 *   Scope: a 99 x 10 window map (the fused kernel), a one-channel model, KWS_PW_PAIR_F16 or KWS_PW_SPLIT_BF16; anything else
 *   is KWS_EUNSUPPORTED.  F_total < T, hop_frames < 1, R < 1, n_total < 1 or a NULL d_pcm / d_logits: KWS_EINVAL.  No front end
 *   or no model: KWS_ESTATE.  Limits (KWS_EUNSUPPORTED beyond): R * F_total <= 2^28 -- the refinement worklist packs
 *   (recording * ceil(F_total / 2) + frame pair) << 2 into 32 bits, and a recording's F_total * numcep floats are a 32-bit
 *   stride of the window kernel; R * W <= 2^30 -- the window index and the persistent kernel's next-window index are ints;
 *   n_total <= 2^30 -- the front-end kernels form sample indices up to a chunk past the end in ints.  The refinement
 *   worklist grows with R * F_total (a tone flags every frame).
 *   Timed under KWS_K_MFCC / KWS_K_MFCC_REFINE / KWS_K_MFCC_F64 and KWS_K_DSCNN.  Asynchronous on the context stream. */
int kws_scan_i16(kws_ctx* ctx, const int16_t* d_pcm, int R, int n_total, int hop_frames, float* d_logits, int32_t* d_label,
                 float* d_feat_out);

/* kws_scan_i16 over float32 samples: d_wav float32 [R, n_total] (device), taken as they are -- no scaling, no clamping, values
 * beyond +-1 pass through as kws_mfcc_f32 passes them.  Same checks, error codes, limits, timing ids and stream behaviour.
 *   Frames: those of kws_frames_f32 (below), refinement and KWS_FE_F64 included.  Windows: bit-identical to kws_forward_f32 on
 *   the 99 gathered rows.  A recording of exactly n_samples samples gives the logits and label of kws_infer_f32, bit for bit.
 *   Grid property: for d_wav[i] = (float)pcm[i] / 32768 (exact) the frames, logits and labels equal kws_scan_i16's on pcm bit for
 *   bit -- the int16 entries' PCM scaling is that exact division.
 *   What differs from the twin: the sample type, and the front-end route -- the wavefront-resident float32 kernel when n_total
 *   is a multiple of 8, d_wav is 16-byte aligned and the geometry is that kernel's; the float32 tile kernel otherwise.  Both give
 *   the same bits. */
int kws_scan_f32(kws_ctx* ctx, const float* d_wav, int R, int n_total, int hop_frames, float* d_logits, int32_t* d_label,
                 float* d_feat_out);

/* Causal decisions over a scan's logits [R, W, C] (C <= 64) -- the decisions a stream would have made at each hop.
 *   p[r, w, :] = softmax(logits[r, w, :]) as kws_softmax_f32 computes it.
 *   Smoothing: s[r, w, c] = mean of p[r, v, c] over v = max(0, w - S + 1) .. w, S = smooth_window in [1, 256]: summed in
 *   float32, oldest first, then divided by the number of terms -- the rule of kws_stream_smooth_f32 (fewer terms while the
 *   history is shorter), as a direct sum per output (no running sum, no drift).
 *   Candidates: k = first argmax of s[r, w, :]; window w is a candidate when k >= first_keyword and s[r, w, k] >= threshold
 *   (first_keyword = 2 skips _silence_ / _unknown_, kws/common/types.py; 0 skips nothing).
 *   Events: walking w upwards with next = 0, a candidate at w >= next is the event (w, k, s[r, w, k]) and sets
 *   next = w + refractory (refractory >= 1; 1: every candidate fires).
 *   d_event_count int32 [R]: the number of events, even beyond max_events.  The first min(count, max_events) events of
 *   recording r go to d_event_window / d_event_label (int32) and d_event_score (float32), each [R, max_events], in window
 *   order; slots beyond the count are not written (max_events == 0: the three may be NULL).  d_smoothed: float32 [R, W, C]
 *   or NULL.  Deterministic: no atomics.  The kernels are not timed; scratch of R * W * (C + 2) floats lives in the context.
 *   A NULL d_logits / d_event_count, R or W < 1, C outside [1, 64], S outside [1, 256], refractory < 1, first_keyword < 0,
 *   max_events < 0: KWS_EINVAL.  R * W > 2^30: KWS_EUNSUPPORTED. */
int kws_scan_detect_f32(kws_ctx* ctx, const float* d_logits, int R, int W, int C, int smooth_window, int first_keyword,
                        float threshold, int refractory, float* d_smoothed, int32_t* d_event_window, int32_t* d_event_label,
                        float* d_event_score, int max_events, int32_t* d_event_count);

/* ---- utterances from recordings (the device side of the reference's one live path, kws/inference/inference_local.py:114-192:
 * an endpointer opens and closes an utterance (:149-166), the captured samples start 600 ms before the trigger (:156,
 * :176-179), normalize scales them to a peak of 16384 (:102-109) and inference pads or trims to one second and classifies once
 * (:67-81).  Build-defined where the reference gates on webrtcvad: the voiced decision is the frame's log energy, as
 * kws_stream_vad_f32) ------------------------------------------------------------------------------------------------ */

/* The MFCC pass of kws_scan_i16 on its own: each of the R recordings is ONE clip of n_total samples under the context's own
 * front end.  d_pcm: int16 [R, n_total] (device).  d_feat_out: float32 [R, F_total, numcep], F_total = 1 + ceil((n_total -
 * frame_len) / frame_step), 1 when n_total <= frame_len (kws_host_scan_shape) -- a recording shorter than a window is fine.
 *   Bit-identical to the d_feat_out of kws_scan_i16 and to kws_mfcc_i16 with B = R on a context configured with n_samples =
 *   n_total, refinement included, and counted by kws_frontend_stats as those count.  The context's own n_samples is neither
 *   used nor changed.  Needs a front end (else KWS_ESTATE), no model.  A NULL pointer, R < 1 or n_total < 1: KWS_EINVAL.
 *   Limits as the scan's (KWS_EUNSUPPORTED beyond): R * F_total <= 2^28, n_total <= 2^30.
 *   Timed under KWS_K_MFCC / KWS_K_MFCC_REFINE / KWS_K_MFCC_F64.  Asynchronous on the context stream; the refinement worklist
 *   grows with R * F_total, so the call may allocate and is not for stream capture. */
int kws_frames_i16(kws_ctx* ctx, const int16_t* d_pcm, int R, int n_total, float* d_feat_out);

/* kws_frames_i16 over float32 samples: d_wav float32 [R, n_total] (device), taken as they are.  Same checks, error codes, limits,
 * timing ids and stream behaviour.
 *   Equal, word for word, to kws_mfcc_f32 with B = R on a context configured with n_samples = n_total: the selective refinement
 *   included, under KWS_FE_F32 and under KWS_FE_F64, and counted by kws_frontend_stats as that call counts.  For d_wav[i] =
 *   (float)pcm[i] / 32768 the rows and the counts equal kws_frames_i16's on pcm (see kws_scan_f32).
 *   What differs from the twin: the sample type and the front-end route (see kws_scan_f32). */
int kws_frames_f32(kws_ctx* ctx, const float* d_wav, int R, int n_total, float* d_feat_out);

/* The endpointer of kws_stream_vad_f32 walked over a whole frame array, with the reference's start point and time-out.
 *   d_feat: float32 [R, F_total, numcep] (kws_frames_i16, or the d_feat_out of kws_scan_i16); only column 0, the log frame
 *   energy, is read; the row stride is the context's numcep; frame_len / frame_step are the context's.  n_total: samples per
 *   recording (it clips an utterance's end).
 *   Per recording, frames f = 0 .. F_total - 1:  v[f] = feat[f][0] > log_energy_threshold (float32, strict; a NaN is
 *   unvoiced; frames before 0 are unvoiced).  c_on[f] / c_off[f] = voiced frames among the last on_window / off_window frames
 *   ending at f.  Walking f upwards with triggered = false, prev_close = -1, count = 0:
 *     not triggered and 10 c_on[f] > 8 on_window: the utterance opens, open = f (:153); nothing else happens at this frame;
 *     triggered and 10 (off_window - c_off[f]) > 9 off_window: close at f, reason 0 (:163-164);
 *     triggered otherwise, max_frames > 0 and f - open + 1 >= max_frames: close at f, reason 1 (build-defined stand-in for
 *       TimeUse > 10, :164, counted from the open: a recording has no "start of listening" per utterance);
 *     after these, still triggered at f == F_total - 1: close there, reason 2 (the recording ended).
 *   A close: start_frame = max(open - pre_roll, prev_close + 1, 0) (the reference starts 20 chunks of 30 ms before the
 *   trigger, :156; pre_roll is in frames), start_sample = start_frame * frame_step, end_sample = min(n_total, f * frame_step +
 *   frame_len); if count < max_utts, slot count of d_utt receives (start_sample, end_sample, open, f, reason); then count += 1,
 *   prev_close = f, triggered = false.
 *   d_utt: int32 [R, max_utts, 5].  d_count: int32 [R], the full count, even beyond max_utts.  Slots at or beyond the count
 *   are not written; max_utts == 0 allows a NULL d_utt.  With max_frames == 0 the opens and the reason-0 closes are exactly
 *   the events of kws_stream_vad_f32 over the same column.
 *   KWS_EINVAL: outside 1 <= on_window <= off_window <= 1024, pre_roll < 0, max_frames not 0 and below 2, max_utts < 0, R,
 *   F_total or n_total < 1, a NULL d_feat / d_count (or d_utt with max_utts > 0).  No front end: KWS_ESTATE.  No log energy in
 *   cepstrum 0: KWS_EUNSUPPORTED (as kws_stream_vad_f32).  R * F_total > 2^28: KWS_EUNSUPPORTED.
 *   Two launches, asynchronous on the context stream, integers only, no atomics: the same bits run to run.  Scratch of
 *   4 * R * ceil(F_total / 64) 64-bit words lives in the context and grows on demand (not for stream capture).  Not timed by
 *   kws_prof_*. */
int kws_segment_f32(kws_ctx* ctx, const float* d_feat, int R, int F_total, int n_total, float log_energy_threshold, int on_window,
                    int off_window, int pre_roll, int max_frames, int32_t* d_utt, int max_utts, int32_t* d_count);

/* normalize (:102-109) followed by fix_length (:70) for U spans of samples: d_span int32 [U, 3] = (recording, start, end).
 *   d_pcm: int16 [R, n_total].  d_clips: int16 [U, n_out]; every element is written.  d_peak: int32 [U] or NULL.
 *   Per span: start and end are clamped to [0, n_total], len = max(0, end - start).  peak = max |x[i]| over the WHOLE span as
 *   an int (|-32768| = 32768; 0 for an empty span) -- not over its first n_out samples: the reference normalises before it
 *   trims.  normalize_to > 0 (the reference's 16384) and peak > 0: times = (double)normalize_to / (double)peak and out[i] =
 *   (int16) trunc((double)x[start + i] * times) for i < min(len, n_out) -- the float64 divide, multiply and truncation towards
 *   zero of Python's int(i * times).  peak == 0 writes zeros (the reference raises ZeroDivisionError).  normalize_to == 0 is a
 *   plain copy.  out[i] = 0 for i >= len.  A recording index outside [0, R) reads nothing: a zero clip and peak = -1.
 *   KWS_EINVAL: normalize_to outside [0, 32767], U, R, n_total or n_out < 1, a NULL d_pcm / d_span / d_clips.  Needs neither a
 *   front end nor a model.  One launch, asynchronous on the context stream, deterministic; not timed by kws_prof_*. */
int kws_cut_i16(kws_ctx* ctx, const int16_t* d_pcm, int R, int n_total, const int32_t* d_span, int U, int normalize_to,
                int16_t* d_clips, int n_out, int32_t* d_peak);

/* kws_cut_i16 over float32 samples.  d_wav: float32 [R, n_total].  d_clips: float32 [U, n_out]; every element is written.
 * d_peak: float32 [U] or NULL.  d_span, its clamping and the recording index outside [0, R) (a zero clip, peak = -1) are
 * kws_cut_i16's.
 *   peak = the largest |x[i]| over the WHOLE span in float32, compared with m > peak, so a NaN never raises it; 0 for an empty
 *   span.  normalize_to > 0 and peak > 0: times = (double)normalize_to / (double)peak and out[i] = (float)((double)x[start + i] *
 *   times) for i < min(len, n_out) -- a float64 divide and multiply, then ONE round-to-nearest conversion.  peak == 0 writes
 *   zeros.  normalize_to == 0 is a bitwise copy.  out[i] = 0 for i >= len.
 *   What differs from the twin: no truncation step (there is no int() to reproduce), normalize_to and the peaks are floats in
 *   full-scale units -- the reference's 16384 is normalize_to = 0.5.
 *   KWS_EINVAL: normalize_to negative or not finite, U, R, n_total or n_out < 1, a NULL d_wav / d_span / d_clips.  Needs neither a
 *   front end nor a model.  One launch, asynchronous on the context stream, deterministic; not timed by kws_prof_*.  A ragged float
 *   batch is cut as ONE recording over the whole buffer, as the note below says for int16. */
int kws_cut_f32(kws_ctx* ctx, const float* d_wav, int R, int n_total, const int32_t* d_span, int U, float normalize_to,
                float* d_clips, int n_out, float* d_peak);

/* Cutting the spans of a ragged batch (below) needs no entry of its own: kws_cut_i16 over the whole buffer as ONE recording
 * (R = 1, n_total = n_pcm, recording index 0), with start[r] added to each span of recording r on the host, gives the clips
 * and peaks kws_cut_i16 gives on that recording alone -- a span lies inside its recording, so the clamp to [0, n_pcm] never
 * bites. */

/* ---- batches of recordings of unequal length: the scan, the frames, the decisions and the endpointer above in ONE call for R
 * recordings that each keep their own length.  Every recording's results are bit-identical to the equal-length entry run on
 * that recording alone.
 *   Layout.  PCM: one device buffer d_pcm of n_pcm int16 samples, 16-byte aligned; recording r is samples [start[r], start[r] +
 *   len[r]).  start (int64 [R]) and len (int32 [R]) are HOST arrays, checked before anything is launched: len[r] >= 1,
 *   start[r] >= 0, start[r] % 8 == 0, start[r] + len[r] <= n_pcm, else KWS_EINVAL; n_pcm <= 2^30 and R <= 2^20, else
 *   KWS_EUNSUPPORTED.  That covers a packed buffer (starts rounded up to 8) and the rectangular output of kws_resample_i16 with
 *   d_len (start[r] = r * n_out, n_out % 8 == 0).  Nothing outside a recording's span is read as part of it -- the one 16-byte
 *   vector that straddles its end is read sample by sample.
 *   Frames: one packed array float32 [F_pack, numcep].  Recording r has F_r = 1 + ceil((len[r] - frame_len) / frame_step) rows
 *   (1 when len[r] <= frame_len) from row frame_off[r]; its row count is rounded up to a multiple of row_multiple and the
 *   rounding rows are written as zeros; frame_off[R] = F_pack <= 2^28.
 *   Windows: with row_multiple = hop_frames the packed array is scanned as ONE recording of F_pack frames by the strided DS-CNN
 *   launch of kws_scan_i16; window w of recording r is packed window win_off[r] + w, win_off[r] = frame_off[r] / hop_frames, W_r =
 *   0 when F_r < T, else (F_r - T) / hop_frames + 1, and W_pack = 0 when F_pack < T, else (F_pack - T) / hop_frames + 1.  Every
 *   win_off[r] + w with w < W_r lies below W_pack.  The packed windows that belong to no recording straddle two recordings: they
 *   are computed and their content is unspecified -- at most ceil((T - 1) / hop_frames) + 1 per recording.
 *   The plan tables are derived on the host and uploaded into context scratch: the device entries may wait for the stream,
 *   allocate, and are not for stream capture. */

/* The ragged front end: kws_frames_i16 for every recording of the batch in one launch (plus the refinement of the frames it
 * flags).  d_feat_out: float32 [F_pack, numcep] as laid out above (kws_host_ragged_plan with hop_frames = row_multiple gives
 * frame_off and F_pack); every row is written.  Rows frame_off[r] .. frame_off[r] + F_r - 1 equal, word for word,
 * kws_frames_i16 on recording r alone, selective float64 refinement included; kws_frontend_stats counts sum F_r frames and the
 * flagged frames of the recordings together.
 *   Routes: the float32 wavefront-resident kernel at its generic geometry (frame_len in (384, 448], 4 * frame_step a multiple of
 *   8, 3 * frame_step + 448 <= 1024 -- the reference's 400 / 160 among them), refinement on or off.  KWS_FE_F64 and every other
 *   geometry: KWS_EUNSUPPORTED.  A NULL pointer, R or n_pcm < 1, row_multiple < 1, d_pcm off a 16-byte boundary, a bad start /
 *   len: KWS_EINVAL.  No front end: KWS_ESTATE.  F_pack > 2^28: KWS_EUNSUPPORTED.
 *   Timed under KWS_K_MFCC / KWS_K_MFCC_REFINE.  Asynchronous on the context stream after the tables' upload. */
int kws_frames_ragged_i16(kws_ctx* ctx, const int16_t* d_pcm, int n_pcm, const int64_t* start, const int32_t* len, int R,
                          int row_multiple, float* d_feat_out);

/* kws_frames_ragged_i16 over float32 samples: one device buffer d_wav of n_wav float32 samples, 16-byte aligned, recording r =
 * samples [start[r], start[r] + len[r]) with start[r] % 8 == 0 (a packed buffer, or the rectangular output of kws_resample_f32
 * with d_len and n_out % 8 == 0).  Same checks, error codes, limits, routes (KWS_FE_F64 and geometries outside the
 * wavefront-resident kernel's: KWS_EUNSUPPORTED), timing ids and stream behaviour.
 *   Rows frame_off[r] .. frame_off[r] + F_r - 1 equal, word for word, kws_frames_f32 on recording r alone, refinement included;
 *   rounding rows are zeros.  Nothing past start[r] + len[r] is read as part of recording r: a vector is 8 samples (two 16-byte
 *   loads) and the one that straddles the end is read sample by sample.  For d_wav[i] = (float)pcm[i] / 32768 the rows equal
 *   kws_frames_ragged_i16's.  What differs from the twin: the sample type.
 *   The decisions and the endpointer of a ragged float batch need nothing new: kws_scan_detect_ragged_f32 and
 *   kws_segment_ragged_f32 take logits and frames. */
int kws_frames_ragged_f32(kws_ctx* ctx, const float* d_wav, int n_wav, const int64_t* start, const int32_t* len, int R,
                          int row_multiple, float* d_feat_out);

/* kws_scan_i16 for a ragged batch: kws_frames_ragged_i16 with row_multiple = hop_frames, then the scan launch over the packed
 * frame array.  d_logits: float32 [W_pack, C]; d_label: int32 [W_pack] or NULL; d_feat_out: float32 [F_pack, numcep] or NULL
 * (a context workspace).  Rows win_off[r] + w, w < W_r, equal kws_scan_i16 on recording r alone (window w), bit for bit; the
 * other rows are unspecified.  A recording shorter than a window is fine (W_r = 0); when every W_r is 0 nothing is launched
 * after the frames.  Scope, model and state checks as kws_scan_i16; argument checks and limits as kws_frames_ragged_i16, and
 * W_pack <= 2^30.  Timed under KWS_K_MFCC / KWS_K_MFCC_REFINE and KWS_K_DSCNN. */
int kws_scan_ragged_i16(kws_ctx* ctx, const int16_t* d_pcm, int n_pcm, const int64_t* start, const int32_t* len, int R, int hop_frames,
                        float* d_logits, int32_t* d_label, float* d_feat_out);

/* kws_scan_ragged_i16 over float32 samples (the buffer of kws_frames_ragged_f32): rows win_off[r] + w, w < W_r, equal kws_scan_f32
 * on recording r alone, bit for bit.  Same checks, error codes, limits, timing ids and stream behaviour; what differs from the
 * twin is the sample type. */
int kws_scan_ragged_f32(kws_ctx* ctx, const float* d_wav, int n_wav, const int64_t* start, const int32_t* len, int R, int hop_frames,
                        float* d_logits, int32_t* d_label, float* d_feat_out);

/* kws_scan_detect_f32 per recording of a ragged scan.  d_logits: float32 [W_pack, C]; win_off, windows: HOST int32 [R]
 * (kws_host_ragged_plan), win_off ascending with win_off[r] >= win_off[r - 1] + windows[r - 1].  Softmax, smoothing, candidates
 * and the refractory walk run per recording: the history never crosses a recording's first window, events carry window
 * indices relative to their own recording, and the packed rows between recordings are never read.  d_event_count int32 [R];
 * the three event arrays [R, max_events]; d_smoothed float32 [W_pack, C] or NULL (rows of no recording are not written).
 * Recording r's results equal kws_scan_detect_f32 on its own [1, W_r, C] logits; W_r = 0 gives count 0.
 *   KWS_EINVAL as kws_scan_detect_f32 (R < 1, C outside [1, 64], ...), a NULL table, a negative count or overlapping windows.
 *   R > 2^20 or more than 2^30 packed windows: KWS_EUNSUPPORTED.  Not timed; scratch of (C + 2) floats per packed window. */
int kws_scan_detect_ragged_f32(kws_ctx* ctx, const float* d_logits, const int32_t* win_off, const int32_t* windows, int R, int C,
                               int smooth_window, int first_keyword, float threshold, int refractory, float* d_smoothed,
                               int32_t* d_event_window, int32_t* d_event_label, float* d_event_score, int max_events,
                               int32_t* d_event_count);

/* kws_segment_f32 per recording of a packed frame array.  d_feat: float32 [F_pack, numcep] (kws_frames_ragged_i16, any
 * row_multiple); frame_off, frames, len: HOST int32 [R] -- the recording's first row, its F_r and its samples (frame_off
 * ascending, rows not overlapping).  Frames before 0 and at or past F_r are unvoiced, the reason-2 close falls at F_r - 1,
 * end_sample is clipped to len[r], and spans are in samples relative to the recording's own start.  d_utt: int32 [R, max_utts,
 * 5]; d_count: int32 [R].  Recording r's results equal kws_segment_f32 on that recording alone.
 *   KWS_EINVAL / KWS_ESTATE / KWS_EUNSUPPORTED as kws_segment_f32, plus: a NULL table, frames[r] or len[r] < 1 or overlapping
 *   rows (KWS_EINVAL); R > 2^20 or rows beyond 2^28 (KWS_EUNSUPPORTED).  Two launches; not timed. */
int kws_segment_ragged_f32(kws_ctx* ctx, const float* d_feat, const int32_t* frame_off, const int32_t* frames, const int32_t* len, int R,
                           float log_energy_threshold, int on_window, int off_window, int pre_roll, int max_frames, int32_t* d_utt,
                           int max_utts, int32_t* d_count);

/* ---- scoring a scan against annotations over a threshold sweep: event-level hits, false alarms, duplicates and latency per
 * class and threshold, on the device, with one read-back of K * C * 4 counters ------------------------------------------- */

/* Events.  For recording r and threshold t the events are exactly those kws_scan_detect_f32 fires with the same smooth_window,
 * first_keyword, refractory and threshold = t: the same softmax, float32 smoothing sums, first argmax, score >= t comparison in
 * float32 and walk -- bit for bit, for any float t (0, above 1; NaN: no events).  The smoothing runs once, not per threshold.
 * Annotations.  truth: HOST int32 [N][4], rows (recording, label, first_window, last_window) in any order, windows relative to
 * the recording's own.  A row is valid when 0 <= recording < R, first_keyword <= label < C and 0 <= first_window <=
 * last_window (last_window may lie beyond the recording's last window: nothing fires there).  Two rows of one recording and
 * one label must not overlap (sharing one window is overlapping); rows of different labels may.
 * Matching.  Per recording and threshold the events are taken in window order.  For an event (w, k) let j be the annotation of
 * that recording with label k and first_window <= w <= last_window (at most one).  No j: a false alarm of class k (also inside
 * an annotation of another label).  j not matched yet at this threshold: a hit of class k, j becomes matched, w - first_window
 * is added to class k's latency sum.  j matched already: a duplicate of class k, neither hit nor false alarm.
 * Counts.  d_counts: uint64 [K][C][4] (device) = hits, false alarms, duplicates, latency sum in windows, summed over the call's
 * recordings; overwritten, not accumulated.  Misses are annotations minus hits.  Integer atomics: deterministic. */

/* Host only: the annotation table validated and sorted.  sorted: int32 [N][4], the rows by (recording, label, first_window);
 * off: int32 [R * C + 1], rows off[r * C + k] .. off[r * C + k + 1] - 1 of sorted are recording r's label k (off[R * C] = N).
 * truth is not modified; nothing is written unless KWS_OK.  N = 0 is valid (truth and sorted may be NULL; off is all zeros).
 *   KWS_EINVAL: a row that is not valid, two overlapping rows of one recording and label, R < 1, C outside [1, 64],
 *   first_keyword < 0, N < 0, a NULL off, or a NULL truth / sorted with N > 0.  N > 2^24 or R > 2^20: KWS_EUNSUPPORTED. */
int kws_host_score_plan(const int32_t* truth, int N, int R, int C, int first_keyword, int32_t* sorted, int32_t* off);

/* The counts above for d_logits float32 [R][W][C] (device) at thresholds HOST float [K], K in [1, 1024], any values in any
 * order, each scored on its own.  truth: HOST, through kws_host_score_plan (its codes pass through).  Launches: softmax, the
 * smoothing kernel of kws_scan_detect_f32 at a threshold of -inf, a memset of d_counts, one sweep (a wavefront per recording
 * and threshold).  Asynchronous on the context stream behind the upload of the tables, which waits for the stream's earlier
 * work; not timed.  Scratch in the context: R * W * (C + 2) floats as kws_scan_detect_f32, and the tables.
 *   KWS_EINVAL: as kws_scan_detect_f32 for what they share (R or W < 1, C outside [1, 64], S outside [1, 256], refractory < 1,
 *   first_keyword < 0, a NULL d_logits), a NULL thresholds / d_counts, K outside [1, 1024], N < 0.  R * W > 2^30:
 *   KWS_EUNSUPPORTED.  A refused call launches nothing and leaves d_counts as it was. */
int kws_scan_score_f32(kws_ctx* ctx, const float* d_logits, int R, int W, int C, int smooth_window, int first_keyword, int refractory,
                       const float* thresholds, int K, const int32_t* truth, int N, uint64_t* d_counts);

/* kws_scan_score_f32 per recording of a packed scan: d_logits float32 [W_pack, C], win_off / windows HOST int32 [R] with the
 * checks and limits of kws_scan_detect_ragged_f32.  The history never crosses a recording's first window, annotations carry
 * window indices relative to their own recording, rows of no recording change nothing, a recording without windows
 * contributes nothing, and when no recording has a window d_counts is zeroed.  The counts equal the sum of kws_scan_score_f32
 * over each recording alone. */
int kws_scan_score_ragged_f32(kws_ctx* ctx, const float* d_logits, const int32_t* win_off, const int32_t* windows, int R, int C,
                              int smooth_window, int first_keyword, int refractory, const float* thresholds, int K, const int32_t* truth,
                              int N, uint64_t* d_counts);

/* ---- live utterances (the same loop, :114-192, for the streams of kws_stream_open: the walk of kws_segment_f32 taken one
 * frame per hop, a PCM history per stream to cut from, events in a queue the host reads without a copy) ------------------ */

/* Host only: the history a stream needs, in samples.  K = ceil(frame_len / frame_step) hops complete a frame.
 *   *history_samples = (pre_roll + max_frames - 1 + K + slack_hops) * frame_step: the longest span an utterance can have,
 *   (pre_roll + max_frames - 1) * frame_step + frame_len, rounded up to whole hops, plus slack_hops hops that may be pushed
 *   between a close and its cut (kws_stream_utt_cut_i16 refuses a span whose start has left the ring).
 *   KWS_EINVAL: frame_len or frame_step < 1, pre_roll < 0, max_frames < 2, slack_hops < 0, a NULL pointer, or a result beyond
 *   INT_MAX. */
int kws_host_stream_utt_history(int frame_len, int frame_step, int pre_roll, int max_frames, int slack_hops, int* history_samples);

/* Arm the open stream set: from here to kws_stream_utt_close (or kws_stream_open / kws_stream_close / kws_set_frontend, which
 * drop it with the streams) every push -- kws_stream_push_i16, kws_stream_push_host_i16, kws_stream_push_rate_i16,
 * kws_stream_push_host_rate_i16 -- enqueues ONE more launch behind its own (with use_graph: behind the replay, outside the
 * captured graph): the step kernel, one workgroup, one thread per stream.  A push's logits and labels are the bits of an
 * unarmed push; an unarmed context launches nothing new.
 *   Stream time counts from this call: sample 0 is the first sample pushed after it, frame f covers samples [f * frame_step,
 *   f * frame_step + frame_len), and the set's push number h (from 1) completes frame h - K; the first K - 1 pushes append PCM
 *   and walk nothing (as kws_stream_vad_f32 reports nothing for them).
 *   The step, per push: (1) APPEND each stream's newest hop to its history ring int16 [n_streams, history_samples] at (hops *
 *   frame_step) mod history_samples.  The hop is read from the CONTEXT'S OWN PCM ring, not from the caller's pointer: the ring
 *   is device-resident, the same for all four entries, holds the RESAMPLED hop for the rate pushes (what the front end heard),
 *   and a step still running when kws_stream_push_host_i16 has returned and its pinned hop slot is being rewritten reads
 *   nothing of that slot.  (2) WALK one frame with exactly the rules of kws_segment_f32 above: v = c0 > threshold (float32,
 *   strict, a NaN is unvoiced; c0 = the newest row of the feature ring); the window counts are kept per stream and updated in
 *   O(1) -- add the new flag, subtract the flag leaving, from a ring of 1024 flag bits; not triggered and 10 c_on > 8
 *   on_window: open = f, nothing else at this frame; triggered and 10 (off_window - c_off) > 9 off_window: close, reason 0;
 *   else triggered and f - open + 1 >= max_frames: close, reason 1.  A close: start_frame = max(open - pre_roll, prev_close + 1,
 *   0), start_sample = start_frame * frame_step, end_sample = f * frame_step + frame_len (never clipped: a walked frame is
 *   complete), prev_close = f.  (3) EMIT: the streams that closed at this step get consecutive sequence numbers in ascending
 *   stream order (wavefront ballots and a prefix over the wavefronts; no atomics: the same bits run to run).  A record is
 *   int64 [6] = (stream, start_sample, end_sample, open_frame, close_frame, reason), written at seq mod max_events to the device
 *   queue and to its mirror in pinned, device-mapped host memory (system-scope stores; the totals and then a completion count
 *   are published behind them, as kws_stream_host_results delivers logits).  A queue of max_events records keeps the newest
 *   max_events; older ones are overwritten.
 *   Needs an open stream set (else KWS_ESTATE) and the log energy in cepstrum 0 (else KWS_EUNSUPPORTED, as kws_stream_vad_f32).
 *   KWS_EINVAL: outside 1 <= on_window <= off_window <= 1024; pre_roll < 0; max_frames < 2 (a live ring is bounded: there is no
 *   "no time-out"); history_samples below kws_host_stream_utt_history(..., slack_hops = 0) for the context's frame geometry or
 *   not a multiple of frame_step; max_events < n_streams (all streams may close at one step).  n_streams > 1024:
 *   KWS_EUNSUPPORTED.  Waits for the context stream, allocates; a second call replaces the first.  Independent of
 *   kws_stream_vad_f32, whose state and results it neither reads nor changes.  No entry below allocates. */
int kws_stream_utt_open(kws_ctx* ctx, float log_energy_threshold, int on_window, int off_window, int pre_roll, int max_frames,
                        int history_samples, int max_events);
/* Waits for the context stream and releases what kws_stream_utt_open allocated; nothing when the context is not armed. */
int kws_stream_utt_close(kws_ctx* ctx);
/* The explicit step, for callers with their own front end (and the tests): d_hop int16 [n_streams, frame_step] (device), if
 * not NULL, is appended; d_energy float32 [n_streams] (device), if not NULL, walks one frame with these energies in place of
 * the feature ring (append first, then walk).  Both NULL: KWS_EINVAL.  The caller keeps the frame's samples appended before it
 * walks the frame (K hops for frame 0); kws_stream_utt_cut_i16 refuses a span that ends beyond the appended samples.
 * KWS_ESTATE: the context is not armed, or a push has stepped this armed set -- and a push is refused (KWS_ESTATE) once this
 * entry has stepped it: the set has ONE frame counter and ONE hop counter, and the two drivers would let them drift apart. */
int kws_stream_utt_step_i16(kws_ctx* ctx, const int16_t* d_hop, const float* d_energy);
/* Close every stream that is inside an utterance at the newest walked frame F - 1, reason 2, prev_close = F - 1 (one launch).
 * A hop-by-hop run followed by a flush equals kws_segment_f32 over the same F frames with n_total beyond reach, an utterance
 * that opened at the very last frame included.  The streams go on afterwards.  Not armed: KWS_ESTATE. */
int kws_stream_utt_flush(kws_ctx* ctx);
/* Wait until the step of the newest enqueued push, step or flush has landed: spins on the completion count in host memory and
 * falls back to the stream after ~2 ms (as kws_stream_wait_host).  *total_events: records emitted since kws_stream_utt_open;
 * *steps: frames walked (either may be NULL).  Not armed: KWS_ESTATE. */
int kws_stream_utt_poll(kws_ctx* ctx, uint64_t* total_events, uint64_t* steps);
/* Copy records first_seq .. first_seq + n - 1 out of the host mirror: out_records int64 [n, 6] (host).  Waits for nothing:
 * sequence numbers at or beyond the total that has landed, and ones no longer in the queue (seq + max_events < total, checked
 * again after the copy), are KWS_EINVAL, as are n < 1 and a NULL pointer.  Not armed: KWS_ESTATE. */
int kws_stream_utt_read(kws_ctx* ctx, uint64_t first_seq, int n, int64_t* out_records);
/* kws_cut_i16 with a ring origin: normalize + fix_length of the spans of U consecutive sequence numbers, one workgroup per
 * span, each record read from the DEVICE queue (no span list is uploaded).  d_clips int16 [U, n_out] (device), every element
 * written; d_peak int32 [U] or NULL.  Peak over the whole span (|-32768| = 32768), float64 divide, multiply and truncation
 * towards zero, zeros beyond the span: on the linear signal the clips and peaks are bit-identical to kws_cut_i16's.  A span
 * crosses the ring's seam at most once.  A zero clip and peak = -1 (kws_cut_i16's refusal of a recording out of range) for: a
 * sequence number not emitted yet or already overwritten in the queue (seq + max_events < total); a span whose start is older
 * than appended - history_samples (cut too late: more than slack_hops hops after the close); a span that ends beyond the
 * appended samples (explicit steps only).  The launch is ordered on the context stream behind every earlier push, so "appended"
 * is what was pushed before this call.  KWS_EINVAL: U or n_out < 1, normalize_to outside [0, 32767], a NULL d_clips.  Not armed:
 * KWS_ESTATE.  Asynchronous, deterministic, not timed by kws_prof_*. */
int kws_stream_utt_cut_i16(kws_ctx* ctx, uint64_t first_seq, int U, int normalize_to, int16_t* d_clips, int n_out, int32_t* d_peak);

/* ---- live keyword events (the decision layer of kws_scan_detect_f32 for the streams of kws_stream_open: one decision per
 * push, "keyword k fired on stream s at hop h" in a queue the host reads without a copy) -------------------------------------- */

/* Arm the open stream set for detection: from here to kws_stream_detect_close (or kws_stream_open / kws_stream_close /
 * kws_set_frontend, which drop it with the streams) every push that asks for logits -- kws_stream_push_i16,
 * kws_stream_push_host_i16, kws_stream_push_rate_i16, kws_stream_push_host_rate_i16 -- enqueues ONE more launch behind its own
 * (with use_graph: behind the replay, outside the captured graph): the decision step, one workgroup, fed with that push's
 * d_logits [n_streams, C].  A push's logits and labels are the bits of an unarmed push; an unarmed context launches nothing new.
 *   The rules are kws_scan_detect_f32's, with stream s as recording s and decision d as window d; decisions count d = 0, 1, ...
 *   from this call.  (1) p = the softmax of the stream's logits (the bits of kws_softmax_f32), stored at slot d mod smooth_window
 *   of a ring float32 [n_streams, smooth_window, C].  (2) s[c] = the sum of the last min(smooth_window, d + 1) posteriors,
 *   oldest first, in float32, divided by their number as a float: a direct sum at every decision, no running sum -- the bits
 *   of kws_scan_detect_f32's d_smoothed for the same logits (kws_stream_smooth_f32 keeps a running sum and gives other bits).
 *   (3) k = the first argmax of s; the stream is a candidate when k >= first_keyword and s[k] >= threshold (a NaN row is none);
 *   a candidate with d >= next[s] is an EVENT and sets next[s] = d + refractory (next starts at 0).  (4) EMIT: the streams that
 *   fired at this step get consecutive sequence numbers in ascending stream order (wavefront ballots and a prefix over the
 *   wavefronts; no atomics: the same bits run to run).  A record is int64 [5] = (stream, d, h, label k, score), the score being
 *   the bits of the float s[k] in the low 32 bits; h is the context's hop count (kws_stream_state's hops, from 1) of the push
 *   that decided, d for explicit steps.  Records are written at seq mod max_events to a device queue and to its mirror in
 *   pinned, device-mapped host memory (system-scope stores; the totals and then a completion count are published behind them,
 *   as kws_stream_utt_open describes).  The queue keeps the newest max_events records; older ones are overwritten.
 *   first_hop: a push whose hop count h is below first_hop decides nothing and advances nothing.  With first_hop = num_frames +
 *   K - 1 (K = ceil(frame_len / frame_step)) the windows that still hold zero rows are skipped, and decision d of a set armed
 *   right after kws_stream_open is window d of kws_scan_i16 at hop_frames = 1; with 0 every push decides.
 *   A push WITHOUT logits on an armed context, a push on a set that kws_stream_detect_step_f32 has stepped, and a push whose
 *   model has another class count than C are refused (KWS_ESTATE, KWS_ESTATE, KWS_EINVAL) -- behind the push's own launches:
 *   the hop has been taken, no decision is made.
 *   Needs an open stream set (else KWS_ESTATE).  KWS_EINVAL: C outside [1, 64]; smooth_window outside [1, 256]; refractory < 1;
 *   first_keyword < 0; first_hop < 0; max_events < n_streams (all streams may fire at one step).  n_streams > 1024:
 *   KWS_EUNSUPPORTED.  Waits for the context stream, allocates; a second call replaces the first.  Independent of
 *   kws_stream_smooth_f32, kws_stream_vad_f32 and kws_stream_utt_*, whose state it neither reads nor changes; armed together
 *   with kws_stream_utt_open a push is followed by two step launches.  No entry below allocates. */
int kws_stream_detect_open(kws_ctx* ctx, int C, int smooth_window, int first_keyword, float threshold, int refractory, int first_hop,
                           int max_events);
/* Waits for the context stream and releases what kws_stream_detect_open allocated; nothing when the context is not armed. */
int kws_stream_detect_close(kws_ctx* ctx);
/* The explicit step, for callers with their own model (and the tests): one decision per stream from d_logits float32
 * [n_streams, C] (device), whatever first_hop says; the record's h is d.  KWS_EINVAL: a NULL pointer.  KWS_ESTATE: the context
 * is not armed, or a push has stepped this armed set (the set has ONE decision counter; see above for the other direction). */
int kws_stream_detect_step_f32(kws_ctx* ctx, const float* d_logits);
/* Wait until the step of the newest enqueued push or explicit step has landed: spins on the completion count in host memory and
 * falls back to the stream after ~2 ms (as kws_stream_utt_poll); returns at once on a set with nothing enqueued.
 * *total_events: records emitted since kws_stream_detect_open; *decisions: decisions made (either may be NULL).  Not armed:
 * KWS_ESTATE. */
int kws_stream_detect_poll(kws_ctx* ctx, uint64_t* total_events, uint64_t* decisions);
/* Copy records first_seq .. first_seq + n - 1 out of the host mirror: out_records int64 [n, 5] (host).  Waits for nothing:
 * sequence numbers at or beyond the total that has landed, and ones no longer in the queue (seq + max_events < total, checked
 * again after the copy), are KWS_EINVAL, as are n < 1 and a NULL pointer.  Not armed: KWS_ESTATE. */
int kws_stream_detect_read(kws_ctx* ctx, uint64_t first_seq, int n, int64_t* out_records);
/* The newest decision's smoothed posteriors and their first argmax (zeros before the first decision): d_smoothed float32
 * [n_streams, C] and d_label int32 [n_streams] (device), two asynchronous copies on the context stream behind every earlier
 * push.  For inspection; the events need neither.  KWS_EINVAL: a NULL pointer.  Not armed: KWS_ESTATE. */
int kws_stream_detect_smoothed(kws_ctx* ctx, float* d_smoothed, int32_t* d_label);

/* ---- sample-rate conversion on the device (replaces the resampling inside librosa.load(path, sr=...),
 * kws/libs/audio_processor.py:120,145; PARITY UNPINNED against librosa's soxr: what is pinned is the project's own host
 * definition, scipy.signal.resample_poly(x, up, down, window=("kaiser", 14.0)) with zero padding, in float64) ---------------- */

/* The definition.  g = gcd(rate_in, rate_out), up = rate_out / g, down = rate_in / g, M = max(up, down), half = 10 * M.
 *   Taps h[j], j = 0 .. 2 * half, float64 = firwin(2 * half + 1, 1 / M, window=("kaiser", 14.0)) * up: with n = j - half,
 *   h0 = (1 / M) * sinc(n / M) * I0(14 * sqrt(1 - (n / half)^2)) / I0(14) and h = up * h0 / sum(h0).
 *   A recording of n_valid samples has the natural length n_nat = ceil(n_valid * up / down), and for k < n_nat
 *     y[k] = sum over m of x[m] * h[half + k * down - m * up],   0 <= m < n_valid, tap index in [0, 2 * half]
 *   -- at most ceil((2 * half + 1) / up) terms (61 for 48 -> 16 kHz, 56 for 44.1 -> 16 kHz, 21 for 8 -> 16 kHz).
 * Limits: max(up, down) <= 1024, KWS_EUNSUPPORTED beyond (8 / 11.025 / 22.05 / 32 / 44.1 / 48 / 96 / 192 kHz -> 16 kHz all fit;
 * the largest table, 640 / 441, holds 12 801 float64 taps, 100 KB); n_in and n_out at most 2^30 and at most 2^31 - 1 workgroups
 * (R * ceil(n_out / outputs_per_workgroup)) per call, KWS_EUNSUPPORTED beyond.
 *
 * kws_resample_i16 / kws_resample_f32: d_in [R, n_in] -> d_out [R, n_out] (device), n_out of the caller's choosing.
 *   d_len: int32 [R] on the device or NULL.  Recording r has len[r] valid samples, clamped to [0, n_in]; NULL: n_in for all.
 *   Samples at or beyond len[r] count as zero whatever the row holds there.  Output k < min(n_out, n_nat(r)) is y[k]; output
 *   k >= n_nat(r) is written as zero.  So n_out = the clip length performs fix_length after resampling, the reference's order
 *   (audio_processor.py:145,148), and a ragged batch needs one launch; kws_host_resample_len gives the natural length.
 *   Arithmetic: products and sums in float64 with the float64 taps read from a device table; each output is ONE chain of
 *   fused multiply-adds over its terms in a fixed order (newest sample first), with zeros where its span leaves [0, len).  An
 *   output's bits depend on its own input span and the rate pair alone: not on R, n_in, n_out, the row, or where k falls in
 *   the launch.  _f32 rounds the sum to float32.  _i16 sums in int16 units without scaling, clamps to [-32768, 32767] and rounds
 *   to nearest, ties to even.  rate_in == rate_out is a copy under the same d_len / n_out rules.
 *   Design cache: the context designs a pair's table on its first use -- float64 on the host, then an upload -- and keeps the
 *   eight pairs used last; a first use therefore drains the stream and allocates, and is NOT for stream capture.  kws_destroy
 *   frees the tables.  The calls need neither a front end nor a model.
 *   R < 1, n_in < 1, n_out < 1, a rate < 1, a NULL d_in / d_out: KWS_EINVAL.  Timed under KWS_K_RESAMPLE.  Asynchronous on the
 *   context stream; no atomics, so two runs give the same bits. */
int kws_resample_i16(kws_ctx* ctx, const int16_t* d_in, int R, int n_in, const int32_t* d_len, int rate_in, int rate_out,
                     int16_t* d_out, int n_out);
int kws_resample_f32(kws_ctx* ctx, const float* d_in, int R, int n_in, const int32_t* d_len, int rate_in, int rate_out,
                     float* d_out, int n_out);

/* ---- streaming sample-rate conversion: the resampler above with state, for live audio that arrives in pieces ----------------
 * up, down, M, half, the taps h and their device table are those of kws_resample_*; rows = ceil((2 * half + 1) / up).
 * The definition.  All streams of a context advance in lockstep.  A stream's signal x[m] is zero for m < first_sample and grows
 *   by n_in samples per push.  For EVERY integer k, negative ones included,
 *     y[k] = sum over m of x[m] * h[half + k * down - m * up]
 *   evaluated as kws_resample_* evaluates it: newest sample q = floor((half + k * down) / up) first, `rows` fused float64
 *   multiply-adds from 0.0 with the taps h[phase + i * up], phase = (half + k * down) - q * up, the table's padded zeros
 *   included; the division and the remainder round towards minus infinity.
 *   Delay: d = ceil(half / down) output samples -- 10 whenever down >= up (0.625 ms at 16 kHz), 20 for 8 -> 16 kHz, 15 for 44.1 ->
 *   64 kHz.  Absolute output j is y[j - d], stored as kws_resample_i16 stores (clamped to int16, rounded to nearest even).  With P
 *   samples received in all (first_sample counts as received) the outputs j < floor(P * up / down) have been emitted: a push from
 *   P0 to P1 emits floor(P1 * up / down) - floor(P0 * up / down) samples, a number the host computes -- nothing is read back.
 *   With this d every emitted output's span lies inside the samples already pushed, so its bits are those kws_resample_i16 gives
 *   the whole signal at index j - d (front-padded by a multiple of down zeros to reach the pre-ringing before the onset).
 *   Equal rates are a copy: d = 0 and every push emits n_in samples.
 *   first_sample must be a multiple of down; the first output index is then the integer first_sample / down * up and the bits
 *   are those of first_sample = 0.  Positions are kept in 64 bits (first_sample below 2^62): 2^31 samples are 12 hours at 48 kHz.
 * State: the last H = rows - 1 + ceil((d * down + down - 1 - half) / up) samples per stream (62 at 48 -> 16 kHz, 58 at 44.1 ->
 *   16 kHz, 20 at 8 -> 16 kHz), which is exactly what the outputs of the next push can reach back to.
 * Limits: max(up, down) <= 1024 and H + max_in <= 6144 (a workgroup stages history and input in LDS as float64), KWS_EUNSUPPORTED
 *   beyond; equal rates have no such limit.
 *
 * kws_host_stream_resample_plan (no GPU): the reduced pair, d and H; any pointer may be NULL.
 * kws_host_stream_resample_count (no GPU): *n_out = what a push of n_in >= 0 samples emits after samples_before samples.
 *   Both: a rate < 1 (or a NULL n_out, n_in < 0): KWS_EINVAL; max(up, down) > 1024: KWS_EUNSUPPORTED.
 * kws_stream_resample_open: state for n_streams streams and pushes of at most max_in samples; needs neither a front end nor a
 *   model.  Designs the pair through the design cache of kws_resample_* (drains the stream: NOT for stream capture), zeroes the
 *   history.  A second open replaces the state; kws_stream_resample_close and kws_destroy free it.  n_streams < 1, max_in < 1, a
 *   rate < 1, first_sample not a multiple of down: KWS_EINVAL.
 * kws_stream_resample_i16: d_in [n_streams, n_in] -> d_out [n_streams, out_cap] (row stride out_cap), both on the device and
 *   not overlapping.  *n_out (host) is set before the launch; out_cap < *n_out is KWS_EINVAL with nothing done.  One launch:
 *   one workgroup per stream up to 1024 outputs per stream, one per 1024 outputs beyond; the history is double-buffered, so
 *   no workgroup reads what another writes.  NULL pointers, n_in < 1 or > max_in: KWS_EINVAL; no open: KWS_ESTATE.  Not timed
 *   by kws_prof_*.  Asynchronous on the context stream; no atomics.
 * kws_stream_push_rate_i16: resample one push into a hop buffer the context owns, then kws_stream_push_i16(ctx, hop, d_logits,
 *   d_label, 0).  Needs kws_stream_open with the same n_streams and rate_out == the front end's sample rate (KWS_ESTATE
 *   otherwise); the push must emit exactly frame_step samples, else KWS_EINVAL with no state touched (48 kHz: 480 in, 44.1 kHz:
 *   441 in, 8 kHz: 80 in for the default hop of 160).  If the streaming push refuses, the resampler's state steps back.
 * kws_stream_push_host_rate_i16: the same from host memory -- h_in [n_streams, n_in] is copied into pinned, device-mapped
 *   memory of n_streams * max_in samples, the resampler reads it from there -- with the results delivered as
 *   kws_stream_push_host_i16 delivers them (kws_stream_host_results / kws_stream_wait_host). */
int kws_host_stream_resample_plan(int rate_in, int rate_out, int* up, int* down, int* delay_out, int* history);
int kws_host_stream_resample_count(int rate_in, int rate_out, uint64_t samples_before, int n_in, int* n_out);
int kws_stream_resample_open(kws_ctx* ctx, int n_streams, int rate_in, int rate_out, int max_in, uint64_t first_sample);
int kws_stream_resample_close(kws_ctx* ctx);
int kws_stream_resample_i16(kws_ctx* ctx, const int16_t* d_in, int n_in, int16_t* d_out, int out_cap, int* n_out);
int kws_stream_push_rate_i16(kws_ctx* ctx, const int16_t* d_in, int n_in, float* d_logits, int32_t* d_label);
int kws_stream_push_host_rate_i16(kws_ctx* ctx, const int16_t* h_in, int n_in, const float** h_logits, const int32_t** h_label);

/* ---- resetting single streams of a live set (build-defined: the reference handles ONE microphone, one capture at a time --
 * kws/inference/inference_local.py:114-192 opens the device, records until the VAD closes, classifies and starts over; it has no
 * set of streams whose members come and go) -----------------------------------------------------------------------------------
 * streams: host int32 [n], indices into the open set; duplicates are allowed.  Enqueued on the context's stream between two
 * pushes: no host synchronisation, no device allocation after the set's first reset, and the indices travel inside the launch
 * (a 1024-bit mask per 1024 streams), so the array may be reused as soon as the call returns.
 * From the next push on, each named stream behaves AS IF IT HAD RECEIVED DIGITAL SILENCE (all-zero samples) EVER SINCE
 * kws_stream_open; what is armed on the set starts over for it.  Every other stream is untouched, bit for bit, and the set's
 * counters run on (hops, frames walked, decisions made, samples appended): records stay in set coordinates, and a stream's own
 * time is the set's minus the hop count at its reset.  Per layer, h0 = pushes so far, K = ceil(frame_len / frame_step):
 *   PCM ring, both halves of the streaming resampler's history: zeros (the resampler's position and phase are the set's and stay).
 *   feature ring: the rows of the frames a silent stream would hold -- frames 0 .. h0 - K, frame f in row f mod num_frames -- get the
 *     row the streaming frame kernel writes for an all-zero frame (taken from that kernel, once per open set, on a scratch set
 *     of one stream; kws_frontend_stats does not move); every other row is zero.  The frames that straddle the reset then come
 *     out of the unchanged frame code as "silence, then the new audio".
 *   kws_stream_utt_*: an utterance open on the stream closes at the newest walked frame with reason 2, as kws_stream_utt_flush
 *     closes it, and is queued (one more step of that queue for kws_stream_utt_poll); flags, window counts and the open frame are
 *     cleared and the previous close is set to hops appended - 1, so no later utterance of the stream starts before the first
 *     sample pushed after the reset.  The history ring stays: utterances closed before the reset remain cuttable.
 *   kws_stream_detect_*: the stream's causal mean runs over the decisions since the reset only (at most smooth_window of them,
 *     same order of addition), its refractory wait is cleared; first_hop stays a gate of the set; queued events stay.
 *   kws_stream_vad_f32: the stream's flags and window counts are cleared.
 *   kws_stream_smooth_f32: while its history is live the reset is REFUSED with KWS_EUNSUPPORTED before anything changes -- that
 *     smoother keeps a running sum and one hop count for all streams; use kws_stream_detect_*.
 * Nothing to reset: the zero-copy result arrays, the time-tile partial sums, the refinement counters, a captured push graph (the
 * reset is a launch outside it; the next replay works on the reset rings).
 * n == 0: KWS_OK, nothing is launched.  KWS_EINVAL, nothing changed: an index outside [0, n_streams), streams == NULL with
 * n > 0, n < 0.  KWS_ESTATE: no open set. */
int kws_stream_reset(kws_ctx* ctx, const int32_t* streams, int n);

/* ---- sparse live sets: streams that leave the set and join it again (build-defined, as the reset above) ------------------------
 * After kws_stream_open every stream is ACTIVE, and a set in which no stream was ever deactivated launches exactly what it
 * launched before these entries existed.  An INACTIVE stream takes no part in anything a push does: its row of the hop buffer
 * is not read (its content may be anything) -- EXCEPT by kws_stream_push_rate_i16 / kws_stream_push_host_rate_i16, whose
 * resampler kernel keeps running over every slot and so READS the idle rows of its input (they must be readable memory; what
 * they hold does not matter, an idle stream's resampler history is zeroed when it is activated) --; its PCM ring, feature ring,
 * endpointer state and posterior ring are not written; its rows of d_logits, d_label and of the zero-copy host arrays are not
 * written and keep what they held; it emits no utterance and no event.  The set's clocks run on: the hop counter, the push
 * count, the utterance unit's frame and append counters, the event unit's decision counter.  The fused push then launches
 * workgroups for the active streams alone, and unless kws_stream_cluster pinned it the default time-tile cluster follows the
 * ACTIVE count (4 up to 64, 2 up to 128, else 1).  A push with no active stream is legal: the hop counter advances, the
 * zero-copy flag is raised, the armed steps tick.
 * kws_stream_deactivate: an utterance open on a named stream closes with reason 2, exactly as kws_stream_reset closes it (its
 *   span stays cuttable); the stream then leaves the set.  Naming an inactive stream is a no-op.
 * kws_stream_activate: the named streams get the whole of kws_stream_reset -- rings, silence rows, resampler history, endpointer
 *   state, the utterance start-over with the previous close at hops appended - 1, the event epoch and refractory wait -- and
 *   then join.  On an active stream it is a plain reset.
 * Both are enqueued on the context's stream between two pushes, with no host synchronisation and no allocation after the set's
 * first deactivation; streams (host int32 [n], duplicates allowed) travels inside the launches.  Checks and codes are
 * kws_stream_reset's: n == 0 KWS_OK; KWS_EINVAL with nothing changed for an index outside [0, n_streams), NULL with n > 0,
 * n < 0; KWS_ESTATE without an open set; KWS_EUNSUPPORTED, before anything changes, while kws_stream_smooth_f32's history is live.
 * kws_stream_active: the host's own record -- no device work, no wait.  out: uint8 [n_streams], 1 = active, or NULL;
 *   n_active: the count, or NULL.
 * Served while some stream is inactive: kws_stream_push_i16 with logits on the product maths (KWS_PW_SPLIT_BF16,
 * KWS_PW_PAIR_F16) without use_graph, kws_stream_push_host_i16, kws_stream_wait_host, both rate pushes, live utterances and live
 * events armed on the set with their poll / read / cut / flush / smoothed entries, kws_stream_state, kws_stream_copy_features,
 * and kws_stream_reset (a no-op on an inactive stream).  REFUSED with KWS_EUNSUPPORTED while any stream is inactive, before any
 * launch and with no hop taken: features-only pushes (d_logits == NULL) and the diagnostic pointwise maths, use_graph,
 * kws_stream_push_cnn_trad_i16, kws_stream_vad_f32, kws_stream_utt_step_i16, kws_stream_detect_step_f32 -- each is a kernel of
 * its own over every slot.  kws_stream_open and kws_stream_close restore "all active". */
int kws_stream_deactivate(kws_ctx* ctx, const int32_t* streams, int n);
int kws_stream_activate(kws_ctx* ctx, const int32_t* streams, int n);
int kws_stream_active(kws_ctx* ctx, uint8_t* out, int* n_active);

/* ---- evaluation statistics on the device (build-defined: the reference computes them on the host, with a
 * round trip per batch -- running_loss += loss.item(), torch.max(outputs, 1), (predicted == labels).sum().item() in
 * train.py:51-54,79-98 and kws/libs/training.py:300-303,347-393 -- and test.py:27-58 derives the per-class report, the
 * one-vs-rest ROC curves and the false-alarm / false-reject rates from posteriors copied to the host) ------------------------ */

/* The context holds ONE evaluation state: integer accumulators in device memory, updated by any number of batches and read
 * back once.  kws_eval_open allocates and zeroes it for num_classes C in [1, 64] and n_bins K, a power of two in [2, 1024] or 0
 * for no histograms (anything else: KWS_EINVAL); a second open replaces the state; kws_destroy frees it.  kws_eval_reset zeroes
 * it (asynchronous on the context stream); kws_eval_close frees it.  Before an open, reset / update / read return KWS_ESTATE. */
int kws_eval_open(kws_ctx* ctx, int num_classes, int n_bins);
int kws_eval_reset(kws_ctx* ctx);
int kws_eval_close(kws_ctx* ctx);

/* One batch into the statistics: d_logits float32 [B, C], d_truth int32 [B] (device pointers), any B >= 1; asynchronous on the
 * context stream, two launches, not timed by kws_prof_* (as kws_scan_detect_f32).  Per row b:
 *   - a truth outside [0, C) makes the row IGNORED: counted in counts[2], nothing else; the label is never used as an index;
 *   - else a NaN or infinite logit makes the row NON-FINITE: counted in counts[3], nothing else;
 *   - an ignored or non-finite row gets zeros in d_dlogits and d_loss_rows;
 *   - every other row: p[c] = the value kws_softmax_f32 writes for the row, bit for bit (the same device function); row loss
 *     l = logf(sum) + m - z[truth] in float32 with the maximum m and the sum of expf(z - m) of that softmax (the cross-entropy
 *     of nn.CrossEntropyLoss, train.py:48); pred = first argmax of the logits (torch.max, training.py:371);
 *     confusion[truth][pred] += 1; counts[1] += (pred == truth); counts[0] += 1; with K > 0, for every class c,
 *     bin = min(K - 1, (int)(p[c] * K)) (the product is exact) and hist_pos[c][bin] += 1 when truth == c, else
 *     hist_neg[c][bin] += 1 -- the counts behind roc_curve(y_test[:, c], y_score[:, c]) of test.py:38 at thresholds j / K;
 *     d_loss_rows[b] = l and d_dlogits[b][c] = (p[c] - (c == truth)) * grad_scale where the pointers are not NULL.
 *     grad_scale = 1 / B gives the gradient of nn.CrossEntropyLoss() at its default mean reduction: the d_dlogits that
 *     kws_dscnn_backward_f32 / kws_cnn_trad_backward_f32 take.  grad_scale is only read when d_dlogits is given.
 * All counters are integers (private 32-bit counters per workgroup in LDS where the 2 C K histogram counters fit, 64-bit atomics
 * into the accumulators), so they do not depend on the order of execution.  loss_sum is a float64 sum of the float32 row
 * losses in an order that depends only on B and on the sequence of calls (per-workgroup partials, added in index order; no
 * float atomics): the same updates after a reset give a bit-identical loss_sum.
 * NULL d_logits / d_truth or B <= 0: KWS_EINVAL. */
int kws_eval_update_f32(kws_ctx* ctx, const float* d_logits, const int32_t* d_truth, int B, float grad_scale, float* d_dlogits,
                        float* d_loss_rows);

/* Waits for the context stream and copies the statistics to HOST memory; any pointer may be NULL.  counts[4] = rows used, rows
 * correct, rows ignored, rows non-finite; loss_sum: one float64, the sum of the used rows' losses; confusion [C][C], row =
 * truth, column = prediction; hist_pos and hist_neg [C][K] each (not written when K is 0). */
int kws_eval_read(kws_ctx* ctx, uint64_t* counts, double* loss_sum, uint64_t* confusion, uint64_t* hist_pos, uint64_t* hist_neg);

/* ---- augmentation of the training transform (kws/libs/audio_processor.py:151-159,172-233) ---------- */

/* out[b][i] = (silence[b] ? 0 : wav[b][i - shift[b]] / 32768, 0 outside the clip) + bg_vol[b] * bg[bg_off[b] + i]
 * as float32 [B, n_samples], ready for kws_mfcc_f32.  d_shift int32 [B] (NULL: no shift), d_bg float32
 * [bg_len] background pool (NULL: no mix) with per-clip offsets int32 [B] and volumes float32 [B],
 * d_silence uint8 [B] (NULL: none).  The random draws stay with the caller (host), as in the reference. */
int kws_augment_i16(kws_ctx* ctx, const int16_t* d_wav, int B, const int32_t* d_shift, const float* d_bg, int bg_len,
                    const int32_t* d_bg_off, const float* d_bg_vol, const uint8_t* d_silence, float* d_out);

/* ---- resident training loader: draws and features on the device ------------------------------------------
 * Together the two entries replace the reference's per-sample transform inside DataLoader workers
 * (kws/libs/data_loader.py:96-105 under train.py:108-121) for a split whose PCM lives in device memory. */

/* The label of a silence clip (kws/common/types.py: LabelIndex.SILENCE_INDEX). */
#define KWS_SILENCE_INDEX 0

/* The four random draws of the training transform (kws/libs/audio_processor.py:151-159, 172-233) for the B dataset
 * indices d_index int32 [B]: time shift, background file, offset inside it, volume.
 *   Generator: Philox4x32-10, key = seed (low word, high word), counter = (dataset index, epoch, 0, 0); one call gives
 *   a clip's four words.  A clip's draws are therefore a pure function of (seed, epoch, dataset index): they do not
 *   depend on B, on the other clips of the batch or on the order inside it.
 *   Word -> integer in [0, m): (uint64(u) * m) >> 32.  Word -> float in [0, 1): (u >> 8) * 2^-24.
 *   word 0: shift uniform on the integers [-time_shift, time_shift) (0 when time_shift is 0);
 *   word 1: file k uniform on [0, K);  word 2: offset = d_bg_start[k] + uniform on [0, d_bg_len[k] - n_samples)
 *           (d_bg_start / d_bg_len int32 [K]: where the pool's files, already tiled beyond n_samples, begin and how long
 *           they are);
 *   word 3: u.  A silence clip (d_label[index] == KWS_SILENCE_INDEX; d_label int32 [N] or NULL: no silence clips) gets
 *           volume u, uniform on [0, 1).  Any other clip gets (u / bg_frequency) * bg_volume when u < bg_frequency -- given
 *           that, u / bg_frequency is uniform on [0, 1) again, so the volume is uniform on [0, bg_volume) with probability
 *           bg_frequency -- else 0 (two float32 roundings: the divide, the multiply).
 *   use_background == 0 mixes noise into silence clips only (audio_processor.py:158); such a clip's other draws, and
 *   every clip's when K == 0, are offset 0 and volume 0.  The distributions are the reference's; its stream of numbers
 *   (NumPy's global state per worker) is not reproducible and is not reproduced.
 * Outputs d_shift int32 [B], d_bg_off int32 [B], d_bg_vol float32 [B], d_silence uint8 [B] have exactly the meaning of
 * kws_augment_i16's arguments.  An index outside [0, N) reads no label.  B <= 0, a NULL index or output pointer, K > 0
 * without its tables, time_shift < 0: KWS_EINVAL.  Asynchronous on the context stream. */
int kws_augment_draw(kws_ctx* ctx, uint64_t seed, uint32_t epoch, const int32_t* d_index, int B, const int32_t* d_label, int N,
                     int time_shift, const int32_t* d_bg_start, const int32_t* d_bg_len, int K, float bg_volume,
                     float bg_frequency, int use_background, int n_samples, int32_t* d_shift, int32_t* d_bg_off,
                     float* d_bg_vol, uint8_t* d_silence);

/* Gather + augment + MFCC in one launch (plus the refinement launch): batch row b is clip d_index[b] of the resident
 * split d_pcm int16 [N, n_samples], augmented as kws_augment_i16 would with the b-th entries of d_shift / d_bg_off /
 * d_bg_vol / d_silence (same NULL conventions), and transformed to d_out float32 [B, 1, num_frames, numcep].  No
 * intermediate signal reaches memory.  The result is bit-identical to gathering the rows, kws_augment_i16 and
 * kws_mfcc_f32, refinement and kws_frontend_stats included.
 *   Scope: KWS_FE_F32 at a geometry the wavefront-resident int16 kernel covers (the reference's: frames of 385..448
 *   samples, n_samples and 4 * frame_step multiples of 8, d_pcm 16-byte aligned).  Anything else, KWS_FE_F64 included:
 *   KWS_EUNSUPPORTED -- compose the three calls instead.  B <= 0, N <= 0, a NULL d_pcm / d_index / d_out, a pool without
 *   length, offsets and volumes: KWS_EINVAL.
 *   An index outside [0, N) is never dereferenced: row 0 is read instead and that batch row's output is unspecified.
 * Asynchronous on the context stream. */
int kws_mfcc_augment_i16(kws_ctx* ctx, const int16_t* d_pcm, int N, const int32_t* d_index, int B, const int32_t* d_shift,
                         const float* d_bg, int bg_len, const int32_t* d_bg_off, const float* d_bg_vol,
                         const uint8_t* d_silence, float* d_out);

/* Diagnostics: the same forward with per-clip shader-clock stamps (s_memtime of thread 0) at the phase
 * boundaries of the DS-CNN kernel, uint64 [B, KWS_DSCNN_STAMPS]: 0 start, 1 features staged, 2/3 conv1
 * done / barrier, 4/5 .. 10/11 blocks 1..4 done / barrier, 12 end; [14], [15] = 100 MHz real-time
 * counter at start / end.  mode: KWS_PW_SPLIT_BF16 (4) / KWS_PW_F32 (1) = the matrix-core kernels, 0 = VALU
 * cross-check variant, 2 / 3 = timing ablations of the f32 kernel (matrix core only / stencil only), 6 = of
 * the split kernel (no stencil): wrong results by construction.  Never used on the product path. */
#define KWS_DSCNN_STAMPS 16
int kws_forward_stamps_f32(kws_ctx* ctx, const float* d_feat, int B, float* d_logits, uint64_t* d_stamps, int mode);

/* ---- sigproc operators (kws/libs/speech_features/sigproc.py) -------------------------------- */

/* preemphasis(signal, coeff) (sigproc.py:93-103), float32 [n] -> float32 [n]. */
int kws_preemphasis_f32(kws_ctx* ctx, const float* d_signal, int n, float coeff, float* d_out);
/* framesig(signal, frame_len, frame_step, winfunc) (sigproc.py:14-52): d_window float32 [frame_len]
 * or NULL for rectangular; d_frames float32 [num_frames, frame_len], num_frames as kws_frontend_shape. */
int kws_framesig_f32(kws_ctx* ctx, const float* d_signal, int n, int frame_len, int frame_step,
                     const float* d_window, float* d_frames);
/* magspec / powspec (sigproc.py:55-90) with NFFT = 512: d_frames float32 [num_frames, frame_len]
 * (frame_len <= 512 is zero-padded, > 512 truncated) -> float32 [num_frames, 257];
 * power != 0 gives 1/NFFT * |X|^2, power == 0 gives |X|. */
int kws_spec512_f32(kws_ctx* ctx, const float* d_frames, int num_frames, int frame_len, int power,
                    float* d_spec);

/* The same for any NFFT (sigproc.py:55-90 takes any): NFFT == 512 runs the kernel above, any other length -- a power of
 * two in [64, 4096] or any value in [2, 2048] -- a float64 transform (FFT / direct DFT) with float32 output. */
int kws_spec_f32(kws_ctx* ctx, const float* d_frames, int num_frames, int frame_len, int nfft, int power, float* d_spec);

/* ---- measurement --------------------------------------------------------------------------- */

/* Per-kernel device timing with HIP events on the context's stream.  kws_prof_enable(ctx, on): 0 = off, 1 = every
 * kernel launch is bracketed by events, n > 1 = every n-th launch of each kernel id is (a pair of events costs the
 * stream ~7 us: 2 % of a 4096-clip step, 8 % of a 1024-clip one, when every launch carries one); kws_prof_read
 * synchronises and returns the summed milliseconds and the number of TIMED launches per kernel id since the last
 * kws_prof_reset.  The kernels of an eager kws_stream_push_i16 are timed
 * too (KWS_K_DSCNN for the one-launch push; KWS_K_STREAM_FRAME + KWS_K_DSCNN for the two-launch routes); a push replayed
 * as a hipGraph is not (events cannot bracket a node). */
enum { KWS_K_MFCC = 0, KWS_K_DSCNN = 1, KWS_K_CNNTRAD_CONV = 2, KWS_K_CNNTRAD_DENSE = 3, KWS_K_STREAM_FRAME = 4, KWS_K_MFCC_F64 = 5, KWS_K_MFCC_REFINE = 6,
       KWS_K_DSCNN_LOAD_STATS = 7, KWS_K_DSCNN_LOAD_PACK = 8, KWS_K_DSCNN_LOAD_FILL = 9, /* the launches of kws_load_dscnn_device */
       KWS_K_RESAMPLE = 10,                                                              /* kws_resample_i16 / kws_resample_f32 */
       KWS_K_COUNT = 11 };
int kws_prof_enable(kws_ctx* ctx, int on);
int kws_prof_reset(kws_ctx* ctx);
int kws_prof_read(kws_ctx* ctx, int kernel_id, double* total_ms, int* launches);
/* Name of the device kernel behind a kernel id (as it appears in rocprofv3 traces). */
const char* kws_kernel_name(int kernel_id);

/* ---- host-only helpers (no GPU needed; used by the CPU test-suite) -------------------------- */

/* nfilt+2 mel bin edges exactly as psf get_filterbanks computes them. */
int kws_host_mel_edges(int nfilt, int nfft, int sample_rate, int* edges_out);
/* Dense float32 [nfilt, nfft/2+1] filterbank expanded from the sparse per-lane tables the kernel
 * uses (so the sparse decomposition can be checked against the oracle's dense matrix on CPU). */
int kws_host_mel_dense(int nfilt, int nfft, int sample_rate, float* fb_out);
/* Lane layout of the sparse mel evaluation: for each of the nfilt+1 inter-edge segments the first lane and the number
 * of lanes (chunks of 8 bins) it occupies; *lanes_used = lanes in use including idle padding; *row_safe = 1 when no
 * segment straddles a 16-lane DPP row (the kernel then shifts with row_shl operands).  first_lane_out / n_lanes_out
 * hold nfilt+1 ints; lanes_used / row_safe may be NULL. */
int kws_host_mel_layout(int nfilt, int nfft, int sample_rate, int* first_lane_out, int* n_lanes_out, int* lanes_used, int* row_safe);
/* float32 [numcep, nfilt] DCT-II(ortho) x lifter table the kernel uses. */
int kws_host_dct_lifter(int nfilt, int numcep, int ceplifter, float* out);
/* The device image of a model as 32-bit words, exactly as kws_load_dscnn_ex / kws_load_cnn_trad upload it for the same
 * blob, built on the host alone.  *need_words (may be NULL) receives the image's size; out_words == NULL only asks for
 * that size, a cap_words below it is KWS_EINVAL; the blob is checked as by the loaders.  scalars (may be NULL) receives
 * the values the context keeps by value:
 *   kws_host_dscnn_image    float[23]: k_c1, k_pw[4] (the weight-scale exponents), c1_abs, c1_bmax, dw_abs[4], dw_bmax[4],
 *                           pw_abs[4], pw_bmax[4] (the bounds behind the per-clip activation scales)
 *   kws_host_cnn_trad_image float[7]:  1/sw of conv1, conv2, lin; w1_abs, b1_max, w2_abs, b2_max */
int kws_host_dscnn_image(const float* blob, size_t n_floats, int num_classes, int input_channels, uint32_t* out_words,
                         size_t cap_words, size_t* need_words, float* scalars);
int kws_host_cnn_trad_image(const float* blob, size_t n_floats, int num_classes, uint32_t* out_words, size_t cap_words,
                            size_t* need_words, float* scalars);
/* The unit descriptor table every DS-CNN load places behind the device image, for the persistent batched forward (more clips
 * than CUs): the per-lane geometry of each (block, tile) unit of the four depthwise-separable blocks on the [1,99,10] map, read
 * by the f16-pair kernel instead of being recomputed for every clip.  It depends on the map geometry alone, not on the weights.  Words
 * [unit][part 2][lane 64][4], unit = unit_base[block - 1] + tile; part 0 = the LDS float indices of the lane's own-column taps in
 * rows h-1, h, h+1 (channel pair 8 * (lane >> 5)) and the store mask (all ones / all zeros); part 1 = the left and right
 * neighbour masks (1.0f / 0.0f) and two zero words.  Size protocol of kws_host_dscnn_image; unit_base (may be NULL) receives
 * five ints: the first unit of blocks 1..4 and the number of units. */
int kws_host_dscnn_units(uint32_t* out_words, size_t cap_words, size_t* need_words, int* unit_base);

/* Frames of a recording of n_total samples taken as one clip (*frames_total = 1 + ceil((n_total - frame_len) / frame_step),
 * 1 when n_total <= frame_len) and windows of a scan over it (*n_windows = (frames_total - window_frames) / hop_frames + 1,
 * rounded down; 0 when the recording is shorter than a window) -- the shapes of kws_scan_i16's outputs.  Either pointer may
 * be NULL.  Non-positive sizes: KWS_EINVAL. */
int kws_host_scan_shape(int n_total, int frame_len, int frame_step, int window_frames, int hop_frames, int* frames_total,
                        int* n_windows);

/* The plan of a ragged batch (see "batches of recordings of unequal length"): for R recordings of len[r] samples,
 * frames[r] = F_r and windows[r] = W_r exactly as kws_host_scan_shape gives them per recording; frame_off [R + 1] with each
 * recording's rows rounded up to a multiple of hop_frames (frame_off[R] = F_pack); win_off[r] = frame_off[r] / hop_frames;
 * *W_pack = the windows of the packed array scanned as one recording.  Any output pointer may be NULL.  A NULL len, R < 1,
 * a length < 1, hop_frames < 1 or another non-positive size: KWS_EINVAL.  R > 2^20 or F_pack > 2^28: KWS_EUNSUPPORTED. */
int kws_host_ragged_plan(const int32_t* len, int R, int frame_len, int frame_step, int window_frames, int hop_frames, int32_t* frames,
                         int32_t* frame_off, int32_t* windows, int32_t* win_off, int* W_pack);

/* Host side of kws_resample_* (no GPU).  kws_host_resample_len: *n_out = ceil(n_in * up / down), the natural length of n_in
 * samples (n_in >= 0).  kws_host_resample_design: the reduced pair, half (the taps number 2 * half + 1), the outputs one
 * workgroup of the kernel owns -- a recording's outputs are cut into tiles of that many from output 0, so tests can place
 * lengths on both sides of a tile edge -- and the taps h[0 .. 2 * half] exactly as the device table holds them (which appends
 * zeros up to a multiple of up).  *need (may be NULL) is always set to the number of taps; taps == NULL only asks for the
 * sizes, a cap below *need is KWS_EINVAL.  Any other pointer may be NULL.  A rate < 1: KWS_EINVAL; max(up, down) > 1024:
 * KWS_EUNSUPPORTED. */
int kws_host_resample_len(int n_in, int rate_in, int rate_out, int* n_out);
int kws_host_resample_design(int rate_in, int rate_out, int* up, int* down, int* half_len, int* outputs_per_workgroup,
                             double* taps, size_t cap, size_t* need);

#ifdef __cplusplus
}
#endif
#endif /* KWS_HIP_H */
