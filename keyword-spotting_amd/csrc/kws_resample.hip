// Sample-rate conversion on the device (include/kws_hip.h: kws_resample_i16 / kws_resample_f32, kws_host_resample_len,
// kws_host_resample_design): a Kaiser-windowed polyphase FIR, the host definition of kws/libs/audio_processor.py
// (scipy.signal.resample_poly with window=("kaiser", 14.0), zero padding) evaluated in float64.  Replaces the resampling inside
// librosa.load(path, sr=...) (audio_processor.py:120,145); parity against librosa's soxr is unpinned.
//
//   y[k] = sum over m of x[m] * h[half + k * down - m * up],   0 <= m < len, tap index in [0, 2 * half]
//
// Mapping: lane = consecutive output.  The other candidate, lane = outputs `up` apart, makes the taps wavefront-uniform but needs
// 64 * down input samples in LDS per wavefront and phase -- 64 * 441 float64 samples are 220 KB for the 44.1 kHz pairs, more than a
// CU has -- so it only suits the pairs that are degenerate anyway.  With consecutive outputs the stores coalesce, a tile's input
// span is tile * down / up + taps-per-output samples whatever the pair, and the LDS reads of a wavefront are down / up samples
// apart: 3 float64 for 48 -> 16 kHz (ds_read_b64 banks by (address / 4) mod 64 inside each half-wave, and 6 l mod 64 takes 32
// different even values for l = 0..31: conflict-free), the same address for lane pairs at 8 -> 16 kHz (a broadcast).
// Tap table: lane k needs h[phase_k + i * up] at step i, phase_k = (half + k * down) mod up.  The natural order of h IS the
// phase layout for this mapping -- row i holds the `up` phases of step i side by side -- so a wavefront's 64 tap reads of one step
// fall into one row of up * 8 bytes (ten 128-byte lines for up = 160).  Rows by phase ([phase][i]) would put the 64 reads into 64
// different lines.  The table is h followed by zeros up to rows * up entries, so every output runs the same `rows` steps.
// up == 1 (48 -> 16 kHz, 96 -> 16 kHz) has one phase: the instantiation UP1 drops the division and reads h[i] through an index
// that is uniform over the workgroup, which the compiler turns into scalar loads with the tap as an SGPR operand of the FMA.
// down == 1 (8 -> 16 kHz) runs the general instantiation: its two phases share one 16-byte piece of a row, one line per step.
//
// Every output is one chain of `rows` float64 FMAs in step order (the newest sample first) from 0.0, fed with zeros where the span
// leaves [0, len): its bits depend on its own input span and the pair alone.  No atomics, no fences, no device-side allocation.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "kws_ctx.h"

namespace kws {

constexpr int RS_MAX_RATIO = 1024;    // max(up, down)
constexpr int RS_ZEROS = 10;          // half = 10 * max(up, down): scipy.signal.resample_poly's half_len
constexpr double RS_BETA = 14.0;      // the project's window, ("kaiser", 14.0)
constexpr int RS_PER_THREAD = 4;      // outputs per thread, a workgroup's tile = 4 * its threads
constexpr int RS_LDS_SAMPLES = 6144;  // float64 samples a workgroup stages at most: 48 KB, three workgroups per CU
constexpr int RS_CACHE_PAIRS = 8;     // designs a context keeps

// What a rate pair needs on the host and the device.
struct ResamplePlan {
    int up = 1, down = 1, half = 0;
    int rows = 0;         // steps per output: ceil((2 half + 1) / up)
    int threads = 256;    // tile = RS_PER_THREAD * threads outputs per workgroup
    int span = 0;         // input samples a tile touches at most: (up - 1 + (tile - 1) down) / up + rows
    bool staged = false;  // the span fits RS_LDS_SAMPLES; otherwise the kernel reads global memory directly
    int tile() const { return RS_PER_THREAD * threads; }
};

struct ResampleDesign {
    ResamplePlan plan;
    DeviceBuffer<double> d_taps;  // [rows * up]: h, then zeros
    unsigned long long used = 0;
};

struct ResampleCache {
    std::vector<ResampleDesign> designs;
    unsigned long long clock = 0;
};

// The streaming resampler's plan and state (the derivation of d and H is with its kernel below).
struct StreamPlan {
    ResamplePlan plan;
    int delay = 0, hist = 0;  // d and H
    bool copy = false;        // equal rates
};

struct StreamResample : StreamPlan {
    int rate_in = 0, rate_out = 0;
    int n_streams = 0, max_in = 0;
    unsigned long long pos = 0;  // samples received, first_sample included
    DeviceBuffer<int16_t> d_hist;  // [2][n_streams][hist]: a push reads one half and writes the other
    int cur = 0;
    DeviceBuffer<int16_t> d_hop;   // [n_streams][frame_step]: the resampled hop of the fused push
    PinnedBuffer<int16_t> h_in;    // [n_streams][max_in], pinned and device-mapped: the input of kws_stream_push_host_rate_i16
};

namespace {

int gcd_int(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// KWS_OK, KWS_EINVAL (a rate below 1) or KWS_EUNSUPPORTED (max(up, down) beyond RS_MAX_RATIO).
int make_plan(int rate_in, int rate_out, ResamplePlan& p) {
    if (rate_in < 1 || rate_out < 1) return KWS_EINVAL;
    const int g = gcd_int(rate_in, rate_out);
    p.up = rate_out / g;
    p.down = rate_in / g;
    const int M = p.up > p.down ? p.up : p.down;
    if (M > RS_MAX_RATIO) return KWS_EUNSUPPORTED;
    p.half = RS_ZEROS * M;
    p.rows = (2 * p.half + p.up) / p.up;
    p.staged = false;
    p.threads = 64;
    for (int threads = 256; threads >= 64; threads /= 2) {
        const int span = (p.up - 1 + (RS_PER_THREAD * threads - 1) * p.down) / p.up + p.rows;
        if (span <= RS_LDS_SAMPLES) {
            p.threads = threads;
            p.staged = true;
            break;
        }
    }
    p.span = (p.up - 1 + (p.tile() - 1) * p.down) / p.up + p.rows;
    return KWS_OK;
}

// I0(x), the power series sum of ((x / 2)^k / k!)^2: all terms positive, so the sum carries a few ulps at most.
double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}

// h[0 .. 2 half] = firwin(2 half + 1, 1 / M, window=("kaiser", 14.0)) * up, as scipy.signal.resample_poly designs it.
void design_taps(const ResamplePlan& p, double* h) {
    const int n_taps = 2 * p.half + 1;
    const double M = (double)(p.up > p.down ? p.up : p.down);
    const double i0_beta = bessel_i0(RS_BETA);
    double sum = 0.0;
    for (int j = 0; j < n_taps; ++j) {
        const double n = (double)(j - p.half);
        const double t = M_PI * (n / M);
        const double sinc = j == p.half ? 1.0 : std::sin(t) / t;
        const double r = n / (double)p.half;
        const double arg = 1.0 - r * r;
        h[j] = (1.0 / M) * sinc * (bessel_i0(RS_BETA * std::sqrt(arg > 0.0 ? arg : 0.0)) / i0_beta);
        sum += h[j];
    }
    for (int j = 0; j < n_taps; ++j) h[j] = h[j] / sum * (double)p.up;
}

__device__ __forceinline__ void store_sample(float* p, double a) { *p = (float)a; }
__device__ __forceinline__ void store_sample(int16_t* p, double a) {
    a = fmin(fmax(a, -32768.0), 32767.0);
    *p = (int16_t)(int)rint(a);  // to nearest, ties to even
}

struct ResampleArgs {
    int n_in, n_out;
    int up, down, half, rows, span;
    int tiles;  // workgroups per recording
};

// One workgroup = RS_PER_THREAD * blockDim.x consecutive outputs of one recording; thread t owns outputs t, t + blockDim.x, ...
// of the tile, so the lanes of a wavefront hold consecutive outputs at every step.
template <typename S, bool UP1, bool STAGED>
__global__ __launch_bounds__(256) void kws_resample_kernel(const S* __restrict__ in, const int32_t* __restrict__ len, S* __restrict__ out,
                                                           const double* __restrict__ taps, const ResampleArgs a) {
    extern __shared__ double xs[];  // STAGED: the tile's input span as float64, zeros outside [0, len)
    const int tid = threadIdx.x, threads = blockDim.x;
    const int r = blockIdx.x / a.tiles;
    const int k0 = (blockIdx.x - r * a.tiles) * (RS_PER_THREAD * threads);
    int L = len ? len[r] : a.n_in;
    L = L < 0 ? 0 : (L > a.n_in ? a.n_in : L);
    const long long n_nat = ((long long)L * a.up + a.down - 1) / a.down;
    const int n_valid = n_nat < (long long)a.n_out ? (int)n_nat : a.n_out;
    const S* const x = in + (size_t)r * a.n_in;
    S* const y = out + (size_t)r * a.n_out;

    if (k0 >= n_valid) {  // a tile beyond the recording's natural length: zeros (uniform over the workgroup)
#pragma unroll
        for (int q = 0; q < RS_PER_THREAD; ++q) {
            const int k = k0 + tid + q * threads;
            if (k < a.n_out) y[k] = (S)0;
        }
        return;
    }

    // the newest sample output k0 reads is q0 = floor((half + k0 down) / up), its phase r0 the remainder
    const long long c0 = (long long)a.half + (long long)k0 * a.down;
    const long long q0 = UP1 ? c0 : c0 / a.up;
    const int r0 = UP1 ? 0 : (int)(c0 - q0 * a.up);
    const long long base = q0 - (a.rows - 1);  // the sample behind span index 0

    if (STAGED) {
        for (int s = tid; s < a.span; s += threads) {
            const long long m = base + s;
            xs[s] = (m >= 0 && m < (long long)L) ? (double)x[m] : 0.0;
        }
        __syncthreads();
    }

    int newest[RS_PER_THREAD], phase[RS_PER_THREAD];  // per output: span index of its newest sample, its first tap
    double acc[RS_PER_THREAD];
#pragma unroll
    for (int q = 0; q < RS_PER_THREAD; ++q) {
        const int e = r0 + (tid + q * threads) * a.down;  // < up + tile * down <= 2^21
        const int mq = UP1 ? e : e / a.up;
        phase[q] = UP1 ? 0 : e - mq * a.up;
        newest[q] = mq + a.rows - 1;
        acc[q] = 0.0;
    }
    // Kept rolled: unrolled, the compiler pairs the LDS reads of neighbouring steps into ds_read2_b64, which moves half the bytes
    // per LDS cycle of ds_read_b64 (one unalternated comparison, DESIGN 4.14: 86.0 us unrolled four times against 74.6 us rolled
    // for 10 minutes at 48 kHz).
#pragma unroll 1
    for (int i = 0; i < a.rows; ++i) {
        const int row = UP1 ? i : i * a.up;
#pragma unroll
        for (int q = 0; q < RS_PER_THREAD; ++q) {
            double v;
            if (STAGED) {
                v = xs[newest[q] - i];
            } else {
                const long long m = base + (newest[q] - i);
                v = (m >= 0 && m < (long long)L) ? (double)x[m] : 0.0;
            }
            acc[q] = fma(v, taps[row + phase[q]], acc[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < RS_PER_THREAD; ++q) {
        const int k = k0 + tid + q * threads;
        if (k < a.n_out) store_sample(&y[k], k < n_valid ? acc[q] : 0.0);
    }
}

// rate_in == rate_out: the copy under the same length rules.
template <typename S>
__global__ __launch_bounds__(256) void kws_resample_copy_kernel(const S* __restrict__ in, const int32_t* __restrict__ len, S* __restrict__ out,
                                                                int n_in, int n_out, int tiles) {
    const int r = blockIdx.x / tiles;
    const int k0 = (blockIdx.x - r * tiles) * (RS_PER_THREAD * 256);
    int L = len ? len[r] : n_in;
    L = L < 0 ? 0 : (L > n_in ? n_in : L);
#pragma unroll
    for (int q = 0; q < RS_PER_THREAD; ++q) {
        const int k = k0 + threadIdx.x + q * 256;
        if (k < n_out) out[(size_t)r * n_out + k] = k < L ? in[(size_t)r * n_in + k] : (S)0;
    }
}

// The design of a pair on the device: found in the cache, or designed on the host, uploaded and kept (the least recently
// used one makes room once RS_CACHE_PAIRS are held; the stream is drained before its table is freed).
int get_design(kws_ctx* c, const ResamplePlan& plan, const char* fn, const ResampleDesign*& out) {
    if (!c->resample) c->resample = new ResampleCache();
    ResampleCache& cache = *c->resample;
    ++cache.clock;
    for (ResampleDesign& d : cache.designs)
        if (d.plan.up == plan.up && d.plan.down == plan.down) {
            d.used = cache.clock;
            out = &d;
            return KWS_OK;
        }
    const size_t n = (size_t)plan.rows * plan.up;
    std::vector<double> h(n, 0.0);
    design_taps(plan, h.data());
    ResampleDesign fresh;
    fresh.plan = plan;
    fresh.used = cache.clock;
    int rc = replace_device_image(c, fresh.d_taps, h.data(), n * sizeof(double), fn);  // drains the stream
    if (rc) return rc;
    if (cache.designs.size() < (size_t)RS_CACHE_PAIRS) {
        cache.designs.push_back(std::move(fresh));
        out = &cache.designs.back();
        return KWS_OK;
    }
    size_t oldest = 0;
    for (size_t i = 1; i < cache.designs.size(); ++i)
        if (cache.designs[i].used < cache.designs[oldest].used) oldest = i;
    cache.designs[oldest] = std::move(fresh);  // frees the oldest pair's table
    out = &cache.designs[oldest];
    return KWS_OK;
}

template <typename S, bool UP1, bool STAGED>
void launch_resample(hipStream_t s, const ResamplePlan& p, const S* d_in, const int32_t* d_len, S* d_out, const double* d_taps,
                     const ResampleArgs& a, int R) {
    hipLaunchKernelGGL((kws_resample_kernel<S, UP1, STAGED>), dim3((unsigned)(R * a.tiles)), dim3(p.threads),
                       STAGED ? (size_t)p.span * sizeof(double) : 0, s, d_in, d_len, d_out, d_taps, a);
}

template <typename S>
int resample(kws_ctx* c, const S* d_in, int R, int n_in, const int32_t* d_len, int rate_in, int rate_out, S* d_out, int n_out,
             const char* fn) {
    KWS_GUARD_BEGIN
    if (!c) return KWS_EINVAL;
    const std::string name(fn);
    if (!d_in || !d_out) return fail(c, KWS_EINVAL, name + ": d_in / d_out is NULL");
    if (R < 1 || n_in < 1 || n_out < 1) return fail(c, KWS_EINVAL, name + ": R, n_in and n_out must be positive");
    ResamplePlan plan;
    int rc = make_plan(rate_in, rate_out, plan);
    if (rc == KWS_EINVAL) return fail(c, rc, name + ": the rates must be positive");
    if (rc) return fail(c, rc, name + ": max(up, down) of the reduced rate pair must be at most 1024");
    if (n_in > (1 << 30) || n_out > (1 << 30)) return fail(c, KWS_EUNSUPPORTED, name + ": more than 2^30 samples per recording");
    const bool copy = plan.up == 1 && plan.down == 1;
    const int tile = copy ? RS_PER_THREAD * 256 : plan.tile();
    const int tiles = (n_out + tile - 1) / tile;
    if ((unsigned long long)R * tiles > 0x7fffffffull) return fail(c, KWS_EUNSUPPORTED, name + ": more than 2^31 workgroups in one call");
    HIP_TRY(c, hipSetDevice(c->device));
    if (copy) {
        ProfScope ps(c, KWS_K_RESAMPLE);
        hipLaunchKernelGGL(kws_resample_copy_kernel<S>, dim3((unsigned)(R * tiles)), dim3(256), 0, c->stream, d_in, d_len, d_out, n_in,
                           n_out, tiles);
        HIP_TRY(c, hipGetLastError());
        return KWS_OK;
    }
    const ResampleDesign* d = nullptr;
    rc = get_design(c, plan, fn, d);
    if (rc) return rc;
    const ResampleArgs a = {n_in, n_out, plan.up, plan.down, plan.half, plan.rows, plan.span, tiles};
    ProfScope ps(c, KWS_K_RESAMPLE);
    if (!plan.staged)
        launch_resample<S, false, false>(c->stream, plan, d_in, d_len, d_out, d->d_taps.get(), a, R);
    else if (plan.up == 1)
        launch_resample<S, true, true>(c->stream, plan, d_in, d_len, d_out, d->d_taps.get(), a, R);
    else
        launch_resample<S, false, true>(c->stream, plan, d_in, d_len, d_out, d->d_taps.get(), a, R);
    HIP_TRY(c, hipGetLastError());
    return KWS_OK;
    KWS_GUARD_END(c, "kws_resample")
}

// ---- the streaming resampler (include/kws_hip.h: kws_stream_resample_*, kws_stream_push_rate_i16) --------------------------
// A stream's signal x[m] is zero before first_sample and grows by n_in samples per push; y[k] of the definition above is then
// defined for every integer k (floor division and the phase remainder round towards minus infinity), and absolute output j is
// y[j - d], d = ceil(half / down).  With P samples received the outputs j < floor(P up / down) have been emitted.
//
// What a push from P0 to P1 samples reads.  Output j of the push has floor(P0 up / down) <= j < floor(P1 up / down), so
// P0 up - (down - 1) <= j down <= P1 up - down.  Its newest sample is q = floor((half + (j - d) down) / up), its oldest
// q - (rows - 1).
//   newest:  half + (j - d) down <= P1 up - (d down - half) - down < P1 up since d down >= half, so q <= P1 - 1: the span of
//            every emitted output ends inside the samples already pushed.
//   oldest:  half + (j - d) down >= P0 up - (d down + down - 1 - half), so q >= P0 - ceil((d down + down - 1 - half) / up) and
//            the oldest sample is at or after P0 - H with
//                H = rows - 1 + ceil((d down + down - 1 - half) / up),
//            which pushes of one sample attain (tests/test_stream_resample_cpu.py), so H is exact: 62 for 1/3, 20 for 2/1, 58 for
//            160/441, 22 for 640/441, 125 for 1/6, 251 for 1/12, 503 for 1/24.
// The state of a stream is therefore its last H samples (zeros at the open: the signal before first_sample).  first_sample is a
// multiple of down, so a shift of the samples by it shifts the outputs by the integer first_sample / down * up and leaves every
// phase alone; positions are kept in 64 bits on the host and only two small numbers reach the kernel: where the first output's
// newest sample sits in history || input (e0) and its phase (r0).
struct StreamResampleArgs {
    int n_in, n_out, out_cap;
    int hist;  // H
    int up, down, rows;  // rows == 0: equal rates, a copy
    int e0, r0;
    int tiles;  // workgroups per stream
};

constexpr int SRS_THREADS = 256;
constexpr int SRS_TILE = 4 * SRS_THREADS;  // outputs per workgroup: a push of up to 1024 outputs per stream is one workgroup per stream
constexpr int SRS_GROUP = 32;              // steps whose tap and sample loads are issued together

// G consecutive steps of an output's chain: the G tap loads and the G sample reads are issued first, the FMAs follow in step order.
template <int G, bool UP1>
__device__ __forceinline__ double srs_steps(double acc, const double* __restrict__ h, const double* v, int up) {
    double hv[G], xv[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        hv[g] = h[UP1 ? g : g * up];
        xv[g] = v[-g];
    }
#pragma unroll
    for (int g = 0; g < G; ++g) acc = fma(xv[g], hv[g], acc);
    return acc;
}

// One workgroup = the outputs [tile * SRS_TILE, (tile + 1) * SRS_TILE) of one stream's push; lane = consecutive output.  Every
// workgroup stages history || input as float64 (at most RS_LDS_SAMPLES); tile 0 writes the stream's new history -- the last H
// samples of history || input, whatever n_in -- after the barrier, into the other half of the history buffer.
// The chain of an output is the batch kernel's: `rows` fused multiply-adds from 0.0, newest sample first.  The loads of
// SRS_GROUP steps are issued before the first of their FMAs, so the chain waits for one load latency per 32 steps, not per
// step; the rows mod 32 steps left over go in groups of 16, 8, 4, 2 and 1 (61 steps: 32 + 16 + 8 + 4 + 1, 56: 32 + 16 + 8).
template <bool UP1>
__global__ __launch_bounds__(SRS_THREADS) void kws_stream_resample_kernel(const int16_t* __restrict__ in, const int16_t* __restrict__ hist_old,
                                                                          int16_t* __restrict__ hist_new, int16_t* __restrict__ out,
                                                                          const double* __restrict__ taps, const StreamResampleArgs a) {
    extern __shared__ double xs[];
    const int tid = threadIdx.x;
    const int s = blockIdx.x / a.tiles;
    const int tile = blockIdx.x - s * a.tiles;
    const int16_t* const x = in + (size_t)s * a.n_in;
    int16_t* const y = out + (size_t)s * a.out_cap;
    const int t_end = min(a.n_out, (tile + 1) * SRS_TILE);

    if (a.rows == 0) {  // equal rates (uniform over the launch)
        for (int t = tile * SRS_TILE + tid; t < t_end; t += SRS_THREADS) y[t] = x[t];
        return;
    }

    const int total = a.hist + a.n_in;
    // four loads per thread in flight: the input may sit in pinned host memory, and a hop (480 + 62 samples) is one such round
    for (int i0 = tid; i0 < total; i0 += 4 * SRS_THREADS) {
        int16_t r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = min(i0 + u * SRS_THREADS, total - 1);  // clamped, so the four loads need no branch between them
            const int16_t* const p = i < a.hist ? hist_old + ((size_t)s * a.hist + i) : x + (i - a.hist);
            r[u] = *p;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * SRS_THREADS;
            if (i < total) xs[i] = (double)r[u];
        }
    }
    __syncthreads();
    if (tile == 0)
        for (int i = tid; i < a.hist; i += SRS_THREADS) hist_new[(size_t)s * a.hist + i] = (int16_t)xs[a.n_in + i];

    for (int t = tile * SRS_TILE + tid; t < t_end; t += SRS_THREADS) {
        const int e = a.r0 + t * a.down;  // < up + 2 * RS_LDS_SAMPLES * down <= 2^24
        const int mq = UP1 ? e : e / a.up;
        const int phase = UP1 ? 0 : e - mq * a.up;
        const int newest = a.e0 + mq;
        double acc = 0.0;
        const double* h = taps + phase;
        const double* v = xs + newest;
        int i = 0;
#pragma unroll 1
        for (; i + SRS_GROUP <= a.rows; i += SRS_GROUP) acc = srs_steps<SRS_GROUP, UP1>(acc, h + (UP1 ? i : i * a.up), v - i, a.up);
        if (a.rows & 16) {
            acc = srs_steps<16, UP1>(acc, h + (UP1 ? i : i * a.up), v - i, a.up);
            i += 16;
        }
        if (a.rows & 8) {
            acc = srs_steps<8, UP1>(acc, h + (UP1 ? i : i * a.up), v - i, a.up);
            i += 8;
        }
        if (a.rows & 4) {
            acc = srs_steps<4, UP1>(acc, h + (UP1 ? i : i * a.up), v - i, a.up);
            i += 4;
        }
        if (a.rows & 2) {
            acc = srs_steps<2, UP1>(acc, h + (UP1 ? i : i * a.up), v - i, a.up);
            i += 2;
        }
        if (a.rows & 1) acc = srs_steps<1, UP1>(acc, h + (UP1 ? i : i * a.up), v - i, a.up);
        store_sample(&y[t], acc);
    }
}

long long floor_div(__int128 a, long long b) {  // b > 0
    __int128 q = a / b;
    if (a % b < 0) --q;
    return (long long)q;
}

// floor(P up / down) for a 64-bit P
unsigned long long outputs_before(unsigned long long P, const ResamplePlan& p) {
    return (unsigned long long)(((unsigned __int128)P * (unsigned)p.up) / (unsigned)p.down);
}

int make_stream_plan(int rate_in, int rate_out, StreamPlan& sp) {
    const int rc = make_plan(rate_in, rate_out, sp.plan);
    if (rc) return rc;
    const ResamplePlan& p = sp.plan;
    sp.copy = p.up == 1 && p.down == 1;
    if (sp.copy) {
        sp.delay = sp.hist = 0;
        return KWS_OK;
    }
    sp.delay = (p.half + p.down - 1) / p.down;
    const int behind = sp.delay * p.down + p.down - 1 - p.half;  // >= 0
    sp.hist = p.rows - 1 + (behind + p.up - 1) / p.up;
    return KWS_OK;
}

// The checks every push shares; *n_out = what this push emits.  Nothing is touched.
int stream_resample_check(kws_ctx* c, const void* in, int n_in, const std::string& name, int* n_out) {
    StreamResample* st = c->stream_resample;
    if (!st) return fail(c, KWS_ESTATE, name + ": call kws_stream_resample_open first");
    if (!in) return fail(c, KWS_EINVAL, name + ": the input pointer is NULL");
    if (n_in < 1 || n_in > st->max_in) return fail(c, KWS_EINVAL, name + ": n_in must be in [1, max_in]");
    *n_out = (int)(outputs_before(st->pos + (unsigned long long)n_in, st->plan) - outputs_before(st->pos, st->plan));
    return KWS_OK;
}

// Enqueue one push of n_in samples per stream that emits n_out (checked by the caller) and advance the state.
int stream_resample_enqueue(kws_ctx* c, const int16_t* d_in, int n_in, int16_t* d_out, int out_cap, int n_out, const char* fn) {
    StreamResample* st = c->stream_resample;
    const ResamplePlan& p = st->plan;
    HIP_TRY(c, hipSetDevice(c->device));
    StreamResampleArgs a = {n_in, n_out, out_cap, st->hist, p.up, p.down, st->copy ? 0 : p.rows, 0, 0, (n_out + SRS_TILE - 1) / SRS_TILE};
    if (a.tiles < 1) a.tiles = 1;  // a push without outputs still advances the history
    const double* d_taps = nullptr;
    if (!st->copy) {
        const ResampleDesign* d = nullptr;
        const int rc = get_design(c, p, fn, d);  // the cache may have dropped the pair since the open: designed again then
        if (rc) return rc;
        d_taps = d->d_taps.get();
        // the first output's newest sample and phase, from the 64-bit position
        const __int128 k0 = (__int128)outputs_before(st->pos, p) - st->delay;
        const __int128 c0 = (__int128)p.half + k0 * p.down;
        const long long q0 = floor_div(c0, p.up);
        a.r0 = (int)(c0 - (__int128)q0 * p.up);
        const __int128 e0 = (__int128)q0 - ((__int128)st->pos - st->hist);
        const __int128 last = e0 + (a.r0 + (__int128)(n_out > 0 ? n_out - 1 : 0) * p.down) / p.up;
        if (n_out > 0 && (e0 < p.rows - 1 || last > st->hist + n_in - 1))
            return fail(c, KWS_EHIP, std::string(fn) + ": internal error, an output's span leaves history || input");
        a.e0 = n_out > 0 ? (int)e0 : p.rows - 1;
    }
    const int16_t* const h_old = st->d_hist.get() + (size_t)st->cur * st->n_streams * st->hist;
    int16_t* const h_new = st->d_hist.get() + (size_t)(st->cur ^ 1) * st->n_streams * st->hist;
    const size_t lds = st->copy ? 0 : (size_t)(st->hist + n_in) * sizeof(double);
    if (!st->copy && p.up == 1)
        hipLaunchKernelGGL(kws_stream_resample_kernel<true>, dim3((unsigned)(st->n_streams * a.tiles)), dim3(SRS_THREADS), lds, c->stream, d_in,
                           h_old, h_new, d_out, d_taps, a);
    else
        hipLaunchKernelGGL(kws_stream_resample_kernel<false>, dim3((unsigned)(st->n_streams * a.tiles)), dim3(SRS_THREADS), lds, c->stream, d_in,
                           h_old, h_new, d_out, d_taps, a);
    HIP_TRY(c, hipGetLastError());
    st->cur ^= 1;
    st->pos += (unsigned long long)n_in;
    return KWS_OK;
}

// A fused push whose second half was refused: the history half the resampler wrote is never read, the position steps back.
void stream_resample_undo(StreamResample* st, int n_in) {
    st->cur ^= 1;
    st->pos -= (unsigned long long)n_in;
}

// The checks of the fused pushes: an open stream set of the same size at the resampler's output rate, a push of one hop.
int stream_push_rate_check(kws_ctx* c, const void* in, int n_in, const std::string& name) {
    StreamResample* st = c->stream_resample;
    if (!st) return fail(c, KWS_ESTATE, name + ": call kws_stream_resample_open first");
    if (!c->n_streams) return fail(c, KWS_ESTATE, name + ": call kws_stream_open first");
    if (c->n_streams != st->n_streams) return fail(c, KWS_ESTATE, name + ": kws_stream_open and kws_stream_resample_open differ in n_streams");
    if (st->rate_out != c->sample_rate) return fail(c, KWS_ESTATE, name + ": the resampler's output rate is not the front end's sample rate");
    int n_out = 0;
    const int rc = stream_resample_check(c, in, n_in, name, &n_out);
    if (rc) return rc;
    if (n_out != c->fp.frame_step)
        return fail(c, KWS_EINVAL, name + ": this push would emit " + std::to_string(n_out) + " samples, a hop is " + std::to_string(c->fp.frame_step));
    return grow_device_buffer(c, st->d_hop, (size_t)st->n_streams * c->fp.frame_step, name.c_str(), "hop buffer");
}

}  // namespace

// kws_stream_reset's side: both halves of a stream's history are cleared, whichever the next push reads.  The set's position and
// phase are shared by its streams and stay.  Nothing when there is no resampler, when it keeps no history (equal rates), or when
// it was opened for another stream count (kws_stream_push_rate_i16 refuses that pairing anyway).
ResampleResetView stream_resample_reset_view(kws_ctx* c) {
    StreamResample* st = c->stream_resample;
    if (!st || !st->d_hist || st->n_streams != c->n_streams) return {nullptr, 0, 0};
    return {st->d_hist.get(), (long long)st->n_streams * st->hist, st->hist};
}

void stream_resample_free(kws_ctx* c) {
    delete c->stream_resample;
    c->stream_resample = nullptr;
}

void resample_free(kws_ctx* c) {
    delete c->resample;
    c->resample = nullptr;
}

}  // namespace kws

using namespace kws;

#pragma GCC visibility push(default)
extern "C" {

int kws_host_resample_len(int n_in, int rate_in, int rate_out, int* n_out) {
    ResamplePlan p;
    if (n_in < 0 || !n_out) return KWS_EINVAL;
    const int rc = make_plan(rate_in, rate_out, p);
    if (rc) return rc;
    const long long n = ((long long)n_in * p.up + p.down - 1) / p.down;
    if (n > 0x7fffffffll) return KWS_EUNSUPPORTED;
    *n_out = (int)n;
    return KWS_OK;
}

int kws_host_resample_design(int rate_in, int rate_out, int* up, int* down, int* half_len, int* outputs_per_workgroup, double* taps,
                             size_t cap, size_t* need) {
    KWS_GUARD_BEGIN
    if (need) *need = 0;
    ResamplePlan p;
    const int rc = make_plan(rate_in, rate_out, p);
    if (rc) return fail(nullptr, rc, rc == KWS_EINVAL ? "kws_host_resample_design: the rates must be positive"
                                                      : "kws_host_resample_design: max(up, down) of the reduced rate pair must be at most 1024");
    const size_t n_taps = 2 * (size_t)p.half + 1;
    if (need) *need = n_taps;
    if (up) *up = p.up;
    if (down) *down = p.down;
    if (half_len) *half_len = p.half;
    if (outputs_per_workgroup) *outputs_per_workgroup = (p.up == 1 && p.down == 1) ? RS_PER_THREAD * 256 : p.tile();
    if (!taps) return KWS_OK;
    if (cap < n_taps) return fail(nullptr, KWS_EINVAL, "kws_host_resample_design: cap is below the number of taps");
    design_taps(p, taps);
    return KWS_OK;
    KWS_GUARD_END(nullptr, "kws_host_resample_design")
}

int kws_resample_i16(kws_ctx* c, const int16_t* d_in, int R, int n_in, const int32_t* d_len, int rate_in, int rate_out, int16_t* d_out,
                     int n_out) {
    return resample(c, d_in, R, n_in, d_len, rate_in, rate_out, d_out, n_out, "kws_resample_i16");
}

int kws_resample_f32(kws_ctx* c, const float* d_in, int R, int n_in, const int32_t* d_len, int rate_in, int rate_out, float* d_out,
                     int n_out) {
    return resample(c, d_in, R, n_in, d_len, rate_in, rate_out, d_out, n_out, "kws_resample_f32");
}

int kws_host_stream_resample_plan(int rate_in, int rate_out, int* up, int* down, int* delay_out, int* history) {
    StreamPlan sp;
    const int rc = make_stream_plan(rate_in, rate_out, sp);
    if (rc) return rc;
    if (up) *up = sp.plan.up;
    if (down) *down = sp.plan.down;
    if (delay_out) *delay_out = sp.delay;
    if (history) *history = sp.hist;
    return KWS_OK;
}

int kws_host_stream_resample_count(int rate_in, int rate_out, uint64_t samples_before, int n_in, int* n_out) {
    if (n_in < 0 || !n_out) return KWS_EINVAL;
    ResamplePlan p;
    const int rc = make_plan(rate_in, rate_out, p);
    if (rc) return rc;
    if (samples_before + (uint64_t)n_in < samples_before) return KWS_EUNSUPPORTED;  // the position leaves 64 bits
    const unsigned long long n = outputs_before(samples_before + (uint64_t)n_in, p) - outputs_before(samples_before, p);
    if (n > 0x7fffffffull) return KWS_EUNSUPPORTED;
    *n_out = (int)n;
    return KWS_OK;
}

int kws_stream_resample_open(kws_ctx* c, int n_streams, int rate_in, int rate_out, int max_in, uint64_t first_sample) {
    KWS_GUARD_BEGIN
    if (!c) return KWS_EINVAL;
    const std::string name = "kws_stream_resample_open";
    if (n_streams < 1 || max_in < 1) return fail(c, KWS_EINVAL, name + ": n_streams and max_in must be positive");
    StreamPlan sp;
    int rc = make_stream_plan(rate_in, rate_out, sp);
    if (rc == KWS_EINVAL) return fail(c, rc, name + ": the rates must be positive");
    if (rc) return fail(c, rc, name + ": max(up, down) of the reduced rate pair must be at most 1024");
    if (first_sample % (uint64_t)sp.plan.down) return fail(c, KWS_EINVAL, name + ": first_sample must be a multiple of down");
    if (first_sample >> 62) return fail(c, KWS_EUNSUPPORTED, name + ": first_sample beyond 2^62");
    if (!sp.copy && (long long)sp.hist + max_in > RS_LDS_SAMPLES)
        return fail(c, KWS_EUNSUPPORTED, name + ": history + max_in exceeds the " + std::to_string(RS_LDS_SAMPLES) + " samples a workgroup stages");
    const long long max_out = ((long long)max_in * sp.plan.up) / sp.plan.down + 1;
    if (max_in > (1 << 30) || (long long)n_streams * ((max_out + SRS_TILE - 1) / SRS_TILE) > 0x7fffffffll)
        return fail(c, KWS_EUNSUPPORTED, name + ": more than 2^31 workgroups in one push");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!sp.copy) {
        const ResampleDesign* d = nullptr;
        rc = get_design(c, sp.plan, name.c_str(), d);  // drains the stream on a first use
        if (rc) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // the state being replaced may still be read
    std::unique_ptr<StreamResample> st(new StreamResample());
    static_cast<StreamPlan&>(*st) = sp;
    st->rate_in = rate_in;
    st->rate_out = rate_out;
    st->n_streams = n_streams;
    st->max_in = max_in;
    st->pos = first_sample;
    const size_t hist_n = 2 * (size_t)n_streams * sp.hist;
    if (hist_n) {
        if (!st->d_hist.alloc(hist_n)) return fail(c, KWS_ENOMEM, name + ": device allocation failed");
        const hipError_t e = hipMemsetAsync(st->d_hist.get(), 0, sizeof(int16_t) * hist_n, c->stream);
        if (e != hipSuccess) return fail_hip(c, e, "kws_stream_resample_open: hipMemsetAsync");
    }
    stream_resample_free(c);
    c->stream_resample = st.release();
    return KWS_OK;
    KWS_GUARD_END(c, "kws_stream_resample_open")
}

int kws_stream_resample_close(kws_ctx* c) {
    if (!c) return KWS_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    stream_resample_free(c);
    return KWS_OK;
}

int kws_stream_resample_i16(kws_ctx* c, const int16_t* d_in, int n_in, int16_t* d_out, int out_cap, int* n_out) {
    KWS_GUARD_BEGIN
    if (!c) return KWS_EINVAL;
    const std::string name = "kws_stream_resample_i16";
    int n = 0;
    const int rc = stream_resample_check(c, d_in, n_in, name, &n);
    if (rc) return rc;
    if (!d_out || !n_out) return fail(c, KWS_EINVAL, name + ": d_out / n_out is NULL");
    if (out_cap < n) return fail(c, KWS_EINVAL, name + ": out_cap is below the " + std::to_string(n) + " samples this push emits");
    *n_out = n;
    return stream_resample_enqueue(c, d_in, n_in, d_out, out_cap, n, "kws_stream_resample_i16");
    KWS_GUARD_END(c, "kws_stream_resample_i16")
}

int kws_stream_push_rate_i16(kws_ctx* c, const int16_t* d_in, int n_in, float* d_logits, int32_t* d_label) {
    KWS_GUARD_BEGIN
    if (!c) return KWS_EINVAL;
    int rc = stream_push_rate_check(c, d_in, n_in, "kws_stream_push_rate_i16");
    if (rc) return rc;
    StreamResample* st = c->stream_resample;
    rc = stream_resample_enqueue(c, d_in, n_in, st->d_hop.get(), c->fp.frame_step, c->fp.frame_step, "kws_stream_push_rate_i16");
    if (rc) return rc;
    rc = kws_stream_push_i16(c, st->d_hop.get(), d_logits, d_label, 0);
    if (rc) stream_resample_undo(st, n_in);
    return rc;
    KWS_GUARD_END(c, "kws_stream_push_rate_i16")
}

int kws_stream_push_host_rate_i16(kws_ctx* c, const int16_t* h_in, int n_in, const float** h_logits, const int32_t** h_label) {
    KWS_GUARD_BEGIN
    if (!c) return KWS_EINVAL;
    int rc = stream_push_rate_check(c, h_in, n_in, "kws_stream_push_host_rate_i16");
    if (rc) return rc;
    StreamResample* st = c->stream_resample;
    rc = host_results_ensure(c);
    if (rc) return rc;
    if (!st->h_in) {
        HIP_TRY(c, hipSetDevice(c->device));
        if (!st->h_in.alloc((size_t)st->n_streams * st->max_in, hipHostMallocMapped | hipHostMallocCoherent))
            return fail(c, KWS_ENOMEM, "kws_stream_push_host_rate_i16: pinned host allocation failed");
    }
    // one slot, as in kws_stream_push_host_i16: this call returns after the push kernel's flag, i.e. after the resampler's reads
    memcpy(st->h_in.get(), h_in, sizeof(int16_t) * (size_t)st->n_streams * n_in);
    rc = stream_resample_enqueue(c, st->h_in.get(), n_in, st->d_hop.get(), c->fp.frame_step, c->fp.frame_step, "kws_stream_push_host_rate_i16");
    if (rc) return rc;
    rc = kws_stream_push_i16(c, st->d_hop.get(), c->d_hr_logits.get(), c->d_hr_label.get(), 0);
    if (rc) {
        stream_resample_undo(st, n_in);
        return rc;
    }
    return kws_stream_wait_host(c, h_logits, h_label);
    KWS_GUARD_END(c, "kws_stream_push_host_rate_i16")
}

}  // extern "C"
#pragma GCC visibility pop
