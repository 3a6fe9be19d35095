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
    double* d_taps = nullptr;  // [rows * up]: h, then zeros
    unsigned long long used = 0;
};

struct ResampleCache {
    std::vector<ResampleDesign> designs;
    unsigned long long clock = 0;
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
        cache.designs.push_back(fresh);
        out = &cache.designs.back();
        return KWS_OK;
    }
    size_t oldest = 0;
    for (size_t i = 1; i < cache.designs.size(); ++i)
        if (cache.designs[i].used < cache.designs[oldest].used) oldest = i;
    (void)hipFree(cache.designs[oldest].d_taps);
    cache.designs[oldest] = fresh;
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
        launch_resample<S, false, false>(c->stream, plan, d_in, d_len, d_out, d->d_taps, a, R);
    else if (plan.up == 1)
        launch_resample<S, true, true>(c->stream, plan, d_in, d_len, d_out, d->d_taps, a, R);
    else
        launch_resample<S, false, true>(c->stream, plan, d_in, d_len, d_out, d->d_taps, a, R);
    HIP_TRY(c, hipGetLastError());
    return KWS_OK;
    KWS_GUARD_END(c, "kws_resample")
}

}  // namespace

void resample_free(kws_ctx* c) {
    if (!c->resample) return;
    for (ResampleDesign& d : c->resample->designs)
        if (d.d_taps) (void)hipFree(d.d_taps);
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

}  // extern "C"
#pragma GCC visibility pop
