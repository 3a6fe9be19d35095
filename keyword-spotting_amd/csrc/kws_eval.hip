// Evaluation statistics on the device (include/kws_hip.h: kws_eval_open / reset / close / update_f32 / read): loss, accuracy,
// confusion matrix and one-vs-rest posterior histograms (the ROC counts) accumulated across any number of batches and read back
// once, with the cross-entropy gradient as a by-product.  Replaces the per-batch loss.item() / torch.max / .sum().item() of the
// reference's loops (train.py:51-54,79-98, kws/libs/training.py:300-303,347-393) and feeds what test.py:27-58 reports.
// (build-defined; the reference computes all of it on the host with torch and sklearn.)
#include <cstring>
#include <vector>

#include "kws_ctx.h"
#include "kws_softmax_dev.h"

namespace kws {
namespace {

constexpr int EVAL_BLOCK = 256;            // rows per workgroup, one thread per row as kws_softmax_f32
constexpr int EVAL_LDS_COUNTERS = 8192;    // 2 C K private 32-bit counters (32 KiB) per workgroup; beyond: global atomics
constexpr size_t EVAL_PART_RESERVE = 4096; // loss partials allocated by kws_eval_open: updates of up to 2^20 rows never allocate
// the accumulators, in 64-bit words
constexpr size_t EVAL_COUNTS = 0, EVAL_LOSS = 4, EVAL_CONFUSION = 5;

inline size_t eval_words(int C, int K) { return EVAL_CONFUSION + (size_t)C * C + 2 * (size_t)C * K; }

// One thread per row.  Integer counters only: the confusion cell and (without LDS) the histogram bins by 64-bit global atomics,
// the four row counts and (with LDS) the bins through private 32-bit counters of the workgroup (at most 256 increments each),
// flushed by 64-bit atomics.  The float32 row losses of a workgroup are summed in float64 by a fixed tree into partial[block]:
// no float atomics, and the order depends on nothing but B.
template <bool LDS_HIST>
__global__ __launch_bounds__(EVAL_BLOCK) void kws_eval_update_kernel(const float* __restrict__ logits, const int32_t* __restrict__ truth,
                                                                     int B, int C, int K, float grad_scale, float* __restrict__ dlogits,
                                                                     float* __restrict__ loss_rows, unsigned long long* __restrict__ state,
                                                                     double* __restrict__ partial) {
    extern __shared__ unsigned int hist[];  // LDS_HIST: [2][C][K], positives then negatives
    __shared__ double red[EVAL_BLOCK];
    __shared__ unsigned int cnt[4];
    const int tid = threadIdx.x;
    const int b = blockIdx.x * EVAL_BLOCK + tid;
    const int CK = C * K;
    unsigned long long* const confusion = state + EVAL_CONFUSION;
    unsigned long long* const bins = confusion + (size_t)C * C;  // hist_pos [C][K], hist_neg [C][K]
    if (tid < 4) cnt[tid] = 0;
    if (LDS_HIST)
        for (int i = tid; i < 2 * CK; i += EVAL_BLOCK) hist[i] = 0;
    __syncthreads();

    float l = 0.f;
    if (b < B) {
        const float* z = logits + (size_t)b * C;
        const int t = truth[b];
        int skip = 0;  // the count a row outside the statistics goes to: 2 ignored (the label is never an index), 3 non-finite
        if (t < 0 || t >= C) {
            skip = 2;
        } else {
            bool finite = true;
            for (int i = 0; i < C; ++i) finite = finite && isfinite(z[i]);
            if (!finite) skip = 3;
        }
        if (skip) {
            atomicAdd(&cnt[skip], 1u);
            if (dlogits)
                for (int i = 0; i < C; ++i) dlogits[(size_t)b * C + i] = 0.f;
        } else {
            float p[MAX_CLASSES];
            float m, sum;
            softmax_row(z, C, p, m, sum);
            l = logf(sum) + m - z[t];
            int pred = 0;  // first maximum wins (torch.max, training.py:371)
            float best = z[0];
            for (int i = 1; i < C; ++i)
                if (z[i] > best) {
                    best = z[i];
                    pred = i;
                }
            atomicAdd(&confusion[(size_t)t * C + pred], 1ull);
            atomicAdd(&cnt[0], 1u);
            if (pred == t) atomicAdd(&cnt[1], 1u);
            if (K > 0) {
                const float Kf = (float)K;  // a power of two: the product is exact, p is finite and in [0, 1]
                for (int i = 0; i < C; ++i) {
                    int bin = (int)(p[i] * Kf);
                    if (bin > K - 1) bin = K - 1;
                    const int slot = (i == t ? 0 : CK) + i * K + bin;
                    if (LDS_HIST)
                        atomicAdd(&hist[slot], 1u);
                    else
                        atomicAdd(&bins[slot], 1ull);
                }
            }
            if (dlogits)
                for (int i = 0; i < C; ++i) dlogits[(size_t)b * C + i] = (p[i] - (i == t ? 1.f : 0.f)) * grad_scale;
        }
        if (loss_rows) loss_rows[b] = l;
    }

    red[tid] = (double)l;
    __syncthreads();
    for (int s = EVAL_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) partial[blockIdx.x] = red[0];
    if (tid < 4 && cnt[tid]) atomicAdd(&state[EVAL_COUNTS + tid], (unsigned long long)cnt[tid]);
    if (LDS_HIST)
        for (int i = tid; i < 2 * CK; i += EVAL_BLOCK) {
            const unsigned int v = hist[i];
            if (v) atomicAdd(&bins[i], (unsigned long long)v);
        }
}

// loss_sum += the workgroups' partials, in index order (one workgroup: the loads are parallel, the additions are one chain)
__global__ __launch_bounds__(EVAL_BLOCK) void kws_eval_loss_kernel(const double* __restrict__ partial, int n,
                                                                   unsigned long long* __restrict__ state) {
    __shared__ double chunk[EVAL_BLOCK];
    double* const loss_sum = reinterpret_cast<double*>(state + EVAL_LOSS);
    double acc = threadIdx.x == 0 ? *loss_sum : 0.0;
    for (int base = 0; base < n; base += EVAL_BLOCK) {
        const int i = base + threadIdx.x;
        chunk[threadIdx.x] = i < n ? partial[i] : 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = n - base < EVAL_BLOCK ? n - base : EVAL_BLOCK;
            for (int k = 0; k < m; ++k) acc += chunk[k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss_sum = acc;
}

}  // namespace

void eval_free(kws_ctx* c) {
    c->d_eval.reset();
    c->d_eval_part.reset();
    c->eval_classes = c->eval_bins = 0;
}

}  // namespace kws

using namespace kws;

#pragma GCC visibility push(default)
extern "C" {

int kws_eval_open(kws_ctx* c, int num_classes, int n_bins) {
    if (!c) return KWS_EINVAL;
    if (num_classes < 1 || num_classes > MAX_CLASSES) return fail(c, KWS_EINVAL, "kws_eval_open: num_classes must be in [1, 64]");
    if (n_bins != 0 && (n_bins < 2 || n_bins > 1024 || (n_bins & (n_bins - 1)) != 0))
        return fail(c, KWS_EINVAL, "kws_eval_open: n_bins must be 0 or a power of two in [2, 1024]");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // an update of the state being replaced may still be running
    eval_free(c);
    const size_t words = eval_words(num_classes, n_bins);
    if (!(c->d_eval.alloc(words) && c->d_eval_part.alloc(EVAL_PART_RESERVE))) {
        eval_free(c);
        return fail(c, KWS_ENOMEM, "kws_eval_open: device allocation failed");
    }
    c->eval_classes = num_classes;
    c->eval_bins = n_bins;
    HIP_TRY(c, hipMemsetAsync(c->d_eval.get(), 0, words * sizeof(unsigned long long), c->stream));
    return KWS_OK;
}

int kws_eval_reset(kws_ctx* c) {
    if (!c) return KWS_EINVAL;
    if (!c->eval_classes) return fail(c, KWS_ESTATE, "kws_eval_reset: call kws_eval_open first");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemsetAsync(c->d_eval.get(), 0, eval_words(c->eval_classes, c->eval_bins) * sizeof(unsigned long long), c->stream));
    return KWS_OK;
}

int kws_eval_close(kws_ctx* c) {
    if (!c) return KWS_EINVAL;
    if (!c->eval_classes) return KWS_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    eval_free(c);
    return KWS_OK;
}

int kws_eval_update_f32(kws_ctx* c, const float* d_logits, const int32_t* d_truth, int B, float grad_scale, float* d_dlogits,
                        float* d_loss_rows) {
    if (!c) return KWS_EINVAL;
    if (!c->eval_classes) return fail(c, KWS_ESTATE, "kws_eval_update_f32: call kws_eval_open first");
    if (!d_logits || !d_truth) return fail(c, KWS_EINVAL, "kws_eval_update_f32: d_logits / d_truth is NULL");
    if (B <= 0) return fail(c, KWS_EINVAL, "kws_eval_update_f32: B must be positive");
    HIP_TRY(c, hipSetDevice(c->device));
    const int C = c->eval_classes, K = c->eval_bins;
    const int blocks = (B + EVAL_BLOCK - 1) / EVAL_BLOCK;
    int rc = grow_device_buffer(c, c->d_eval_part, (size_t)blocks, "kws_eval_update_f32", "loss partial");
    if (rc) return rc;
    const float scale = d_dlogits ? grad_scale : 0.f;
    const int counters = 2 * C * K;
    if (K > 0 && counters <= EVAL_LDS_COUNTERS)
        hipLaunchKernelGGL(kws_eval_update_kernel<true>, dim3(blocks), dim3(EVAL_BLOCK), counters * sizeof(unsigned int), c->stream,
                           d_logits, d_truth, B, C, K, scale, d_dlogits, d_loss_rows, c->d_eval.get(), c->d_eval_part.get());
    else
        hipLaunchKernelGGL(kws_eval_update_kernel<false>, dim3(blocks), dim3(EVAL_BLOCK), 0, c->stream, d_logits, d_truth, B, C, K,
                           scale, d_dlogits, d_loss_rows, c->d_eval.get(), c->d_eval_part.get());
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(kws_eval_loss_kernel, dim3(1), dim3(EVAL_BLOCK), 0, c->stream, c->d_eval_part.get(), blocks, c->d_eval.get());
    HIP_TRY(c, hipGetLastError());
    return KWS_OK;
}

int kws_eval_read(kws_ctx* c, uint64_t* counts, double* loss_sum, uint64_t* confusion, uint64_t* hist_pos, uint64_t* hist_neg) {
    KWS_GUARD_BEGIN
    if (!c) return KWS_EINVAL;
    if (!c->eval_classes) return fail(c, KWS_ESTATE, "kws_eval_read: call kws_eval_open first");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const size_t C = (size_t)c->eval_classes, K = (size_t)c->eval_bins;
    std::vector<unsigned long long> h(eval_words((int)C, (int)K));
    HIP_TRY(c, hipMemcpy(h.data(), c->d_eval.get(), h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    const unsigned long long* conf = h.data() + EVAL_CONFUSION;
    if (counts) std::memcpy(counts, h.data() + EVAL_COUNTS, 4 * sizeof(uint64_t));
    if (loss_sum) std::memcpy(loss_sum, h.data() + EVAL_LOSS, sizeof(double));
    if (confusion) std::memcpy(confusion, conf, C * C * sizeof(uint64_t));
    if (hist_pos && K) std::memcpy(hist_pos, conf + C * C, C * K * sizeof(uint64_t));
    if (hist_neg && K) std::memcpy(hist_neg, conf + C * C + C * K, C * K * sizeof(uint64_t));
    return KWS_OK;
    KWS_GUARD_END(c, "kws_eval_read")
}

}  // extern "C"
#pragma GCC visibility pop
