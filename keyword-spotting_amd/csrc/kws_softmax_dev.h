// The softmax of one row of logits, shared by the decision layer (kws_decide.hip: kws_softmax_f32, the posterior smoothing) and
// the evaluation statistics (kws_eval.hip), so that a posterior is one value, bit for bit, wherever it is computed.
#pragma once
#include <hip/hip_runtime.h>

namespace kws {

// one thread per clip / stream: C <= 64 values, the work is launch latency, not arithmetic.  m = the row maximum, sum = the sum
// of expf(z - m) in index order: logf(sum) + m is the row's log-sum-exp.
__device__ __forceinline__ void softmax_row(const float* __restrict__ z, int C, float* __restrict__ p, float& m_out, float& sum_out) {
    float m = z[0];
    for (int i = 1; i < C; ++i) m = fmaxf(m, z[i]);
    float sum = 0.f;
    for (int i = 0; i < C; ++i) {
        const float e = expf(z[i] - m);
        p[i] = e;
        sum += e;
    }
    const float inv = 1.0f / sum;
    for (int i = 0; i < C; ++i) p[i] *= inv;
    m_out = m;
    sum_out = sum;
}

__device__ __forceinline__ void softmax_row(const float* __restrict__ z, int C, float* __restrict__ p) {
    float m, sum;
    softmax_row(z, C, p, m, sum);
}

}  // namespace kws
