// Scoring a scan against annotations over a threshold sweep (include/kws_hip.h: kws_host_score_plan, kws_scan_score_f32,
// kws_scan_score_ragged_f32): the softmax and the smoothing kernels of kws_scan_detect_f32 once at a threshold of -inf, then one
// refractory walk per (recording, threshold) that matches every event against the recording's annotation intervals as it fires
// and counts hits, false alarms, duplicates and the hits' latency per class.
#include <algorithm>
#include <array>
#include <climits>
#include <cstring>
#include <limits>

#include "kws_ctx.h"
#include "kws_scan_dev.h"

using namespace kws;

namespace {

constexpr int SWEEP_WAVES = 4;  // wavefronts of a workgroup: consecutive thresholds over ONE recording, whose windows they share in cache

// One wavefront per (recording r = blockIdx.x, threshold t).  cand / score: what the smoothing kernel left at a threshold of
// -inf (the argmax where it is a keyword, else -1; the smoothed score), so a window is a candidate when cand >= 0 and
// score >= thr[t] -- the comparison kws_scan_detect_f32 makes.  span: (first packed window, windows) per recording, or NULL for
// R recordings of W windows each.  ival[off[r * C + k] .. off[r * C + k + 1]) = (first_window, last_window) of recording r's
// annotations of label k, ascending and disjoint (kws_host_score_plan).
// The event's window and label are wave-uniform.  Lane c keeps class c's counters, a cursor into class c's list with that interval
// in registers, and the interval the class hit last.  Events come in window order and a label's intervals are ascending and
// disjoint, so the cursor only moves forward -- to the first interval that ends at or after the event, which is the only one that
// can hold it -- and an interval was matched before exactly when it is the last hit.  Most events cost no load at all: a walk
// loads each of its recording's intervals once.  (A binary search per event with wave-uniform loads gives the same counts; its
// five dependent loads per event made the sweep of the benchmark 7.1 ms where this takes 5.0 ms)
// counts: uint64 [K][C][4] = hits, false alarms, duplicates, latency sum; zeroed before the launch, integer atomics.
__global__ __launch_bounds__(64 * SWEEP_WAVES) void kws_score_sweep_kernel(const int32_t* __restrict__ cand, const float* __restrict__ score,
                                                                           const int2* __restrict__ span, int W, int C, int refractory,
                                                                           const float* __restrict__ thr, int K,
                                                                           const int2* __restrict__ ival, const int32_t* __restrict__ off,
                                                                           unsigned long long* __restrict__ counts) {
    const int r = blockIdx.x, lane = threadIdx.x & 63;
    const int t = blockIdx.y * SWEEP_WAVES + (threadIdx.x >> 6);
    if (t >= K) return;
    size_t base = (size_t)r * W;
    int Wr = W;
    if (span) {
        const int2 sp = span[r];
        base = (size_t)sp.x;
        Wr = sp.y;
    }
    const int32_t* cr = cand + base;
    const float* sr = score + base;
    const int32_t* list = off + (size_t)r * C;
    const float th = thr[t];
    unsigned int hits = 0, alarms = 0, dups = 0;  // at most one event per window, 2^30 windows
    unsigned long long latency = 0;
    int last_hit = -1;
    // lane c: the first interval of class c not yet behind the walk, INT_MAX where the list has run out (nothing is inside)
    int cur = 0, end = 0, iv_first = INT_MAX, iv_last = INT_MAX;
    if (lane < C) {
        cur = list[lane];
        end = list[lane + 1];
        if (cur < end) {
            const int2 iv = ival[cur];
            iv_first = iv.x;
            iv_last = iv.y;
        }
    }
    int k = -1;
    scan_walk(
        Wr, refractory,
        [&](int w0) {
            const int w = w0 + lane;
            k = w < Wr ? cr[w] : -1;
            const float sc = w < Wr ? sr[w] : 0.f;
            return __ballot(k >= 0 && sc >= th);  // false for a NaN threshold
        },
        [&](int w0, int f, int) {
            const int w = w0 + f;
            const int label = __builtin_amdgcn_readlane(k, f);  // in [first_keyword, C)
            if (lane == label) {
                while (w > iv_last) {  // never once the list has run out
                    ++cur;
                    iv_first = iv_last = INT_MAX;
                    if (cur < end) {
                        const int2 iv = ival[cur];
                        iv_first = iv.x;
                        iv_last = iv.y;
                    }
                }
                if (w < iv_first) ++alarms;
                else if (cur == last_hit) ++dups;
                else {
                    ++hits;
                    latency += (unsigned long long)(w - iv_first);
                    last_hit = cur;
                }
            }
        });
    if (lane < C) {
        unsigned long long* out = counts + ((size_t)t * C + lane) * 4;
        if (hits) atomicAdd(out + 0, (unsigned long long)hits);
        if (alarms) atomicAdd(out + 1, (unsigned long long)alarms);
        if (dups) atomicAdd(out + 2, (unsigned long long)dups);
        if (latency) atomicAdd(out + 3, latency);
    }
}

// The annotation table, validated and sorted (kws_host_score_plan): rows by (recording, label, first_window), off[r * C + k] = the
// first row of recording r's label k, off[R * C] = N.  Nothing is written unless the table is valid.
int score_plan(const int32_t* truth, int N, int R, int C, int first_keyword, std::vector<std::array<int32_t, 4>>& rows,
               std::vector<int32_t>& off) {
    if (R < 1 || C < 1 || C > MAX_CLASSES || first_keyword < 0 || N < 0 || (N > 0 && !truth)) return KWS_EINVAL;
    if (N > (1 << 24) || R > (1 << 20)) return KWS_EUNSUPPORTED;
    rows.resize((size_t)N);
    for (int i = 0; i < N; ++i) {
        const int32_t* t = truth + (size_t)i * 4;
        if (t[0] < 0 || t[0] >= R || t[1] < first_keyword || t[1] >= C || t[2] < 0 || t[2] > t[3]) return KWS_EINVAL;
        rows[i] = {t[0], t[1], t[2], t[3]};
    }
    std::sort(rows.begin(), rows.end());  // (recording, label, first_window, last_window)
    for (int i = 1; i < N; ++i)
        if (rows[i][0] == rows[i - 1][0] && rows[i][1] == rows[i - 1][1] && rows[i][2] <= rows[i - 1][3]) return KWS_EINVAL;
    off.assign((size_t)R * C + 1, 0);
    for (int i = 0; i < N; ++i) ++off[(size_t)rows[i][0] * C + rows[i][1] + 1];
    for (size_t i = 1; i < off.size(); ++i) off[i] += off[i - 1];
    return KWS_OK;
}

// The two entries' own arguments, ahead of those they share with kws_scan_detect_f32 (decision_check).
int score_check(kws_ctx* c, const std::string& f, const float* d_logits, const float* thresholds, int K, int N, const uint64_t* d_counts) {
    if (!d_logits || !d_counts || !thresholds) return fail(c, KWS_EINVAL, f + ": d_logits / thresholds / d_counts is NULL");
    if (K < 1 || K > 1024 || N < 0) return fail(c, KWS_EINVAL, f + ": need K in [1, 1024] and N >= 0");
    return KWS_OK;
}

// The tables of one call in one upload, 8-byte members first: span [R] (ragged only), intervals [N], then off [R C + 1] and the
// thresholds [K].
struct ScoreTables {
    const int2* span = nullptr;
    const int2* ival = nullptr;
    const int32_t* off = nullptr;
    const float* thr = nullptr;
};
int score_tables(kws_ctx* c, const std::string& f, const std::vector<int2>* span, const int32_t* truth, int N, int R, int C, int first_keyword,
                 const float* thresholds, int K, ScoreTables* out) {
    std::vector<std::array<int32_t, 4>> rows;
    std::vector<int32_t> off;
    const int rc = score_plan(truth, N, R, C, first_keyword, rows, off);
    if (rc == KWS_EUNSUPPORTED) return fail(c, rc, f + ": more than 2^24 annotations or 2^20 recordings in one call");
    if (rc) return fail(c, rc, f + ": the annotations need 0 <= recording < R, first_keyword <= label < C, 0 <= first_window <= "
                                   "last_window, and no two overlapping rows of one recording and label");
    const size_t n_span = span ? span->size() : 0;
    const size_t b_span = sizeof(int2) * n_span, b_ival = sizeof(int2) * (size_t)N, b_off = sizeof(int32_t) * off.size();
    std::vector<unsigned char> host(b_span + b_ival + b_off + sizeof(float) * (size_t)K);
    if (n_span) memcpy(host.data(), span->data(), b_span);
    int2* iv = reinterpret_cast<int2*>(host.data() + b_span);
    for (int i = 0; i < N; ++i) iv[i] = make_int2(rows[i][2], rows[i][3]);
    memcpy(host.data() + b_span + b_ival, off.data(), b_off);
    memcpy(host.data() + b_span + b_ival + b_off, thresholds, sizeof(float) * (size_t)K);
    const unsigned char* d = nullptr;
    if (int up = upload_ragged_tables(c, host.data(), host.size(), f.c_str(), reinterpret_cast<const void**>(&d))) return up;
    out->span = span ? reinterpret_cast<const int2*>(d) : nullptr;
    out->ival = reinterpret_cast<const int2*>(d + b_span);
    out->off = reinterpret_cast<const int32_t*>(d + b_span + b_ival);
    out->thr = reinterpret_cast<const float*>(d + b_span + b_ival + b_off);
    return KWS_OK;
}

// The smoothing at a threshold of -inf over the batch, then the sweep.
int score_windows(kws_ctx* c, const std::string& f, const WindowBatch& b, const ScoreTables& tb, const float* d_logits, int C, int smooth_window,
                  int first_keyword, int refractory, int K, uint64_t* d_counts) {
    ScanScratch ws;
    if (int rc = scan_posteriors(c, f.c_str(), b, tb.span, d_logits, C, smooth_window, first_keyword, -std::numeric_limits<float>::infinity(), nullptr, ws))
        return rc;
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(d_counts);
    HIP_TRY(c, hipMemsetAsync(counts, 0, sizeof(unsigned long long) * (size_t)K * C * 4, c->stream));
    hipLaunchKernelGGL(kws_score_sweep_kernel, dim3(b.R, (K + SWEEP_WAVES - 1) / SWEEP_WAVES), dim3(64 * SWEEP_WAVES), 0, c->stream, ws.cand, ws.score,
                       tb.span, b.W, C, refractory, tb.thr, K, tb.ival, tb.off, counts);
    HIP_TRY(c, hipGetLastError());
    return KWS_OK;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int kws_host_score_plan(const int32_t* truth, int N, int R, int C, int first_keyword, int32_t* sorted, int32_t* off) {
    try {
        if (!off || (N > 0 && !sorted)) return KWS_EINVAL;
        std::vector<std::array<int32_t, 4>> rows;
        std::vector<int32_t> o;
        const int rc = score_plan(truth, N, R, C, first_keyword, rows, o);
        if (rc) return rc;
        if (N > 0) memcpy(sorted, rows.data(), sizeof(int32_t) * 4 * (size_t)N);
        memcpy(off, o.data(), sizeof(int32_t) * o.size());
        return KWS_OK;
    } catch (...) {
        return KWS_ENOMEM;
    }
}

int kws_scan_score_f32(kws_ctx* c, const float* d_logits, int R, int W, int C, int smooth_window, int first_keyword, int refractory,
                       const float* thresholds, int K, const int32_t* truth, int N, uint64_t* d_counts) {
    KWS_GUARD_BEGIN
    if (!c) return KWS_EINVAL;
    const std::string f = "kws_scan_score_f32";
    if (int rc = score_check(c, f, d_logits, thresholds, K, N, d_counts)) return rc;
    if (int rc = decision_check(c, f.c_str(), R, C, smooth_window, first_keyword, refractory)) return rc;
    WindowBatch b;
    if (int rc = scan_equal_windows(c, f.c_str(), R, W, b)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    ScoreTables tb;
    if (int rc = score_tables(c, f, nullptr, truth, N, R, C, first_keyword, thresholds, K, &tb)) return rc;
    return score_windows(c, f, b, tb, d_logits, C, smooth_window, first_keyword, refractory, K, d_counts);
    KWS_GUARD_END(c, "kws_scan_score_f32")
}

int kws_scan_score_ragged_f32(kws_ctx* c, const float* d_logits, const int32_t* win_off, const int32_t* windows, int R, int C,
                              int smooth_window, int first_keyword, int refractory, const float* thresholds, int K, const int32_t* truth,
                              int N, uint64_t* d_counts) {
    KWS_GUARD_BEGIN
    if (!c) return KWS_EINVAL;
    const std::string f = "kws_scan_score_ragged_f32";
    if (int rc = score_check(c, f, d_logits, thresholds, K, N, d_counts)) return rc;
    if (int rc = decision_check(c, f.c_str(), R, C, smooth_window, first_keyword, refractory)) return rc;
    if (!win_off || !windows) return fail(c, KWS_EINVAL, f + ": win_off / windows is NULL");
    WindowBatch b;
    if (int rc = scan_ragged_spans(c, f.c_str(), win_off, windows, R, b)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    ScoreTables tb;  // also when nothing has a window: a bad table is refused all the same
    if (int rc = score_tables(c, f, &b.span, truth, N, R, C, first_keyword, thresholds, K, &tb)) return rc;
    if (b.total == 0) {  // no recording has a window: nothing fires
        HIP_TRY(c, hipMemsetAsync(d_counts, 0, sizeof(uint64_t) * (size_t)K * C * 4, c->stream));
        return KWS_OK;
    }
    return score_windows(c, f, b, tb, d_logits, C, smooth_window, first_keyword, refractory, K, d_counts);
    KWS_GUARD_END(c, "kws_scan_score_ragged_f32")
}

}  // extern "C"
#pragma GCC visibility pop
