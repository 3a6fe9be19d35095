// The refractory walk over one recording's windows, shared by the event kernels of kws_scan_detect_f32 (kws_scan.hip) and the
// threshold sweep of kws_scan_score_f32 (kws_score.hip).  What a candidate is and what happens at an event are the caller's.
#pragma once
#include <hip/hip_runtime.h>

namespace kws {

// One wavefront per recording, 64 windows per step: the first candidate lane at or after `next` fires, `next` moves `refractory`
// windows on, and the step repeats until no candidate lane is left.  Everything the walk itself holds is wave-uniform.
//   candidates(w0): loads the step's windows w0 .. w0 + 63 (lane l: window w0 + l; lanes at or past W are no candidates) and
//                   returns the ballot of the candidate lanes;
//   fire(w0, f, count): the event at window w0 + f, the count-th of the recording; lane f holds that window's loads.
// Returns the number of events.
template <typename Candidates, typename Fire>
__device__ __forceinline__ int scan_walk(int W, int refractory, Candidates candidates, Fire fire) {
    long long next = 0;
    int count = 0;
    for (int w0 = 0; w0 < W; w0 += 64) {
        unsigned long long left = candidates(w0);
        while (left) {
            const int f = __builtin_ctzll(left);
            left &= left - 1;  // lanes below f are gone already
            if (w0 + f < next) continue;
            fire(w0, f, count);
            ++count;
            next = (long long)w0 + f + refractory;
        }
    }
    return count;
}

}  // namespace kws
