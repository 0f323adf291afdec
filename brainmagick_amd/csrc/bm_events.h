// What the kernels that read a recording's resident events share (features.hip, segment_eval.hip, wer.hip): one event
// kind's table entry, the wavefront-wide search over its sorted times, and the rule that reads a segment's word label off
// the WordHash channel.
#pragma once
#include "bm_common.h"

struct BmEventKind {                // one event kind of one recording; start is non-decreasing
    const double* start;
    const double* dur;
    const double* runmax;           // runmax[i] = max over j <= i of start[j] + dur[j]
    long n;
};

// First index of the non-decreasing x[0 .. n) with x[i] >= v (n when there is none), found by a whole wavefront: its 64
// lanes probe 64 evenly spaced elements per round, so a table of n events costs ceil(log64 n) dependent loads where a
// binary search costs log2 n (a window's prologue is a chain of dependent loads: its latency, not its bandwidth, is what
// a workgroup waits for).  The arguments are uniform over the wavefront; every lane returns the same index.
__device__ __forceinline__ int bm_events_lower_bound(const double* __restrict__ x, int n, double v) {
    const int lane = threadIdx.x & (BM_WAVE - 1);
    int lo = 0, hi = n;                                     // the answer lies in [lo, hi]
    while (lo < hi) {
        const int step = (hi - lo + BM_WAVE - 1) / BM_WAVE;
        const int idx = lo + lane * step;
        const bool ge = idx < hi ? x[idx] >= v : true;
        const unsigned long long hit = __ballot(ge);
        const int first = hit ? __ffsll((long long)hit) - 1 : BM_WAVE;        // probes before `first` are below v
        const int base = lo;
        lo = first == 0 ? base : base + (first - 1) * step + 1;
        hi = min(hi, base + first * step);
    }
    return lo;
}

// ---- the word label of a segment ----------------------------------------------------------------------------------------
// p = &x[b][c][t0] of the WordHash channel.  The label is the first non-zero of p[0], p[-1] (only if t0 > 0), p[1],
// p[-2] (only if t0 > 1), p[2], ... up to REACH samples to either side -- the chain of torch.where(wh == 0, ..., wh) of
// bm/wer.py:58-64 (REACH 2) and scripts/run_eval_probs.py:122-130 (REACH 1) with its guards: -0.0 counts as zero and a
// NaN does not, as `wh == 0` decides.  The caller has checked 0 <= t0 and t0 + REACH < T.  Every load is issued before
// the chain.  Returns the chosen value: 0 when every candidate is zero.
template <int REACH>
__device__ __forceinline__ float bm_word_label_pick(const float* __restrict__ p, int t0) {
    float v = p[0];
    float before[REACH], after[REACH];
#pragma unroll
    for (int d = 1; d <= REACH; ++d) {
        before[d - 1] = t0 >= d ? p[-d] : 0.f;
        after[d - 1] = p[d];
    }
#pragma unroll
    for (int d = 1; d <= REACH; ++d) {
        if (v == 0.f && t0 >= d) v = before[d - 1];
        if (v == 0.f) v = after[d - 1];
    }
    return v;
}

// What a chosen value is as a label: the exact integer of the fp32 value (int64).  is_zero: no candidate was non-zero
// (label 0).  is_illegal: the value is not finite or |v| >= 2^63 (label 0), or not an integer (label = the value
// truncated towards zero).  Which flag bit either raises, and whether all-zero is an error, is the kernel's own.
struct BmWordLabel {
    long label;
    bool is_zero, is_illegal;
};
__device__ __forceinline__ BmWordLabel bm_word_label_classify(float v) {
    BmWordLabel w = {0, false, false};
    if (v == 0.f) {
        w.is_zero = true;
    } else if (!(fabsf(v) < 9223372036854775808.f)) {       // NaN, +-inf, |v| >= 2^63
        w.is_illegal = true;
    } else {
        w.label = (long)v;
        if (truncf(v) != v) w.is_illegal = true;
    }
    return w;
}
