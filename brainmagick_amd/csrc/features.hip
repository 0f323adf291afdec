// The features of a batch built from events that are resident on the device: FeaturesBuilder.__call__
// (bm/features/base.py:68-122) with Feature.get_on_overlap (base.py:238-267), DataSlice.overlap / slice_in_parent
// (bm/events.py:80-111), MelSpectrum.get (bm/features/audio.py:78-83) and _BaseWav2Vec._get_cached_tensor +
// Wav2Vec*.get_on_overlap (audio.py:211-274), as ONE launch per batch that writes features [B][F][T] fp32 and the mask
// [B][1][T], every element exactly once.  Every output is a copy of a table value, an array entry or a default: there is
// no floating-point arithmetic on values, only on indices.
//
// Index arithmetic: the reference's, in fp64, with rint for Python's round (both round half to even), written term
// for term as the reference computes it -- also where it recomputes a stop as start + duration.  Contraction is OFF
// for this file (the pragma below): a * b + c fused into one rounding would move a half-way index.
//   window      start, dur from the host (Python's division: no device division); stop = start + dur;
//               p0 = rint(start sr)
//   candidate   e.start + e.duration >= start  and  e.start < stop
//   overlap     o0 = max(start, e.start); o1 = o0 + (min(stop, e.start + e.duration) - o0); a = rint(o0 sr);
//               n = rint(o1 sr) - a; skipped when n < 1; paints window samples [a - p0, a - p0 + n)
//   constant    the event's value row
//   resampled   n_e = rint(((e.start + e.duration) - e.start) sr); first = min(max(0, -rint((e.start - o0) sr)), n_e - 1);
//               sample j reads resampled column k = min(first + j, n_e - 1) (the min is the reference's one-sample
//               replicate pad; where the reference would assert -- a shortfall of 2 or more -- the last column repeats);
//               resampled column k is source column k when L == n_e, else min((long)floorf((float)k ((float)L / n_e)),
//               L - 1): torch's nearest rule, in fp32 as torch computes it
//   chunk       er = L / e.duration (from the host); c0 = min(rint((o0 - e.start) er), L - 1);
//               c1 = min(max(c0 + 1, rint((o1 - e.start) er)), L); n_c = c1 - c0; sample j reads source column c0 + j
//               when n_c == n, else c0 + min((long)floorf((float)j ((float)n_c / n)), n_c - 1)
// Within a kind a later event overwrites an earlier one; kinds write disjoint channels.
//
// Walk: a workgroup owns one segment and one slab of FT_SLAB channels.  For every event kind that has a feature in the
// slab (and the mask's kind, in slab 0):
//   1. two searches bound the window's candidates: events are sorted by start, so e.start < stop is a prefix
//      [0, hi); the running maximum of start + duration is non-decreasing, so no event before lo = the first index whose
//      running maximum reaches the window's start can overlap.  Every event of [lo, hi) is tested itself.  A search is
//      a binary search widened to the wavefront: 64 probes per round (bm_events_lower_bound).
//   2. FT_THREADS candidates at a time: thread i computes the paint range of candidate i into LDS; then every thread
//      walks the candidates IN ORDER and records the last one that paints each of ITS window samples (thread t owns the
//      samples t, t + FT_THREADS, ...: one writer per sample, so "the later event wins" needs no atomic and has one
//      order).  owner[t] lives in LDS only to stay out of registers / scratch: no other thread reads it.
//   3. per feature of the kind: the source column of each owned sample (fp64, per thread), then the channel loop with t
//      along the lanes -- a constant row broadcasts, array reads and the stores run along consecutive columns.
// A recording index outside [0, R) is checked before any table address is formed: the segment is defaults, its mask
// false (all true without an event mask) and *flag is raised by a plain store of the constant 1.
// No atomics, no scratch, no workgroup waits for another.
//
// Measured (profiles/features_builder_vs_gather.txt; B 256, T 361, events of 200 s, a word every 0.31 s for the mask,
// interleaved with what it is compared to): 46 us for 120 mel channels (resampled) and 198 us for 1024 wav2vec channels
// (chunk; 379 MB written at 1.9 TB/s), against 29 and 169 us for the two bm_segment_gather launches over full-length
// arrays that the launch replaces (x1.57 and x1.17: SLOWER), and 281 / 843 us for torch ops.  What bounds it is the
// latency of a workgroup's chain of dependent loads (segment -> tables -> searches -> candidates -> event -> array), not
// bandwidth: hence the wavefront-wide searches and the FT_ILP loads in flight per lane.  A lane owns samples t, t + 256:
// at T = 361 the second round runs 105 of 256 lanes.
#include "bm_events.h"

#pragma clang fp contract(off)

#define FT_THREADS 256
#define FT_TMAX 4096                // samples per window (as segments.hip)
#define FT_SLAB 16                  // channels per workgroup
#define FT_ILP 8                    // loads a lane issues before it stores the first one
#define FT_MAXF 32                  // features per builder (the plan travels as a kernel argument)

enum { FT_CONSTANT = 0, FT_RESAMPLED = 1, FT_CHUNK = 2 };

struct FtSrc {                      // one feature of one recording
    const void* data;               // constant: float [n][dim]; resampled / chunk: FtArr [n]
};
struct FtArr {                      // one event's array [dim][L], read in place
    const float* base;
    long L;
    double er;                      // chunk: L / duration (0 when the duration is 0: such an event never paints)
};
struct FtFeat {
    int kind, rule, ch0, dim;
    float dflt;
};
struct FtPlan {
    FtFeat f[FT_MAXF];
};

extern "C" long bm_features_table_entry_bytes(int which) {
    return which == 0 ? (long)sizeof(BmEventKind) : which == 1 ? (long)sizeof(FtSrc) : which == 2 ? (long)sizeof(FtArr) : -1L;
}

extern "C" int bm_features_kind_fill(void* entry, const double* start, const double* dur, const double* runmax, long n) {
    BM_REQUIRE(entry && n >= 0 && n < (1L << 30) && (n == 0 || (start && dur && runmax)),
               "features table: bad event kind (%ld events)", n);
    BM_REQUIRE((((uintptr_t)start | (uintptr_t)dur | (uintptr_t)runmax) & 7) == 0,
               "features table: the event times are not 8-byte aligned");
    BmEventKind* e = (BmEventKind*)entry;
    e->start = start;
    e->dur = dur;
    e->runmax = runmax;
    e->n = n;
    return BM_OK;
}

extern "C" int bm_features_source_fill(void* entry, const void* data) {
    BM_REQUIRE(entry, "features table: null entry");
    BM_REQUIRE(((uintptr_t)data & 3) == 0, "features table: the values are not 4-byte aligned");
    ((FtSrc*)entry)->data = data;
    return BM_OK;
}

extern "C" int bm_features_array_fill(void* entry, const float* base, long L, double er) {
    BM_REQUIRE(entry && base && L >= 1 && L < (1L << 31), "features table: bad event array (%ld columns; 1 <= L < 2^31)", L);
    BM_REQUIRE(((uintptr_t)base & 3) == 0, "features table: an event array is not 4-byte aligned");
    FtArr* e = (FtArr*)entry;
    e->base = base;
    e->L = L;
    e->er = er;
    return BM_OK;
}

struct FtOverlap {
    double o0, o1;                  // the overlap, seconds
    double w0;                      // first painted window sample, a - p0 (an integer)
    double n;                       // painted samples (an integer; < 1: the event is skipped)
};

// DataSlice.overlap + start_ind / duration_ind / slice_in_parent (bm/events.py:80-111).  False: not a candidate, or
// nothing to paint.
__device__ __forceinline__ bool ft_overlap(double ws, double wstop, double p0, double sr, double es, double ed,
                                           FtOverlap& ov) {
    const double estop = es + ed;
    if (!(estop >= ws && es < wstop)) return false;
    ov.o0 = ws >= es ? ws : es;
    const double stop = wstop <= estop ? wstop : estop;
    ov.o1 = ov.o0 + (stop - ov.o0);
    const double a = rint(ov.o0 * sr);
    ov.n = rint(ov.o1 * sr) - a;
    ov.w0 = a - p0;
    return ov.n >= 1.0;
}

// Source column of paint sample j (0 <= j < ov.n) of an array event, in [0, L).
__device__ __forceinline__ long ft_column(int rule, const FtOverlap& ov, double j, double sr, double es, double ed,
                                          long L, double er) {
    long col;
    if (rule == FT_RESAMPLED) {
        const double ne = rint(((es + ed) - es) * sr);
        double first = -rint((es - ov.o0) * sr);
        first = first > 0.0 ? first : 0.0;
        first = first < ne - 1.0 ? first : ne - 1.0;
        double k = first + j;
        k = k < ne - 1.0 ? k : ne - 1.0;
        if ((double)L == ne) {
            col = (long)k;
        } else {
            const float scale = (float)L / (float)ne;
            col = (long)floorf((float)(long)k * scale);
        }
    } else {
        const double lm1 = (double)(L - 1);
        double c0 = rint((ov.o0 - es) * er);
        c0 = c0 < lm1 ? c0 : lm1;
        double c1 = rint((ov.o1 - es) * er);
        c1 = c1 > c0 + 1.0 ? c1 : c0 + 1.0;
        c1 = c1 < (double)L ? c1 : (double)L;
        const double nc = c1 - c0;
        if (nc == ov.n) {
            col = (long)(c0 + j);
        } else {
            const float scale = (float)nc / (float)ov.n;
            long q = (long)floorf((float)(long)j * scale);
            q = q < (long)nc - 1 ? q : (long)nc - 1;
            col = (long)c0 + q;
        }
    }
    col = col < L - 1 ? col : L - 1;        // the rule's own min(., L - 1); never below 0 on validated tables
    return col > 0 ? col : 0;
}

__global__ __launch_bounds__(FT_THREADS) void segment_features_kernel(
    const FtPlan plan, int NF, int NK, int mask_kind, const BmEventKind* __restrict__ kinds, const FtSrc* __restrict__ srcs,
    int R, const int* __restrict__ rec, const double* __restrict__ wstart, const double* __restrict__ wdur, int F, int T, double sr, float* __restrict__ dst, unsigned char* __restrict__ mask, int* flag) {
    __shared__ int owner[FT_TMAX];
    __shared__ int cw0[FT_THREADS];
    __shared__ int cw1[FT_THREADS];
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int c_lo = blockIdx.x * FT_SLAB;
    const int c_hi = min(F, c_lo + FT_SLAB);
    const bool mask_slab = blockIdx.x == 0;
    const int r = rec[b];                                      // rec, wstart, wdur: from the batch's first segment on
    const bool valid = (unsigned)r < (unsigned)R;
    if (!valid && tid == 0) *flag = 1;
    const double ws = wstart[b];
    const double wstop = ws + wdur[b];
    const double p0 = rint(ws * sr);
    if (mask_slab && mask_kind < 0)
        for (int w = tid; w < T; w += FT_THREADS) mask[(long)b * T + w] = 1;

    for (int k = 0; k < NK; ++k) {
        bool needed = mask_slab && k == mask_kind;
        for (int f = 0; f < NF; ++f)
            needed = needed || (plan.f[f].kind == k && plan.f[f].ch0 < c_hi && plan.f[f].ch0 + plan.f[f].dim > c_lo);
        if (!needed) continue;                                          // uniform over the workgroup

        // 1 + 2: the last event of the kind that paints each window sample (-1: none)
        for (int w = tid; w < T; w += FT_THREADS) owner[w] = -1;
        BmEventKind K;
        K.start = K.dur = K.runmax = nullptr;
        K.n = 0;
        if (valid) K = kinds[(long)r * NK + k];
        if (K.n > 0) {
            const int hi = bm_events_lower_bound(K.start, (int)K.n, wstop);   // n < 2^30: bm_features_kind_fill
            const int lo = bm_events_lower_bound(K.runmax, (int)K.n, ws);
            for (int base = lo; base < hi; base += FT_THREADS) {
                __syncthreads();                                        // the previous chunk has been read
                const int e = base + tid;
                int p = 0, q = 0;
                if (e < hi) {
                    FtOverlap ov;
                    if (ft_overlap(ws, wstop, p0, sr, K.start[e], K.dur[e], ov)) {
                        const double a = ov.w0 > 0.0 ? ov.w0 : 0.0;                     // never clips a validated window
                        const double z = ov.w0 + ov.n < (double)T ? ov.w0 + ov.n : (double)T;
                        if (a < z) {
                            p = (int)a;
                            q = (int)z;
                        }
                    }
                }
                cw0[tid] = p;
                cw1[tid] = q;
                __syncthreads();
                const int cnt = min(hi - base, FT_THREADS);
                for (int i = 0; i < cnt; ++i) {
                    const int p_i = cw0[i], q_i = cw1[i];
                    for (int w = tid; w < q_i; w += FT_THREADS)
                        if (w >= p_i) owner[w] = base + i;
                }
            }
        }
        if (mask_slab && k == mask_kind)
            for (int w = tid; w < T; w += FT_THREADS) mask[(long)b * T + w] = owner[w] >= 0 ? 1 : 0;

        // 3: the features of this kind that have channels in the slab
        for (int f = 0; f < NF; ++f) {
            const FtFeat ft = plan.f[f];
            if (ft.kind != k || ft.ch0 >= c_hi || ft.ch0 + ft.dim <= c_lo) continue;
            const int c0 = max(c_lo, ft.ch0) - ft.ch0, c1 = min(c_hi, ft.ch0 + ft.dim) - ft.ch0;
            float* __restrict__ out = dst + ((long)b * F + ft.ch0) * T;
            const void* data = valid ? srcs[(long)r * NF + f].data : nullptr;
            for (int w = tid; w < T; w += FT_THREADS) {
                const int e = owner[w];
                const float* __restrict__ src = nullptr;                // element c of the sample: src[c * stride]
                long stride = 0;
                if (e >= 0) {
                    if (ft.rule == FT_CONSTANT) {
                        src = (const float*)data + (long)e * ft.dim;
                        stride = 1;
                    } else {
                        const double es = K.start[e], ed = K.dur[e];
                        FtOverlap ov;
                        ft_overlap(ws, wstop, p0, sr, es, ed, ov);      // true: e painted w
                        const FtArr A = ((const FtArr*)data)[e];
                        src = A.base + ft_column(ft.rule, ov, (double)w - ov.w0, sr, es, ed, A.L, A.er);
                        stride = A.L;
                    }
                }
                float* __restrict__ o = out + (long)c0 * T + w;
                if (c1 - c0 == FT_SLAB) {
                    // a whole slab (the common case of a wide feature): FT_ILP loads are issued before their stores
                    for (int h = 0; h < FT_SLAB; h += FT_ILP) {
                        float v[FT_ILP];
                        if (src) {
                            const float* __restrict__ p = src + (long)(c0 + h) * stride;
#pragma unroll
                            for (int u = 0; u < FT_ILP; ++u) v[u] = p[(long)u * stride];
                        } else {
#pragma unroll
                            for (int u = 0; u < FT_ILP; ++u) v[u] = ft.dflt;
                        }
#pragma unroll
                        for (int u = 0; u < FT_ILP; ++u) o[(long)(h + u) * T] = v[u];
                    }
                } else {
                    for (int c = c0; c < c1; ++c) o[(long)(c - c0) * T] = src ? src[(long)c * stride] : ft.dflt;
                }
            }
        }
    }
}

extern "C" int bm_segment_features(const int* feat_table, const float* feat_default, int NF, int NK, int mask_kind,
                                   const void* kinds, const void* srcs, int R, const int* rec, const double* wstart,
                                   const double* wdur, long n_index, long first, int B, int F, int T, double sr,
                                   float* dst, unsigned char* mask, int* flag, void* stream) {
    BM_REQUIRE(B >= 0 && F >= 0 && T > 0 && R >= 0 && NF >= 0 && NK >= 0,
               "segment_features: bad shape B = %d, F = %d, T = %d, R = %d, %d features of %d kinds", B, F, T, R, NF, NK);
    BM_REQUIRE(mask_kind >= -1 && mask_kind < NK, "segment_features: the mask's kind %d of %d", mask_kind, NK);
    BM_REQUIRE(sr > 0.0 && sr < 1e12, "segment_features: sample rate %g", sr);
    BM_REQUIRE(first >= 0 && first + B <= n_index, "segment_features: segments [%ld, %ld) of %ld", first, first + B, n_index);
    if (NF > FT_MAXF)
        return bm_set_error(BM_ERR_UNSUPPORTED, "segment_features: %d features, the limit is %d", NF, FT_MAXF);
    if (T > FT_TMAX)
        return bm_set_error(BM_ERR_UNSUPPORTED, "segment_features: T = %d exceeds the limit of %d samples per window", T,
                            FT_TMAX);
    BM_REQUIRE(B <= 65535, "segment_features: B = %d, the limit is 65535", B);
    BM_REQUIRE(NF == 0 || (feat_table && feat_default), "segment_features: null feature table");
    // the plan (HOST memory): rows {kind, rule, first channel, channels}; the rows tile [0, F) in order, so that every
    // channel is written by exactly one feature
    FtPlan plan;
    int next = 0;
    for (int f = 0; f < NF; ++f) {
        const int* row = feat_table + 4 * f;
        BM_REQUIRE(row[0] >= 0 && row[0] < NK && row[1] >= FT_CONSTANT && row[1] <= FT_CHUNK && row[3] >= 1 && row[2] == next,
                   "segment_features: feature %d = {kind %d, rule %d, channels %d + %d} (of %d kinds; expected channel %d)",
                   f, row[0], row[1], row[2], row[3], NK, next);
        plan.f[f].kind = row[0];
        plan.f[f].rule = row[1];
        plan.f[f].ch0 = row[2];
        plan.f[f].dim = row[3];
        plan.f[f].dflt = feat_default[f];
        next += row[3];
    }
    for (int f = NF; f < FT_MAXF; ++f) plan.f[f] = FtFeat{-1, 0, 0, 0, 0.f};
    BM_REQUIRE(next == F, "segment_features: the features have %d channels, the batch %d", next, F);
    if (B == 0) return BM_OK;
    BM_REQUIRE(rec && wstart && wdur && mask && flag && (F == 0 || dst) && (NK == 0 || R == 0 || kinds) &&
               (NF == 0 || R == 0 || srcs), "segment_features: null pointer");
    BM_REQUIRE(((uintptr_t)dst & 3) == 0 && (((uintptr_t)wstart | (uintptr_t)wdur) & 7) == 0,
               "segment_features: dst is not 4-byte aligned, or the window times are not 8-byte aligned");
    const int slabs = F > 0 ? cdiv(F, FT_SLAB) : 1;
    hipLaunchKernelGGL(segment_features_kernel, dim3(slabs, B), dim3(FT_THREADS), 0, (hipStream_t)stream, plan, NF, NK,
                       mask_kind, (const BmEventKind*)kinds, (const FtSrc*)srcs, R, rec + first, wstart + first, wdur + first, F, T, sr, dst,
                       mask, flag);
    return bm_check_launch("segment_features");
}
