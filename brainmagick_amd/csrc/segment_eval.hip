// The segment-level evaluation's collection (scripts/run_eval_probs.py:27-57, 105-130, 141-149, 155-158): the labels of
// every kept test segment, one launch per test batch, and the first occurrence of every segment over the collected epoch.
//
// bm_segment_eval_labels -- for the kept rows of a batch in ascending order, rank r: dest[n0 + r][0 .. 7) =
//     word_hash, word_index, sequence_id, segment_id, subject_index, recording_index, word_event        (int64)
//   word_hash   the word-label rule of bm_events.h with a reach of 1 sample (:122-130; bm/wer.py has reach 2).  All zero
//               is legal (the assert of :131 is commented out) and stored as 0; a value that is no legal label raises
//               bit 1.
//   word_event  the index, in the recording's word table, of the LAST word event in table order that covers column t0
//               by the arithmetic of _get_extra_info (:43-47), in fp64 and uncontracted:
//                   a = sr * (ev.start - wstart);  b = a + sr * ev.duration;
//                   covered iff max(0, trunc(a)) <= t0 < min(T, trunc(b))
//               (int() truncates; the features builder rounds: they differ at half-sample onsets).  trunc(b) < 0 is an
//               empty span.  The reference paints every word event of the window's selection in order and reads column
//               t0: the last one that covers it.  An event outside the selection cannot cover a column of [0, T), so no
//               selection is made.  -1: no event covers t0.
//   word_index, sequence_id, segment_id    row word_event of the recording's word-info array [n][3]; -1, -1, 0 without a
//               covering event (segment 0 is the reference's hash("-1_-1"), shared by every such row).
//   subject_index, recording_index         the epoch's arrays at the row.
// Flag word (one int32, owned by retrieval.py): 1 the word hash is no legal label; 2 n0 + rank reached dest_rows
// (nothing is written there); 4 the row's recording index is outside [0, R), checked before any table address is formed
// (the row gets the no-word values).
//
// Walk: a wavefront owns one row, a workgroup SE_WAVES consecutive rows.  ONE workgroup striding over the batch, as
// wer.hip does, does not suffice here: a row is a chain of dependent loads (row -> recording -> tables -> two searches ->
// candidates -> word info), and with a row per lane the searches would be per-lane binary searches of log2 n dependent
// loads each; with a row per wavefront they are the wavefront-wide searches of features.hip (ceil(log64 n) rounds) and
// the rows of a batch run on as many compute units as there are rows / SE_WAVES.  The rank needs no other workgroup:
// every workgroup counts the kept rows in front of its own from the mask bytes (a few hundred, cached), by per-lane
// counts folded over the wavefront and through LDS, plus the kept rows of its earlier wavefronts.  One writer per
// element of dest (lanes 0 .. 6 of the row's wavefront).  The flag's bits are folded per workgroup; a workgroup that has
// any adds them with ONE atomicOr (several workgroups share the word; an OR does not depend on the order of arrival).
// Two runs give the same bits.
//
// Candidate bounds (both conservative by one sample, every event between them is tested itself): a covering event has
// a < t0 + 1, so start < wstart + (t0 + 2) / sr -- a prefix [0, hi) of the table sorted by start; and b >= t0 + 1, so
// no event in front of lo = the first index whose running maximum of start + duration reaches wstart + (t0 - 1) / sr.
// The candidates are walked from the back, 64 at a time; the first chunk with a hit ends the walk.  Every loop is
// bounded by the table length.
//
// bm_first_occurrence -- the `seen_segment_hashes` loop of :141-149 over the whole epoch (first occurrences in row
// order do not depend on the batching): launch 1 atomicMin(&first[ids[i]], i) into an int32 table the caller filled with
// INT_MAX (an integer minimum does not depend on the order of arrival); launch 2 mask[i] = first[ids[i]] == i and
// first_row[i] = first[ids[i]].  An id outside [0, n_ids) is checked before the table is addressed: bit 8, mask 0,
// first_row -1.
#include <climits>

#include "bm_block.h"
#include "bm_events.h"

#pragma clang fp contract(off)

#define SE_THREADS 256
#define SE_WAVES (SE_THREADS / BM_WAVE)
#define SE_COLS 7

struct SeInfo {                     // one recording's word info [n][3] int64: word_index, sequence_id, segment_id
    const long* rows;
    long n;
};

extern "C" long bm_segment_eval_info_entry_bytes(void) { return (long)sizeof(SeInfo); }

extern "C" int bm_segment_eval_info_fill(void* entry, const long* rows, long n) {
    BM_REQUIRE(entry && n >= 0 && n < (1L << 30) && (n == 0 || rows), "segment_eval info: bad word info (%ld words)", n);
    BM_REQUIRE(((uintptr_t)rows & 7) == 0, "segment_eval info: the word info is not 8-byte aligned");
    SeInfo* e = (SeInfo*)entry;
    e->rows = rows;
    e->n = n;
    return BM_OK;
}

__global__ __launch_bounds__(SE_THREADS) void segment_eval_labels_kernel(
    const float* __restrict__ x, long row_stride, long offset, int t0, int T, const unsigned char* __restrict__ mask, int B,
    const int* __restrict__ rec, const double* __restrict__ wstart, const long* __restrict__ subject,
    const long* __restrict__ recording, const BmEventKind* __restrict__ kinds, int NK, int word_kind,
    const SeInfo* __restrict__ infos, int R, double sr, double reach_hi, double reach_lo, long* __restrict__ dest,
    long dest_rows, long n0, int* flag) {
    __shared__ int wave_n[SE_WAVES];
    __shared__ int wave_keep[SE_WAVES];
    __shared__ int wave_bits[SE_WAVES];
    const int tid = threadIdx.x;
    const int lane = tid & (BM_WAVE - 1), wave = tid >> 6;
    const int b0 = blockIdx.x * SE_WAVES;
    const int b = b0 + wave;
    const bool keep = b < B && (!mask || mask[b] != 0);                  // uniform over the wavefront
    int cnt = 0;
    for (int i = tid; i < b0; i += SE_THREADS) cnt += (!mask || mask[i] != 0) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) {
        wave_n[wave] = cnt;
        wave_keep[wave] = keep ? 1 : 0;
    }
    __syncthreads();
    long rank = n0;
#pragma unroll
    for (int w = 0; w < SE_WAVES; ++w) rank += wave_n[w] + (w < wave ? wave_keep[w] : 0);

    int bits = 0;
    if (keep) {
        const float* p = x + (long)b * row_stride + offset;              // &x[b][c][t0]; the host checked 0 <= t0, t0 + 1 < T
        const BmWordLabel w = bm_word_label_classify(bm_word_label_pick<1>(p, t0));
        if (w.is_illegal) bits |= 1;

        const int r = rec[b];
        const bool valid = (unsigned)r < (unsigned)R;
        if (!valid) bits |= 4;
        long event = -1;
        BmEventKind K;
        K.start = K.dur = K.runmax = nullptr;
        K.n = 0;
        SeInfo I;
        I.rows = nullptr;
        I.n = 0;
        if (valid) {
            K = kinds[(long)r * NK + word_kind];
            I = infos[r];
        }
        const int n = (int)(K.n < I.n ? K.n : I.n);                      // < 2^30: the fills; equal on checked tables
        if (n > 0) {
            const double ws = wstart[b];
            const int hi = bm_events_lower_bound(K.start, n, ws + reach_hi);
            const int lo = bm_events_lower_bound(K.runmax, n, ws + reach_lo);
            for (int top = hi; top > lo; top -= BM_WAVE) {
                const int e = top - 1 - lane;                            // lane 0 tests the last candidate
                bool covered = false;
                if (e >= lo) {
                    const double a = sr * (K.start[e] - ws);
                    const double z = a + sr * K.dur[e];
                    const double ta = trunc(a), tz = trunc(z);
                    const double s0 = ta > 0.0 ? ta : 0.0;
                    const double s1 = tz < (double)T ? tz : (double)T;
                    covered = s0 <= (double)t0 && (double)t0 < s1;
                }
                const unsigned long long hit = __ballot(covered);
                if (hit) {
                    event = top - 1 - (__ffsll((long long)hit) - 1);
                    break;                                               // uniform: `hit` is the wavefront's
                }
            }
        }
        if (rank < dest_rows) {
            if (lane < SE_COLS) {
                long value;
                if (lane == 0)
                    value = w.label;
                else if (lane <= 3)
                    value = event >= 0 ? I.rows[event * 3 + (lane - 1)] : (lane == 3 ? 0L : -1L);
                else if (lane == 4)
                    value = subject[b];
                else if (lane == 5)
                    value = recording[b];
                else
                    value = event;
                dest[rank * SE_COLS + lane] = value;
            }
        } else {
            bits |= 2;
        }
    }
    const int all = bm_block_or<SE_WAVES>(bits, wave_bits);          // bits: uniform over the wavefront
    if (tid == 0 && all) atomicOr(flag, all);
}

extern "C" int bm_segment_eval_labels(const float* x, int B, int F, int T, int c, int t0, const unsigned char* mask,
                                      const int* rec, const double* wstart, const long* subject_index,
                                      const long* recording_index, long n_index, long first, const void* kinds, int NK,
                                      int word_kind, const void* infos, int R, double sr, long* dest, long dest_rows,
                                      long n0, int* flag, void* stream) {
    BM_REQUIRE(B >= 0 && F > 0 && T > 0 && R >= 0, "segment_eval_labels: bad shape B = %d, F = %d, T = %d, R = %d", B, F, T, R);
    BM_REQUIRE(c >= 0 && c < F, "segment_eval_labels: channel %d of %d", c, F);
    BM_REQUIRE(t0 >= 0 && (long)t0 + 1 < T, "segment_eval_labels: check_at_time = %d needs samples %d .. %d of a window of %d",
               t0, t0 - 1, t0 + 1, T);
    BM_REQUIRE(NK > 0 && word_kind >= 0 && word_kind < NK, "segment_eval_labels: the word kind %d of %d", word_kind, NK);
    BM_REQUIRE(sr > 0.0 && sr < 1e12, "segment_eval_labels: sample rate %g", sr);
    BM_REQUIRE(first >= 0 && first + B <= n_index, "segment_eval_labels: segments [%ld, %ld) of %ld", first, first + B, n_index);
    BM_REQUIRE(n0 >= 0 && dest_rows >= 0 && n0 <= dest_rows, "segment_eval_labels: first row %ld of %ld", n0, dest_rows);
    if (B == 0) return BM_OK;
    BM_REQUIRE(x && dest && flag && rec && wstart && subject_index && recording_index && (R == 0 || (kinds && infos)),
               "segment_eval_labels: null pointer");
    BM_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)rec & 3) == 0 && ((uintptr_t)flag & 3) == 0 &&
               (((uintptr_t)dest | (uintptr_t)wstart | (uintptr_t)subject_index | (uintptr_t)recording_index) & 7) == 0,
               "segment_eval_labels: misaligned pointer");
    hipLaunchKernelGGL(segment_eval_labels_kernel, dim3(cdiv(B, SE_WAVES)), dim3(SE_THREADS), 0, (hipStream_t)stream, x,
                       (long)F * T, (long)c * T + t0, t0, T, mask, B, rec + first, wstart + first, subject_index + first,
                       recording_index + first, (const BmEventKind*)kinds, NK, word_kind, (const SeInfo*)infos, R, sr,
                       (t0 + 2) / sr, (t0 - 1) / sr, dest, dest_rows, n0, flag);
    return bm_check_launch("segment_eval_labels");
}

__global__ __launch_bounds__(SE_THREADS) void first_occurrence_min_kernel(const long* __restrict__ ids, int N, long n_ids,
                                                                          int* __restrict__ first) {
    const int i = blockIdx.x * SE_THREADS + threadIdx.x;
    if (i >= N) return;
    const long id = ids[i];
    if (id >= 0 && id < n_ids) atomicMin(&first[id], i);
}

__global__ __launch_bounds__(SE_THREADS) void first_occurrence_mask_kernel(const long* __restrict__ ids, int N, long n_ids,
                                                                           const int* __restrict__ first,
                                                                           unsigned char* __restrict__ mask,
                                                                           int* __restrict__ first_row, int* flag) {
    __shared__ int wave_bits[SE_WAVES];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * SE_THREADS + tid;
    int bits = 0;
    if (i < N) {
        const long id = ids[i];
        int f = -1;
        if (id >= 0 && id < n_ids)
            f = first[id];
        else
            bits = 8;
        mask[i] = f == i ? 1 : 0;
        first_row[i] = f;
    }
    const int all = bm_block_or<SE_WAVES>(bm_wave_or(bits), wave_bits);
    if (tid == 0 && all) atomicOr(flag, all);
}

extern "C" int bm_first_occurrence(const long* ids, long N, long n_ids, int* first, unsigned char* mask, int* first_row,
                                   int* flag, void* stream) {
    BM_REQUIRE(N >= 0 && N < (1L << 31), "first_occurrence: %ld rows; 0 <= N < 2^31", N);
    BM_REQUIRE(n_ids >= 0, "first_occurrence: %ld ids", n_ids);
    if (N == 0) return BM_OK;
    BM_REQUIRE(ids && mask && first_row && flag && (n_ids == 0 || first), "first_occurrence: null pointer");
    BM_REQUIRE(((uintptr_t)ids & 7) == 0 && (((uintptr_t)first | (uintptr_t)first_row | (uintptr_t)flag) & 3) == 0,
               "first_occurrence: misaligned pointer");
    const int blocks = cdiv(N, SE_THREADS);
    hipLaunchKernelGGL(first_occurrence_min_kernel, dim3(blocks), dim3(SE_THREADS), 0, (hipStream_t)stream, ids, (int)N,
                       n_ids, first);
    int rc = bm_check_launch("first_occurrence (min)");
    if (rc != BM_OK) return rc;
    hipLaunchKernelGGL(first_occurrence_mask_kernel, dim3(blocks), dim3(SE_THREADS), 0, (hipStream_t)stream, ids, (int)N,
                       n_ids, first, mask, first_row, flag);
    return bm_check_launch("first_occurrence (mask)");
}
