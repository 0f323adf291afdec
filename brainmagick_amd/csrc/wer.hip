// The word label of every kept test segment (bm/wer.py:48, 58-66): the collection half of the word-level retrieval
// metric, one launch per test batch.
//     x      = the batch's full features [B][F][T] fp32, read in place (channel c = the WordHash feature)
//     mask   = reject_mask [B] bytes (true = the segment was kept), or null: every row is kept
//     dest[n0 + r] = label of the kept row of rank r, rows in ascending order: the order of `word_hash[reject_mask]`
// The label is the word-label rule of bm_events.h with a reach of 2 samples (bm/wer.py:58-64).
//
// Flag word (one int32, owned by retrieval.py -- not the Solver's):
//     1  every candidate of a kept row is zero (the reference's `assert (wh != 0).all()`, bm/wer.py:65); dest gets 0
//     2  the chosen value is not finite, not an integer, or |v| >= 2^63; dest gets 0 (not finite, too large) or the
//        value truncated towards zero
//     4  n0 + rank reached dest_len: nothing is written there (the host checks the length first; this is the kernel's
//        own bound)
// The rows that raise a bit do not disturb the others: every kept row gets its element, and only those are written.
//
// Walk: ONE workgroup of WH_THREADS lanes strides over the rows.  A row's rank = kept rows of earlier strides (a
// running count every lane holds) + kept rows of earlier wavefronts of the stride (LDS) + kept lower lanes of its own
// wavefront (ballot + popcount).  No atomics anywhere: the flag's bits are OR-ed over the wavefront, folded through LDS
// and stored by lane 0 alone -- the launch is the word's only writer on its stream.  Two runs give the same bits.
// A batch is a few hundred rows and the launch reads 5 floats and a byte per row: it is launch latency, and one
// workgroup keeps it free of a second pass or a cross-workgroup scan.
#include "bm_block.h"
#include "bm_events.h"

#define WH_THREADS 256
#define WH_WAVES (WH_THREADS / BM_WAVE)

__global__ __launch_bounds__(WH_THREADS) void word_hash_pick_kernel(const float* __restrict__ x, long row_stride,
                                                                    long offset, int t0,
                                                                    const unsigned char* __restrict__ mask, int B,
                                                                    long* __restrict__ dest, long dest_len, long n0,
                                                                    int* flag) {
    __shared__ int wave_n[WH_WAVES];
    __shared__ int wave_bits[WH_WAVES];
    const int tid = threadIdx.x;
    const int lane = tid & (BM_WAVE - 1), wave = tid >> 6;
    long base = n0;
    int bits = 0;
    for (int b0 = 0; b0 < B; b0 += WH_THREADS) {
        const int b = b0 + tid;
        const bool keep = b < B && (!mask || mask[b] != 0);
        const unsigned long long kept = __ballot(keep);
        if (lane == 0) wave_n[wave] = __popcll(kept);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < WH_WAVES; ++w) {
            const int n = wave_n[w];
            before += w < wave ? n : 0;
            total += n;
        }
        if (keep) {
            const float* p = x + (long)b * row_stride + offset;       // &x[b][c][t0]; the host checked 0 <= t0, t0 + 2 < T
            const BmWordLabel w = bm_word_label_classify(bm_word_label_pick<2>(p, t0));
            bits |= w.is_zero ? 1 : w.is_illegal ? 2 : 0;
            const long r = base + before + __popcll(kept & ((1ull << lane) - 1ull));
            if (r < dest_len)
                dest[r] = w.label;
            else
                bits |= 4;
        }
        base += total;
        __syncthreads();                                              // wave_n is rewritten by the next stride
    }
    const int all = bm_block_or<WH_WAVES>(bm_wave_or(bits), wave_bits);
    if (tid == 0 && all) *flag = *flag | all;
}

extern "C" int bm_word_hash_pick(const float* x, int B, int F, int T, int c, int t0, const unsigned char* mask,
                                 long* dest, long dest_len, long n0, int* flag, void* stream) {
    BM_REQUIRE(B >= 0 && F > 0 && T > 0, "word_hash_pick: bad shape B = %d, F = %d, T = %d", B, F, T);
    BM_REQUIRE(c >= 0 && c < F, "word_hash_pick: channel %d of %d", c, F);
    BM_REQUIRE(t0 >= 0 && (long)t0 + 2 < T, "word_hash_pick: check_at_time = %d needs samples %d .. %d of a window of %d",
               t0, t0 - 2, t0 + 2, T);
    BM_REQUIRE(n0 >= 0 && dest_len >= 0 && n0 <= dest_len, "word_hash_pick: first index %ld of %ld", n0, dest_len);
    if (B == 0) return BM_OK;
    BM_REQUIRE(x && dest && flag, "word_hash_pick: null pointer");
    BM_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)dest & 7) == 0 && ((uintptr_t)flag & 3) == 0,
               "word_hash_pick: misaligned pointer");
    hipLaunchKernelGGL(word_hash_pick_kernel, dim3(1), dim3(WH_THREADS), 0, (hipStream_t)stream, x, (long)F * T,
                       (long)c * T + t0, t0, mask, B, dest, dest_len, n0, flag);
    return bm_check_launch("word_hash_pick");
}
