// The data loader's batch (bm/dataset.py:349-364 __getitem__, 263-278 collate_fn, 172-175 the baseline of mne.Epochs) as a
// gather of windows out of recordings that are resident on the device:
//     dst[b][c][t] = src_r[c][start_b + t] - mean_b,c     for c < rows_r,         +0.0 for rows_r <= c < C,
// r = rec[first + b], start_b = start[first + b]; mean_b,c = the mean of the row's window samples [b0, b1] (inclusive),
// or nothing at all when b0 < 0 (no baseline: the features, or baseline=None -- the bits of the source pass through).
// The recordings are read IN PLACE through a device table (SgRec: address, samples per row, rows -- as spectral.hip
// describes its matrices): no launch per recording, no concatenated copy.  rec / start are the arrays of a whole epoch,
// a batch is the offset `first` into them.  One launch per tensor; bytes (the features mask) have a kernel of their own.
//
// Range check: a row's source address is formed by ONE thread, after it has checked rec against [0, R) and start against
// [0, n - T]; every other thread only sees the finished pointer (or null: the whole segment is +0.0 and bit 0 of *flag
// is raised by a plain store of the constant 1 -- no atomic, every writer stores the same word).
//
// Walk (fp32): the output is one flat array of B * C rows of T floats; a workgroup owns RB = min(SG_LDS / T,
// SG_RMAX) consecutive rows, i.e. one contiguous span of the output.
//   1. thread i < rows of the span: the descriptor of row i (checked source pointer) into LDS.
//   2. all threads: the span's samples into LDS, flat -- a wavefront reads 64 consecutive floats of a source row (source
//      rows are only 4-byte aligned: start is arbitrary), SG_UNROLL loads in flight per lane.  The LDS image is shifted by
//      (address of the span / 4) % 4 floats, so that 16-byte groups of the OUTPUT are 16-byte groups of LDS.
//   3. thread i < rows: the baseline mean of row i -- an fp64 sum of the staged fp32 samples in ascending t, divided
//      once: ONE order, so a segment has the same bits alone or among others, on every grid and in every compute mode.
//   4. all threads: (float)((double)x - mean) -- one rounding -- as 16-byte stores over the aligned body of the span
//      (T is usually odd: rows are not 16-byte aligned, the flat span is) and 4-byte stores on its at most 3 + 3 edge
//      elements.  Every element of dst is written exactly once, by the workgroup that owns its row.
// A NaN inside the baseline window makes the mean, hence the row, NaN; outside it, it passes through as x - mean does.
// No atomics, no workgroup waits for another, no scratch.
//
// Measured at the cfg5 mix (256 segments of 273 / 128 channels padded to 273, T = 361, baseline 0..60, recordings of
// 1 GB resident: from HBM; profiles/segment_loader_vs_torch.txt): 48 us for the MEG (175 MB read + written: 3.6 TB/s,
// 0.7 of what a plain device copy reaches on the same box), 25 us for 120 feature rows.  What bounds it: with the stores
// switched off the MEG launch takes 38 us, with the source loads switched off 35 us; the features 14.5 and 14.3 of
// their 25 -- a workgroup's loads and its stores run one after the other (two barriers between them) and only other
// workgroups of the CU fill the gaps, so the launch costs nearly the sum of its two halves; the baseline pass (one lane
// per row) is about 13 us of the load half.  Neither the 4-byte loads nor the 16-byte stores alone are the limit.
// Staging size and depth were measured (same box, interleaved, MEG / features in us): 8192 floats with 4 loads in
// flight 60 / 31, with 8 54 / 29; 4096 with 4 50 / 27, with 8 47 / 25 (kept), with 16 51 / 27; 2048 with 8 54 / 27;
// 3072 with 12 52 / 26; 512 threads 52 / 26.  Tried and dropped: a persistent workgroup that holds the NEXT span's 16
// loads in registers while it averages and stores the current one (53 / 27: the wait for those loads at the top of the
// loop also waits for the stores behind them, as lowpass.hip found).
#include "bm_common.h"

#define SG_THREADS 256
#define SG_LDS 4096                 // floats of staged samples per workgroup (+ 4 of alignment shift)
#define SG_UNROLL 8                 // source loads a lane issues before it stores the first one to LDS
#define SG_RMAX SG_THREADS          // rows per workgroup: one descriptor thread per row

struct SgRec {
    const void* base;       // rows x n elements, unit stride inside a row, n elements between rows
    long n;                 // samples per row
    int rows;               // C_r
    int pad_;
};

extern "C" long bm_segment_table_entry_bytes(void) { return (long)sizeof(SgRec); }

extern "C" int bm_segment_table_fill(void* entry, const void* base, long n, int rows) {
    BM_REQUIRE(entry && n >= 0 && rows >= 0 && (rows == 0 || n == 0 || base), "segment table: bad recording (%d rows of %ld)",
               rows, n);
    SgRec* e = (SgRec*)entry;
    e->base = base;
    e->n = n;
    e->rows = rows;
    e->pad_ = 0;
    return BM_OK;
}

// A pointer that went through LDS has lost its address space: say again that it is global memory (a global_load, not
// a flat one that also waits on the LDS counter).
typedef const float __attribute__((address_space(1))) * SgGlobalF;
typedef const unsigned char __attribute__((address_space(1))) * SgGlobalB;
__device__ __forceinline__ SgGlobalF sg_global(const float* p) { return reinterpret_cast<SgGlobalF>(reinterpret_cast<uintptr_t>(p)); }

// The checked source of output row (b, c): null when the row is +0.0 (a padded channel, or a segment out of range --
// then *flag is raised).  Nothing is read through an unchecked index and no address is formed from one.
template <typename E>
__device__ __forceinline__ const E* sg_row_source(const SgRec* __restrict__ table, int R, const int* __restrict__ rec,
                                                  const int* __restrict__ start, long first, int b, int c, int T,
                                                  int* flag) {
    const int r = rec[first + b];
    const long st = start[first + b];
    if ((unsigned)r >= (unsigned)R) {
        *flag = 1;
        return nullptr;
    }
    const SgRec m = table[r];
    if (st < 0 || st > m.n - T) {
        *flag = 1;
        return nullptr;
    }
    if (c >= m.rows) return nullptr;
    return (const E*)m.base + (long)c * m.n + st;
}

template <bool BASE>
__global__ __launch_bounds__(SG_THREADS) void segment_gather_kernel(const SgRec* __restrict__ table, int R,
                                                                    const int* __restrict__ rec,
                                                                    const int* __restrict__ start, long first, int rows,
                                                                    int C, int T, int bl0, int bl1, int RB, int shift0,
                                                                    BmFastDiv div_c, BmFastDiv div_t,
                                                                    float* __restrict__ dst, int* flag) {
    __shared__ __attribute__((aligned(16))) float smp[SG_LDS + 4];
    __shared__ const float* src[SG_RMAX];
    __shared__ double mean[SG_RMAX];
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * RB;
    const int nr = min(RB, rows - row0);
    const long e0 = (long)row0 * T;                         // first output element of the span
    const int n = nr * T;
    const int sh = (int)((e0 + shift0) & 3);                // LDS index of element e: e - e0 + sh
    if (tid < nr) {
        const unsigned row = (unsigned)(row0 + tid);
        const unsigned b = bm_div(row, div_c);
        src[tid] = sg_row_source<float>(table, R, rec, start, first, (int)b, (int)(row - b * C), T, flag);
    }
    __syncthreads();
    for (int i0 = tid; i0 < n; i0 += SG_UNROLL * SG_THREADS) {     // SG_UNROLL loads issued before the first is stored
        float v[SG_UNROLL];
#pragma unroll
        for (int u = 0; u < SG_UNROLL; ++u) {
            const int i = i0 + u * SG_THREADS;
            v[u] = 0.f;
            if (i < n) {
                const unsigned r = bm_div((unsigned)i, div_t);
                const float* p = src[r];
                if (p) v[u] = *sg_global(p + (i - (int)r * T));
            }
        }
#pragma unroll
        for (int u = 0; u < SG_UNROLL; ++u) {
            const int i = i0 + u * SG_THREADS;
            if (i < n) smp[sh + i] = v[u];
        }
    }
    if (BASE) {
        __syncthreads();
        if (tid < nr) {
            double m = 0.0;
            if (src[tid]) {
                const float* x = smp + sh + tid * T;
                double s = 0.0;
                int t = bl0;
                for (; t + 8 <= bl1 + 1; t += 8) {              // eight LDS reads in flight, the additions in order
                    float a[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) a[u] = x[t + u];
#pragma unroll
                    for (int u = 0; u < 8; ++u) s += (double)a[u];
                }
                for (; t <= bl1; ++t) s += (double)x[t];
                m = s / (double)(bl1 - bl0 + 1);
            }
            mean[tid] = m;
        }
    }
    __syncthreads();
    float* base = dst + e0 - sh;                            // base + j: the element staged at smp[j]; 16-byte aligned
    const int end = sh + n;
    for (int j = tid * 4; j < end; j += SG_THREADS * 4) {
        const f32x4 v = *(const f32x4*)(smp + j);
        float o[4] = {v.x, v.y, v.z, v.w};
        if (BASE) {
            const int l = j - sh;                               // may be negative in the first group: those are skipped
            unsigned r = l >= 0 ? bm_div((unsigned)l, div_t) : 0u;
            int t = l - (int)r * T;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (t >= T) {                                   // T >= 1: at most one row ends per element
                    t -= T;
                    ++r;
                }
                if (l + k >= 0 && j + k < end) o[k] = (float)((double)o[k] - mean[r]);
                ++t;
            }
        }
        if (j >= sh && j + 4 <= end) {
            f32x4 w;
            w.x = o[0];
            w.y = o[1];
            w.z = o[2];
            w.w = o[3];
            *(f32x4*)(base + j) = w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j + k >= sh && j + k < end) base[j + k] = o[k];
        }
    }
}

// Bytes (the features mask, [M][n] per recording): one element per thread over the flat output, no baseline.  Every
// thread checks its own segment (rec, start and the table entry are re-read per byte, from cache) and stores one byte:
// sized for the M = 1 mask of the reference (92 KB per batch, launch latency).  A mask of many rows would want the row
// descriptors and the wide stores of the fp32 kernel; nothing here stops it, it is only slow.
__global__ __launch_bounds__(SG_THREADS) void segment_gather_bytes_kernel(const SgRec* __restrict__ table, int R,
                                                                          const int* __restrict__ rec,
                                                                          const int* __restrict__ start, long first,
                                                                          long total, int C, int T, BmFastDiv div_c,
                                                                          BmFastDiv div_t, unsigned char* __restrict__ dst,
                                                                          int* flag) {
    const long e = (long)blockIdx.x * SG_THREADS + threadIdx.x;
    if (e >= total) return;
    const unsigned row = bm_div((unsigned)e, div_t);
    const int t = (int)(e - (long)row * T);
    const unsigned b = bm_div(row, div_c);
    const unsigned char* p = sg_row_source<unsigned char>(table, R, rec, start, first, (int)b, (int)(row - b * C), T, flag);
    dst[e] = p ? *reinterpret_cast<SgGlobalB>(reinterpret_cast<uintptr_t>(p + t)) : (unsigned char)0;
}

extern "C" int bm_segment_gather(const void* table, int R, const int* rec, const int* start, long n_index, long first,
                                 int B, int C, int T, int base0, int base1, int elem_bytes, void* dst, int* flag,
                                 void* stream) {
    BM_REQUIRE(B >= 0 && C >= 0 && T > 0 && R >= 0, "segment_gather: bad shape B = %d, C = %d, T = %d, R = %d", B, C, T, R);
    BM_REQUIRE(elem_bytes == 4 || elem_bytes == 1, "segment_gather: elements of %d bytes (4: fp32, 1: bytes)", elem_bytes);
    BM_REQUIRE(first >= 0 && first + B <= n_index, "segment_gather: segments [%ld, %ld) of %ld", first, first + B, n_index);
    BM_REQUIRE((long)B * C * T < (1L << 31), "segment_gather: B * C * T = %ld, the limit is 2^31", (long)B * C * T);
    const bool has_base = base0 >= 0;
    BM_REQUIRE(!has_base || (elem_bytes == 4 && base0 <= base1 && base1 < T),
               "segment_gather: baseline [%d, %d] of a window of %d (fp32 only)", base0, base1, T);
    if (B == 0 || C == 0) return BM_OK;
    BM_REQUIRE(table && rec && start && dst && flag, "segment_gather: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const SgRec* tb = (const SgRec*)table;
    const BmFastDiv div_c = bm_fastdiv((unsigned)C), div_t = bm_fastdiv((unsigned)T);
    if (elem_bytes == 1) {
        const long total = (long)B * C * T;
        hipLaunchKernelGGL(segment_gather_bytes_kernel, dim3(cdiv(total, SG_THREADS)), dim3(SG_THREADS), 0, s, tb, R, rec,
                           start, first, total, C, T, div_c, div_t, (unsigned char*)dst, flag);
        return bm_check_launch("segment_gather");
    }
    if (T > SG_LDS)
        return bm_set_error(BM_ERR_UNSUPPORTED, "segment_gather: T = %d exceeds the limit of %d samples per window (a "
                            "workgroup stages whole rows)", T, SG_LDS);
    BM_REQUIRE(((uintptr_t)dst & 3) == 0, "segment_gather: dst is not 4-byte aligned");
    const int rows = B * C;
    int RB = SG_LDS / T;
    RB = RB > SG_RMAX ? SG_RMAX : RB;
    const int shift0 = (int)(((uintptr_t)dst >> 2) & 3);
    const int blocks = cdiv(rows, RB);
#define SG_LAUNCH(BASE)                                                                                               \
    hipLaunchKernelGGL((segment_gather_kernel<BASE>), dim3(blocks), dim3(SG_THREADS), 0, s, tb, R, rec, start, first, \
                       rows, C, T, base0, base1, RB, shift0, div_c, div_t, (float*)dst, flag)
    if (has_base)
        SG_LAUNCH(true);
    else
        SG_LAUNCH(false);
#undef SG_LAUNCH
    return bm_check_launch("segment_gather");
}
