// Weight packing and the amax scan of compute mode "f16x2" (the scale rule: mfma_split.h; the consumers: conv_nn_h2w.hip,
// gemm_nt_h2w.hip).
// Packed weights: [g][chunk32][tap][plane][4 groups][Mpad] 16-byte slots (8 f16 channels), followed by the
// per-row inverse scales [G][Mpad] fp32.
#include "conv_h2_common.h"

// bytes of the packed buffer: f16 planes [G][chunk32][KS][2][4][Mpad][8] + fp32 inverse row scales [G][Mpad]
extern "C" long bm_packed_weight_bytes_h2(int G, int M, int Cin, int KS) {
    const long mpad = bm_conv_h2_mpad(M);
    return (long)G * cdiv(Cin, 32) * KS * 2 * 4 * mpad * 8 * 2 + (long)G * mpad * 4;
}

// One workgroup per (group, padded row): row maximum -> power-of-two scale -> the row's 16-byte slots of both
// planes (zeros for padded rows / channels) and its inverse scale.
struct PackH2Job {
    const float* src;
    unsigned short* dst;
    float* wscale;
    const float* alpha;
    long sg, sm, sc, sj;
    int M, Cin, KS, flip, Mpad, nchunk;
    int block0, nblocks;      // workgroups [block0, block0 + nblocks) of a batched launch belong to this job
};

// PACK_ROWS consecutive rows per workgroup of 256 threads (one wavefront per row), staged through LDS so that both
// source layouts are read along their contiguous direction: the forward layout a whole row at a time, the
// transposed (data-gradient) layout PACK_ROWS x KS contiguous floats per channel -- read element by element it
// touched a different cache line with every value and the 36 MB of parameters took 175 us to pack.
#define PACK_ROWS 4

__device__ __forceinline__ void pack_h2_rows(const PackH2Job& jb, int block, float* tile, float* rs) {
    const float* __restrict__ src = jb.src;
    const int M = jb.M, Cin = jb.Cin, KS = jb.KS, Mpad = jb.Mpad, nchunk = jb.nchunk, flip = jb.flip;
    const long sg = jb.sg, sm = jb.sm, sc = jb.sc, sj = jb.sj;
    const int rows_per_group = Mpad / PACK_ROWS;
    const int g = block / rows_per_group, m0 = (block - g * rows_per_group) * PACK_ROWS;
    const float alpha = jb.alpha ? *jb.alpha : 1.f;
    const int nk = Cin * KS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // 1. tile[r][c * KS + j] = alpha * w[m0 + r][c][j]; the faster of (row, channel) in memory runs inside
    const float* base = src + g * sg + (long)m0 * sm;
    const bool rows_inside = sm < sc;
    for (int idx = tid; idx < PACK_ROWS * nk; idx += blockDim.x) {
        int r, c, j;
        if (rows_inside) {                  // idx = (c * PACK_ROWS + r) * KS + j
            j = idx % KS;
            const int t = idx / KS;
            r = t % PACK_ROWS;
            c = t / PACK_ROWS;
        } else {                            // idx = (r * Cin + c) * KS + j
            j = idx % KS;
            const int t = idx / KS;
            c = t % Cin;
            r = t / Cin;
        }
        tile[r * nk + c * KS + j] = (m0 + r < M) ? alpha * base[r * sm + c * sc + j * sj] : 0.f;
    }
    __syncthreads();
    // 2. row maxima -> scales (wavefront w owns row w)
    {
        float mx = 0.f;
        for (int i = lane; i < nk; i += 64) mx = fmaxf(mx, fabsf(tile[wave * nk + i]));
        mx = bm_wave_max(mx);
        float s, inv;
        bm_scale_from_amax(mx, s, inv);
        if (lane == 0) {
            rs[wave] = s;
            jb.wscale[(long)g * Mpad + m0 + wave] = inv;
        }
    }
    __syncthreads();
    // 3. the rows' 16-byte slots of both planes: slot q = (chunk, tap, 8-channel group); rows run fastest so that
    //    neighbouring threads write neighbouring 16-byte slots
    const int nslots = nchunk * KS * 4;
    const long plane_stride = (long)4 * Mpad * 8;           // f16 elements of one plane of one (chunk, tap)
    for (int t = tid; t < PACK_ROWS * nslots; t += blockDim.x) {
        const int r = t % PACK_ROWS, q = t / PACK_ROWS;
        const int kg = q & 3;
        const int j = (q >> 2) % KS;
        const int chunk = (q >> 2) / KS;
        const int jj = flip ? KS - 1 - j : j;
        const float sr = rs[r];
        alignas(16) unsigned short hi[8];
        alignas(16) unsigned short lo[8];
#pragma unroll
        for (int e8 = 0; e8 < 8; ++e8) {
            const int c = chunk * 32 + kg * 8 + e8;
            const float v = c < Cin ? tile[r * nk + c * KS + jj] * sr : 0.f;
            const _Float16 a = (_Float16)v;
            const _Float16 l = (_Float16)(v - (float)a);
            hi[e8] = __builtin_bit_cast(unsigned short, a);
            lo[e8] = __builtin_bit_cast(unsigned short, l);
        }
        const long stage = ((long)g * nchunk + chunk) * KS + j;
        unsigned short* out = jb.dst + stage * 2 * plane_stride + ((long)kg * Mpad + m0 + r) * 8;
        *reinterpret_cast<uint4*>(out) = *reinterpret_cast<const uint4*>(hi);
        *reinterpret_cast<uint4*>(out + plane_stride) = *reinterpret_cast<const uint4*>(lo);
    }
}

__global__ __launch_bounds__(256) void pack_weights_h2_kernel(PackH2Job jb) {
    extern __shared__ float pack_smem[];
    pack_h2_rows(jb, blockIdx.x, pack_smem + PACK_ROWS, pack_smem);
}

// every weight tensor of a model in ONE launch: `jobs` (device memory) sorted by block0
__global__ __launch_bounds__(256) void pack_weights_h2_batch_kernel(const PackH2Job* __restrict__ jobs, int njobs) {
    extern __shared__ float pack_smem[];
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {                                   // last job with block0 <= blockIdx.x
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const PackH2Job jb = jobs[lo];
    pack_h2_rows(jb, blockIdx.x - jb.block0, pack_smem + PACK_ROWS, pack_smem);
}

static int pack_h2_fill(PackH2Job& jb, const float* src, void* dst, int G, int M, int Cin, int KS, long sg, long sm,
                        long sc, long sj, int flip, const float* alpha_ptr) {
    BM_REQUIRE(src && dst, "pack_weights_h2: null pointer");
    BM_REQUIRE(G > 0 && M > 0 && Cin > 0 && KS > 0, "pack_weights_h2: bad dims");
    jb.Mpad = bm_conv_h2_mpad(M);
    jb.nchunk = cdiv(Cin, 32);
    const long f16_elems = (long)G * jb.nchunk * KS * 2 * 4 * jb.Mpad * 8;
    jb.src = src; jb.dst = (unsigned short*)dst;
    jb.wscale = reinterpret_cast<float*>(reinterpret_cast<char*>(dst) + f16_elems * 2);
    jb.alpha = alpha_ptr;
    jb.sg = sg; jb.sm = sm; jb.sc = sc; jb.sj = sj;
    jb.M = M; jb.Cin = Cin; jb.KS = KS; jb.flip = flip;
    BM_REQUIRE(Cin * KS <= PACK_MAX_NK, "pack_weights_h2: Cin * KS = %d exceeds %d", Cin * KS, PACK_MAX_NK);
    jb.block0 = 0; jb.nblocks = G * jb.Mpad / PACK_ROWS;
    return BM_OK;
}

extern "C" int bm_pack_weights_h2(const float* src, void* dst, int G, int M, int Cin, int KS, long sg, long sm,
                                  long sc, long sj, int flip, const float* alpha_ptr, void* stream) {
    PackH2Job jb;
    if (int rc = pack_h2_fill(jb, src, dst, G, M, Cin, KS, sg, sm, sc, sj, flip, alpha_ptr)) return rc;
    hipLaunchKernelGGL(pack_weights_h2_kernel, dim3((unsigned)jb.nblocks), dim3(256),
                       (size_t)(PACK_ROWS + PACK_ROWS * Cin * KS) * sizeof(float), (hipStream_t)stream, jb);
    return bm_check_launch("pack_weights_h2");
}

// Batched packing.  The host builds a table of jobs (bm_pack_h2_job_bytes() bytes each, filled by
// bm_pack_h2_job_fill, which returns the job's workgroup count or a negative error), copies it to the device
// once, and re-packs every weight tensor of the model with one launch per optimizer step.
extern "C" int bm_pack_h2_job_bytes() { return (int)sizeof(PackH2Job); }

extern "C" int bm_pack_h2_job_fill(void* job, const float* src, void* dst, int G, int M, int Cin, int KS, long sg,
                                   long sm, long sc, long sj, int flip, const float* alpha_ptr, int block0) {
    if (!job) return -1;
    PackH2Job jb;
    if (pack_h2_fill(jb, src, dst, G, M, Cin, KS, sg, sm, sc, sj, flip, alpha_ptr)) return -1;
    jb.block0 = block0;
    memcpy(job, &jb, sizeof(jb));
    return jb.nblocks;
}

extern "C" int bm_pack_weights_h2_batch(const void* jobs_dev, int njobs, int total_blocks, int max_nk, void* stream) {
    BM_REQUIRE(jobs_dev && njobs > 0 && total_blocks > 0, "pack_weights_h2_batch: bad arguments");
    BM_REQUIRE(max_nk > 0 && max_nk <= PACK_MAX_NK, "pack_weights_h2_batch: max_nk = %d (largest Cin * KS of the jobs)", max_nk);
    hipLaunchKernelGGL(pack_weights_h2_batch_kernel, dim3((unsigned)total_blocks), dim3(256),
                       (size_t)(PACK_ROWS + PACK_ROWS * max_nk) * sizeof(float), (hipStream_t)stream,
                       (const PackH2Job*)jobs_dev, njobs);
    return bm_check_launch("pack_weights_h2_batch");
}

// max |x[i]| as <= 256 per-workgroup partial maxima (ws) folded by bm_amax_finalize into the slot `out`
// (BM_AMAX_SHARDS floats whose maximum is the answer).  A non-finite input yields a non-finite or NaN-free
// maximum of the finite part; the non-finite values themselves propagate through the consumer's split.
__global__ __launch_bounds__(1024) void amax_kernel(const float* __restrict__ x, long n, float* __restrict__ ws,
                                                    int* __restrict__ nonfinite) {
    __shared__ float sh[16];
    float mx = 0.f;
    unsigned top = 0u;                                  // largest |x| bit pattern: >= 0x7f800000 <=> inf / nan seen
    // a tensor that is only 4-byte aligned (a batch slice such as meg[1:] with C * T odd): `head` scalar elements
    // up to the first 16-byte boundary, the vector body from there, the scalar tail behind it
    long head = (long)((16u - (unsigned)((uintptr_t)x & 15u)) & 15u) >> 2;
    if (head > n) head = n;
    const long n4 = (n - head) >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(x + head);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const float4 v = x4[i];
        mx = fmaxf(fmaxf(mx, fabsf(v.x)), fmaxf(fabsf(v.y), fmaxf(fabsf(v.z), fabsf(v.w))));
        top = max(max(top, __float_as_uint(v.x) & 0x7fffffffu),
                  max(__float_as_uint(v.y) & 0x7fffffffu, max(__float_as_uint(v.z) & 0x7fffffffu,
                                                               __float_as_uint(v.w) & 0x7fffffffu)));
    }
    if (blockIdx.x == 0) {
        const long tail0 = head + (n4 << 2);
        for (long i = threadIdx.x; i < head + (n - tail0); i += blockDim.x) {
            const long k = i < head ? i : tail0 + (i - head);
            mx = fmaxf(mx, fabsf(x[k]));
            top = max(top, __float_as_uint(x[k]) & 0x7fffffffu);
        }
    }
    if (nonfinite && top >= 0x7f800000u) atomicOr(nonfinite, 1);     // rare: at most one atomic per thread
    bm_publish_amax(mx, ws, sh);
}

// `nonfinite_flag` (nullable, device int): set to 1 if x holds an inf or a nan -- the reference's
// `torch.isfinite(x).all()` asserts (bm/solver.py:258-260) ride on the pass that the f16x2 scale needs anyway.
extern "C" int bm_amax_checked(const float* x, long n, float* out, float* ws, int* nonfinite_flag, void* stream) {
    BM_REQUIRE(x && out && ws && n >= 0, "amax: bad arguments");
    BM_REQUIRE(((uintptr_t)x & 3) == 0, "amax: x must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    long blocks = (n / 4 + 1023) / 1024;
    blocks = blocks < 1 ? 1 : (blocks > 256 ? 256 : blocks);
    hipLaunchKernelGGL(amax_kernel, dim3((unsigned)blocks), dim3(1024), 0, s, x, n, ws, nonfinite_flag);
    if (int rc = bm_check_launch("amax")) return rc;
    return bm_amax_finalize(ws, (int)blocks, out, s);
}

extern "C" int bm_amax(const float* x, long n, float* out, float* ws, void* stream) {
    return bm_amax_checked(x, n, out, ws, nullptr, stream);
}
