// The wave table of the audio units (mel.hip, resample.hip, pitch.hip): ONE definition of its entry, its limit, the host
// walk over its lengths, and what a kernel does with a sample before it stages it -- the (shift, scale) of bm_wave_moments
// and the two ways of indexing past the ends of a waveform.  The staging loops differ in layout (chunk pitch, flat,
// doubles) and stay in their units; the table's two host entry points are in mel.hip, beside bm_wave_moments.
#pragma once
#include "bm_common.h"

// A 1-D fp32 waveform on the device, read in place (4-byte aligned), and where its result goes (null for bm_wave_moments).
struct BmWave {
    const float* x;
    float* out;
    long L;
};
static_assert(sizeof(BmWave) == 24, "the wave table entry is {address, address, long}: bm_wave_table_entry_bytes");

#define BM_WAVE_MAX_WAVES 65535         // gridDim.y

// What every launcher over a wave table checks, and its gridDim.x: the largest tiles_of(L) (at least 1), 0 without
// waveforms (nothing to launch: BM_OK), or MINUS the error: n_waves > BM_WAVE_MAX_WAVES, no table or lengths (HOST memory:
// the table's own), an L outside min_len < L < 2^31 -- `lower` names min_len in the unit's own words, e.g. "w_len = ".
template <typename TilesOf>
static inline long bm_wave_tiles(const char* who, const void* table, const long* lengths, int n_waves, long min_len,
                                 const char* lower, TilesOf tiles_of) {
    if (n_waves < 0 || n_waves > BM_WAVE_MAX_WAVES)
        return -bm_set_error(BM_ERR_ARG, "%s: %d waveforms, the limit is %d", who, n_waves, BM_WAVE_MAX_WAVES);
    if (n_waves > 0 && !(table && lengths)) return -bm_set_error(BM_ERR_ARG, "%s: null pointer", who);
    long tiles = 0;
    for (int w = 0; w < n_waves; ++w) {
        if (lengths[w] <= min_len || lengths[w] >= (1L << 31))
            return -bm_set_error(BM_ERR_ARG, "%s: waveform %d has %ld samples (%s%ld < L < 2^31)", who, w, lengths[w], lower,
                                 min_len);
        const long t = tiles_of(lengths[w]);
        tiles = t > tiles ? t : tiles;
    }
    return tiles;
}

// (shift, scale) of waveform w: what bm_wave_moments stored, (0, 1) without moments.  A sample enters a kernel as
// (float)(((double)x - shift) * scale): in fp64, rounded once.
struct BmWaveNorm {
    double shift, scale;
};
__device__ __forceinline__ BmWaveNorm bm_wave_norm(const double* __restrict__ mom, unsigned w) {
    return mom ? BmWaveNorm{mom[2 * w], mom[2 * w + 1]} : BmWaveNorm{0.0, 1.0};
}
__device__ __forceinline__ float bm_wave_normed(float x, const BmWaveNorm& n) {
    return (float)(((double)x - n.shift) * n.scale);
}

// Sample s of a waveform padded by its end samples ("replicate") as an index into [0, L).  Len: int or long, as the kernel
// holds L (L - 1 is formed in it).
template <typename Len>
__device__ __forceinline__ long bm_wave_replicate(long s, Len L) {
    return s < 0 ? 0 : s > L - 1 ? L - 1 : s;
}
// The same for a padding by reflection (torch's "reflect": the end samples are not repeated).  One reflection lands inside
// when the padding is shorter than L; the clamp behind it never moves such an index.
template <typename Len>
__device__ __forceinline__ long bm_wave_reflect(long s, Len L) {
    s = s < 0 ? -s : s;
    s = s >= L ? 2L * (L - 1) - s : s;
    return bm_wave_replicate(s, L);
}
