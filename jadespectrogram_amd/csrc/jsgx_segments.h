// libjsgx.so, what sections 15 and 17 share on the device (include/jsgx.h): the order of the floats as unsigned keys, and the rule that
// turns a pair's list of boundaries into its segments u[0] < ... < u[U-1] ("Segments" of section 15).  One copy, in jsgx_sync.hip
// ("sync_segments") and in jsgx_agglo.hip ("agglo_segments").
#pragma once
#include <hip/hip_runtime.h>

namespace jsgx {

constexpr int kSegThreads = 256;          // the workgroup of a pair
constexpr int kSegWaves = kSegThreads / 64;

// HPSS's hp_key: unsigned order = the order of the floats, -0 below +0, the infinities at the ends (a NaN beyond them)
__device__ __forceinline__ unsigned key_of(float v) {
    const unsigned b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float unkey(unsigned k) { return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k); }

struct SegmentsK {
    const int* bounds;
    long long bounds_pitch;
    const int* n_bounds;
    int* segments;
    long long segments_pitch;
    int* n_segments;
    int N, max_bounds, bounds_all, max_segments, pad;
};

// The segments of pair p by a workgroup of kSegThreads lanes: the boundaries are checked (one pass), then clipped, padded and freed of
// repeats by a prefix count over 256 entries a step (ballots inside a wavefront, four totals through LDS).  Writes n_segments[p] and
// the entries of u the caller takes; returns U (0 or at least 1; every lane the same), or -1 for a refused pair.
__device__ __forceinline__ int segments_of_pair(const SegmentsK& g, int p, int (*wave_total)[kSegWaves], int* wave_bad) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = g.n_bounds ? g.n_bounds[p] : g.bounds_all;
    const int m = n < g.max_bounds ? n : g.max_bounds;
    const long long b0 = p * g.bounds_pitch;          // bounds may be NULL with max_bounds == 0: then m <= 0 and nothing is read
    int bad = n < 0;
    for (int i = 1 + tid; i < m; i += kSegThreads) bad |= g.bounds[b0 + i] < g.bounds[b0 + i - 1];
    const bool some = __ballot(bad) != 0;
    if (lane == 0) wave_bad[w] = some;
    __syncthreads();
    if (wave_bad[0] | wave_bad[1] | wave_bad[2] | wave_bad[3]) {
        if (tid == 0) g.n_segments[p] = -1;
        return -1;
    }
    const int L = m + 2 * g.pad, N = g.N;
    // s[i], 0 <= i < L
    auto entry = [&](int i) {
        if (g.pad && i == 0) return 0;
        if (g.pad && i == L - 1) return N;
        const int v = g.bounds[b0 + i - g.pad];
        return v < 0 ? 0 : v > N ? N : v;
    };
    int* seg = g.segments + p * g.segments_pitch;
    int kept = 0;          // the entries of u in front of this step
    for (int i0 = 0, step = 0; i0 < L; i0 += kSegThreads, ++step) {
        const int i = i0 + tid;
        int v = 0;
        bool keep = false;
        if (i < L) {
            v = entry(i);
            keep = i == 0 || v != entry(i - 1);
        }
        const unsigned long long votes = __ballot(keep);
        if (lane == 0) wave_total[step & 1][w] = __popcll(votes);
        __syncthreads();          // the other buffer is the one the step before read
        int at = kept + __popcll(votes & ((1ull << lane) - 1)), all = 0;
#pragma unroll
        for (int q = 0; q < kSegWaves; ++q) {
            const int c = wave_total[step & 1][q];
            at += q < w ? c : 0;
            all += c;
        }
        if (keep && at >= 1 && at <= g.max_segments) {
            seg[at] = v;
            if (at == 1) seg[0] = entry(0);          // u[0] is written only where there is a u[1]
        }
        kept += all;
    }
    if (tid == 0) g.n_segments[p] = kept > 0 ? kept - 1 : 0;
    return kept;
}

}  // namespace jsgx
