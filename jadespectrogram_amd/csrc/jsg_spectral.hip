// libjsg.so, spectral shape descriptors (include/jsg.h, section 2l).  A unit of its own; the refusals and the plan are in
// jsg_spectral_host.cpp.
//
// spectral_regs_kernel<NC, FK>: 256 threads, no LDS, no scratch, no atomics.  A group of W lanes (W = 64 where K > 32, else the
// smallest power of two >= K; W = 64 whenever NC > 1) owns a frame; lane l holds S[l], S[l + W], ... -- at most NC values, so every
// load is one coalesced row of W floats -- and keeps them in registers from the first pass (E, N1, mx, L) over the second (M2 needs
// the centroid) to the scan, which overwrites them with cum[], and the search (k* needs cum[K-1]): the plane crosses memory once,
// with non-temporal loads.  A group has FK frames in flight that lie 256 / W apart (all their loads are issued before the first sum,
// 8 to 65 per lane), so a workgroup takes FK * 256 / W consecutive frames per step of its grid stride.  The lane's NC frequencies
// f[l + jW] are the same for every frame: they are loaded once per workgroup and stay in registers too.  The six steps of a chunk's
// scan are lane shifts within the group; the chunks' scans do not depend on each other, only the chain of the bases does.  The passes
// run over all NC chunks without a branch between them, so that the chains of different chunks overlap: a chunk past K holds +0,
// which leaves E, N1, mx and the prefix sum as they are, and is masked out of L, M2 and the search.
//
// spectral_stream_kernel (K > 64 * 65): one frame per wave at a time, the chunks walked eight at a time; the first pass takes the sums
// and cum[K-1], the second (M2, the search) re-reads the frame and the table through the caches, so its loads are plain ones.
//
// An output that is NULL does not cost its separable work (wave-uniform branches): no scan without the rolloff, no logarithm without
// flatness_db, no second pass without the spread.  Every float operation of the definitions is written out (contraction is off; the
// fused multiply-add is explicit; the divide and the square root are the correctly rounded ones of the default compile mode).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "jsg_exact_math.h"
#include "jsg_internal.h"

namespace jsg {

// what a launch wants: the separable work, and which outputs are given (bit tests of one word, where tests of seven pointers would
// each be held as a lane mask)
enum { SP_N1 = 1, SP_M2 = 2, SP_LOG = 4, SP_SCAN = 8, SP_ENERGY = 16, SP_CENTROID = 32, SP_SPREAD = 64, SP_ROLLOFF = 128, SP_BIN = 256, SP_FLATNESS = 512, SP_CREST = 1024 };

struct SpArgs {
    const float* in;
    long long frame_pitch, row_pitch;
    const float* freqs;
    float *energy, *centroid, *spread, *rolloff;
    int* rolloff_bin;
    float *flatness_db, *crest;
    long long out_pitch;
    long long n_items, groups;              // groups = work items per row
    int T, K, W, want;
    float roll;
};

// The compiler may not carry a value derived from this across the point where it stands: the per-chunk predicates and addresses are
// cheap to form again and would otherwise be hoisted out of the frame loop, NC of each, into registers that the frame needs.
__device__ __forceinline__ int sp_fresh(int v) {
    asm volatile("" : "+v"(v));
    return v;
}
__device__ __forceinline__ int sp_fresh_uniform(int v) {         // the same, for a value that every lane shares
    asm volatile("" : "+s"(v));
    return v;
}

struct SpSums {
    float E, N1, mx, L;
};

// one value of a lane into the sums of the first pass; ok: the bin exists (a bin past K is +0 and leaves E, N1 and mx as they are)
__device__ __forceinline__ void sp_take(SpSums& s, float v, float f, bool ok, int want) {
#pragma clang fp contract(off)
    s.E = s.E + v;
    if (want & SP_N1) s.N1 = __builtin_fmaf(f, v, s.N1);
    s.mx = (v > s.mx || v != v) ? v : s.mx;
    if (want & SP_LOG) {
        const float db = jsg_exact_db(v);
        s.L = ok ? s.L + db : s.L;
    }
}

__device__ __forceinline__ float sp_tree(float s, int W) {
#pragma clang fp contract(off)
    for (int o = W >> 1; o >= 1; o >>= 1) s = s + __shfl_xor(s, o);
    return s;
}

__device__ __forceinline__ float sp_tree_max(float m, int W) {
    for (int o = W >> 1; o >= 1; o >>= 1) {
        const float v = __shfl_xor(m, o);
        m = (v > m || v != v) ? v : m;
    }
    return m;
}

__device__ __forceinline__ int sp_tree_min(int m, int W) {
    for (int o = W >> 1; o >= 1; o >>= 1) m = min(m, __shfl_xor(m, o));
    return m;
}

// the same over the N frames a group has in flight, step by step, so that the frames' chains overlap
template <int N>
__device__ __forceinline__ void sp_tree(float (&v)[N], int W) {
#pragma clang fp contract(off)
    for (int o = W >> 1; o >= 1; o >>= 1) {
#pragma unroll
        for (int f = 0; f < N; ++f) v[f] = v[f] + __shfl_xor(v[f], o);
    }
}

template <int N>
__device__ __forceinline__ void sp_tree_max(float (&m)[N], int W) {
    for (int o = W >> 1; o >= 1; o >>= 1) {
#pragma unroll
        for (int f = 0; f < N; ++f) {
            const float v = __shfl_xor(m[f], o);
            m[f] = (v > m[f] || v != v) ? v : m[f];
        }
    }
}

template <int N>
__device__ __forceinline__ void sp_tree_min(int (&m)[N], int W) {
    for (int o = W >> 1; o >= 1; o >>= 1) {
#pragma unroll
        for (int f = 0; f < N; ++f) m[f] = min(m[f], __shfl_xor(m[f], o));
    }
}

template <int N>
__device__ __forceinline__ void sp_scan(float (&x)[N], int l, int W) {
#pragma clang fp contract(off)
    for (int o = 1; o < W; o <<= 1) {
#pragma unroll
        for (int f = 0; f < N; ++f) {
            const float t = __shfl_up(x[f], o, W);
            x[f] = l >= o ? x[f] + t : x[f];
        }
    }
}

// the inclusive scan of a chunk within the group of W lanes
__device__ __forceinline__ float sp_scan(float x, int l, int W) {
#pragma clang fp contract(off)
    for (int o = 1; o < W; o <<= 1) {
        const float t = __shfl_up(x, o, W);
        x = l >= o ? x + t : x;
    }
    return x;
}

// what a frame's sums give, written by lane 0 of the group; kstar < 0: no rolloff was searched
__device__ __forceinline__ void sp_store(const SpArgs& a, int want, long long at, const SpSums& s, float M2, float thr, int kstar) {
#pragma clang fp contract(off)
    const float Kf = (float)a.K;
    const bool zero = s.E == 0.f;
    if (want & SP_ENERGY) a.energy[at] = s.E;
    if (want & SP_CENTROID) a.centroid[at] = zero ? 0.f : s.N1 / s.E;
    if (want & SP_SPREAD) a.spread[at] = zero ? 0.f : __builtin_sqrtf(M2 / s.E);
    if (want & SP_CREST) a.crest[at] = zero ? 0.f : s.mx / (s.E / Kf);
    if (want & SP_FLATNESS) a.flatness_db[at] = s.L / Kf - jsg_exact_db(s.E / Kf);
    const bool nan = thr != thr;
    if (want & SP_ROLLOFF) a.rolloff[at] = nan ? thr : a.freqs[kstar];
    if (want & SP_BIN) a.rolloff_bin[at] = nan ? -1 : kstar;
}

template <int NC, int FK>
__global__ __launch_bounds__(kSpThreads) void spectral_regs_kernel(const SpArgs a) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, W = NC > 1 ? 64 : a.W, l = tid & (W - 1), sub = tid / W, per = kSpThreads / W;
    const int K = a.K;
    float fr[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int k = l + j * W;
        fr[j] = ((a.want & SP_N1) && k < K) ? a.freqs[k] : 0.f;
    }
    const int jlast0 = (K - 1) / W, llast = (K - 1) & (W - 1);        // NC == 1: K <= W, the one chunk is the last
    for (long long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const long long r = item / a.groups;
        const long long t0 = (item - r * a.groups) * (per * FK) + sub;
        const float* row = a.in + r * a.row_pitch;
        const int want = sp_fresh_uniform(a.want);
        const int Wf = NC > 1 ? 64 : sp_fresh_uniform(W);           // the loops over the lanes of a group are formed per item
        const int perf = NC > 1 ? kSpThreads / 64 : sp_fresh_uniform(per);
        float x[FK][NC];
#pragma unroll
        for (int f = 0; f < FK; ++f) {
            const long long t = t0 + f * perf;
            const bool live = t < a.T;
            const float* p = row + (live ? t : 0) * a.frame_pitch + l;
            const bool tail = live && sp_fresh(l) <= llast;
            const int jlast = (NC == 1 ? 0 : sp_fresh_uniform(jlast0));
            // only chunk jlast can be partial: the chunks before it are loaded whole, the ones past it not at all
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                x[f][j] = 0.f;
                if (j < jlast) {
                    if (live) x[f][j] = __builtin_nontemporal_load(p + j * W);
                } else if (j == jlast) {
                    if (tail) x[f][j] = __builtin_nontemporal_load(p + j * W);
                }
            }
        }
        // The passes run stage by stage over the FK frames (and all NC chunks) without a branch between them, so that the dependent
        // chains of different frames and chunks overlap.  A frame past T holds +0 and is not stored.
        float E[FK], N1[FK], mx[FK], L[FK], M2[FK], thr[FK];
        int kstar[FK];
        {
            const bool tail = sp_fresh(l) <= llast;
            const int jlast = (NC == 1 ? 0 : sp_fresh_uniform(jlast0));
#pragma unroll
            for (int f = 0; f < FK; ++f) {
                SpSums s{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < NC; ++j) sp_take(s, x[f][j], fr[j], j < jlast || (j == jlast && tail), want);
                E[f] = s.E, N1[f] = s.N1, mx[f] = s.mx, L[f] = s.L, M2[f] = 0.f, thr[f] = 0.f, kstar[f] = -1;
            }
        }
        sp_tree<FK>(E, Wf);
        if (want & SP_N1) sp_tree<FK>(N1, Wf);
        sp_tree_max<FK>(mx, Wf);
        if (want & SP_LOG) sp_tree<FK>(L, Wf);
        if (want & SP_M2) {
            const bool tail = sp_fresh(l) <= llast;
            const int jlast = (NC == 1 ? 0 : sp_fresh_uniform(jlast0));
#pragma unroll
            for (int f = 0; f < FK; ++f) {
                const float c = E[f] == 0.f ? 0.f : N1[f] / E[f];
#pragma unroll
                for (int j = 0; j < NC; ++j) {
                    const float d = fr[j] - c;
                    const float dd = d * d;
                    M2[f] = (j < jlast || (j == jlast && tail)) ? __builtin_fmaf(dd, x[f][j], M2[f]) : M2[f];
                }
            }
            sp_tree<FK>(M2, Wf);
        }
        if (want & SP_SCAN) {
            float base[FK], tot[FK];
            int cand[FK];
#pragma unroll
            for (int f = 0; f < FK; ++f) base[f] = 0.f, tot[f] = 0.f, cand[f] = INT_MAX;
            int jlast = (NC == 1 ? 0 : sp_fresh_uniform(jlast0));
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                float sc[FK];
#pragma unroll
                for (int f = 0; f < FK; ++f) sc[f] = x[f][j];
                sp_scan<FK>(sc, l, Wf);
#pragma unroll
                for (int f = 0; f < FK; ++f) {
                    x[f][j] = base[f] + sc[f];                          // cum[jW + l]
                    base[f] = base[f] + __shfl(sc[f], W - 1, W);
                }
            }
#pragma unroll
            for (int j = 0; j < NC; ++j)
                if (j == jlast) {
#pragma unroll
                    for (int f = 0; f < FK; ++f) tot[f] = __shfl(x[f][j], llast, W);
                }
            const int lf = sp_fresh(l);
            const bool tail = lf <= llast;
            jlast = (NC == 1 ? 0 : sp_fresh_uniform(jlast0));
#pragma unroll
            for (int f = 0; f < FK; ++f) {
                thr[f] = a.roll * tot[f];
#pragma unroll
                for (int j = NC - 1; j >= 0; --j)
                    if ((j < jlast || (j == jlast && tail)) && x[f][j] >= thr[f]) cand[f] = lf + j * W;
            }
            sp_tree_min<FK>(cand, Wf);
#pragma unroll
            for (int f = 0; f < FK; ++f) kstar[f] = cand[f] == INT_MAX ? K - 1 : cand[f];
        }
        if (l == 0) {
#pragma unroll
            for (int f = 0; f < FK; ++f) {
                const long long t = t0 + f * perf;
                if (t < a.T) sp_store(a, want, r * a.out_pitch + t, SpSums{E[f], N1[f], mx[f], L[f]}, M2[f], thr[f], kstar[f]);
            }
        }
    }
}

constexpr int SP_U = 8;                     // chunks of the streaming path whose loads are issued together

__global__ __launch_bounds__(kSpThreads) void spectral_stream_kernel(const SpArgs a) {
#pragma clang fp contract(off)
    constexpr int W = 64;
    const int tid = threadIdx.x, l = tid & 63, sub = tid >> 6;
    for (long long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const long long r = item / a.groups;
        const long long t = (item - r * a.groups) * (kSpThreads / W) + sub;
        if (t >= a.T) continue;                     // the same for every lane of the wave
        const int want = sp_fresh_uniform(a.want), K = sp_fresh_uniform(a.K), nc = (K + W - 1) / W;
        const int jlast = (K - 1) / W, llast = (K - 1) & (W - 1);
        const float* p = a.in + r * a.row_pitch + t * a.frame_pitch;
        SpSums s{0.f, 0.f, 0.f, 0.f};
        float base = 0.f, tot = 0.f;
        for (int j0 = 0; j0 < nc; j0 += SP_U) {
            float v[SP_U], f[SP_U];
#pragma unroll
            for (int u = 0; u < SP_U; ++u) {
                const int k = l + (j0 + u) * W;
                v[u] = k < K ? p[k] : 0.f;
                f[u] = ((want & SP_N1) && k < K) ? a.freqs[k] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < SP_U; ++u) {
                const int j = j0 + u;
                if (j * W >= K) continue;
                sp_take(s, v[u], f[u], l + j * W < K, want);
                if (want & SP_SCAN) {
                    const float sc = sp_scan(v[u], l, W);
                    if (j == jlast) tot = __shfl(base + sc, llast, W);
                    base = base + __shfl(sc, W - 1, W);
                }
            }
        }
        s.E = sp_tree(s.E, W);
        if (want & SP_N1) s.N1 = sp_tree(s.N1, W);
        s.mx = sp_tree_max(s.mx, W);
        if (want & SP_LOG) s.L = sp_tree(s.L, W);
        float M2 = 0.f, thr = 0.f;
        int kstar = -1;
        if (want & (SP_M2 | SP_SCAN)) {
            const float c = s.E == 0.f ? 0.f : s.N1 / s.E;
            thr = a.roll * tot;
            int cand = INT_MAX;
            base = 0.f;
            for (int j0 = 0; j0 < nc; j0 += SP_U) {
                float v[SP_U], f[SP_U];
#pragma unroll
                for (int u = 0; u < SP_U; ++u) {
                    const int k = l + (j0 + u) * W;
                    v[u] = k < K ? p[k] : 0.f;
                    f[u] = ((want & SP_M2) && k < K) ? a.freqs[k] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < SP_U; ++u) {
                    const int j = j0 + u, k = l + j * W;
                    if (j * W >= K) continue;
                    if (want & SP_M2) {
                        const float d = f[u] - c;
                        const float dd = d * d;
                        M2 = k < K ? __builtin_fmaf(dd, v[u], M2) : M2;
                    }
                    if (want & SP_SCAN) {
                        const float sc = sp_scan(v[u], l, W);
                        const float cum = base + sc;
                        if (k < K && cum >= thr) cand = min(cand, k);
                        base = base + __shfl(sc, W - 1, W);
                    }
                }
            }
            if (want & SP_M2) M2 = sp_tree(M2, W);
            if (want & SP_SCAN) {
                cand = sp_tree_min(cand, W);
                kstar = cand == INT_MAX ? K - 1 : cand;
            }
        }
        if (l == 0) sp_store(a, want, r * a.out_pitch + t, s, M2, thr, kstar);
    }
}

}  // namespace jsg

using namespace jsg;

namespace {

template <int NC, int FK>
void sp_enqueue(const SpArgs& k, const dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL((spectral_regs_kernel<NC, FK>), grid, dim3(kSpThreads), 0, s, k);
}

}  // namespace

extern "C" int jsg_spectral_shape_launch(const jsg_spectral_args* g, void* stream) {
    static const char* who = "jsg_spectral_shape_launch";
    int dev = -1;
    int rc = spectral_check(g, who);
    if (rc == JSG_OK) rc = current_device(&dev, who);
    if (rc != JSG_OK) return rc;
    // every refusal is behind us
    SpectralPlan p{};
    spectral_resolve(g, &p);
    SpArgs k{};
    const bool multi = g->rows > 1;
    k.in = g->in;
    k.frame_pitch = g->frame_pitch;
    k.row_pitch = multi ? g->row_pitch : 0;
    k.freqs = g->freqs;
    k.energy = g->energy;
    k.centroid = g->centroid;
    k.spread = g->spread;
    k.rolloff = g->rolloff;
    k.rolloff_bin = g->rolloff_bin;
    k.flatness_db = g->flatness_db;
    k.crest = g->crest;
    k.out_pitch = multi ? g->out_pitch : 0;
    k.groups = p.groups;
    k.n_items = (long long)g->rows * p.groups;
    k.T = (int)g->n_frames;
    k.K = g->n_bins;
    k.W = p.W;
    k.roll = g->roll_percent;
    k.want = ((g->centroid || g->spread) ? SP_N1 : 0) | (g->spread ? SP_M2 : 0) | (g->flatness_db ? SP_LOG : 0) | ((g->rolloff || g->rolloff_bin) ? SP_SCAN : 0)
           | (g->energy ? SP_ENERGY : 0) | (g->centroid ? SP_CENTROID : 0) | (g->spread ? SP_SPREAD : 0) | (g->rolloff ? SP_ROLLOFF : 0) | (g->rolloff_bin ? SP_BIN : 0)
           | (g->flatness_db ? SP_FLATNESS : 0) | (g->crest ? SP_CREST : 0);
    // what a compute unit holds at a time by the registers of the path (tools/kernel_regs.py), two generations of it where that is 8
    const int per_cu = p.NC == kSpMaxRegs ? 2 : p.NC == 33 ? 3 : 8;
    const dim3 grid(resident_grid(k.n_items, dev, per_cu));
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (p.NC) {
        case 1: sp_enqueue<1, 8>(k, grid, s); break;
        case 2: sp_enqueue<2, 8>(k, grid, s); break;
        case 4: sp_enqueue<4, 4>(k, grid, s); break;
        case 9: sp_enqueue<9, 2>(k, grid, s); break;
        case 17: sp_enqueue<17, 2>(k, grid, s); break;
        case 33: sp_enqueue<33, 1>(k, grid, s); break;
        case kSpMaxRegs: sp_enqueue<kSpMaxRegs, 1>(k, grid, s); break;
        default: hipLaunchKernelGGL(spectral_stream_kernel, grid, dim3(kSpThreads), 0, s, k); break;
    }
    return finish_launch(who);
}
