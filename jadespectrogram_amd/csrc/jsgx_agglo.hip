// libjsgx.so, temporally constrained agglomerative segmentation (include/jsgx.h section 17): the kernels and the launcher.
//   "agglo_segments"  a workgroup a pair: section 15's rule (jsgx_segments.h)
//   "agglo_copy"      a wavefront a frame, lane = feature: X into the plane of sums, the cost of every frame with its successor (as a
//                     key), the workgroup's non-finite vote
//   "agglo_offsets"   a workgroup a pair: the votes, the over-long stretches, the prefix sums of min(k, len), n_out and the verdict
//   "agglo_wave"      a wavefront a stretch of up to 64 frames, four to a workgroup; keys and links one per lane in LDS
//   "agglo_group"     a workgroup of one wavefront a longer stretch; keys and links of every frame and a minimum for every block of 64
//                     frames in LDS
// A stretch belongs to one wavefront from its first step to its last, so no barrier stands in a step: what lane 0 writes to LDS the
// wavefront reads behind a wavefront fence.  The sums of feature f are read and written by lane f mod 64 alone.
#include "jsgx_internal.h"
#include "jsgx_segments.h"

namespace jsgx {

namespace {

constexpr int kThreads = JSGX_AGGLO_THREADS;
constexpr int kWaves = kThreads / 64;
constexpr int kShort = JSGX_AGGLO_SHORT;
constexpr int kCopyFrames = JSGX_AGGLO_COPY_FRAMES;
constexpr unsigned kDead = 0xFFFFFFFFu;          // above the key of every cost: the NaN of a cost is JSGX_SYNC_NAN_BITS, key 0xFFC00000
static_assert(kThreads == kSegThreads && kWaves == 4 && kShort == 64 && kCopyFrames % kWaves == 0, "include/jsgx.h");
static_assert(kWaves * kShort * 8 == JSGX_AGGLO_LDS_BYTES && JSGX_AGGLO_GROUP_THREADS == 64, "include/jsgx.h");
static_assert(JSGX_AGGLO_MAX_STRETCH <= 65535 && 8 * JSGX_AGGLO_MAX_STRETCH + 8 * ((JSGX_AGGLO_MAX_STRETCH + 63) / 64) == JSGX_AGGLO_LDS_LIMIT, "16-bit links; include/jsgx.h");
static_assert(JSGX_AGGLO_LDS_LIMIT <= 163840, "the LDS a workgroup may declare");

struct AggloK {
    const float* x;
    long long x_frame_pitch, x_pair_pitch;
    SegmentsK seg;
    int* out_bounds;
    long long out_pitch;
    int* n_out;
    int* order;
    float* height;
    long long tree_pitch;
    // the scratch
    float* sums;              // [pairs][N][F]
    unsigned* cost;           // [pairs][N]: key of the cost of frame t with frame t + 1
    int* votes;               // [pairs][n_votes]
    int* offsets;             // [pairs][stretches]
    int* verdict;             // [pairs]: 1 where the merge kernels have work
    int N, F, k, max_out, stretches, n_votes, longest;
};

// what lane 0 wrote to LDS, for the whole wavefront: the hardware serves a wavefront's LDS instructions in order, the fence keeps the
// compiler from moving them
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long o = __shfl_xor(v, s);
        v = o < v ? o : v;
    }
    return v;
}

// Q of the header, then the cost of the pair (m_a frames, m_b frames)
__device__ __forceinline__ float cost_of(float q, int m_a, int m_b) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) q = __fadd_rn(q, __shfl_xor(q, s));
    const float w = __fdiv_rn(__fmul_rn((float)m_a, (float)m_b), (float)(m_a + m_b));
    const float c = __fmul_rn(w, q);
    return c != c ? __uint_as_float(JSGX_SYNC_NAN_BITS) : c;
}

__global__ __launch_bounds__(kThreads) void agglo_segments_kernel(const AggloK g) {
    __shared__ int wave_total[2][kWaves], wave_bad[kWaves];
    segments_of_pair(g.seg, blockIdx.x, wave_total, wave_bad);
}

__global__ __launch_bounds__(kThreads) void agglo_copy_kernel(const AggloK g) {
    __shared__ int wave_bad[kWaves];
    const int p = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ns = g.seg.n_segments[p];
    if (ns <= 0) return;          // a refused pair, or one without a stretch: "agglo_offsets" reads no vote of it
    const int* seg = g.seg.segments + p * g.seg.segments_pitch;
    const int u0 = seg[0], u_end = seg[ns];
    const float* x = g.x + p * g.x_pair_pitch;
    int bad = 0;
    for (int i = w; i < kCopyFrames; i += kWaves) {
        const int t = kCopyFrames * blockIdx.x + i;
        if (t < u0 || t >= u_end) continue;          // u_end <= N
        const float* r0 = x + t * g.x_frame_pitch;
        const bool next = t + 1 < u_end;
        float* to = g.sums + ((long long)p * g.N + t) * g.F;
        float q = 0.f;
        for (int f = lane; f < g.F; f += 64) {
            const float a = r0[f], b = next ? r0[g.x_frame_pitch + f] : a;
            to[f] = a;
            bad |= !(__builtin_fabsf(a) < __builtin_inff());
            const float d = __fsub_rn(a, b);
            q = __builtin_fmaf(d, d, q);
        }
        const float c = cost_of(q, 1, 1);
        if (lane == 0) g.cost[(long long)p * g.N + t] = key_of(c);
    }
    const bool some = __ballot(bad) != 0;
    if (lane == 0) wave_bad[w] = some;
    __syncthreads();
    if (threadIdx.x == 0) g.votes[(long long)p * g.n_votes + blockIdx.x] = wave_bad[0] | wave_bad[1] | wave_bad[2] | wave_bad[3];
}

__global__ __launch_bounds__(kThreads) void agglo_offsets_kernel(const AggloK g) {
    __shared__ int wave_total[2][kWaves], wave_bad[kWaves];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int ns = g.seg.n_segments[p];
    if (ns <= 0) {
        if (tid == 0) g.n_out[p] = ns < 0 ? -1 : 0, g.verdict[p] = 0;
        return;
    }
    const int* seg = g.seg.segments + p * g.seg.segments_pitch;
    int bad = 0;
    for (int i = tid; i < g.n_votes; i += kThreads) bad |= g.votes[(long long)p * g.n_votes + i];
    for (int o = tid; o < ns; o += kThreads) bad |= seg[o + 1] - seg[o] > JSGX_AGGLO_MAX_STRETCH;
    const bool some = __ballot(bad) != 0;
    if (lane == 0) wave_bad[w] = some;
    __syncthreads();
    if (wave_bad[0] | wave_bad[1] | wave_bad[2] | wave_bad[3]) {
        if (tid == 0) g.n_out[p] = -1, g.verdict[p] = 0;
        return;
    }
    int* offsets = g.offsets + (long long)p * g.stretches;          // ns <= stretches
    int before = 0;
    for (int o0 = 0, step = 0; o0 < ns; o0 += kThreads, ++step) {
        const int o = o0 + tid;
        int len = 0;
        if (o < ns) len = seg[o + 1] - seg[o];
        const int mine = len < g.k ? len : g.k;
        int incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            incl += lane >= d ? up : 0;
        }
        if (lane == 63) wave_total[step & 1][w] = incl;
        __syncthreads();          // the other buffer is the one the step before read
        int at = before + incl - mine, all = 0;
#pragma unroll
        for (int q = 0; q < kWaves; ++q) {
            const int c = wave_total[step & 1][q];
            at += q < w ? c : 0;
            all += c;
        }
        if (o < ns) offsets[o] = at;
        before += all;
    }
    if (tid == 0) g.n_out[p] = before, g.verdict[p] = 1;
}

// One stretch, the frames u0 .. u0 + L - 1 of pair p, by one wavefront.  key[t]: the key of the cost of the cluster that starts at frame
// u0 + t with its right neighbour (kDead: no cluster starts there, or the last one); lt, rt: the starts of its neighbours (rt == L: none).
// LONG: bmin[b] = the least (key << 32 | t) of block b of 64 frames.
template <bool LONG>
__device__ __forceinline__ void merge_stretch(const AggloK& g, int p, int o, int u0, int L, int lane, unsigned* key, unsigned short* lt, unsigned short* rt,
                                              unsigned long long* bmin) {
    const int kk = g.k < L ? g.k : L;
    float* S = g.sums + ((long long)p * g.N + u0) * g.F;
    const unsigned* first = g.cost + (long long)p * g.N + u0;
    const int F = g.F;
    for (int t = lane; t < L; t += 64) {
        key[t] = t < L - 1 ? first[t] : kDead;
        lt[t] = (unsigned short)(t - 1);
        rt[t] = (unsigned short)(t + 1);
    }
    wave_sync();
    const int nb = (L + 63) >> 6;
    auto refresh = [&](int b) {
        const int t = 64 * b + lane;
        const unsigned long long v = wave_min(t < L ? ((unsigned long long)key[t] << 32 | (unsigned)t) : ~0ull);
        if (lane == 0) bmin[b] = v;
    };
    if (LONG) {
        for (int b = 0; b < nb; ++b) refresh(b);
        wave_sync();
    }
    for (int step = 0, live = L; live > kk; ++step, --live) {
        unsigned long long best = ~0ull;
        if (LONG) {
            for (int i = lane; i < nb; i += 64) best = bmin[i] < best ? bmin[i] : best;
        } else if (lane < L) {
            best = (unsigned long long)key[lane] << 32 | (unsigned)lane;
        }
        best = wave_min(best);
        const int a = (int)(unsigned)best;          // live > 1: a pair exists, a < L - 1
        const int b = rt[a], c = rt[b], l = a > 0 ? (int)lt[a] : -1;
        const int m_c = c < L ? (int)rt[c] - c : 0;
        if (g.order && lane == 0) {
            const long long at = p * g.tree_pitch + u0 + step;
            g.order[at] = u0 + b;
            g.height[at] = unkey((unsigned)(best >> 32));
        }
        const float f_ab = (float)(c - a), f_l = (float)(a - l), f_c = (float)m_c;
        float* sa = S + (size_t)a * F;
        const float *sb = S + (size_t)b * F, *sl = S + (size_t)(l < 0 ? a : l) * F, *sc = S + (size_t)(c < L ? c : a) * F;
        float q_l = 0.f, q_r = 0.f;
        for (int f = lane; f < F; f += 64) {
            const float s = __fadd_rn(sa[f], sb[f]);
            const float vl = sl[f], vc = sc[f];
            sa[f] = s;
            const float m = __fdiv_rn(s, f_ab);
            if (l >= 0) {
                const float d = __fsub_rn(__fdiv_rn(vl, f_l), m);
                q_l = __builtin_fmaf(d, d, q_l);
            }
            if (c < L) {
                const float d = __fsub_rn(m, __fdiv_rn(vc, f_c));
                q_r = __builtin_fmaf(d, d, q_r);
            }
        }
        unsigned key_l = kDead, key_r = kDead;
        if (l >= 0) key_l = key_of(cost_of(q_l, a - l, c - a));
        if (c < L) key_r = key_of(cost_of(q_r, c - a, m_c));
        wave_sync();
        if (lane == 0) {
            rt[a] = (unsigned short)c;
            if (c < L) lt[c] = (unsigned short)a;
            key[b] = kDead;
            key[a] = key_r;
            if (l >= 0) key[l] = key_l;
        }
        wave_sync();
        if (LONG) {
            const int ba = a >> 6, bb = b >> 6, bl = l >> 6;          // l = -1: block -1, never a's
            refresh(ba);
            if (bb != ba) refresh(bb);
            if (l >= 0 && bl != ba) refresh(bl);
            wave_sync();
        }
    }
    // the starts that are left: frame t > 0 is one where its left neighbour still points at it
    int at = g.offsets[(long long)p * g.stretches + o];
    int* out = g.out_bounds + p * g.out_pitch;
    for (int t0 = 0; t0 < L; t0 += 64) {
        const int t = t0 + lane;
        const bool alive = t < L && (t == 0 || rt[lt[t]] == t);
        const unsigned long long votes = __ballot(alive);
        const int mine = at + __popcll(votes & ((1ull << lane) - 1));
        if (alive && mine < g.max_out) out[mine] = u0 + t;
        at += __popcll(votes);
    }
}

__global__ __launch_bounds__(kThreads) void agglo_wave_kernel(const AggloK g) {
    __shared__ unsigned key[kWaves][kShort];
    __shared__ unsigned short lt[kWaves][kShort], rt[kWaves][kShort];
    const int p = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (g.verdict[p] == 0) return;
    const int o = kWaves * blockIdx.x + w;
    if (o >= g.seg.n_segments[p]) return;
    const int* seg = g.seg.segments + p * g.seg.segments_pitch;
    const int u0 = seg[o], L = seg[o + 1] - u0;
    if (L > kShort) return;          // "agglo_group" takes it
    merge_stretch<false>(g, p, o, u0, L, lane, key[w], lt[w], rt[w], nullptr);
}

__global__ __launch_bounds__(JSGX_AGGLO_GROUP_THREADS) void agglo_group_kernel(const AggloK g) {
    extern __shared__ unsigned long long dyn[];          // [ceil(longest / 64)] minima, [longest] keys, [longest] lt, [longest] rt
    const int p = blockIdx.y, o = blockIdx.x;
    if (g.verdict[p] == 0 || o >= g.seg.n_segments[p]) return;
    const int* seg = g.seg.segments + p * g.seg.segments_pitch;
    const int u0 = seg[o], L = seg[o + 1] - u0;
    if (L <= kShort) return;          // "agglo_wave" takes it;  L <= longest: the verdict refuses a longer one
    unsigned* key = reinterpret_cast<unsigned*>(dyn + ((g.longest + 63) >> 6));
    unsigned short* lt = reinterpret_cast<unsigned short*>(key + g.longest);
    merge_stretch<true>(g, p, o, u0, L, threadIdx.x, key, lt, lt + g.longest, dyn);
}

jsg::OncePerDevice g_agglo_once;

}  // namespace

}  // namespace jsgx

using namespace jsgx;

extern "C" int jsgx_agglomerative_launch(const jsgx_agglomerative_args* g, void* scratch, int64_t scratch_bytes, void* stream) {
    static const char* who = "jsgx_agglomerative_launch";
    AggloSpans spans;
    int rc = agglo_check(g, who, &spans);
    if (rc == JSGX_OK) rc = agglo_check_scratch(g, who, spans, scratch, scratch_bytes);
    if (rc != JSGX_OK) return rc;
    int dev = -1;
    if ((rc = current_device(&dev, who)) != JSGX_OK) return rc;
    // every refusal is behind us
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const AggloPlan plan = agglo_plan(g);
    const bool many = g->pairs > 1;
    AggloK k{};
    k.x = g->x, k.x_frame_pitch = g->x_frame_pitch, k.x_pair_pitch = many ? g->x_pair_pitch : 0;
    k.seg = SegmentsK{g->bounds, many ? g->bounds_pitch : 0, g->n_bounds, g->segments, many ? g->segments_pitch : 0, g->n_segments,
                      g->n_frames, g->max_bounds, g->bounds_all, g->max_segments, g->pad};
    k.out_bounds = g->out_bounds, k.out_pitch = many ? g->out_pitch : 0, k.n_out = g->n_out;
    k.order = g->order, k.height = g->height, k.tree_pitch = many ? g->tree_pitch : 0;
    float* words = static_cast<float*>(scratch);
    k.sums = words, k.cost = reinterpret_cast<unsigned*>(words + plan.off_cost), k.votes = reinterpret_cast<int*>(words + plan.off_votes);
    k.offsets = reinterpret_cast<int*>(words + plan.off_offsets), k.verdict = reinterpret_cast<int*>(words + plan.off_verdict);
    k.N = g->n_frames, k.F = g->n_features, k.k = g->n_clusters, k.max_out = g->max_out;
    k.stretches = (int)plan.stretches, k.n_votes = (int)plan.votes, k.longest = (int)plan.longest;
    const unsigned P = (unsigned)g->pairs;
    hipLaunchKernelGGL(agglo_segments_kernel, dim3(P), dim3(kThreads), 0, s, k);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return finish_launch(who, err);
    if (plan.stretches > 0) {
        hipLaunchKernelGGL(agglo_copy_kernel, dim3((unsigned)plan.votes, P), dim3(kThreads), 0, s, k);
        if ((err = hipGetLastError()) != hipSuccess) return finish_launch(who, err);
    }
    hipLaunchKernelGGL(agglo_offsets_kernel, dim3(P), dim3(kThreads), 0, s, k);
    if ((err = hipGetLastError()) != hipSuccess || plan.stretches == 0) return finish_launch(who, err);
    hipLaunchKernelGGL(agglo_wave_kernel, dim3((unsigned)((plan.stretches + kWaves - 1) / kWaves), P), dim3(kThreads), 0, s, k);
    if ((err = hipGetLastError()) != hipSuccess || g->n_frames <= kShort) return finish_launch(who, err);
    return finish_launch(who, jsg::launch_large_lds(g_agglo_once, dev, 1u, agglo_group_kernel, JSGX_AGGLO_LDS_LIMIT, dim3((unsigned)plan.stretches, P),
                                                    dim3(JSGX_AGGLO_GROUP_THREADS), (size_t)plan.lds_bytes, s, k));
}
