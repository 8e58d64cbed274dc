// libjsgx.so, aggregation of a plane over segments and time-delay embedding (include/jsgx.h sections 15 and 16): the kernels and the
// launchers.
//   "sync_segments"   a workgroup a pair: the boundaries are checked (one pass), then clipped, padded and freed of repeats by a prefix
//                     count over 256 entries a step (ballots inside a wavefront, four totals through LDS): jsgx_segments.h
//   "sync_aggregate"  lane = feature; a workgroup owns four segments and 64 features.  A team is one wavefront (a segment each) or the
//                     four of the workgroup (the segments one after the other); every aggregate is written once for a team of
//                     either size, so no result depends on which one served it.  The median selects the k-th smallest key bit by bit.
//   "stack_memory"    a workgroup a run of whole output frames, lanes along the row; the row index advances by addition, the step of
//                     a column is one float multiply and a correction
#include "jsgx_internal.h"
#include "jsgx_segments.h"

namespace jsgx {

namespace {

constexpr int kThreads = JSGX_SYNC_THREADS;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = JSGX_SYNC_CHUNK;
constexpr int kWaveMax = JSGX_SYNC_WAVE_MAX;
constexpr int kStage = JSGX_SYNC_STAGE;
static_assert(kWaves == 4 && kWaves * kWaveMax <= kStage && 4 * 64 * kStage <= JSGX_SYNC_LDS_TILE, "the tile holds a staged segment, or one a wavefront");
static_assert(2 * 2 * kWaves * 64 * 4 == JSGX_SYNC_LDS_BYTES, "include/jsgx.h");
static_assert(JSGX_STACK_THREADS == 256 && kThreads == kSegThreads, "include/jsgx.h");

struct SyncK {
    const float* x;
    long long x_frame_pitch, x_pair_pitch;
    const int* bounds;
    long long bounds_pitch;
    const int* n_bounds;
    int* segments;
    long long segments_pitch;
    int* n_segments;
    float* out;
    long long out_frame_pitch, out_pair_pitch;
    int N, F, max_bounds, bounds_all, max_segments, pad;
};

__global__ __launch_bounds__(kThreads) void sync_segments_kernel(const SyncK g) {
    __shared__ int wave_total[2][kWaves], wave_bad[kWaves];
    const SegmentsK s{g.bounds, g.bounds_pitch, g.n_bounds, g.segments, g.segments_pitch, g.n_segments, g.N, g.max_bounds, g.bounds_all, g.max_segments, g.pad};
    segments_of_pair(s, blockIdx.x, wave_total, wave_bad);          // jsgx_segments.h: the rule, shared with section 17
}

// What the wavefronts of a team hand each other: two values a lane, in two buffers that alternate, so that one barrier a round is
// enough (a wavefront writes the other buffer only behind the barrier that ends everyone's reads of it).  A team of one shares nothing.
template <int TEAM>
struct Team {
    unsigned (*red)[2][kWaves][64];
    int tw, lane, round;
    __device__ __forceinline__ void barrier() const {
        if (TEAM > 1) __syncthreads();
    }
    __device__ __forceinline__ void put(unsigned a, unsigned b) {
        if (TEAM == 1) return;
        red[round & 1][0][tw][lane] = a, red[round & 1][1][tw][lane] = b;
        __syncthreads();
    }
    __device__ __forceinline__ unsigned get(int slot, int q) const { return red[round & 1][slot][q][lane]; }
    __device__ __forceinline__ void next() { ++round; }
    __device__ __forceinline__ unsigned sum(unsigned v) {
        if (TEAM == 1) return v;
        put(v, 0);
        unsigned s = 0;
#pragma unroll
        for (int q = 0; q < TEAM; ++q) s += get(0, q);
        next();
        return s;
    }
};

// One output of lane's feature over the frames t0 .. t1-1 (xf: X[0][f]; pitch: elements between frames), by a team of TEAM wavefronts of
// which this is number tw.  live: the lane has a feature.  tile: the team's keys in LDS, [frame][64].
template <int AGG, int TEAM>
__device__ __forceinline__ float aggregate(const float* xf, long long pitch, int t0, int t1, bool live, unsigned* tile, Team<TEAM>& team) {
    const int cnt = t1 - t0, tw = team.tw, lane = team.lane;
    const float* first = xf + t0 * pitch;
    if (AGG == JSGX_SYNC_MEAN) {
        const int chunks = (cnt + kChunk - 1) / kChunk;
        float tot = 0.f;
        for (int r = 0; r < chunks; r += TEAM) {
            const int j = r + tw;
            float part = 0.f;
            if (j < chunks && live) {
                const int a = j * kChunk, e = a + kChunk < cnt ? a + kChunk : cnt;
#pragma unroll 8
                for (int t = a; t < e; ++t) part += first[t * pitch];
            }
            if (TEAM == 1) {
                tot += part;
            } else {
                team.put(__float_as_uint(part), 0);
                const int have = chunks - r < TEAM ? chunks - r : TEAM;
                for (int q = 0; q < have; ++q) tot += __uint_as_float(team.get(0, q));
                team.next();
            }
        }
        const float mean = __fdiv_rn(tot, (float)cnt);
        return mean != mean ? __uint_as_float(JSGX_SYNC_NAN_BITS) : mean;
    } else if (AGG == JSGX_SYNC_MIN || AGG == JSGX_SYNC_MAX) {
        unsigned best = AGG == JSGX_SYNC_MIN ? 0xFFFFFFFFu : 0u, nan = 0;
        if (live) {
#pragma unroll 8
            for (int t = tw; t < cnt; t += TEAM) {
                const float v = first[t * pitch];
                const unsigned k = key_of(v);
                nan |= v != v;
                best = AGG == JSGX_SYNC_MIN ? (k < best ? k : best) : (k > best ? k : best);
            }
        }
        if (TEAM > 1) {
            team.put(best, nan);
#pragma unroll
            for (int q = 0; q < TEAM; ++q) {
                const unsigned k = team.get(0, q);
                best = AGG == JSGX_SYNC_MIN ? (k < best ? k : best) : (k > best ? k : best);
                nan |= team.get(1, q);
            }
            team.next();
        }
        return nan ? __uint_as_float(JSGX_SYNC_NAN_BITS) : unkey(best);
    } else {
        const bool staged = cnt <= (TEAM == 1 ? kWaveMax : kStage);
        unsigned nan = 0;
        for (int t = tw; t < cnt; t += TEAM) {
            const float v = live ? first[t * pitch] : 0.f;
            nan |= v != v;
            if (staged) tile[t * 64 + lane] = key_of(v);
        }
        team.barrier();
        // the k-th smallest key, most significant bit first: `pre` holds the bits found, `k` the rank among the keys that begin with them
        int k = (cnt - 1) >> 1;
        unsigned pre = 0;
        for (int b = 31; b >= 0; --b) {
            unsigned zeros = 0;          // keys that begin with pre and have bit b clear
            if (staged) {
#pragma unroll 2
                for (int t = tw; t < cnt; t += TEAM) zeros += ((tile[t * 64 + lane] ^ pre) >> b) == 0;
            } else if (live) {
#pragma unroll 4
                for (int t = tw; t < cnt; t += TEAM) zeros += ((key_of(first[t * pitch]) ^ pre) >> b) == 0;
            }
            zeros = team.sum(zeros);
            if (k >= (int)zeros) k -= (int)zeros, pre |= 1u << b;
        }
        float med = unkey(pre);
        if (!(cnt & 1)) {
            // its successor in the sorted list: pre again where it repeats, else the least key above it
            unsigned upto = 0, above = 0xFFFFFFFFu;
            if (staged || live) {
                for (int t = tw; t < cnt; t += TEAM) {
                    const unsigned key = staged ? tile[t * 64 + lane] : key_of(first[t * pitch]);
                    upto += key <= pre;
                    above = key > pre && key < above ? key : above;
                }
            }
            if (TEAM > 1) {
                team.put(upto, above);
                upto = 0;
#pragma unroll
                for (int q = 0; q < TEAM; ++q) {
                    upto += team.get(0, q);
                    const unsigned a = team.get(1, q);
                    above = a < above ? a : above;
                }
                team.next();
            }
            const float hi = (int)upto > cnt / 2 ? med : unkey(above);
            med = 0.5f * (med + hi);          // a NaN where the two are the two infinities
        }
        if (TEAM > 1) nan = team.sum(nan);
        return nan || med != med ? __uint_as_float(JSGX_SYNC_NAN_BITS) : med;
    }
}

template <int AGG>
__global__ __launch_bounds__(kThreads) void sync_aggregate_kernel(const SyncK g) {
    extern __shared__ unsigned tile[];          // median: [kStage][64] keys
    __shared__ unsigned red[2][2][kWaves][64];
    const int p = blockIdx.z, o0 = kWaves * blockIdx.x;
    int ns = g.n_segments[p];
    ns = ns < g.max_segments ? ns : g.max_segments;
    if (o0 >= ns) return;          // also a refused pair
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int mine = ns - o0 < kWaves ? ns - o0 : kWaves;
    const int* seg = g.segments + p * g.segments_pitch + o0;
    int longest = 0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) {
        const int c = i < mine ? seg[i + 1] - seg[i] : 0;
        longest = c > longest ? c : longest;
    }
    const int f = 64 * blockIdx.y + lane;
    const bool live = f < g.F;
    const float* xf = g.x + p * g.x_pair_pitch + f;
    float* of = g.out + p * g.out_pair_pitch + f;
    if (longest <= (AGG == JSGX_SYNC_MEDIAN ? kWaveMax : kChunk)) {
        if (w >= mine) return;
        Team<1> team{red, 0, lane, 0};
        const float v = aggregate<AGG, 1>(xf, g.x_frame_pitch, seg[w], seg[w + 1], live, tile + w * kWaveMax * 64, team);
        if (live) of[(o0 + w) * g.out_frame_pitch] = v;
    } else {
        Team<kWaves> team{red, w, lane, 0};
        for (int i = 0; i < mine; ++i) {
            const float v = aggregate<AGG, kWaves>(xf, g.x_frame_pitch, seg[i], seg[i + 1], live, tile, team);
            if (w == 0 && live) of[(o0 + i) * g.out_frame_pitch] = v;
            __syncthreads();          // the tile is the next segment's
        }
    }
}

struct StackK {
    const unsigned* x;
    long long x_frame_pitch, x_pair_pitch;
    unsigned* out;
    long long out_frame_pitch, out_pair_pitch;
    int N, F, W, delay, mode, G;
    int rows_step, cols_step;          // kThreads = rows_step * W + cols_step
    unsigned fill;
    float inv_F;
};

__global__ __launch_bounds__(JSGX_STACK_THREADS) void stack_memory_kernel(const StackK g) {
    const long long t0 = (long long)blockIdx.x * g.G;
    const int rows = g.N - t0 < g.G ? (int)(g.N - t0) : g.G;
    const int total = rows * g.W;          // at most 2^21 + 4096
    const unsigned* x = g.x + blockIdx.z * g.x_pair_pitch;
    unsigned* out = g.out + blockIdx.z * g.out_pair_pitch;
    const unsigned F = g.F;
    int i = threadIdx.x;
    int dt = i / g.W, c = i - dt * g.W;
    for (; i < total; i += JSGX_STACK_THREADS) {
        // s = c / F: c < 2^20 is a float exactly and the product is off by less than one
        unsigned s = (unsigned)(__uint2float_rn((unsigned)c) * g.inv_F);
        unsigned f = (unsigned)c - s * F;
        if ((int)f < 0) --s, f += F;
        else if (f >= F) ++s, f -= F;
        const long long t = t0 + dt;
        long long src = t - (long long)s * g.delay;
        const bool inside = src >= 0 && src < g.N;
        src = src < 0 ? 0 : src >= g.N ? g.N - 1 : src;
        unsigned v = g.fill;
        if (inside || g.mode == JSGX_STACK_EDGE) v = x[src * g.x_frame_pitch + f];
        out[t * g.out_frame_pitch + c] = v;
        c += g.cols_step, dt += g.rows_step;
        if (c >= g.W) c -= g.W, ++dt;
    }
}

jsg::OncePerDevice g_sync_once;

}  // namespace

}  // namespace jsgx

using namespace jsgx;

extern "C" int jsgx_sync_launch(const jsgx_sync_args* g, void* stream) {
    static const char* who = "jsgx_sync_launch";
    int rc = sync_check(g, who);
    if (rc != JSGX_OK) return rc;
    int dev = -1;
    if ((rc = current_device(&dev, who)) != JSGX_OK) return rc;
    // every refusal is behind us
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const SyncPlan plan = sync_plan(g);
    const bool many = g->pairs > 1;
    SyncK k{};
    k.x = g->x, k.x_frame_pitch = g->x_frame_pitch, k.x_pair_pitch = many ? g->x_pair_pitch : 0;
    k.bounds = g->bounds, k.bounds_pitch = many ? g->bounds_pitch : 0, k.n_bounds = g->n_bounds;
    k.segments = g->segments, k.segments_pitch = many ? g->segments_pitch : 0, k.n_segments = g->n_segments;
    k.out = g->out, k.out_frame_pitch = g->out_frame_pitch, k.out_pair_pitch = many ? g->out_pair_pitch : 0;
    k.N = g->n_frames, k.F = g->n_features, k.max_bounds = g->max_bounds, k.bounds_all = g->bounds_all, k.max_segments = g->max_segments, k.pad = g->pad;
    hipLaunchKernelGGL(sync_segments_kernel, dim3((unsigned)g->pairs), dim3(kThreads), 0, s, k);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess || plan.segments == 0) return finish_launch(who, err);
    const dim3 grid((unsigned)((plan.segments + kWaves - 1) / kWaves), (unsigned)((g->n_features + 63) / 64), (unsigned)g->pairs);
    switch (g->aggregate) {
        case JSGX_SYNC_MEAN: hipLaunchKernelGGL(sync_aggregate_kernel<JSGX_SYNC_MEAN>, grid, dim3(kThreads), 0, s, k); break;
        case JSGX_SYNC_MIN: hipLaunchKernelGGL(sync_aggregate_kernel<JSGX_SYNC_MIN>, grid, dim3(kThreads), 0, s, k); break;
        case JSGX_SYNC_MAX: hipLaunchKernelGGL(sync_aggregate_kernel<JSGX_SYNC_MAX>, grid, dim3(kThreads), 0, s, k); break;
        default:
            return finish_launch(who, jsg::launch_large_lds(g_sync_once, dev, 1u, sync_aggregate_kernel<JSGX_SYNC_MEDIAN>, JSGX_SYNC_LDS_TILE, grid, dim3(kThreads),
                                                            4 * 64 * kStage, s, k));
    }
    return finish_launch(who, hipGetLastError());
}

extern "C" int jsgx_stack_memory_launch(const jsgx_stack_memory_args* g, void* stream) {
    static const char* who = "jsgx_stack_memory_launch";
    int rc = stack_memory_check(g, who);
    if (rc != JSGX_OK) return rc;
    int dev = -1;
    if ((rc = current_device(&dev, who)) != JSGX_OK) return rc;
    const bool many = g->pairs > 1;
    StackK k{};
    k.x = reinterpret_cast<const unsigned*>(g->x), k.x_frame_pitch = g->x_frame_pitch, k.x_pair_pitch = many ? g->x_pair_pitch : 0;
    k.out = reinterpret_cast<unsigned*>(g->out), k.out_frame_pitch = g->out_frame_pitch, k.out_pair_pitch = many ? g->out_pair_pitch : 0;
    k.N = g->n_frames, k.F = g->n_features, k.W = g->n_steps * g->n_features, k.delay = g->delay, k.mode = g->mode;
    k.G = stack_frames_per_group(k.N, k.W);
    k.rows_step = JSGX_STACK_THREADS / k.W, k.cols_step = JSGX_STACK_THREADS % k.W;
    k.fill = bits_of_float(g->fill), k.inv_F = 1.0f / (float)g->n_features;
    const dim3 grid((unsigned)(((long long)k.N + k.G - 1) / k.G), 1, (unsigned)g->pairs);
    hipLaunchKernelGGL(stack_memory_kernel, grid, dim3(JSGX_STACK_THREADS), 0, reinterpret_cast<hipStream_t>(stream), k);
    return finish_launch(who, hipGetLastError());
}
