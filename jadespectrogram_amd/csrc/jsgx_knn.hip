// libjsgx.so, the k nearest frames, the recurrence plane and the neighbour aggregation (include/jsgx.h sections 6 to 8): the kernels and
// their launchers.  The refusals, the plan and the scratch size are in jsgx_knn_host.cpp.
//
// "knn_64" is the cost tile of jsgx_cost_tile.h, the function that "cdist_64x64" stores (one function: the costs are the same bits), with
// the selection behind it.  A workgroup owns 64 rows of one pair and sweeps its share of the column tiles in ascending order.  The LDS:
//   panels   the two of the cost tile; once a tile's costs are in registers the same 17408 bytes take the tile, 64 rows of 68 words
//   lists    per row k float costs, then per row k 16-bit indices: the k best of the columns swept so far, ascending by (c, j)
//   pending  per row up to 64 survivors (cost, 16-bit index) that wait for their merge, in the order they came: ascending j
//   sorted   per wavefront 64 costs: those of the candidates of one merge in their order
//   lens     the entries of every row's list, and of its pending survivors; the k-th cost of every full list
// A wavefront serves the rows 16 w .. 16 w + 15 of the tile; lane l holds column j0 + l.  Everything a wavefront does to a row's list it
// does alone, so the rows need no workgroup barrier; the two barriers per tile are those around the tile itself.
#include <hip/hip_runtime.h>

#include "jsgx_cost_tile.h"

namespace jsgx {

struct KnnArgs {
    Plane<const float> x, y;
    Plane<int> nn_index;
    Plane<float> nn_dist;
    float* part_dist;           // S > 1: [p][i][s][r]
    int* part_index;
    int n, m, K, k, width, S, tiles;
};

constexpr int kRowsPerWave = JSGX_KNN_STRIP / (JSGX_KNN_THREADS / 64), kPending = 64;
static_assert(2 * kPanel * kPitch * 4 + 4 * 64 * 4 + 12 * JSGX_KNN_STRIP + 6 * kPending * JSGX_KNN_STRIP == JSGX_KNN_LDS_STATIC, "include/jsgx.h states the LDS");
static_assert(JSGX_KNN_LDS_STATIC + 6 * JSGX_KNN_STRIP * JSGX_KNN_MAX_K <= JSGX_KNN_LDS_LIMIT, "the lists of the largest k fit");
static_assert(JSGX_KNN_MAX_K <= 4 * 64, "a lane holds four entries of a list");

// the LDS of one wavefront is consistent among its lanes from here on
__device__ __forceinline__ void wave_sync() {
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
}

// One wavefront merges the candidates of `mask` (lane l holds (c, j); every one of them beats the k-th entry or the list is not full) into
// the sorted list (Lc, Lj) of `len` entries, by rank: the survivors' costs are laid down sorted in sc; a survivor goes to its rank + the
// list entries with cost <= its own, a list entry to its index + the survivors with cost < its own.  Equal costs: the list entry has
// the lower j, and among survivors the lower lane has.  Every lane reads before any lane writes.  Returns the new length.
__device__ __forceinline__ int merge_by_rank(float* Lc, unsigned short* Lj, int len, int k, float* sc, int lane, float c, int j,
                                             unsigned long long mask) {
    const bool mine = (mask >> lane) & 1;
    int rank = 0;
    for (unsigned long long rest = mask; rest; rest &= rest - 1) {
        const int s = __builtin_ctzll(rest);
        const float cs = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c), s));       // s is the same in every lane
        rank += (cs < c || (cs == c && s < lane)) ? 1 : 0;
    }
    const int ns = __builtin_popcountll(mask);
    if (mine) sc[rank] = c;
    float ec[4];
    unsigned short ej[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = lane + 64 * q;
        ec[q] = e < len ? Lc[e] : 0.f;
        ej[q] = e < len ? Lj[e] : (unsigned short)0;
    }
    wave_sync();
    int place = k;
    if (mine) {
        int lo = 0, hi = len;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (Lc[mid] <= c) lo = mid + 1; else hi = mid;
        }
        place = rank + lo;
    }
    int ep[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int lo = 0, hi = lane + 64 * q < len ? ns : 0;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sc[mid] < ec[q]) lo = mid + 1; else hi = mid;
        }
        ep[q] = lane + 64 * q + lo;
    }
    wave_sync();
    if (mine && place < k) {
        Lc[place] = c;
        Lj[place] = (unsigned short)j;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (lane + 64 * q < len && ep[q] < k) {
            Lc[ep[q]] = ec[q];
            Lj[ep[q]] = ej[q];
        }
    }
    wave_sync();
    return len + ns < k ? len + ns : k;
}

template <int METRIC>
__global__ __launch_bounds__(JSGX_KNN_THREADS) void knn_kernel(KnnArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float panels[2 * kPanel * kPitch];
    __shared__ float sorted_c[4 * 64];
    __shared__ int lens[JSGX_KNN_STRIP], pends[JSGX_KNN_STRIP];
    __shared__ float kth[JSGX_KNN_STRIP];                          // the k-th cost of a full list, a NaN before
    __shared__ float pend_c[JSGX_KNN_STRIP * kPending];
    __shared__ unsigned short pend_j[JSGX_KNN_STRIP * kPending];
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    float* ct = panels;                                            // the tile, once the panels are spent
    float* list_c = reinterpret_cast<float*>(dyn);                 // [64][k]
    unsigned short* list_j = reinterpret_cast<unsigned short*>(dyn + 4 * JSGX_KNN_STRIP * a.k);
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.y * kTile, s_part = blockIdx.x, k = a.k;
    const int t_begin = (int)((long long)s_part * a.tiles / a.S), t_end = (int)((long long)(s_part + 1) * a.tiles / a.S);
    const CostTileArgs seqs{a.x.row(blockIdx.z, 0), a.x.pitch, a.y.row(blockIdx.z, 0), a.y.pitch, a.n, a.m, a.K, panels, panels + kPanel * kPitch};
    if (tid < JSGX_KNN_STRIP) {
        lens[tid] = pends[tid] = 0;
        kth[tid] = __builtin_nanf("");
    }
    for (int t = t_begin; t < t_end; ++t) {
        const int j0 = t * kTile;
        const CostTile tile = cost_tile<METRIC>(seqs, i0, j0);
        __syncthreads();                                           // the panels are spent: the tile takes their place
#pragma unroll
        for (int r = 0; r < 4; ++r)
            *reinterpret_cast<float4*>(&ct[(4 * ti + r) * kPitch + 4 * tj]) = make_float4(tile.c[r][0], tile.c[r][1], tile.c[r][2], tile.c[r][3]);
        __syncthreads();
        // The selection is one wavefront per SIMD waiting on its own LDS reads, and its loops are sensitive to where they lie in a 64-byte
        // fetch line: 20 bytes more in front of them cost 2.8 % (profiles/knn_bench.md).  It starts on a line, whatever the cost tile takes.
        asm volatile(".p2align 6");
        const int j = j0 + lane;
        // every row of the wavefront first: one read of the cost and of the row's k-th cost, one ballot; `todo` keeps the rows with a survivor.
        // kth is a NaN while a list is not full, and then every candidate passes; an equal cost loses: every j of the list is lower
        unsigned todo = 0;
#pragma unroll 4
        for (int rr = 0; rr < kRowsPerWave; ++rr) {
            const int row = wave * kRowsPerWave + rr, i = i0 + row;
            const float c = ct[row * kPitch + lane];
            const int gap = i > j ? i - j : j - i;
            const bool pass = i < a.n && j < a.m && gap >= a.width && c == c && !(c >= kth[row]);
            if (__ballot(pass) != 0) todo |= 1u << rr;
        }
        while (todo != 0) {
            const int rr = __builtin_ctz(todo);
            todo &= todo - 1;
            const int row = wave * kRowsPerWave + rr, i = i0 + row;
            const float c = ct[row * kPitch + lane];
            const int gap = i > j ? i - j : j - i;
            bool pass = i < a.n && j < a.m && gap >= a.width && c == c && !(c >= kth[row]);
            unsigned long long mask = __ballot(pass);
            int len = __builtin_amdgcn_readfirstlane(lens[row]), pend = __builtin_amdgcn_readfirstlane(pends[row]);
            int add = __builtin_popcountll(mask);
            float* Pc = pend_c + row * kPending;
            unsigned short* Pj = pend_j + row * kPending;
            if (pend + add > kPending) {                           // no room: the waiting survivors go into the list first
                float* Lc = list_c + row * k;
                len = merge_by_rank(Lc, list_j + row * k, len, k, sorted_c + 64 * wave, lane, lane < pend ? Pc[lane] : 0.f, lane < pend ? (int)Pj[lane] : 0,
                                    pend == 64 ? ~0ull : (1ull << pend) - 1);
                pend = 0;
                if (len == k) pass = pass && c < Lc[k - 1];        // against the new k-th cost
                mask = __ballot(pass);
                add = __builtin_popcountll(mask);
                if (lane == 0) {
                    lens[row] = len;
                    if (len == k) kth[row] = Lc[k - 1];
                }
            }
            // the places of a row are written here and read by a merge of a later tile, behind a workgroup barrier: no fence between rows
            if (pass) {
                const int at = pend + __builtin_popcountll(mask & ((1ull << lane) - 1));
                Pc[at] = c;
                Pj[at] = (unsigned short)j;
            }
            if (lane == 0) pends[row] = pend + add;
        }
    }
    wave_sync();
    for (int rr = 0; rr < kRowsPerWave; ++rr) {                    // what still waits
        const int row = wave * kRowsPerWave + rr;
        const int pend = __builtin_amdgcn_readfirstlane(pends[row]);
        if (pend == 0) continue;
        const int len = merge_by_rank(list_c + row * k, list_j + row * k, __builtin_amdgcn_readfirstlane(lens[row]), k, sorted_c + 64 * wave, lane,
                                      lane < pend ? pend_c[row * kPending + lane] : 0.f, lane < pend ? (int)pend_j[row * kPending + lane] : 0,
                                      pend == 64 ? ~0ull : (1ull << pend) - 1);
        if (lane == 0) lens[row] = len;
        wave_sync();
    }
    __syncthreads();
    for (int rr = 0; rr < kRowsPerWave; ++rr) {
        const int row = wave * kRowsPerWave + rr, i = i0 + row;
        if (i >= a.n) break;
        const int len = lens[row];
        float* od;
        int* oi;
        if (a.S == 1) {
            od = a.nn_dist.row(blockIdx.z, i);
            oi = a.nn_index.row(blockIdx.z, i);
        } else {
            const long long at = (((long long)blockIdx.z * a.n + i) * a.S + s_part) * k;
            od = a.part_dist + at;
            oi = a.part_index + at;
        }
        for (int r = lane; r < k; r += 64) {
            od[r] = r < len ? list_c[row * k + r] : __builtin_inff();
            oi[r] = r < len ? (int)list_j[row * k + r] : -1;
        }
    }
}

struct KnnMergeArgs {
    const float* part_dist;     // [row][s][r]
    const int* part_index;
    Plane<int> nn_index;
    Plane<float> nn_dist;
    long long rows;             // pairs * n
    int n, k, S;
};

// "knn_merge": one wavefront per row folds the S partial lists, in ascending s and each in its own order, into one list with the merge
// above.  A partial list is sorted, so its first chunk of 64 without a survivor ends it.
__global__ __launch_bounds__(JSGX_KNN_MERGE_THREADS) void knn_merge_kernel(KnnMergeArgs a) {
    __shared__ float sorted_c[4 * 64];
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, k = a.k;
    const long long row = (long long)blockIdx.x * 4 + wave;
    if (row >= a.rows) return;                                     // whole wavefronts leave; there is no workgroup barrier below
    float* Lc = reinterpret_cast<float*>(dyn) + wave * k;
    unsigned short* Lj = reinterpret_cast<unsigned short*>(dyn + 4 * 4 * k) + wave * k;
    int len = 0;
    for (int s = 0; s < a.S; ++s) {
        const long long at = (row * a.S + s) * k;
        for (int q0 = 0; q0 < k; q0 += 64) {
            const int r = q0 + lane;
            const int j = r < k ? a.part_index[at + r] : -1;
            const float c = r < k ? a.part_dist[at + r] : 0.f;
            bool pass = j >= 0;
            if (len == k) pass = pass && c < Lc[k - 1];
            const unsigned long long mask = __ballot(pass);
            if (mask == 0) break;
            len = merge_by_rank(Lc, Lj, len, k, sorted_c + 64 * wave, lane, c, j, mask);
        }
    }
    float* od = a.nn_dist.row(row / a.n, row % a.n);
    int* oi = a.nn_index.row(row / a.n, row % a.n);
    for (int r = lane; r < k; r += 64) {
        od[r] = r < len ? Lc[r] : __builtin_inff();
        oi[r] = r < len ? (int)Lj[r] : -1;
    }
}

struct RecArgs {
    Plane<const int> nn_index;
    Plane<const float> nn_dist;
    const float* bandwidth;
    Plane<float> out;
    int n, m, k, mode, sym, diag;
};

static_assert(4 * JSGX_REC_CHUNK + 8 * JSGX_KNN_MAX_K == JSGX_REC_LDS_BYTES && JSGX_KNN_MAX_K <= JSGX_REC_THREADS, "include/jsgx.h states the LDS");

// "recurrence_rows": a workgroup per row.  Lane r < k resolves entry r of the row's list (the link, with sym the look into the other
// row's list, and the value); the row is then built in LDS piece by piece and stored once.
__global__ __launch_bounds__(JSGX_REC_THREADS) void recurrence_kernel(RecArgs a) {
#pragma clang fp contract(off)
    __shared__ float piece[JSGX_REC_CHUNK];
    __shared__ int link_j[JSGX_KNN_MAX_K];
    __shared__ float link_v[JSGX_KNN_MAX_K];
    const int tid = threadIdx.x, i = blockIdx.x;
    if (tid < JSGX_KNN_MAX_K) {
        int j = tid < a.k ? a.nn_index.row(blockIdx.y, i)[tid] : -1;
        if (j < 0 || j >= a.m || (a.diag && j == i)) j = -1;      // the diagonal is written by its own rule
        if (j >= 0 && a.sym) {
            const int* other = a.nn_index.row(blockIdx.y, j);
            bool mutual = false;
            for (int r = 0; r < a.k; ++r) mutual = mutual || other[r] == i;
            if (!mutual) j = -1;
        }
        float v = 1.0f;
        if (j >= 0 && a.mode != JSGX_REC_CONNECTIVITY) {
            v = a.nn_dist.row(blockIdx.y, i)[tid];
            if (a.mode == JSGX_REC_AFFINITY) {
                const float bw = a.bandwidth[blockIdx.y];
                v = (!(bw > 0.f) || v != v) ? __builtin_nanf("") : exp_neg(-(v / bw));
            }
        }
        link_j[tid] = j;
        link_v[tid] = v;
    }
    float* out = a.out.row(blockIdx.y, i);
    for (int c0 = 0; c0 < a.m; c0 += JSGX_REC_CHUNK) {
        const int width = a.m - c0 < JSGX_REC_CHUNK ? a.m - c0 : JSGX_REC_CHUNK;
        __syncthreads();
        for (int t = tid; t < width; t += JSGX_REC_THREADS) piece[t] = 0.f;
        __syncthreads();
        if (tid < JSGX_KNN_MAX_K) {
            const int j = link_j[tid];
            if (j >= c0 && j < c0 + width) piece[j - c0] = link_v[tid];
        }
        if (tid == JSGX_REC_THREADS - 1 && a.diag && i >= c0 && i < c0 + width) piece[i - c0] = a.mode == JSGX_REC_DISTANCE ? 0.0f : 1.0f;
        __syncthreads();
        for (int t = tid; t < width; t += JSGX_REC_THREADS) out[c0 + t] = piece[t];
    }
}

struct NnfArgs {
    Plane<const float> s;
    Plane<const int> nn_index;
    Plane<const float> weights;
    Plane<float> out;
    int n, F, k;
};

// "nn_filter_rows": one wavefront per row, lane l the features l, l + 64, ...; r ascends, as the header states the sums.
__global__ __launch_bounds__(JSGX_NNF_THREADS) void nn_filter_kernel(NnfArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.x, lane = threadIdx.x;
    const int* idx = a.nn_index.row(blockIdx.y, i);
    const float* w = a.weights.p ? a.weights.row(blockIdx.y, i) : nullptr;
    float* out = a.out.row(blockIdx.y, i);
    for (int f = lane; f < a.F; f += JSGX_NNF_THREADS) {
        float acc = 0.f, den = 0.f;
        int cnt = 0;
        for (int r = 0; r < a.k; ++r) {
            const int j = idx[r];
            if (j < 0 || j >= a.n) continue;
            const float v = a.s.row(blockIdx.y, j)[f];
            ++cnt;
            if (w) {
                acc = __builtin_fmaf(w[r], v, acc);
                den = den + w[r];
            } else {
                acc = acc + v;
            }
        }
        if (!w) den = (float)cnt;
        out[f] = (cnt == 0 || den == 0.f) ? a.s.row(blockIdx.y, i)[f] : acc / den;
    }
}

namespace {
jsg::OncePerDevice g_knn_once;
std::atomic<int> g_cu_count[64];

// the compute units of the device, asked once per device
int cu_count(int dev) {
    if (dev >= 0 && dev < 64) {
        const int known = g_cu_count[dev].load(std::memory_order_relaxed);
        if (known > 0) return known;
    }
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 1;
    if (dev >= 0 && dev < 64) g_cu_count[dev].store(n, std::memory_order_relaxed);
    return n;
}
}  // namespace

}  // namespace jsgx

using namespace jsgx;

extern "C" int jsgx_knn_launch(const jsgx_knn_args* g, void* scratch, int64_t scratch_bytes, void* stream) {
    static const char* who = "jsgx_knn_launch";
    int rc = knn_check(g, who);
    if (rc != JSGX_OK) return rc;
    const int64_t need = knn_plan(g, 0).scratch_bytes;
    if (need != 0 && (rc = check_scratch(who, scratch, scratch_bytes, need, "jsgx_knn_scratch_bytes")) != JSGX_OK) return rc;
    int dev = -1;
    if ((rc = current_device(&dev, who)) != JSGX_OK) return rc;
    // every refusal is behind us
    const KnnPlan p = knn_plan(g, g->split != 0 ? 1 : cu_count(dev));
    KnnArgs k{};
    k.x = sequence_of(g->x, g->x_frame_pitch, g->x_pair_pitch);
    k.y = sequence_of(g->y, g->y_frame_pitch, g->y_pair_pitch);
    k.nn_index = plane_of(g->nn_index, g->index_pitch, g->index_pair_pitch, g->pairs);
    k.nn_dist = plane_of(g->nn_dist, g->dist_pitch, g->dist_pair_pitch, g->pairs);
    const long long entries = (long long)g->pairs * g->n * g->k * p.S;
    k.part_dist = p.S > 1 ? static_cast<float*>(scratch) : nullptr;
    k.part_index = p.S > 1 ? static_cast<int*>(scratch) + entries : nullptr;
    k.n = g->n;
    k.m = g->m;
    k.K = g->n_features;
    k.k = g->k;
    k.width = g->width;
    k.S = p.S;
    k.tiles = p.tiles;
    const dim3 grid((unsigned)p.S, (unsigned)((g->n + JSGX_KNN_STRIP - 1) / JSGX_KNN_STRIP), (unsigned)g->pairs);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int lds_max = JSGX_KNN_LDS_LIMIT - JSGX_KNN_LDS_STATIC;
    hipError_t err;
    if (g->metric == JSGX_METRIC_SQEUCLIDEAN)
        err = jsg::launch_large_lds(g_knn_once, dev, 1u, knn_kernel<JSGX_METRIC_SQEUCLIDEAN>, lds_max, grid, dim3(JSGX_KNN_THREADS), (size_t)p.lds_dynamic, s, k);
    else if (g->metric == JSGX_METRIC_EUCLIDEAN)
        err = jsg::launch_large_lds(g_knn_once, dev, 2u, knn_kernel<JSGX_METRIC_EUCLIDEAN>, lds_max, grid, dim3(JSGX_KNN_THREADS), (size_t)p.lds_dynamic, s, k);
    else
        err = jsg::launch_large_lds(g_knn_once, dev, 4u, knn_kernel<JSGX_METRIC_COSINE>, lds_max, grid, dim3(JSGX_KNN_THREADS), (size_t)p.lds_dynamic, s, k);
    if (err == hipSuccess && p.S > 1) {
        KnnMergeArgs q{};
        q.part_dist = k.part_dist;
        q.part_index = k.part_index;
        q.nn_index = k.nn_index;
        q.nn_dist = k.nn_dist;
        q.rows = (long long)g->pairs * g->n;
        q.n = g->n;
        q.k = g->k;
        q.S = p.S;
        hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((q.rows + 3) / 4)), dim3(JSGX_KNN_MERGE_THREADS), (size_t)(4 * 6 * g->k), s, q);
        err = hipGetLastError();
    }
    return finish_launch(who, err);
}

extern "C" int jsgx_recurrence_launch(const jsgx_recurrence_args* g, void* stream) {
    static const char* who = "jsgx_recurrence_launch";
    int rc = recurrence_check(g, who);
    if (rc != JSGX_OK) return rc;
    int dev = -1;
    if ((rc = current_device(&dev, who)) != JSGX_OK) return rc;
    RecArgs k{};
    k.nn_index = plane_of(g->nn_index, g->index_pitch, g->index_pair_pitch, g->pairs);
    k.nn_dist = plane_of(g->nn_dist, g->dist_pitch, g->dist_pair_pitch, g->pairs);
    k.bandwidth = g->bandwidth;
    k.out = plane_of(g->out, g->out_pitch, g->out_pair_pitch, g->pairs);
    k.n = g->n;
    k.m = g->m;
    k.k = g->k;
    k.mode = g->mode;
    k.sym = g->sym;
    k.diag = g->diag;
    hipLaunchKernelGGL(recurrence_kernel, dim3((unsigned)g->n, (unsigned)g->pairs), dim3(JSGX_REC_THREADS), 0, reinterpret_cast<hipStream_t>(stream), k);
    return finish_launch(who, hipGetLastError());
}

extern "C" int jsgx_nn_filter_launch(const jsgx_nn_filter_args* g, void* stream) {
    static const char* who = "jsgx_nn_filter_launch";
    int rc = nn_filter_check(g, who);
    if (rc != JSGX_OK) return rc;
    int dev = -1;
    if ((rc = current_device(&dev, who)) != JSGX_OK) return rc;
    NnfArgs k{};
    k.s = plane_of(g->s, g->s_frame_pitch, g->s_pair_pitch, g->pairs);
    k.nn_index = plane_of(g->nn_index, g->index_pitch, g->index_pair_pitch, g->pairs);
    k.weights = plane_of(g->weights, g->weights_pitch, g->weights_pair_pitch, g->pairs);
    k.out = plane_of(g->out, g->out_frame_pitch, g->out_pair_pitch, g->pairs);
    k.n = g->n;
    k.F = g->n_features;
    k.k = g->k;
    hipLaunchKernelGGL(nn_filter_kernel, dim3((unsigned)g->n, (unsigned)g->pairs), dim3(JSGX_NNF_THREADS), 0, reinterpret_cast<hipStream_t>(stream), k);
    return finish_launch(who, hipGetLastError());
}
