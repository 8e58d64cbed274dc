// libjsgx.so, non-negative matrix factorisation (include/jsgx.h section 12): the kernels and the launcher.  Every long sum is a chain of
// v_mfma_f32_16x16x4_f32 (float32 in, float32 accumulate): on gfx950 that is bit for bit the k-ascending fmaf chain from its accumulator
// input, which is the order the header states.  A workgroup stages 64 x 64 panels into LDS, zero-filled outside the planes (fmaf(+0,
// +0, acc) = acc on non-negative data), and each of its four wavefronts owns 16 x 16 output tiles.
//
// An operand of a product sum over k is read as element (idx, k): idx the row of the left factor or the column of the right one.  A
// panel holds it either idx-major ("KC": k along a row of 68 words) or k-major ("KM": idx along a row of 80 words).  Lane l of a
// wavefront reads (idx0 + (l & 15), k0 + (l >> 4)): 16 rows of 68 words and 4 offsets, or 4 rows of 80 words and 16 offsets, fall on 64
// different banks.  The result tile has its column on l & 15 and row 4 (l >> 4) + j in register j.
#include "jsgx_internal.h"

namespace jsgx {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = JSGX_NMF_THREADS;
constexpr int kPanel = 64;                     // rows and columns of a staged panel
constexpr int kPitchKC = 68, kPitchKM = 80;    // words of a panel row
constexpr int kPanelWords = kPanel * kPitchKM;
static_assert(2 * 4 * kPanelWords == JSGX_NMF_LDS_BYTES, "include/jsgx.h states the LDS");
static_assert(JSGX_NMF_CHUNK_K % kPanel == 0 && JSGX_NMF_CHUNK_T % kPanel == 0, "a chunk is whole panels");
static_assert(JSGX_NMF_MAX_COMPONENTS == kPanel, "every component fits one panel");

struct NmfArgs {
    const float* v;
    long long v_pitch, v_problem_pitch;
    float* a;
    long long a_pitch, a_problem_pitch;
    float* c;
    long long c_pitch, c_problem_pitch;
    int T, K, r;
    float *g, *g2, *gpart, *n2part;            // the scratch: [P][r][r], [P][r][r], [P][chunks_g][r][r], [P][cT][r][K]
    int chunks_g, chunks_t;
};

// A thread's share of a 64 x 64 panel on its way from memory: column threadIdx.x & 63 of rows (threadIdx.x >> 6) + 4 j, and how much of
// the panel lies inside the plane.
struct Piece {
    float x[kPanel * kPanel / kThreads];
    int rows, cols;
};
// rows x cols (each >= 1, may be > 64) of a row-major source.  A lane outside reads src[0], which every caller owns: the loads are
// unconditional, so all are issued before the first is waited for; put() drops what lay outside
__device__ __forceinline__ void fetch(Piece& piece, const float* src, long long src_pitch, long long rows, long long cols) {
    const int col = threadIdx.x & (kPanel - 1), row0 = threadIdx.x >> 6;
    piece.rows = rows < kPanel ? (int)rows : kPanel, piece.cols = cols < kPanel ? (int)cols : kPanel;
#pragma unroll
    for (int j = 0; j < kPanel * kPanel / kThreads; ++j) {
        const int row = row0 + j * (kThreads / kPanel);
        piece.x[j] = src[row < piece.rows && col < piece.cols ? row * src_pitch + col : 0];
    }
}
// into the panel, +0 outside the plane
__device__ __forceinline__ void put(float* panel, int pitch, const Piece& piece) {
    const int col = threadIdx.x & (kPanel - 1), row0 = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < kPanel * kPanel / kThreads; ++j) {
        const int row = row0 + j * (kThreads / kPanel);
        panel[row * pitch + col] = row < piece.rows && col < piece.cols ? piece.x[j] : 0.f;
    }
}
__device__ __forceinline__ void stage(float* panel, int pitch, const float* src, long long src_pitch, long long rows, long long cols) {
    Piece piece;
    fetch(piece, src, src_pitch, rows, cols);
    put(panel, pitch, piece);
}

template <bool KM>
__device__ __forceinline__ float operand(const float* panel, int idx, int k) {
    return KM ? panel[k * kPitchKM + idx] : panel[idx * kPitchKC + k];
}

__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0); }

__device__ __forceinline__ int round_up4(long long n) { return n >= kPanel ? kPanel : (int)((n + 3) & ~3LL); }

// A after the multiplicative update, as the header states it
__device__ __forceinline__ float updated(float old, float num, float den) {
    const float dz = den != 0.f ? den : JSGX_NMF_EPSILON;
    return old * __fdiv_rn(num, dz);
}

// "nmf_gram": the chain of one chunk of G = C C^T (FRAMES false: the chunk is of bins) or of G2 = A^T A (FRAMES true: of frames).
// The CT x CT tiles of 16 x 16 go round the four wavefronts, NS to each; a slot behind the last tile repeats tile 0 and is not stored, so
// the loop has no branch.  grid (chunk, problem)
template <bool FRAMES, int CT>
__global__ __launch_bounds__(kThreads) void nmf_gram_kernel(NmfArgs g) {
    __shared__ float panel[kPanelWords];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, h = lane >> 4;
    const long long p = blockIdx.y, q = blockIdx.x;
    const long long n = FRAMES ? g.T : g.K, L = FRAMES ? JSGX_NMF_CHUNK_T : JSGX_NMF_CHUNK_K;
    const long long lo = q * L, hi = lo + L < n ? lo + L : n;
    const float* src = FRAMES ? g.a + p * g.a_problem_pitch : g.c + p * g.c_problem_pitch;
    constexpr int tiles = CT * CT, NS = (tiles + 3) / 4;
    f32x4 acc[NS];
    int left[NS], right[NS];                    // the first index of either operand of a slot's tile
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int tile = wave + 4 * s < tiles ? wave + 4 * s : 0;
        acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
        left[s] = 16 * (tile / CT) + i, right[s] = 16 * (tile % CT) + i;
    }
    // the next panel is on its way from memory while this one is multiplied
    Piece next;
    auto fetch_panel = [&](long long kb) {
        if (FRAMES)
            fetch(next, src + kb * g.a_pitch, g.a_pitch, hi - kb, g.r);
        else
            fetch(next, src + kb, g.c_pitch, g.r, hi - kb);
    };
    fetch_panel(lo);
    for (long long kb = lo; kb < hi; kb += kPanel) {
        __syncthreads();
        put(panel, FRAMES ? kPitchKM : kPitchKC, next);
        __syncthreads();
        if (kb + kPanel < hi) fetch_panel(kb + kPanel);
#pragma unroll
        for (int k0 = 0; k0 < kPanel; k0 += 4) {          // the whole panel: behind the chunk's end it holds +0
#pragma unroll
            for (int s = 0; s < NS; ++s) acc[s] = mfma(operand<FRAMES>(panel, left[s], k0 + h), operand<FRAMES>(panel, right[s], k0 + h), acc[s]);
        }
    }
    float* out = g.gpart + (p * g.chunks_g + q) * g.r * g.r;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int tile = wave + 4 * s;
        if (tile >= tiles) continue;
        const int col = 16 * (tile % CT) + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = 16 * (tile / CT) + 4 * h + j;
            if (row < g.r && col < g.r) out[row * g.r + col] = acc[s][j];
        }
    }
}

// "nmf_chunk_sum": the chunks' partials of every element in ascending order, plain adds: part [P][chunks and more][elems] -> out
// [P][elems] at its own problem pitch.  out may be chunk 0 of part itself: a lane reads its own element's partials and writes that
// element alone.  grid (ceil(elems / 256), problem)
__global__ __launch_bounds__(kThreads) void nmf_chunk_sum_kernel(const float* part, long long elems, long long part_problem_pitch, int chunks, float* out,
                                                                 long long out_problem_pitch) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x, p = blockIdx.y;
    if (e >= elems) return;
    const float* mine = part + p * part_problem_pitch + e;
    float sum = mine[0];
#pragma unroll 8
    for (int q = 1; q < chunks; ++q) sum = sum + mine[q * elems];
    out[p * out_problem_pitch + e] = sum;
}

// "nmf_update_a": a strip of 64 frames, 16 to a wavefront; CT tiles of 16 components.  grid (strip, problem)
template <int CT>
__global__ __launch_bounds__(kThreads) void nmf_update_a_kernel(NmfArgs g) {
    __shared__ float lds[2 * kPanelWords];
    float *pv = lds, *pc = lds + kPanelWords;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, h = lane >> 4;
    const long long p = blockIdx.y, t0 = (long long)blockIdx.x * kPanel;
    const float* v = g.v + p * g.v_problem_pitch + t0 * g.v_pitch;
    const float* c = g.c + p * g.c_problem_pitch;
    float* a = g.a + p * g.a_problem_pitch + t0 * g.a_pitch;
    const int rows = g.T - t0 < kPanel ? (int)(g.T - t0) : kPanel;          // the frames of this strip
    f32x4 sum[CT], acc[CT];
    // panel by panel along k, the next one on its way from memory while this one is multiplied; a chunk is whole panels but for the last
    Piece next_v, next_c;
    fetch(next_v, v, g.v_pitch, rows, g.K);
    fetch(next_c, c, g.c_pitch, g.r, g.K);
    for (int kb = 0; kb < g.K; kb += kPanel) {
        if (kb % JSGX_NMF_CHUNK_K == 0) {
#pragma unroll
            for (int n = 0; n < CT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        put(pv, kPitchKC, next_v);
        put(pc, kPitchKC, next_c);
        __syncthreads();
        const int kb1 = kb + kPanel;
        if (kb1 < g.K) {
            fetch(next_v, v + kb1, g.v_pitch, rows, g.K - kb1);
            fetch(next_c, c + kb1, g.c_pitch, g.r, g.K - kb1);
        }
#pragma unroll
        for (int k0 = 0; k0 < kPanel; k0 += 4) {          // the whole panel: behind bin K it holds +0
            const float x = operand<false>(pv, 16 * wave + i, k0 + h);
#pragma unroll
            for (int n = 0; n < CT; ++n) acc[n] = mfma(x, operand<false>(pc, 16 * n + i, k0 + h), acc[n]);
        }
        if (kb1 % JSGX_NMF_CHUNK_K == 0 || kb1 >= g.K) {
#pragma unroll
            for (int n = 0; n < CT; ++n) sum[n] = kb < JSGX_NMF_CHUNK_K ? acc[n] : sum[n] + acc[n];
        }
    }
    // D[t][c] = chain over c' of A[t][c'] G[c'][c]: the strip of A idx-major, G k-major
    __syncthreads();
    stage(pv, kPitchKC, a, g.a_pitch, rows, g.r);
    stage(pc, kPitchKM, g.g + p * g.r * g.r, g.r, g.r, g.r);
    __syncthreads();
    const int kn = round_up4(g.r);
#pragma unroll
    for (int n = 0; n < CT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < kn; k0 += 4) {
        const float x = operand<false>(pv, 16 * wave + i, k0 + h);
#pragma unroll
        for (int n = 0; n < CT; ++n) acc[n] = mfma(x, operand<true>(pc, 16 * n + i, k0 + h), acc[n]);
    }
#pragma unroll
    for (int n = 0; n < CT; ++n) {
        const int comp = 16 * n + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int frame = 16 * wave + 4 * h + j;
            if (frame < rows && comp < g.r) a[frame * g.a_pitch + comp] = updated(pv[frame * kPitchKC + comp], sum[n][j], acc[n][j]);
        }
    }
}

// "nmf_partial_c": the chain of one frame chunk of N2[c][k] for a tile of 64 bins, 16 to a wavefront.  grid (bin tile, chunk, problem)
template <int CT>
__global__ __launch_bounds__(kThreads) void nmf_partial_c_kernel(NmfArgs g) {
    __shared__ float lds[2 * kPanelWords];
    float *pa = lds, *pv = lds + kPanelWords;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, h = lane >> 4;
    const long long p = blockIdx.z, q = blockIdx.y;
    const int b0 = blockIdx.x * kPanel;
    const long long lo = q * JSGX_NMF_CHUNK_T, hi = lo + JSGX_NMF_CHUNK_T < g.T ? lo + JSGX_NMF_CHUNK_T : g.T;
    const float* v = g.v + p * g.v_problem_pitch + b0;
    const float* a = g.a + p * g.a_problem_pitch;
    f32x4 acc[CT];
#pragma unroll
    for (int n = 0; n < CT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    Piece next_a, next_v;
    fetch(next_a, a + lo * g.a_pitch, g.a_pitch, hi - lo, g.r);
    fetch(next_v, v + lo * g.v_pitch, g.v_pitch, hi - lo, g.K - b0);
    for (long long tb = lo; tb < hi; tb += kPanel) {
        __syncthreads();
        put(pa, kPitchKM, next_a);
        put(pv, kPitchKM, next_v);
        __syncthreads();
        const long long tb1 = tb + kPanel;
        if (tb1 < hi) {
            fetch(next_a, a + tb1 * g.a_pitch, g.a_pitch, hi - tb1, g.r);
            fetch(next_v, v + tb1 * g.v_pitch, g.v_pitch, hi - tb1, g.K - b0);
        }
#pragma unroll
        for (int k0 = 0; k0 < kPanel; k0 += 4) {          // the whole panel: behind the chunk's end it holds +0
            const float y = operand<true>(pv, 16 * wave + i, k0 + h);
#pragma unroll
            for (int n = 0; n < CT; ++n) acc[n] = mfma(operand<true>(pa, 16 * n + i, k0 + h), y, acc[n]);
        }
    }
    float* out = g.n2part + (p * g.chunks_t + q) * g.r * g.K;
    const int bin = b0 + 16 * wave + i;
#pragma unroll
    for (int n = 0; n < CT; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int comp = 16 * n + 4 * h + j;
            if (comp < g.r && bin < g.K) out[(long long)comp * g.K + bin] = acc[n][j];
        }
}

// "nmf_update_c": a tile of 64 bins, every component: the workgroup alone reads and writes these columns of C.  grid (bin tile, problem)
template <int CT>
__global__ __launch_bounds__(kThreads) void nmf_update_c_kernel(NmfArgs g) {
    __shared__ float lds[2 * kPanelWords];
    float *pg = lds, *pc = lds + kPanelWords;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, h = lane >> 4;
    const long long p = blockIdx.y;
    const int b0 = blockIdx.x * kPanel;
    float* c = g.c + p * g.c_problem_pitch + b0;
    // D2[c][k] = chain over c' of G2[c][c'] C[c'][k]: G2 idx-major, the columns of C k-major
    stage(pg, kPitchKC, g.g2 + p * g.r * g.r, g.r, g.r, g.r);
    stage(pc, kPitchKM, c, g.c_pitch, g.r, g.K - b0);
    __syncthreads();
    const int kn = round_up4(g.r);
    f32x4 acc[CT];
#pragma unroll
    for (int n = 0; n < CT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < kn; k0 += 4) {
        const float y = operand<true>(pc, 16 * wave + i, k0 + h);
#pragma unroll
        for (int n = 0; n < CT; ++n) acc[n] = mfma(operand<false>(pg, 16 * n + i, k0 + h), y, acc[n]);
    }
    const int col = 16 * wave + i;
    if (b0 + col >= g.K) return;
    const float* n2 = g.n2part + p * g.chunks_t * g.r * g.K + b0 + col;          // chunk 0 holds the sum (nmf_chunk_sum)
#pragma unroll
    for (int n = 0; n < CT; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int comp = 16 * n + 4 * h + j;
            if (comp >= g.r) continue;
            c[comp * g.c_pitch + col] = updated(pc[comp * kPitchKM + col], n2[(long long)comp * g.K], acc[n][j]);
        }
}

template <template <int> class Launch>
void by_tiles(int ct, const dim3& grid, hipStream_t s, const NmfArgs& k) {
    switch (ct) {
        case 1: Launch<1>::go(grid, s, k); break;
        case 2: Launch<2>::go(grid, s, k); break;
        case 3: Launch<3>::go(grid, s, k); break;
        default: Launch<4>::go(grid, s, k); break;
    }
}
template <int CT>
struct GramOfC {
    static void go(const dim3& grid, hipStream_t s, const NmfArgs& k) { hipLaunchKernelGGL((nmf_gram_kernel<false, CT>), grid, dim3(kThreads), 0, s, k); }
};
template <int CT>
struct GramOfA {
    static void go(const dim3& grid, hipStream_t s, const NmfArgs& k) { hipLaunchKernelGGL((nmf_gram_kernel<true, CT>), grid, dim3(kThreads), 0, s, k); }
};
template <int CT>
struct UpdateA {
    static void go(const dim3& grid, hipStream_t s, const NmfArgs& k) { hipLaunchKernelGGL(nmf_update_a_kernel<CT>, grid, dim3(kThreads), 0, s, k); }
};
template <int CT>
struct PartialC {
    static void go(const dim3& grid, hipStream_t s, const NmfArgs& k) { hipLaunchKernelGGL(nmf_partial_c_kernel<CT>, grid, dim3(kThreads), 0, s, k); }
};
template <int CT>
struct UpdateC {
    static void go(const dim3& grid, hipStream_t s, const NmfArgs& k) { hipLaunchKernelGGL(nmf_update_c_kernel<CT>, grid, dim3(kThreads), 0, s, k); }
};

}  // namespace

}  // namespace jsgx

using namespace jsgx;

extern "C" int jsgx_nmf_launch(const jsgx_nmf_args* g, void* scratch, int64_t scratch_bytes, void* stream) {
    static const char* who = "jsgx_nmf_launch";
    NmfSpans spans;
    int rc = nmf_check(g, who, &spans);
    if (rc == JSGX_OK) rc = nmf_check_scratch(g, who, spans, scratch, scratch_bytes);
    if (rc != JSGX_OK) return rc;
    int dev = -1;
    if ((rc = current_device(&dev, who)) != JSGX_OK) return rc;
    // every refusal is behind us
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const NmfScratch lay = nmf_scratch(g);
    const bool many = g->problems > 1;
    NmfArgs k{};
    k.v = g->v, k.v_pitch = g->v_pitch, k.v_problem_pitch = many ? g->v_problem_pitch : 0;
    k.a = g->a, k.a_pitch = g->a_pitch, k.a_problem_pitch = many ? g->a_problem_pitch : 0;
    k.c = g->c, k.c_pitch = g->c_pitch, k.c_problem_pitch = many ? g->c_problem_pitch : 0;
    k.T = g->n_frames, k.K = g->n_bins, k.r = g->n_components;
    float* base = static_cast<float*>(scratch);
    k.g = base, k.g2 = base + lay.off_g2, k.gpart = base + lay.off_gpart, k.n2part = base + lay.off_n2part;
    k.chunks_g = (int)lay.chunks_g, k.chunks_t = (int)lay.chunks_t;
    const unsigned P = (unsigned)g->problems;
    const int ct = (k.r + 15) / 16;
    const long long rr = (long long)k.r * k.r, rK = (long long)k.r * k.K;
    const dim3 sum_grid((unsigned)((rr + kThreads - 1) / kThreads), P), n2_grid((unsigned)((rK + kThreads - 1) / kThreads), P);
    const dim3 strips((unsigned)(((long long)k.T + kPanel - 1) / kPanel), P);
    const unsigned bin_tiles = (unsigned)((k.K + kPanel - 1) / kPanel);
    for (int it = 0; it < g->n_iter; ++it) {
        if (it == 0 || g->update_components) {
            by_tiles<GramOfC>(ct, dim3((unsigned)lay.chunks_k, P), s, k);
            hipLaunchKernelGGL(nmf_chunk_sum_kernel, sum_grid, dim3(kThreads), 0, s, k.gpart, rr, lay.chunks_g * rr, (int)lay.chunks_k, k.g, rr);
        }
        by_tiles<UpdateA>(ct, strips, s, k);
        if (!g->update_components) continue;
        by_tiles<GramOfA>(ct, dim3((unsigned)lay.chunks_t, P), s, k);
        hipLaunchKernelGGL(nmf_chunk_sum_kernel, sum_grid, dim3(kThreads), 0, s, k.gpart, rr, lay.chunks_g * rr, (int)lay.chunks_t, k.g2, rr);
        by_tiles<PartialC>(ct, dim3(bin_tiles, (unsigned)lay.chunks_t, P), s, k);
        hipLaunchKernelGGL(nmf_chunk_sum_kernel, n2_grid, dim3(kThreads), 0, s, k.n2part, rK, lay.chunks_t * rK, (int)lay.chunks_t, k.n2part, lay.chunks_t * rK);
        by_tiles<UpdateC>(ct, dim3(bin_tiles, P), s, k);
    }
    return finish_launch(who, hipGetLastError());
}
