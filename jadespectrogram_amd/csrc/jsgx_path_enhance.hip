// libjsgx.so, path enhancement of a recurrence plane and its time-lag conversion (include/jsgx.h sections 10 and 11): the kernels and their
// launchers.  The refusals, the plan and the filter-bank builder are in jsgx_path_enhance_host.cpp.
//
// path_enhance_kernel.  A workgroup of 256 lanes owns a 64 x 64 output tile and stages the tile with its halo (reach_i rows above and
// below, reach_j columns left and right) once into LDS, +0 outside the plane: adding w * (+0) leaves the bits of a chain that started at
// +0 (the header), so the hot loop has no bounds.  The window has `pitch` words a row, 1 (mod 4).
//   lane = lx + 8 ly (+ 64 wave):  the lane holds the outputs of rows wy * 32 + ly + 8 k (k < 4) and columns wx * 32 + 4 lx + c (c < 4),
//   wx = wave & 1, wy = wave >> 1.  A ds_read_b32 of a wavefront is served in two halves of 32 lanes, lx < 8 and four consecutive ly: their
//   words lie at 4 lx + ly * pitch, and with pitch = 1 (mod 4) these are 32 different banks.
// The tap list is the same for every lane, so the eight taps from t on are fetched with scalar loads and their weights enter v_fma_f32 as
// scalar operands.  The builder emits a table's taps in row-major order, so a row's taps follow each other with dj falling by one: such a
// run of L taps (L = 8, 4, 2 or 1, a uniform branch) reads L + 3 words per output row and feeds 4 L fused multiply-adds with them,
// instead of 4 L reads; every output still takes its taps in list order, one fmaf each.
//
// lag_columns_kernel (axis 1).  out[l][j] = in[(l + j) mod L][j]: the source of a 64 x 64 output tile is a parallelogram, 127 row pieces of
// 64 columns.  They are read as whole 256-byte lines into LDS (64 words a piece: the read of a lane row, one word per bank) and written
// out as whole lines.  From lag the piece of output (r, c) is r - c + 63 instead of r + c.
// lag_rows_kernel (axis 0).  out[i][c] = in[i][(c +- i) mod L]: a rotation of every row; reads and writes run along the row.
#include <hip/hip_runtime.h>

#include "jsgx_internal.h"

namespace jsgx {

constexpr int kPeTile = JSGX_PE_TILE;
constexpr int kPeRows = 4, kPeThreads = JSGX_PE_THREADS, kPeWaves = kPeThreads / 64;          // the output rows a lane holds
static_assert(kPeTile == 64 && kPeThreads == 256 && kPeRows * 8 * (kPeWaves / 2) == kPeTile, "the lane layout below");
static_assert(4 * (kPeTile + 2 * JSGX_PE_MAX_REACH) * (((kPeTile + 2 * JSGX_PE_MAX_REACH + 3) & ~3) + 1) <= JSGX_PE_LDS_LIMIT, "the largest window fits the LDS");
static_assert((2 * JSGX_LAG_TILE - 1) * JSGX_LAG_TILE * 4 == JSGX_LAG_LDS_BYTES, "include/jsgx.h states the LDS");

struct PeArgs {
    Plane<const float> r;
    Plane<float> out;
    const float* tap_w;
    const int* tap_at;
    const int* first;
    int n, m, n_filters, n_taps, reach_i, reach_j, clip, pitch;
};

// A run of L taps at one di whose dj falls by one from tap to tap: `p` is the lane's word for the LAST tap of the run (the lowest
// column); tap t of the run reads column c + (L - 1 - t) of the words from there.
template <int L>
__device__ __forceinline__ void pe_run(const float* p, int row_stride, const float (&w)[8], float (&acc)[kPeRows][4]) {
#pragma unroll
    for (int k = 0; k < kPeRows; ++k) {
        float v[L + 3];
#pragma unroll
        for (int q = 0; q < L + 3; ++q) v[q] = p[k * row_stride + q];
#pragma unroll
        for (int t = 0; t < L; ++t)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[k][c] = __builtin_fmaf(w[t], v[c + L - 1 - t], acc[k][c]);
    }
}

__global__ __launch_bounds__(kPeThreads) void path_enhance_kernel(PeArgs a) {
    extern __shared__ __attribute__((aligned(16))) float win[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.y * kPeTile, j0 = blockIdx.x * kPeTile;
    const int ri = a.reach_i, rj = a.reach_j, pitch = a.pitch;
    const int rows = kPeTile + 2 * ri, cols = kPeTile + 2 * rj;
    // ---- the window: a wavefront takes every fourth row, its lanes run along the row
    {
        const float* R = a.r.row(blockIdx.z, 0);
        for (int wr = wave; wr < rows; wr += kPeWaves) {
            const int gi = i0 - ri + wr;
            const bool row_in = gi >= 0 && gi < a.n;
            const float* src = R + (long long)(row_in ? gi : 0) * a.r.pitch;
            for (int c = lane; c < cols; c += 64) {
                const int gj = j0 - rj + c;
                win[wr * pitch + c] = row_in && gj >= 0 && gj < a.m ? src[gj] : 0.f;
            }
        }
    }
    __syncthreads();
    const int lx = lane & 7, ly = lane >> 3, wx = wave & 1, wy = wave >> 1;
    const int row0 = wy * 8 * kPeRows + ly, col0 = wx * 32 + 4 * lx;
    const float* base = win + row0 * pitch + col0;
    const int row_stride = 8 * pitch;
    float best[kPeRows][4];
    const int n_taps = a.n_taps;
    for (int f = 0; f < a.n_filters; ++f) {
        int t = a.first[f], end = a.first[f + 1];
        t = t < 0 ? 0 : (t > n_taps ? n_taps : t);
        end = end < 0 ? 0 : (end > n_taps ? n_taps : end);
        float acc[kPeRows][4];
#pragma unroll
        for (int k = 0; k < kPeRows; ++k)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[k][c] = 0.f;
        while (t < end) {
            // the eight taps from t on (behind the end of the list the last one again): uniform addresses, so these are scalar loads
            int at[8];
            float w[8];
            if (t + 8 <= n_taps) {
#pragma unroll
                for (int k = 0; k < 8; ++k) at[k] = a.tap_at[t + k], w[k] = a.tap_w[t + k];
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int q = t + k < n_taps ? t + k : n_taps - 1;
                    at[k] = a.tap_at[q], w[k] = a.tap_w[q];
                }
            }
            const int di = at[0] >> 16, dj = (int)(short)(at[0] & 0xffff);
            if (di > ri || di < -ri || dj > rj || dj < -rj) {       // a tap beyond the reach is skipped
                ++t;
                continue;
            }
            int L = 1;
            bool run = true;
#pragma unroll
            for (int k = 1; k < 8; ++k) {
                run = run && t + k < end && dj - k >= -rj && at[k] == (int)(((unsigned)di << 16) | ((unsigned)(dj - k) & 0xffffu));
                L += run ? 1 : 0;
            }
            const float* p = base + (di + ri) * pitch + (dj + rj);
            if (L == 8) {
                pe_run<8>(p - 7, row_stride, w, acc);
                t += 8;
            } else if (L >= 4) {
                pe_run<4>(p - 3, row_stride, w, acc);
                t += 4;
            } else if (L >= 2) {
                pe_run<2>(p - 1, row_stride, w, acc);
                t += 2;
            } else {
                pe_run<1>(p, row_stride, w, acc);
                t += 1;
            }
        }
#pragma unroll
        for (int k = 0; k < kPeRows; ++k)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float v = acc[k][c];
                if (f == 0 || v > best[k][c] || v != v) best[k][c] = v;        // np.maximum: a NaN wins and stays
            }
    }
#pragma unroll
    for (int k = 0; k < kPeRows; ++k) {
        const int gi = i0 + row0 + 8 * k;
        if (gi >= a.n) continue;
        float* o = a.out.row(blockIdx.z, gi) + j0 + col0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float v = best[k][c];
            if (a.clip && v < 0.f) v = 0.f;
            if (j0 + col0 + c < a.m) o[c] = v;
        }
    }
}

struct LagArgs {
    Plane<const float> in;
    Plane<float> out;
    int L, in_rows, in_cols, out_rows, out_cols;
};

template <bool INVERSE>
__global__ __launch_bounds__(JSGX_LAG_THREADS) void lag_columns_kernel(LagArgs a) {
    constexpr int T = JSGX_LAG_TILE;
    __shared__ float piece[(2 * T - 1) * T];
    const int lc = threadIdx.x & (T - 1), lr = threadIdx.x >> 6;
    const int r0 = blockIdx.y * T, j0 = blockIdx.x * T;
    const long long first = INVERSE ? (long long)r0 - j0 - (T - 1) : (long long)r0 + j0;        // the source row of piece 0, before the modulus
    const int j = j0 + lc;
    const float* in = a.in.row(blockIdx.z, 0);
    for (int q = lr; q < 2 * T - 1; q += JSGX_LAG_THREADS / T) {
        long long src = (first + q) % a.L;
        src = src < 0 ? src + a.L : src;
        piece[q * T + lc] = src < a.in_rows && j < a.in_cols ? in[src * a.in.pitch + j] : 0.f;
    }
    __syncthreads();
    if (j >= a.out_cols) return;
    for (int r = lr; r < T && r0 + r < a.out_rows; r += JSGX_LAG_THREADS / T) {
        const int q = INVERSE ? r - lc + (T - 1) : r + lc;
        a.out.row(blockIdx.z, r0 + r)[j] = piece[q * T + lc];
    }
}

constexpr int kLagRowChunk = 4 * JSGX_LAG_THREADS;          // the elements of a row that a workgroup moves

template <bool INVERSE>
__global__ __launch_bounds__(JSGX_LAG_THREADS) void lag_rows_kernel(LagArgs a, int chunks) {
    const int i = blockIdx.x / chunks, chunk = blockIdx.x - i * chunks;
    const float* in = a.in.row(blockIdx.y, i);
    float* out = a.out.row(blockIdx.y, i);
    const int shift = i % a.L;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = chunk * kLagRowChunk + u * JSGX_LAG_THREADS + threadIdx.x;
        if (c >= a.out_cols) continue;
        int src = INVERSE ? c - shift : c + shift;          // c < L and shift < L: one correction
        src = src < 0 ? src + a.L : (src >= a.L ? src - a.L : src);
        out[c] = src < a.in_cols ? in[src] : 0.f;
    }
}

static jsg::OncePerDevice g_pe_once;

}  // namespace jsgx

using namespace jsgx;

extern "C" int jsgx_path_enhance_launch(const jsgx_path_enhance_args* g, void* stream) {
    static const char* who = "jsgx_path_enhance_launch";
    int rc = path_enhance_check(g, who);
    if (rc != JSGX_OK) return rc;
    int dev = -1;
    if ((rc = current_device(&dev, who)) != JSGX_OK) return rc;
    // every refusal is behind us
    PeArgs k{};
    k.r = plane_of(g->r, g->r_pitch, g->r_pair_pitch, g->pairs);
    k.out = plane_of(g->out, g->out_pitch, g->out_pair_pitch, g->pairs);
    k.tap_w = g->tap_w, k.tap_at = g->tap_at, k.first = g->filter_first;
    k.n = g->n, k.m = g->m, k.n_filters = g->n_filters, k.n_taps = g->n_taps, k.reach_i = g->reach_i, k.reach_j = g->reach_j, k.clip = g->clip;
    k.pitch = pe_window_pitch(g->reach_j);
    const dim3 grid((unsigned)((g->m + kPeTile - 1) / kPeTile), (unsigned)((g->n + kPeTile - 1) / kPeTile), (unsigned)g->pairs);
    const hipError_t err = jsg::launch_large_lds(g_pe_once, dev, 1u, path_enhance_kernel, JSGX_PE_LDS_LIMIT, grid, dim3(kPeThreads),
                                                 (size_t)pe_lds_bytes(g->reach_i, g->reach_j), reinterpret_cast<hipStream_t>(stream), k);
    return finish_launch(who, err);
}

extern "C" int jsgx_lag_launch(const jsgx_lag_args* g, void* stream) {
    static const char* who = "jsgx_lag_launch";
    int rc = lag_check(g, who);
    if (rc != JSGX_OK) return rc;
    int dev = -1;
    if ((rc = current_device(&dev, who)) != JSGX_OK) return rc;
    // every refusal is behind us
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const LagShape shape = lag_shape(g->n, g->pad, g->axis, g->inverse);
    LagArgs k{};
    k.in = plane_of(g->in, g->in_pitch, g->in_pair_pitch, g->pairs);
    k.out = plane_of(g->out, g->out_pitch, g->out_pair_pitch, g->pairs);
    k.L = shape.L, k.in_rows = shape.in_rows, k.in_cols = shape.in_cols, k.out_rows = shape.out_rows, k.out_cols = shape.out_cols;
    if (g->axis == 1) {
        const dim3 grid((unsigned)((shape.out_cols + JSGX_LAG_TILE - 1) / JSGX_LAG_TILE), (unsigned)((shape.out_rows + JSGX_LAG_TILE - 1) / JSGX_LAG_TILE), (unsigned)g->pairs);
        if (g->inverse)
            hipLaunchKernelGGL(lag_columns_kernel<true>, grid, dim3(JSGX_LAG_THREADS), 0, s, k);
        else
            hipLaunchKernelGGL(lag_columns_kernel<false>, grid, dim3(JSGX_LAG_THREADS), 0, s, k);
    } else {
        const int chunks = (shape.out_cols + kLagRowChunk - 1) / kLagRowChunk;
        const dim3 grid((unsigned)shape.out_rows * (unsigned)chunks, (unsigned)g->pairs);
        if (g->inverse)
            hipLaunchKernelGGL(lag_rows_kernel<true>, grid, dim3(JSGX_LAG_THREADS), 0, s, k, chunks);
        else
            hipLaunchKernelGGL(lag_rows_kernel<false>, grid, dim3(JSGX_LAG_THREADS), 0, s, k, chunks);
    }
    return finish_launch(who, hipGetLastError());
}
