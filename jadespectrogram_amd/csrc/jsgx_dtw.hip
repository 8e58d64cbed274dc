// libjsgx.so, dynamic time warping over a cost plane (include/jsgx.h section 3): the two kernels and their launcher.  The refusals, the
// scratch size and the plan are in jsgx_dtw_host.cpp.
//
// dtw_kernel.  D is cut into tiles of 64 x 64; the launcher enqueues one launch per tile anti-diagonal over pairs x (tiles on it),
// one wavefront per tile.  A tile depends on the tiles above, left and above-left of it, all on earlier anti-diagonals, so it reads
// its top row, left column and corner from D in global memory and never waits for another workgroup.  Inside the tile the sweep is
// skewed: lane l owns row l and at step s computes column c = s - l.  Its three neighbours are
//     left  (l, c-1)     its own value of the step before
//     up    (l-1, c)     what lane l-1 computed in the step before: one wave shift per step
//     diag  (l-1, c-1)   the `up` of the step before
// and for lane 0 the top row (top[0] is the corner), for column 0 the left column.  The shift is a DPP wave_shr:1 (one v_mov with
// a DPP modifier on the dependent chain, whose old operand hands lane 0 its top-row value; built with -DJSGX_DTW_SHFL it is
// __shfl_up, a ds_bpermute through the LDS pipe, for the comparison that profiles/dtw_bench.md reports).
//   tile[64][64]    C on the way in, D on the way out, in place (a cell's C is read before the step that writes its D); the global
//                   accesses are whole 256-byte lines; lane l reads word l * 64 + s - l: 64 different banks
//   top[65 + 3]     D of the row above the tile, from the corner on; +inf outside the matrix
// The tile is as wide as it is high because the chain of dependent steps decides the time: a tile takes cols + 63 steps and the tiles
// of one tile row follow each other, so N x M costs about (N / 64 + M / cols) (cols + 63) steps, least near cols = 64 (measured:
// profiles/dtw_bench.md).
// A tile wholly outside the band is filled with +inf and C is not read.
//
// dtw_backtrace_kernel.  One wavefront per pair.  The walk is serial, so the wavefront fetches the 32 x 32 window of D and C whose
// last cell is the current one (one round trip to memory, 16 loads of each per lane), lane 0 walks inside it while the three predecessors
// are in the window (at least 31 steps), and the window is fetched again around the cell the walk stands on.  The path is written backwards
// into the scratch and copied out reversed by all lanes.
#include <hip/hip_runtime.h>

#include <climits>

#include "jsgx_internal.h"

namespace jsgx {

constexpr int kRows = JSGX_DTW_TILE_ROWS, kCols = JSGX_DTW_TILE_COLS, kLanes = JSGX_DTW_THREADS;
constexpr int kTop = kCols + 4;
static_assert(kRows == kLanes && kLanes == 64, "lane l owns row l of a tile: one wavefront");
static_assert(kCols % 64 == 0, "a row pitch that is a multiple of 64 words keeps the skewed reads on 64 banks");
static_assert((kRows * kCols + kTop) * 4 == JSGX_DTW_LDS_BYTES, "include/jsgx.h states the LDS");

struct DtwArgs {
    Plane<const float> cost;
    Plane<float> acc;
    int n, m, subseq, band;
    float wm0, wm1, wm2, wa0, wa1, wa2;
    int diagonal, ti_first;         // this launch: the tiles (ti_first + blockIdx.x, diagonal - ti)
};

struct BacktraceArgs {
    Plane<const float> cost, acc;
    int n, m, subseq;
    float wm0, wm1, wm2, wa0, wa1, wa2;
    int* path_i;
    int* path_j;
    long long path_pitch;
    int* path_len;
    float* total;
    int* scratch;                   // [pairs][2][n + m - 1], or null without paths
};

// the value of lane l - 1; lane 0 receives `lane0` (it has no source lane: the DPP move leaves its old value)
__device__ __forceinline__ float from_lane_below(float v, float lane0) {
#if defined(JSGX_DTW_SHFL)
    const float shifted = __shfl_up(v, 1);
    return threadIdx.x == 0 ? lane0 : shifted;
#else
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(lane0), __float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
#endif
}

// D of a cell that is not an initial one, from its cost and its three predecessors (include/jsgx.h, "Recurrence"); *k: the step taken
__device__ __forceinline__ float dtw_cell(float c, float diag, float left, float up, float wm0, float wm1, float wm2, float wa0, float wa1, float wa2, int* k) {
#pragma clang fp contract(off)
    const float e0 = wm0 * c + wa0, e1 = wm1 * c + wa1, e2 = wm2 * c + wa2;
    const float v0 = diag + e0, v1 = left + e1, v2 = up + e2;
    float best = v0;
    int step = 0;
    if (v1 < best) {
        best = v1;
        step = 1;
    }
    if (v2 < best) {
        best = v2;
        step = 2;
    }
    *k = step;
    return best;
}

// The skewed sweep of one tile.  What a step needs from LDS (the cell's cost, lane 0's value of the top row) is read two steps ahead, so
// that only arithmetic is on the chain from one step's D to the next: the lane move, three additions, two compare-and-selects and the
// selects of the edge rules.
template <bool BANDED, bool TOP>         // TOP: the tile holds row 0 of the matrix, whose cells are initial ones (all of them with subseq)
__device__ __forceinline__ void dtw_sweep(float* tile, const float* top, const DtwArgs& a, int l, int i0, int j0, int rows, int cols, float left_edge, float diag_edge,
                                          long long n1, long long m1, long long lim) {
#pragma clang fp contract(off)
    const float inf = __builtin_inff();
    float* row = tile + l * kCols;
    const bool first_row = TOP && l == 0;
    long long band_value = (long long)(j0 - l) * n1 - (long long)(i0 + l) * m1;      // j (N-1) - i (M-1) at step 0
    const int steps = cols + rows - 1;
    // column s - l of the lane's row and entry s + 1 of the top row, both kept inside the arrays (a step outside the tile computes nothing that is used)
#define JSGX_COL(s) ((s) - l < 0 ? 0 : ((s) - l >= kCols ? kCols - 1 : (s) - l))
#define JSGX_TOP(s) (((s) >= kCols ? kCols - 1 : (s)) + 1)
    float cost0 = row[JSGX_COL(0)], cost1 = row[JSGX_COL(1)];
    float top0 = top[JSGX_TOP(0)], top1 = top[JSGX_TOP(1)];
    float last = 0.f, up_before = 0.f;
    const bool row_inside = l < rows;
    for (int s = 0; s < steps; ++s) {
        const float cost2 = row[JSGX_COL(s + 2)], top2 = top[JSGX_TOP(s + 2)];
        const int c = s - l;
        const float up = from_lane_below(last, top0);                               // (l-1, c): lane l-1's value of the step before; lane 0: the top row
        const float diag = c == 0 ? diag_edge : up_before;                          // (l-1, c-1): the `up` of the step before (lane 0: the top row again)
        const float left = c == 0 ? left_edge : last;                               // (l, c-1)
        int k;
        float d = dtw_cell(cost0, diag, left, up, a.wm0, a.wm1, a.wm2, a.wa0, a.wa1, a.wa2, &k);
        if (BANDED) {
            if (band_value > lim || band_value < -lim) d = inf;
            band_value += n1;
        }
        if (TOP && first_row && (a.subseq || j0 + c == 0)) d = cost0;
        if (row_inside && (unsigned)c < (unsigned)cols) row[c] = d;
        last = d;
        up_before = up;
        cost0 = cost1, cost1 = cost2, top0 = top1, top1 = top2;
    }
#undef JSGX_COL
#undef JSGX_TOP
}

__global__ __launch_bounds__(kLanes) void dtw_kernel(DtwArgs a) {
    __shared__ float tile[kRows * kCols];
    __shared__ float top[kTop];
    const int l = threadIdx.x;
    const int ti = a.ti_first + blockIdx.x, tj = a.diagonal - ti;
    const int i0 = ti * kRows, j0 = tj * kCols;
    const int rows = a.n - i0 < kRows ? a.n - i0 : kRows, cols = a.m - j0 < kCols ? a.m - j0 : kCols;
    const float inf = __builtin_inff();
    const float* C = a.cost.row(blockIdx.y, i0) + j0;
    float* Dp = a.acc.row(blockIdx.y, 0);                          // the pair's plane
    float* D = a.acc.row(blockIdx.y, i0) + j0;                     // the tile
    const long long n1 = a.n - 1, m1 = a.m - 1, lim = (long long)a.band * (n1 > 1 ? n1 : 1);
    const bool banded = a.band != 0;
    if (banded) {
        // j (N-1) - i (M-1) is largest at the tile's top right cell and smallest at its bottom left one
        const long long hi = (long long)(j0 + cols - 1) * n1 - (long long)i0 * m1, lo = (long long)j0 * n1 - (long long)(i0 + rows - 1) * m1;
        if (lo > lim || hi < -lim) {
            for (int r = 0; r < rows; ++r)
                for (int c = l; c < cols; c += kLanes) D[(long long)r * a.acc.pitch + c] = inf;
            return;
        }
    }
    // every load below is issued without a branch, from an address kept inside the matrix, and what lies outside is replaced afterwards:
    // the loads of a batch are in flight together.  Tile cells outside the matrix hold copies of cells inside; no step that is used reads them.
    const long long ap = a.acc.pitch;
    const int row_above = i0 > 0 ? i0 - 1 : 0, col_before = j0 > 0 ? j0 - 1 : 0;
    const float corner_value = Dp[row_above * ap + col_before];
    const float left_value = D[(long long)(l < rows ? l : rows - 1) * ap + (col_before - j0)];
#pragma unroll
    for (int c0 = 0; c0 < kCols; c0 += kLanes) {
        const int c = c0 + l < cols ? c0 + l : cols - 1;
        const float top_value = Dp[row_above * ap + j0 + c];
#pragma unroll
        for (int r0 = 0; r0 < kRows; r0 += 16) {
            float v[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) v[q] = C[(long long)(r0 + q < rows ? r0 + q : rows - 1) * a.cost.pitch + c];
#pragma unroll
            for (int q = 0; q < 16; ++q) tile[(r0 + q) * kCols + c0 + l] = v[q];
        }
        top[1 + c0 + l] = (i0 > 0 && c0 + l < cols) ? top_value : inf;
    }
    if (l == 0) top[0] = (i0 > 0 && j0 > 0) ? corner_value : inf;
    const float left_edge = (j0 > 0 && l < rows) ? left_value : inf;
    __syncthreads();
    const float diag_edge = from_lane_below(left_edge, top[0]);    // (l-1, -1); lane 0: the corner
    if (banded && i0 == 0)
        dtw_sweep<true, true>(tile, top, a, l, i0, j0, rows, cols, left_edge, diag_edge, n1, m1, lim);
    else if (banded)
        dtw_sweep<true, false>(tile, top, a, l, i0, j0, rows, cols, left_edge, diag_edge, n1, m1, lim);
    else if (i0 == 0)
        dtw_sweep<false, true>(tile, top, a, l, i0, j0, rows, cols, left_edge, diag_edge, n1, m1, lim);
    else
        dtw_sweep<false, false>(tile, top, a, l, i0, j0, rows, cols, left_edge, diag_edge, n1, m1, lim);
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < rows; ++r)
        for (int c = l; c < cols; c += kLanes) D[(long long)r * a.acc.pitch + c] = tile[r * kCols + c];
}

constexpr int kWin = 32;                  // the window of the backtrace: kWin x kWin cells of D and of C, 16 loads of each per lane

__global__ __launch_bounds__(kLanes) void dtw_backtrace_kernel(BacktraceArgs a) {
#pragma clang fp contract(off)
    __shared__ float wd[kWin * kWin], wc[kWin * kWin], red_v[kLanes];
    __shared__ int red_j[kLanes], red_nan[kLanes];
    __shared__ int state[4];            // i, j, the cells recorded, 0 walking / 1 at the start / -1 no path
    const int l = threadIdx.x, p = blockIdx.x;
    const float inf = __builtin_inff();
    const float* C = a.cost.row(p, 0);
    const float* D = a.acc.row(p, 0);
    const int longest = a.n + a.m - 1;
    int* rev_i = a.scratch ? a.scratch + (long long)p * 2 * longest : nullptr;
    int* rev_j = rev_i ? rev_i + longest : nullptr;
    // ---- the end cell
    int end_j = a.m - 1, no_path = 0;
    if (a.subseq) {
        const float* last_row = D + (long long)(a.n - 1) * a.acc.pitch;
        float best = inf;
        int best_j = INT_MAX, nan = 0;
        for (int j = l; j < a.m; j += kLanes) {             // j ascends: a strict comparison keeps the lowest
            const float v = last_row[j];
            nan |= v != v;
            if (best_j == INT_MAX || v < best) {
                best = v;
                best_j = j;
            }
        }
        red_v[l] = best;
        red_j[l] = best_j;
        red_nan[l] = nan;
        __syncthreads();
        if (l == 0) {
            for (int q = 0; q < kLanes; ++q) {
                nan |= red_nan[q];
                if (red_j[q] != INT_MAX && (red_v[q] < best || (red_v[q] == best && red_j[q] < best_j))) {
                    best = red_v[q];
                    best_j = red_j[q];
                }
            }
            state[0] = best_j;
            state[1] = nan;
        }
        __syncthreads();
        end_j = state[0];
        no_path = state[1];
        __syncthreads();
    }
    if (l == 0) {
        state[0] = a.n - 1;
        state[1] = end_j;
        state[2] = 0;
        state[3] = no_path ? -1 : 0;
    }
    // ---- the walk, window by window
    for (;;) {
        __syncthreads();
        const int i = state[0], j = state[1], status = state[3];
        if (status != 0) break;
#pragma unroll
        for (int u = 0; u < kWin * kWin / kLanes; ++u) {    // unconditional loads from addresses kept inside the matrix: all in flight together
            const int q = u * kLanes + l;
            const int gi = i - (kWin - 1) + q / kWin, gj = j - (kWin - 1) + q % kWin;
            const bool in = gi >= 0 && gj >= 0;             // gi <= i < n and gj <= j < m
            const long long ri = gi < 0 ? 0 : gi, rj = gj < 0 ? 0 : gj;
            const float dv = D[ri * a.acc.pitch + rj], cv = C[ri * a.cost.pitch + rj];
            wd[q] = in ? dv : inf;
            wc[q] = cv;
        }
        __syncthreads();
        if (l == 0) {
            int r = kWin - 1, c = kWin - 1, ci = i, cj = j, count = state[2], st = 0;
            while (r > 0 && c > 0) {
                // the cell, its cost and its three predecessors in one batch of LDS reads, ahead of the checks
                const float d = wd[r * kWin + c], cost = wc[r * kWin + c];
                const float diag = wd[(r - 1) * kWin + c - 1], left = wd[r * kWin + c - 1], up = wd[(r - 1) * kWin + c];
                int k;
                dtw_cell(cost, diag, left, up, a.wm0, a.wm1, a.wm2, a.wa0, a.wa1, a.wa2, &k);
                if (d != d || d == inf || count >= longest) {
                    st = -1;
                    break;
                }
                if (rev_i) {
                    rev_i[count] = ci;
                    rev_j[count] = cj;
                }
                ++count;
                if (ci == 0 && (a.subseq || cj == 0)) {
                    st = 1;
                    break;
                }
                const int di = k != 1, dj = k != 2;
                ci -= di, r -= di, cj -= dj, c -= dj;
                if (ci < 0 || cj < 0) {                     // a predecessor outside the matrix is +inf and never the best of a finite cell
                    st = -1;
                    break;
                }
            }
            state[0] = ci;
            state[1] = cj;
            state[2] = count;
            state[3] = st;
        }
    }
    const int L = state[2];
    if (state[3] < 0) {
        if (l == 0 && a.path_len) a.path_len[p] = -1;
        return;
    }
    if (a.path_i) {
        int* out_i = a.path_i + p * a.path_pitch;
        int* out_j = a.path_j + p * a.path_pitch;
        for (int q = l; q < L; q += kLanes) {
            out_i[q] = rev_i[L - 1 - q];
            out_j[q] = rev_j[L - 1 - q];
        }
    }
    if (l == 0) {
        if (a.path_len) a.path_len[p] = L;
        if (a.total) a.total[p] = D[(long long)(a.n - 1) * a.acc.pitch + end_j];
    }
}

}  // namespace jsgx

using namespace jsgx;

extern "C" int jsgx_dtw_launch(const jsgx_dtw_args* g, void* scratch, int64_t scratch_bytes, void* stream) {
    static const char* who = "jsgx_dtw_launch";
    int rc = dtw_check(g, who);
    if (rc != JSGX_OK) return rc;
    const int64_t need = dtw_scratch_bytes(g);
    if (need > 0 && (rc = check_scratch(who, scratch, scratch_bytes, need, "jsgx_dtw_scratch_bytes")) != JSGX_OK) return rc;
    int dev = -1;
    if ((rc = current_device(&dev, who)) != JSGX_OK) return rc;
    // every refusal is behind us
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    DtwArgs k{};
    k.cost = plane_of(g->cost, g->cost_pitch, g->cost_pair_pitch, g->pairs);
    k.acc = plane_of(g->acc, g->acc_pitch, g->acc_pair_pitch, g->pairs);
    k.n = g->n;
    k.m = g->m;
    k.subseq = g->subseq;
    k.band = g->band;
    k.wm0 = g->weights_mul[0], k.wm1 = g->weights_mul[1], k.wm2 = g->weights_mul[2];
    k.wa0 = g->weights_add[0], k.wa1 = g->weights_add[1], k.wa2 = g->weights_add[2];
    const DtwTiles tiles = dtw_tiles(g->n, g->m);
    for (int d = 0; d < tiles.diagonals(); ++d) {
        const int first = d - (tiles.j - 1) > 0 ? d - (tiles.j - 1) : 0, last = d < tiles.i - 1 ? d : tiles.i - 1;
        k.diagonal = d;
        k.ti_first = first;
        hipLaunchKernelGGL(dtw_kernel, dim3((unsigned)(last - first + 1), (unsigned)g->pairs), dim3(kLanes), 0, s, k);
    }
    if (g->path_len || g->total) {
        BacktraceArgs b{};
        b.cost = k.cost;
        b.acc = plane_of<const float>(g->acc, g->acc_pitch, g->acc_pair_pitch, g->pairs);
        b.n = g->n, b.m = g->m, b.subseq = g->subseq;
        b.wm0 = k.wm0, b.wm1 = k.wm1, b.wm2 = k.wm2, b.wa0 = k.wa0, b.wa1 = k.wa1, b.wa2 = k.wa2;
        b.path_i = g->path_i;
        b.path_j = g->path_j;
        b.path_pitch = g->pairs > 1 ? g->path_pitch : 0;
        b.path_len = g->path_len;
        b.total = g->total;
        b.scratch = need > 0 ? static_cast<int*>(scratch) : nullptr;
        hipLaunchKernelGGL(dtw_backtrace_kernel, dim3((unsigned)g->pairs), dim3(kLanes), 0, s, b);
    }
    return finish_launch(who, hipGetLastError());
}
