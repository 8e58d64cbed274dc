// libjsgx.so, dynamic time warping over a cost plane (include/jsgx.h section 3): the two kernels and their launcher.  The refusals, the
// scratch size and the plan are in jsgx_dtw_host.cpp; the tiles, their launches, the staging, the lane move and the backtrace's window and
// path output are jsgx_plane_tiles.h, shared with jsgx_rqa.hip.
//
// dtw_kernel.  A tile reads its top row, left column and corner from D in global memory.  Inside the tile the sweep is skewed: lane l
// owns row l and at step s computes column c = s - l.  Its three neighbours are
//     left  (l, c-1)     its own value of the step before
//     up    (l-1, c)     what lane l-1 computed in the step before: one lane move per step
//     diag  (l-1, c-1)   the `up` of the step before
// and for lane 0 the top row (top[0] is the corner), for column 0 the left column.
//   tile[64][64]    C on the way in, D on the way out (a cell's C is read before the step that writes its D); lane l reads word
//                   l * 64 + s - l: 64 different banks
//   top[65 + 3]     D of the row above the tile, from the corner on; +inf outside the matrix
// The tile is as wide as it is high because the chain of dependent steps decides the time: a tile takes cols + 63 steps and the tiles
// of one tile row follow each other, so N x M costs about (N / 64 + M / cols) (cols + 63) steps, least near cols = 64 (measured:
// profiles/dtw_bench.md).
// A tile wholly outside the band is filled with +inf and C is not read.
//
// dtw_backtrace_kernel.  The window holds D (+inf outside the matrix) and C; lane 0 walks inside it while the three predecessors are in
// the window (at least 31 steps).
#include <hip/hip_runtime.h>

#include <climits>

#include "jsgx_plane_tiles.h"

namespace jsgx {

constexpr int kTop = kCols + 4;
static_assert((kRows * kCols + kTop) * 4 == JSGX_DTW_LDS_BYTES, "include/jsgx.h states the LDS");

struct DtwArgs {
    Plane<const float> cost;
    Plane<float> acc;
    int n, m, subseq, band;
    float wm0, wm1, wm2, wa0, wa1, wa2;
    TileDiagonal at;
};

struct BacktraceArgs {
    Plane<const float> cost, acc;
    int n, m, subseq;
    float wm0, wm1, wm2, wa0, wa1, wa2;
    PathOut out;                    // longest: n + m - 1
    float* total;
};

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
    // a.at.place(a.n, a.m), spelled out: through the struct the sweep keeps its instructions and gets other registers, and one tile alone
    // takes 19.66 us instead of 19.37 us (profiles/dtw_bench.md)
    const int ti = a.at.ti_first + blockIdx.x, tj = a.at.diagonal - ti;
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
            if (l < cols)
                for (int r = 0; r < rows; ++r) D[(long long)r * a.acc.pitch + l] = inf;
            return;
        }
    }
    // the halo is loaded as the tile is: without a branch, from addresses kept inside the matrix, and what lies outside is replaced afterwards
    const long long ap = a.acc.pitch;
    const int row_above = i0 > 0 ? i0 - 1 : 0, col_before = j0 > 0 ? j0 - 1 : 0;
    const float corner_value = Dp[row_above * ap + col_before];
    const float left_value = D[(long long)(l < rows ? l : rows - 1) * ap + (col_before - j0)];
    const float top_value = Dp[row_above * ap + j0 + (l < cols ? l : cols - 1)];
    stage_tile(tile, C, a.cost.pitch, rows, cols, l);
    top[1 + l] = (i0 > 0 && l < cols) ? top_value : inf;
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
    store_tile(D, a.acc.pitch, tile, rows, cols, l);
}

__global__ __launch_bounds__(kLanes) void dtw_backtrace_kernel(BacktraceArgs a) {
#pragma clang fp contract(off)
    __shared__ float wd[kWin * kWin], wc[kWin * kWin], red_v[kLanes];
    __shared__ int red_j[kLanes], red_nan[kLanes];
    __shared__ int state[4];            // set_walk(); the status: 0 walking / 1 at the start / -1 no path
    const int l = threadIdx.x, p = blockIdx.x;
    const float inf = __builtin_inff();
    const float* C = a.cost.row(p, 0);
    const float* D = a.acc.row(p, 0);
    int* rev = a.out.reversed(p);
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
    if (l == 0) set_walk(state, a.n - 1, end_j, 0, no_path ? -1 : 0);
    // ---- the walk, window by window
    for (;;) {
        __syncthreads();
        const int i = state[0], j = state[1], status = state[3];
        if (status != 0) break;
        fetch_window<true>(wd, D, a.acc.pitch, i, j, l);
        fetch_window<false>(wc, C, a.cost.pitch, i, j, l);
        __syncthreads();
        if (l == 0) {
            int r = kWin - 1, c = kWin - 1, ci = i, cj = j, count = state[2], st = 0;
            while (r > 0 && c > 0) {
                // the cell, its cost and its three predecessors in one batch of LDS reads, ahead of the checks
                const float d = wd[r * kWin + c], cost = wc[r * kWin + c];
                const float diag = wd[(r - 1) * kWin + c - 1], left = wd[r * kWin + c - 1], up = wd[(r - 1) * kWin + c];
                int k;
                dtw_cell(cost, diag, left, up, a.wm0, a.wm1, a.wm2, a.wa0, a.wa1, a.wa2, &k);
                if (d != d || d == inf || count >= a.out.longest) {
                    st = -1;
                    break;
                }
                a.out.record(rev, count++, ci, cj);
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
            set_walk(state, ci, cj, count, st);
        }
    }
    const int L = state[2];
    if (state[3] < 0) {
        if (l == 0 && a.out.path_len) a.out.path_len[p] = -1;
        return;
    }
    a.out.copy_out(rev, p, L, l);
    if (l == 0) {
        if (a.out.path_len) a.out.path_len[p] = L;
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
    enqueue_diagonals(dtw_kernel, k, dtw_tiles(g->n, g->m), g->pairs, s);
    if (g->path_len || g->total) {
        BacktraceArgs b{};
        b.cost = k.cost;
        b.acc = plane_of<const float>(g->acc, g->acc_pitch, g->acc_pair_pitch, g->pairs);
        b.n = g->n, b.m = g->m, b.subseq = g->subseq;
        b.wm0 = k.wm0, b.wm1 = k.wm1, b.wm2 = k.wm2, b.wa0 = k.wa0, b.wa1 = k.wa1, b.wa2 = k.wa2;
        b.out = path_out(g, scratch, g->n + g->m - 1);
        b.total = g->total;
        hipLaunchKernelGGL(dtw_backtrace_kernel, dim3((unsigned)g->pairs), dim3(kLanes), 0, s, b);
    }
    return finish_launch(who, hipGetLastError());
}
