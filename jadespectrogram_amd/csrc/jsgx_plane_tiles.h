// libjsgx.so, what the two plane recurrences share on the device: dynamic time warping (jsgx_dtw.hip, include/jsgx.h section 3) and recurrence
// quantification alignment (jsgx_rqa.hip, section 9).  Each unit keeps its cell rule, its sweep, its halos and its end cell.
//
// Forward.  The n x m plane is cut into tiles of 64 x 64 (dtw_tiles(), jsgx_internal.h).  A cell depends on earlier rows and columns only, so
// a tile depends on the tiles above, left and above-left of it, all on earlier tile anti-diagonals: enqueue_diagonals() enqueues one launch
// per anti-diagonal over pairs x (tiles on it), one wavefront per tile, and a tile reads its halo from the plane in global memory and never
// waits for another workgroup.  The tile lives in LDS, input on the way in and output on the way out, in place (stage_tile(), store_tile());
// the global accesses are whole 256-byte lines.  Values travel up the lanes by from_lane_below().
//
// Backtrace.  One wavefront per pair.  The walk is serial, so the wavefront fetches the 32 x 32 window of each plane whose last cell is the
// current one (fetch_window(): one round trip to memory, 16 loads per lane and plane), lane 0 walks inside it while the predecessors of its
// cell are in the window, and the window is fetched again around the cell the walk stands on.  PathOut takes the path: backwards into the
// scratch, then copied out reversed by all lanes.
#pragma once

#include "jsgx_internal.h"

namespace jsgx {

constexpr int kRows = JSGX_DTW_TILE_ROWS, kCols = JSGX_DTW_TILE_COLS, kLanes = JSGX_DTW_THREADS, kWin = JSGX_RQA_WINDOW;
static_assert(kLanes == 64 && JSGX_RQA_THREADS == kLanes, "a tile is one wavefront");
static_assert(kRows == kLanes && kCols == kLanes, "a lane owns a row or a column of a tile; a row pitch of 64 words keeps a skewed read on 64 banks");
static_assert(kRows % 16 == 0 && kWin * kWin % kLanes == 0, "whole batches of loads");

// the value of lane l - 1; lane 0 receives `lane0` (it has no source lane: the DPP move leaves its old value).  A DPP wave_shr:1, one v_mov
// with a DPP modifier on the dependent chain; built with -DJSGX_DTW_SHFL it is __shfl_up, a ds_bpermute through the LDS pipe, for the
// comparison that profiles/dtw_bench.md reports.
__device__ __forceinline__ float from_lane_below(float v, float lane0) {
#if defined(JSGX_DTW_SHFL)
    const float shifted = __shfl_up(v, 1);
    return threadIdx.x == 0 ? lane0 : shifted;
#else
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(lane0), __float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
#endif
}

// The tile of a workgroup: its place among the tiles, its first cell and what of it lies inside the matrix.
struct TilePlace {
    int ti, tj, i0, j0, rows, cols;
};
// One launch: the tiles (ti_first + blockIdx.x, diagonal - ti).  The member `at` of a forward kernel's arguments (dtw_kernel spells place() out).
struct TileDiagonal {
    int diagonal, ti_first;
    __device__ __forceinline__ TilePlace place(int n, int m) const {
        const int ti = ti_first + blockIdx.x, tj = diagonal - ti, i0 = ti * kRows, j0 = tj * kCols;
        return {ti, tj, i0, j0, n - i0 < kRows ? n - i0 : kRows, m - j0 < kCols ? m - j0 : kCols};
    }
};
template <class Args>
void enqueue_diagonals(void (*kernel)(Args), Args k, const DtwTiles& tiles, int pairs, hipStream_t s) {
    for (int d = 0; d < tiles.diagonals(); ++d) {
        const TileRange on = tiles_on_diagonal(tiles, d);
        k.at = {d, on.first};
        hipLaunchKernelGGL(kernel, dim3((unsigned)(on.last - on.first + 1), (unsigned)pairs), dim3(kLanes), 0, s, k);
    }
}

// The tile whose first cell is src[0] into LDS, lane l its column l, in batches of 16 rows.  Every load is issued without a branch, from an
// address kept inside the matrix, so the loads of a batch are in flight together; a tile cell outside the matrix holds a copy of a cell
// inside and no step that is used reads it.  store_tile(): what lies inside the matrix, back to dst[0] and on.
__device__ __forceinline__ void stage_tile(float* tile, const float* src, long long pitch, int rows, int cols, int l) {
    const int c = l < cols ? l : cols - 1;
#pragma unroll
    for (int r0 = 0; r0 < kRows; r0 += 16) {
        float v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = src[(long long)(r0 + q < rows ? r0 + q : rows - 1) * pitch + c];
#pragma unroll
        for (int q = 0; q < 16; ++q) tile[(r0 + q) * kCols + l] = v[q];
    }
}
__device__ __forceinline__ void store_tile(float* dst, long long pitch, const float* tile, int rows, int cols, int l) {
    if (l >= cols) return;
#pragma unroll 8
    for (int r = 0; r < rows; ++r) dst[(long long)r * pitch + l] = tile[r * kCols + l];
}

// The kWin x kWin window of a pair's plane whose last cell is (i, j) into LDS: unconditional loads from addresses kept inside the matrix,
// all in flight together.  A cell outside the matrix is a copy of a cell inside, or +inf with OUTSIDE_INF.
template <bool OUTSIDE_INF>
__device__ __forceinline__ void fetch_window(float* lds, const float* plane, long long pitch, int i, int j, int l) {
#pragma unroll
    for (int u = 0; u < kWin * kWin / kLanes; ++u) {
        const int q = u * kLanes + l;
        const int gi = i - (kWin - 1) + q / kWin, gj = j - (kWin - 1) + q % kWin;       // gi <= i < n and gj <= j < m
        const float v = plane[(long long)(gi < 0 ? 0 : gi) * pitch + (gj < 0 ? 0 : gj)];
        lds[q] = OUTSIDE_INF && (gi < 0 || gj < 0) ? __builtin_inff() : v;
    }
}

// What a walk hands from one window to the next, in LDS: the cell it stands on, the cells recorded, and its status (0: walking).
__device__ __forceinline__ void set_walk(int* state, int i, int j, int count, int status) { state[0] = i, state[1] = j, state[2] = count, state[3] = status; }

// Where a backtrace leaves its path: the caller's outputs and the scratch [pairs][2][longest] that takes the path backwards, null without
// paths.  path_out() fills it from either argument block: one pair has no path pitch, whatever the field holds.
struct PathOut {
    int* path_i;
    int* path_j;
    long long path_pitch;
    int* path_len;
    int* scratch;
    int longest;
    __device__ __forceinline__ int* reversed(int pair) const { return scratch ? scratch + (long long)pair * 2 * longest : nullptr; }
    // cell number `count` of the walk, by the walking lane
    __device__ __forceinline__ void record(int* rev, int count, int i, int j) const {
        if (!rev) return;
        rev[count] = i;
        rev[longest + count] = j;
    }
    // the L cells recorded, first cell first, by all lanes
    __device__ __forceinline__ void copy_out(const int* rev, int pair, int L, int l) const {
        if (!path_i) return;
        for (int q = l; q < L; q += kLanes) {
            path_i[pair * path_pitch + q] = rev[L - 1 - q];
            path_j[pair * path_pitch + q] = rev[longest + L - 1 - q];
        }
    }
};
template <class Args>
PathOut path_out(const Args* g, void* scratch, int longest) {
    return {g->path_i, g->path_j, g->pairs > 1 ? g->path_pitch : 0, g->path_len, g->path_i ? static_cast<int*>(scratch) : nullptr, longest};
}

}  // namespace jsgx
