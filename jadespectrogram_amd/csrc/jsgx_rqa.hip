// libjsgx.so, recurrence quantification alignment over a similarity plane (include/jsgx.h section 9): the two kernels and their launcher.
// The refusals, the scratch size and the plan are in jsgx_rqa_host.cpp; the tiles, their launches, the staging, the lane move and the
// backtrace's window and path output are jsgx_plane_tiles.h, shared with jsgx_dtw.hip.
//
// rqa_kernel.  The three predecessors of a cell, (i-1, j-1), (i-1, j-2) and (i-2, j-1), lie in an earlier row and an earlier column, so a
// tile reads from S in global memory the two rows above it, the two columns left of it and the corner between them, with the same cells
// of R.  Inside the tile the cells of a row are independent: lane l owns column l and the rows are walked top to bottom.  At row i the
// lane holds S(i-1, j) of its own column; its predecessors are
//     a  (i-1, j-1)   the row above moved up one lane: one lane move, which hands lane 0 the left halo
//     b  (i-1, j-2)   a moved once more (lane 0: the second halo column)
//     c  (i-2, j-1)   the a of the step before
// and what a gap from each of them costs (gap_onset from a link, gap_extend else) travels beside them the same way, so the flags of the
// predecessors cost three more register moves and no memory access.  A tile takes 64 steps; a step needs the row above, which is the step
// before, so the steps still form a chain: the move, a subtraction, two compare-and-selects, an addition and the selects of the non-link
// rule.
//   tile[64][64]    R on the way in, S on the way out; lane l reads word r * 64 + l
//   left[64]        per row of the tile: S of the two halo columns at the row above, and the two penalties, one 16-byte read per step
// Both are read two steps ahead, so that only arithmetic is on the chain, and the sweep is written four rows a round so that what was
// read ahead changes names instead of registers (the compiler does not unroll a loop of wave moves by itself: 16 % at 16384 x 16384,
// profiles/rqa_bench.md).  Lanes right of the matrix compute values that only lanes further
// right read (the moves go up the lanes) and store nothing.  The tiles that hold row 0 or column 0 take the BORDER form of the sweep, with
// the border rule and the candidates' bounds; every other tile has all three candidates at every cell.
// With a backtrace output the tile also keeps its best (S, i, j) -- the largest S > 0, then the lowest i, then the lowest j -- and writes
// it to the scratch, 8 bytes a tile.
//
// rqa_backtrace_kernel.  It reduces the tiles' entries by the same key, which is a total order, so the end cell does not depend on the
// tiling.  The window holds S and R; lane 0 walks inside it while two rows and two columns remain behind the cell (or the matrix ends), at
// least 15 steps.  The step of a cell is recomputed by rqa_cell, the forward kernel's own routine.
#include <hip/hip_runtime.h>

#include "jsgx_plane_tiles.h"

namespace jsgx {

static_assert((kRows * kCols + 4 * kRows) * 4 == JSGX_RQA_LDS_BYTES, "include/jsgx.h states the LDS");
static_assert(JSGX_DTW_MAX_LEN <= 65536, "the key of a cell is i * 65536 + j in 32 bits");

struct RqaTileArgs {
    Plane<const float> sim;
    Plane<float> score;
    Plane<signed char> step;        // p null without a step plane
    uint2* best;                    // [pairs][tiles]: the bits of S and i * 65536 + j; null without a backtrace output
    int n, m, tiles, tiles_j;       // tiles: of one pair
    float onset, extend;
    TileDiagonal at;
};

struct RqaBacktraceArgs {
    Plane<const float> sim, score;
    const uint2* best;
    int n, m, tiles;
    float onset, extend;
    PathOut out;                    // longest: min(n, m)
    int* end;
    float* total;
};

// S of a cell off the border from its R, S of its predecessors a (k = 0), b (k = 1), c (k = 2) and what a gap from each costs
// (include/jsgx.h, "Every other cell"); has1, has2: k = 1 and k = 2 are candidates; *k: the step
template <bool KNIGHT>
__device__ __forceinline__ float rqa_cell(float r, float a, float b, float c, float pa, float pb, float pc, bool has1, bool has2, int* k) {
#pragma clang fp contract(off)
    const bool link = r > 0.f;
    float best = link ? a : a - pa;
    int step = 0;
    if (KNIGHT) {
        const float v1 = link ? b : b - pb, v2 = link ? c : c - pc;
        if (has1 && v1 > best) {
            best = v1;
            step = 1;
        }
        if (has2 && v2 > best) {
            best = v2;
            step = 2;
        }
    }
    const bool keep = link || best > 0.f;
    *k = keep ? step : -1;
    return link ? best + r : (keep ? best : 0.f);
}

// The rows of one tile, top to bottom.  s1, p1: S of the row above the tile in the lane's column and the penalty of a gap from it;
// c, pc: S(i0 - 2, j - 1) and its penalty.  *best_s, *best_r: the largest S > 0 of the lane's column and the first tile row that has it.
template <bool KNIGHT, bool STEP, bool BORDER>
__device__ __forceinline__ void rqa_sweep(float* tile, const float4* left, const RqaTileArgs& a, int l, int i0, int j0, int rows, int cols, float s1, float p1, float c,
                                          float pc, signed char* step_out, float* best_s, int* best_r) {
#pragma clang fp contract(off)
    float* col = tile + l;
    const int j = j0 + l;
    float4 h0 = left[0], h1 = left[1];
    float r0 = col[0], r1 = col[kCols];
    float bs = 0.f;
    int br = 0;
    // four rows a round, unrolled, so that the operands read ahead change names and not registers; a tile whose rows are no multiple of
    // four walks up to three rows of the LDS tile that lie below the matrix and keeps nothing of them
    for (int r4 = 0; r4 < rows; r4 += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = r4 + u;
            const int ahead = r + 2 < kRows ? r + 2 : kRows - 1;
            const float4 h2 = left[ahead];
            const float r2 = col[ahead * kCols];
            const float sa = from_lane_below(s1, h0.x), pa = from_lane_below(p1, h0.z);
            const float sb = KNIGHT ? from_lane_below(sa, h0.y) : 0.f, pb = KNIGHT ? from_lane_below(pa, h0.w) : 0.f;
            const int i = i0 + r;
            int k;
            float s = rqa_cell<KNIGHT>(r0, sa, sb, c, pa, pb, pc, !BORDER || j >= 2, !BORDER || i >= 2, &k);
            if (BORDER && (i == 0 || j == 0)) {
                s = r0;
                k = r0 > 0.f ? -2 : -1;
            }
            col[r * kCols] = s;
            if (STEP) {
                if (l < cols && r < rows) *step_out = (signed char)k;
                step_out += a.step.pitch;
            }
            if (s > bs && r < rows) {       // strict: the first row of the largest; a NaN never
                bs = s;
                br = r;
            }
            c = sa, pc = pa;
            s1 = s, p1 = r0 > 0.f ? a.onset : a.extend;
            h0 = h1, h1 = h2, r0 = r1, r1 = r2;
        }
    }
    *best_s = bs;
    *best_r = br;
}

// the larger of two cells by the key of the end cell: S, then the lower i * 65536 + j
__device__ __forceinline__ void rqa_keep_better(float* s, unsigned* key, float os, unsigned okey) {
    if (os > *s || (os == *s && okey < *key)) {
        *s = os;
        *key = okey;
    }
}

__device__ __forceinline__ void rqa_reduce_best(float* s, unsigned* key) {
#pragma unroll
    for (int h = kLanes / 2; h > 0; h /= 2) {
        const float os = __shfl_down(*s, h);
        const unsigned okey = (unsigned)__shfl_down((int)*key, h);
        rqa_keep_better(s, key, os, okey);
    }
}

template <bool KNIGHT, bool STEP>
__global__ __launch_bounds__(kLanes) void rqa_kernel(RqaTileArgs a) {
    __shared__ float tile[kRows * kCols];
    __shared__ float4 left[kRows];
    const int l = threadIdx.x;
    const auto [ti, tj, i0, j0, rows, cols] = a.at.place(a.n, a.m);
    const float* Rp = a.sim.row(blockIdx.y, 0);                    // the pair's planes
    const float* Sp = a.score.row(blockIdx.y, 0);
    const float* R = a.sim.row(blockIdx.y, i0) + j0;               // the tile
    float* S = a.score.row(blockIdx.y, i0) + j0;
    // the halo is loaded as the tile is: without a branch, from addresses kept inside the matrix.  A halo cell outside the matrix holds a
    // copy of a cell inside; the BORDER form reads none of them.
    const long long rp = a.sim.pitch, sp = a.score.pitch;
    const long long above1 = i0 > 0 ? i0 - 1 : 0, above2 = i0 > 1 ? i0 - 2 : 0, before1 = j0 > 0 ? j0 - 1 : 0, before2 = j0 > 1 ? j0 - 2 : 0;
    const int lc = l < cols ? l : cols - 1;
    const long long lrow = i0 + l - 1 < 0 ? 0 : (i0 + l - 1 < a.n ? i0 + l - 1 : a.n - 1);
    const float top_s1 = Sp[above1 * sp + j0 + lc], top_s2 = Sp[above2 * sp + j0 + lc], top_r1 = Rp[above1 * rp + j0 + lc], top_r2 = Rp[above2 * rp + j0 + lc];
    const float corner_s = Sp[above2 * sp + before1], corner_r = Rp[above2 * rp + before1];
    const float left_s1 = Sp[lrow * sp + before1], left_s2 = Sp[lrow * sp + before2], left_r1 = Rp[lrow * rp + before1], left_r2 = Rp[lrow * rp + before2];
    stage_tile(tile, R, rp, rows, cols, l);
    const float on = a.onset, ex = a.extend;
    left[l] = make_float4(left_s1, left_s2, left_r1 > 0.f ? on : ex, left_r2 > 0.f ? on : ex);
    __syncthreads();
    const float p1 = top_r1 > 0.f ? on : ex, p2 = top_r2 > 0.f ? on : ex;
    const float c = from_lane_below(top_s2, corner_s), pc = from_lane_below(p2, corner_r > 0.f ? on : ex);          // (i0 - 2, j - 1)
    signed char* step_out = STEP ? a.step.row(blockIdx.y, i0) + j0 + l : nullptr;
    float bs;
    int br;
    if (i0 == 0 || j0 == 0)
        rqa_sweep<KNIGHT, STEP, true>(tile, left, a, l, i0, j0, rows, cols, top_s1, p1, c, pc, step_out, &bs, &br);
    else
        rqa_sweep<KNIGHT, STEP, false>(tile, left, a, l, i0, j0, rows, cols, top_s1, p1, c, pc, step_out, &bs, &br);
    __syncthreads();
    store_tile(S, sp, tile, rows, cols, l);
    if (a.best) {
        unsigned key = ((unsigned)(i0 + br) << 16) | (unsigned)(j0 + l);
        if (!(l < cols && bs > 0.f)) {          // a lane right of the matrix, or a column without S > 0: no cell
            bs = 0.f;
            key = 0xffffffffu;
        }
        rqa_reduce_best(&bs, &key);
        if (l == 0) a.best[(long long)blockIdx.y * a.tiles + (long long)ti * a.tiles_j + tj] = make_uint2(__float_as_uint(bs), key);
    }
}

template <bool KNIGHT>
__global__ __launch_bounds__(kLanes) void rqa_backtrace_kernel(RqaBacktraceArgs a) {
#pragma clang fp contract(off)
    __shared__ float ws[kWin * kWin], wr[kWin * kWin];
    __shared__ int state[4];            // set_walk(); the status: 0 walking / 1 done
    const int l = threadIdx.x, p = blockIdx.x;
    const float* R = a.sim.row(p, 0);
    const float* S = a.score.row(p, 0);
    const int longest = a.out.longest;
    // ---- the end cell: the best of the tiles' best
    float bs = 0.f;
    unsigned key = 0xffffffffu;
    const uint2* entry = a.best + (long long)p * a.tiles;
    for (int q0 = 0; q0 < a.tiles; q0 += 8 * kLanes) {       // eight loads in flight per lane: 256 x 256 tiles are 1024 entries a lane
        uint2 e[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int q = q0 + u * kLanes + l;
            e[u] = entry[q < a.tiles ? q : a.tiles - 1];     // a copy of the last entry changes nothing: the key is a total order
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) rqa_keep_better(&bs, &key, __uint_as_float(e[u].x), e[u].y);
    }
    rqa_reduce_best(&bs, &key);
    bs = __shfl(bs, 0);
    key = (unsigned)__shfl((int)key, 0);
    if (!(bs > 0.f)) {                  // no cell with S > 0: a result
        if (l == 0) {
            if (a.out.path_len) a.out.path_len[p] = 0;
            if (a.total) a.total[p] = 0.f;
            if (a.end) a.end[2 * p] = a.end[2 * p + 1] = -1;
        }
        return;
    }
    const int end_i = (int)(key >> 16), end_j = (int)(key & 0xffffu);
    if (l == 0) {
        if (a.total) a.total[p] = bs;
        if (a.end) a.end[2 * p] = end_i, a.end[2 * p + 1] = end_j;
    }
    if (!a.out.path_len) return;
    int* rev = a.out.reversed(p);
    if (l == 0) set_walk(state, end_i, end_j, 0, 0);
    // ---- the walk, window by window: every round records a cell or ends, and a path has at most `longest` cells
    for (int round = 0; round <= longest; ++round) {
        __syncthreads();
        const int i = state[0], j = state[1];
        if (state[3] != 0) break;
        fetch_window<false>(ws, S, a.score.pitch, i, j, l);
        fetch_window<false>(wr, R, a.sim.pitch, i, j, l);
        __syncthreads();
        if (l == 0) {
            int r = kWin - 1, c = kWin - 1, ci = i, cj = j, count = state[2], st = 0;
            // a cell is decided here while its predecessors are in the window: two rows and two columns behind it, or fewer where the matrix ends
            while (r >= (ci < 2 ? ci : 2) && c >= (cj < 2 ? cj : 2)) {
                const float rv = wr[r * kWin + c];
                int k;
                if (ci == 0 || cj == 0) {
                    k = rv > 0.f ? -2 : -1;
                } else {
                    const bool has1 = KNIGHT && cj >= 2, has2 = KNIGHT && ci >= 2;
                    const int qa = (r - 1) * kWin + c - 1, qb = has1 ? qa - 1 : qa, qc = has2 ? qa - kWin : qa;
                    const float pa = wr[qa] > 0.f ? a.onset : a.extend, pb = wr[qb] > 0.f ? a.onset : a.extend, pc = wr[qc] > 0.f ? a.onset : a.extend;
                    rqa_cell<KNIGHT>(rv, ws[qa], ws[qb], ws[qc], pa, pb, pc, has1, has2, &k);
                }
                if (k == -1 || count >= longest) {          // not part of the path
                    st = 1;
                    break;
                }
                a.out.record(rev, count++, ci, cj);
                if (k == -2) {
                    st = 1;
                    break;
                }
                const int di = k == 2 ? 2 : 1, dj = k == 1 ? 2 : 1;
                ci -= di, r -= di, cj -= dj, c -= dj;
            }
            set_walk(state, ci, cj, count, st);
        }
    }
    __syncthreads();
    const int L = state[2];
    a.out.copy_out(rev, p, L, l);
    if (l == 0) a.out.path_len[p] = L;
}

}  // namespace jsgx

using namespace jsgx;

extern "C" int jsgx_rqa_launch(const jsgx_rqa_args* g, void* scratch, int64_t scratch_bytes, void* stream) {
    static const char* who = "jsgx_rqa_launch";
    int rc = rqa_check(g, who);
    if (rc != JSGX_OK) return rc;
    const RqaScratch need = rqa_scratch(g);
    if (need.bytes > 0 && (rc = check_scratch(who, scratch, scratch_bytes, need.bytes, "jsgx_rqa_scratch_bytes")) != JSGX_OK) return rc;
    int dev = -1;
    if ((rc = current_device(&dev, who)) != JSGX_OK) return rc;
    // every refusal is behind us
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool backtrace = g->path_len || g->end || g->total;
    const DtwTiles tiles = dtw_tiles(g->n, g->m);
    RqaTileArgs k{};
    k.sim = plane_of(g->sim, g->sim_pitch, g->sim_pair_pitch, g->pairs);
    k.score = plane_of(g->score, g->score_pitch, g->score_pair_pitch, g->pairs);
    k.step = plane_of(reinterpret_cast<signed char*>(g->step), g->step_pitch, g->step_pair_pitch, g->pairs);
    k.best = backtrace ? static_cast<uint2*>(scratch) : nullptr;
    k.n = g->n, k.m = g->m, k.tiles = (int)need.tiles, k.tiles_j = tiles.j;
    k.onset = g->gap_onset, k.extend = g->gap_extend;
    void (*const forward[2][2])(RqaTileArgs) = {{rqa_kernel<false, false>, rqa_kernel<false, true>}, {rqa_kernel<true, false>, rqa_kernel<true, true>}};
    enqueue_diagonals(forward[g->knight][g->step != nullptr], k, tiles, g->pairs, s);
    if (backtrace) {
        RqaBacktraceArgs b{};
        b.sim = k.sim;
        b.score = plane_of<const float>(g->score, g->score_pitch, g->score_pair_pitch, g->pairs);
        b.best = k.best;
        b.n = g->n, b.m = g->m, b.tiles = (int)need.tiles;
        b.onset = g->gap_onset, b.extend = g->gap_extend;
        b.out = path_out(g, static_cast<char*>(scratch) + need.off_paths, g->n < g->m ? g->n : g->m);
        b.end = g->end;
        b.total = g->total;
        if (g->knight)
            hipLaunchKernelGGL(rqa_backtrace_kernel<true>, dim3((unsigned)g->pairs), dim3(kLanes), 0, s, b);
        else
            hipLaunchKernelGGL(rqa_backtrace_kernel<false>, dim3((unsigned)g->pairs), dim3(kLanes), 0, s, b);
    }
    return finish_launch(who, hipGetLastError());
}
