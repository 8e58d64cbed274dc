// libjsgx.so, the pairwise cost and dynamic time warping (include/jsgx.h sections 2 and 3): the refusals, the scratch size and the
// plans, on the host and without a device.  The kernels and their launchers are in jsgx_cdist.hip and jsgx_dtw.hip; the error text
// (jsgx::fail) is in jsgx_beat_host.cpp.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "jsgx_internal.h"

namespace jsgx {

namespace {
typedef __int128 i128;

i128 addr(const void* p) { return (i128)reinterpret_cast<uintptr_t>(p); }
uintptr_t bits_of(const void* p) { return reinterpret_cast<uintptr_t>(p); }
bool overlap(i128 a0, i128 a_bytes, i128 b0, i128 b_bytes) { return a0 && b0 && a0 < b0 + b_bytes && b0 < a0 + a_bytes; }
// the floats of `pairs` planes of rows x cols at these pitches (a pair pitch of 0: one plane)
i128 extent(i128 pairs, i128 pair_pitch, i128 rows, i128 pitch, i128 cols) { return (pairs - 1) * pair_pitch + (rows - 1) * pitch + cols; }
}  // namespace

int cdist_check(const jsgx_cdist_args* g, const char* who) {
    if (!g) return fail(JSGX_ERR_INVALID, who, "null argument");
    if (!g->x) return fail(JSGX_ERR_INVALID, who, "null x");
    if (!g->y) return fail(JSGX_ERR_INVALID, who, "null y");
    if (!g->cost) return fail(JSGX_ERR_INVALID, who, "null cost");
    if (((bits_of(g->x) | bits_of(g->y) | bits_of(g->cost)) & 3) != 0) return fail(JSGX_ERR_INVALID, who, "pointers must be 4-byte aligned");
    if (g->pairs < 1 || g->pairs > 65535) return fail(JSGX_ERR_INVALID, who, "pairs must be in 1..65535");
    if (g->n_features < 1 || g->n_features > JSGX_CDIST_MAX_FEATURES) return fail(JSGX_ERR_INVALID, who, "n_features must be in 1..1024");
    if (g->n < 1 || g->n > JSGX_DTW_MAX_LEN) return fail(JSGX_ERR_INVALID, who, "n must be in 1..65536");
    if (g->m < 1 || g->m > JSGX_DTW_MAX_LEN) return fail(JSGX_ERR_INVALID, who, "m must be in 1..65536");
    if (g->metric < JSGX_METRIC_SQEUCLIDEAN || g->metric > JSGX_METRIC_COSINE) return fail(JSGX_ERR_INVALID, who, "metric must be in 0..2");
    if (g->reserved0 != 0) return fail(JSGX_ERR_INVALID, who, "reserved0 must be 0");
    const i128 K = g->n_features, N = g->n, M = g->m, P = g->pairs;
    if (g->x_frame_pitch < K) return fail(JSGX_ERR_INVALID, who, "x_frame_pitch smaller than n_features");
    if (g->y_frame_pitch < K) return fail(JSGX_ERR_INVALID, who, "y_frame_pitch smaller than n_features");
    if (g->x_pair_pitch != 0 && g->x_pair_pitch < extent(1, 0, N, g->x_frame_pitch, K)) return fail(JSGX_ERR_INVALID, who, "x_pair_pitch does not cover a sequence");
    if (g->y_pair_pitch != 0 && g->y_pair_pitch < extent(1, 0, M, g->y_frame_pitch, K)) return fail(JSGX_ERR_INVALID, who, "y_pair_pitch does not cover a sequence");
    if (g->cost_pitch < M) return fail(JSGX_ERR_INVALID, who, "cost_pitch smaller than m");
    if (P > 1 && g->cost_pair_pitch < extent(1, 0, N, g->cost_pitch, M)) return fail(JSGX_ERR_INVALID, who, "cost_pair_pitch does not cover a plane");
    const i128 cost_bytes = 4 * extent(P, P > 1 ? g->cost_pair_pitch : 0, N, g->cost_pitch, M);
    if (overlap(addr(g->cost), cost_bytes, addr(g->x), 4 * extent(P, g->x_pair_pitch, N, g->x_frame_pitch, K))) return fail(JSGX_ERR_INVALID, who, "cost overlaps x");
    if (overlap(addr(g->cost), cost_bytes, addr(g->y), 4 * extent(P, g->y_pair_pitch, M, g->y_frame_pitch, K))) return fail(JSGX_ERR_INVALID, who, "cost overlaps y");
    return JSGX_OK;
}

int dtw_check(const jsgx_dtw_args* g, const char* who) {
    if (!g) return fail(JSGX_ERR_INVALID, who, "null argument");
    if (!g->cost) return fail(JSGX_ERR_INVALID, who, "null cost");
    if (!g->acc) return fail(JSGX_ERR_INVALID, who, "null acc");
    if (!g->path_i != !g->path_j) return fail(JSGX_ERR_INVALID, who, "path_i and path_j go together");
    if (g->path_i && !g->path_len) return fail(JSGX_ERR_INVALID, who, "null path_len with paths");
    if (((bits_of(g->cost) | bits_of(g->acc) | bits_of(g->path_i) | bits_of(g->path_j) | bits_of(g->path_len) | bits_of(g->total)) & 3) != 0)
        return fail(JSGX_ERR_INVALID, who, "pointers must be 4-byte aligned");
    if (g->pairs < 1 || g->pairs > 65535) return fail(JSGX_ERR_INVALID, who, "pairs must be in 1..65535");
    if (g->n < 1 || g->n > JSGX_DTW_MAX_LEN) return fail(JSGX_ERR_INVALID, who, "n must be in 1..65536");
    if (g->m < 1 || g->m > JSGX_DTW_MAX_LEN) return fail(JSGX_ERR_INVALID, who, "m must be in 1..65536");
    if (g->subseq != 0 && g->subseq != 1) return fail(JSGX_ERR_INVALID, who, "subseq must be 0 or 1");
    if (g->band < 0 || g->band > JSGX_DTW_MAX_LEN) return fail(JSGX_ERR_INVALID, who, "band must be in 0..65536");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(g->weights_mul[k]) || !std::isfinite(g->weights_add[k])) return fail(JSGX_ERR_INVALID, who, "weights must be finite");
    if (g->reserved0 != 0) return fail(JSGX_ERR_INVALID, who, "reserved0 must be 0");
    if (g->band != 0 && g->subseq) return fail(JSGX_ERR_INVALID, who, "band and subseq exclude each other");
    const i128 N = g->n, M = g->m, P = g->pairs;
    const bool multi = g->pairs > 1;
    if (g->path_i && g->max_path < N + M - 1) return fail(JSGX_ERR_INVALID, who, "max_path smaller than n + m - 1");
    if (g->cost_pitch < M) return fail(JSGX_ERR_INVALID, who, "cost_pitch smaller than m");
    if (multi && g->cost_pair_pitch < extent(1, 0, N, g->cost_pitch, M)) return fail(JSGX_ERR_INVALID, who, "cost_pair_pitch does not cover a plane");
    if (g->acc_pitch < M) return fail(JSGX_ERR_INVALID, who, "acc_pitch smaller than m");
    if (multi && g->acc_pair_pitch < extent(1, 0, N, g->acc_pitch, M)) return fail(JSGX_ERR_INVALID, who, "acc_pair_pitch does not cover a plane");
    if (multi && g->path_i && g->path_pitch < g->max_path) return fail(JSGX_ERR_INVALID, who, "path_pitch smaller than max_path");
    const i128 cost0 = addr(g->cost), cost_bytes = 4 * extent(P, multi ? g->cost_pair_pitch : 0, N, g->cost_pitch, M);
    const i128 acc0 = addr(g->acc), acc_bytes = 4 * extent(P, multi ? g->acc_pair_pitch : 0, N, g->acc_pitch, M);
    const i128 path_bytes = g->path_i ? 4 * ((P - 1) * (multi ? g->path_pitch : 0) + g->max_path) : 0;
    const i128 out[4] = {addr(g->path_i), addr(g->path_j), addr(g->path_len), addr(g->total)};
    const i128 out_bytes[4] = {path_bytes, path_bytes, 4 * P, 4 * P};
    if (overlap(acc0, acc_bytes, cost0, cost_bytes)) return fail(JSGX_ERR_INVALID, who, "acc overlaps cost");
    for (int i = 0; i < 4; ++i)
        if (overlap(out[i], out_bytes[i], cost0, cost_bytes)) return fail(JSGX_ERR_INVALID, who, "an output overlaps cost");
    for (int i = 0; i < 4; ++i)
        if (overlap(out[i], out_bytes[i], acc0, acc_bytes)) return fail(JSGX_ERR_INVALID, who, "an output overlaps acc");
    return JSGX_OK;
}

int64_t dtw_scratch_bytes(const jsgx_dtw_args* g) { return g->path_i ? 8ll * g->pairs * ((int64_t)g->n + g->m - 1) : 0; }

int dtw_launches(const jsgx_dtw_args* g) {
    const int tiles_i = (g->n + JSGX_DTW_TILE_ROWS - 1) / JSGX_DTW_TILE_ROWS, tiles_j = (g->m + JSGX_DTW_TILE_COLS - 1) / JSGX_DTW_TILE_COLS;
    return tiles_i + tiles_j - 1 + ((g->path_len || g->total) ? 1 : 0);
}

}  // namespace jsgx

using namespace jsgx;

extern "C" {

int jsgx_cdist_plan(const jsgx_cdist_args* g, char* name, int name_len, int32_t* threads, int32_t* lds_bytes) {
    static const char* who = "jsgx_cdist_plan";
    if (name && name_len < 16) return fail(JSGX_ERR_INVALID, who, "bad argument");
    const int rc = cdist_check(g, who);
    if (rc != JSGX_OK) return rc;
    if (name) std::strncpy(name, "cdist_64x64", name_len);
    if (threads) *threads = JSGX_CDIST_THREADS;
    if (lds_bytes) *lds_bytes = JSGX_CDIST_LDS_BYTES;
    return JSGX_OK;
}

int64_t jsgx_dtw_scratch_bytes(const jsgx_dtw_args* g) {
    const int rc = dtw_check(g, "jsgx_dtw_scratch_bytes");
    return rc != JSGX_OK ? rc : dtw_scratch_bytes(g);
}

int jsgx_dtw_plan(const jsgx_dtw_args* g, char* name, int name_len, int32_t* tile_rows, int32_t* tile_cols, int32_t* n_launches, int32_t* threads,
                  int32_t* lds_bytes) {
    static const char* who = "jsgx_dtw_plan";
    if (name && name_len < 16) return fail(JSGX_ERR_INVALID, who, "bad argument");
    const int rc = dtw_check(g, who);
    if (rc != JSGX_OK) return rc;
    if (name) std::strncpy(name, "dtw_tiles", name_len);
    if (tile_rows) *tile_rows = JSGX_DTW_TILE_ROWS;
    if (tile_cols) *tile_cols = JSGX_DTW_TILE_COLS;
    if (n_launches) *n_launches = dtw_launches(g);
    if (threads) *threads = JSGX_DTW_THREADS;
    if (lds_bytes) *lds_bytes = JSGX_DTW_LDS_BYTES;
    return JSGX_OK;
}

}  // extern "C"
