// libjsgx.so, the pairwise cost and dynamic time warping (include/jsgx.h sections 2 and 3): the refusals, the scratch size and the
// plans, on the host and without a device.  The kernels and their launchers are in jsgx_cdist.hip and jsgx_dtw.hip; the error text
// (jsgx::fail) is in jsgx_beat_host.cpp.  The span and overlap arithmetic is jsg_spans.h, a header without state that both libraries take.
#include <cmath>
#include <cstdint>

#include "jsgx_internal.h"

namespace jsgx {

namespace {
using jsg::addr;
using jsg::i128;
using jsg::overlap;
}  // namespace

int cdist_check(const jsgx_cdist_args* g, const char* who) {
    if (!g) return fail(JSGX_ERR_INVALID, who, "null argument");
    if (!g->x) return fail(JSGX_ERR_INVALID, who, "null x");
    if (!g->y) return fail(JSGX_ERR_INVALID, who, "null y");
    if (!g->cost) return fail(JSGX_ERR_INVALID, who, "null cost");
    if (!jsg::aligned4(g->x, g->y, g->cost)) return fail(JSGX_ERR_INVALID, who, "pointers must be 4-byte aligned");
    if (g->pairs < 1 || g->pairs > 65535) return fail(JSGX_ERR_INVALID, who, "pairs must be in 1..65535");
    if (g->n_features < 1 || g->n_features > JSGX_CDIST_MAX_FEATURES) return fail(JSGX_ERR_INVALID, who, "n_features must be in 1..1024");
    if (g->n < 1 || g->n > JSGX_DTW_MAX_LEN) return fail(JSGX_ERR_INVALID, who, "n must be in 1..65536");
    if (g->m < 1 || g->m > JSGX_DTW_MAX_LEN) return fail(JSGX_ERR_INVALID, who, "m must be in 1..65536");
    if (g->metric < JSGX_METRIC_SQEUCLIDEAN || g->metric > JSGX_METRIC_COSINE) return fail(JSGX_ERR_INVALID, who, "metric must be in 0..2");
    if (g->reserved0 != 0) return fail(JSGX_ERR_INVALID, who, "reserved0 must be 0");
    i128 x_bytes, y_bytes, cost_bytes;
    int rc = check_xy(g, who, &x_bytes, &y_bytes);
    if (rc == JSGX_OK) rc = check_plane(who, "cost", "", "m", g->n, g->m, g->cost_pitch, g->cost_pair_pitch, g->pairs, &cost_bytes);
    if (rc != JSGX_OK) return rc;
    if (overlap(addr(g->cost), cost_bytes, addr(g->x), x_bytes)) return fail(JSGX_ERR_INVALID, who, "cost overlaps x");
    if (overlap(addr(g->cost), cost_bytes, addr(g->y), y_bytes)) return fail(JSGX_ERR_INVALID, who, "cost overlaps y");
    return JSGX_OK;
}

int dtw_check(const jsgx_dtw_args* g, const char* who) {
    if (!g) return fail(JSGX_ERR_INVALID, who, "null argument");
    if (!g->cost) return fail(JSGX_ERR_INVALID, who, "null cost");
    if (!g->acc) return fail(JSGX_ERR_INVALID, who, "null acc");
    int rc = check_path_pointers(g, who);
    if (rc != JSGX_OK) return rc;
    if (!jsg::aligned4(g->cost, g->acc, g->path_i, g->path_j, g->path_len, g->total))
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
    const long long N = g->n, M = g->m, P = g->pairs;
    if ((rc = check_max_path(g, who, N + M - 1, "max_path smaller than n + m - 1")) != JSGX_OK) return rc;
    i128 cost_bytes, acc_bytes, path_bytes;
    rc = check_plane(who, "cost", "", "m", N, M, g->cost_pitch, g->cost_pair_pitch, P, &cost_bytes);
    if (rc == JSGX_OK) rc = check_plane(who, "acc", "", "m", N, M, g->acc_pitch, g->acc_pair_pitch, P, &acc_bytes);
    if (rc == JSGX_OK) rc = check_path_pitch(g, who, &path_bytes);
    if (rc != JSGX_OK) return rc;
    const i128 cost0 = addr(g->cost), acc0 = addr(g->acc);
    const i128 out[4] = {addr(g->path_i), addr(g->path_j), addr(g->path_len), addr(g->total)};
    const i128 out_bytes[4] = {path_bytes, path_bytes, 4 * (i128)P, 4 * (i128)P};
    if (overlap(acc0, acc_bytes, cost0, cost_bytes)) return fail(JSGX_ERR_INVALID, who, "acc overlaps cost");
    for (int i = 0; i < 4; ++i)
        if (overlap(out[i], out_bytes[i], cost0, cost_bytes)) return fail(JSGX_ERR_INVALID, who, "an output overlaps cost");
    for (int i = 0; i < 4; ++i)
        if (overlap(out[i], out_bytes[i], acc0, acc_bytes)) return fail(JSGX_ERR_INVALID, who, "an output overlaps acc");
    return JSGX_OK;
}

int64_t dtw_scratch_bytes(const jsgx_dtw_args* g) { return g->path_i ? 8ll * g->pairs * ((int64_t)g->n + g->m - 1) : 0; }

}  // namespace jsgx

using namespace jsgx;

extern "C" {

int jsgx_cdist_plan(const jsgx_cdist_args* g, char* name, int name_len, int32_t* threads, int32_t* lds_bytes) {
    static const char* who = "jsgx_cdist_plan";
    int rc = check_name_buffer(who, name, name_len, 16);
    if (rc == JSGX_OK) rc = cdist_check(g, who);
    if (rc != JSGX_OK) return rc;
    put_name(name, name_len, "cdist_64x64");
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
    int rc = check_name_buffer(who, name, name_len, 16);
    if (rc == JSGX_OK) rc = dtw_check(g, who);
    if (rc != JSGX_OK) return rc;
    put_name(name, name_len, "dtw_tiles");
    put_tiles_plan(tile_rows, tile_cols, n_launches, threads, lds_bytes, tile_launches(g->n, g->m, g->path_len || g->total), JSGX_DTW_THREADS, JSGX_DTW_LDS_BYTES);
    return JSGX_OK;
}

}  // extern "C"
