// libjsgx.so, the k nearest frames, the recurrence plane and the neighbour aggregation (include/jsgx.h sections 6 to 8): the refusals,
// the scratch size and the plan, on the host and without a device.  The kernels and their launchers are in jsgx_knn.hip; the error text
// (jsgx::fail) is in jsgx_beat_host.cpp.
#include <cstdint>

#include "jsgx_internal.h"

namespace jsgx {

namespace {
using jsg::addr;
using jsg::i128;
using jsg::overlap;
}  // namespace

int knn_check(const jsgx_knn_args* g, const char* who) {
    if (!g) return fail(JSGX_ERR_INVALID, who, "null argument");
    if (!g->x) return fail(JSGX_ERR_INVALID, who, "null x");
    if (!g->y) return fail(JSGX_ERR_INVALID, who, "null y");
    if (!g->nn_index) return fail(JSGX_ERR_INVALID, who, "null nn_index");
    if (!g->nn_dist) return fail(JSGX_ERR_INVALID, who, "null nn_dist");
    if (!jsg::aligned4(g->x, g->y, g->nn_index, g->nn_dist)) return fail(JSGX_ERR_INVALID, who, "pointers must be 4-byte aligned");
    if (g->pairs < 1 || g->pairs > 65535) return fail(JSGX_ERR_INVALID, who, "pairs must be in 1..65535");
    if (g->n_features < 1 || g->n_features > JSGX_CDIST_MAX_FEATURES) return fail(JSGX_ERR_INVALID, who, "n_features must be in 1..1024");
    if (g->n < 1 || g->n > JSGX_DTW_MAX_LEN) return fail(JSGX_ERR_INVALID, who, "n must be in 1..65536");
    if (g->m < 1 || g->m > JSGX_DTW_MAX_LEN) return fail(JSGX_ERR_INVALID, who, "m must be in 1..65536");
    if (g->metric < JSGX_METRIC_SQEUCLIDEAN || g->metric > JSGX_METRIC_COSINE) return fail(JSGX_ERR_INVALID, who, "metric must be in 0..2");
    if (g->k < 1 || g->k > JSGX_KNN_MAX_K) return fail(JSGX_ERR_INVALID, who, "k must be in 1..256");
    if (g->width < 0) return fail(JSGX_ERR_INVALID, who, "width must be >= 0");
    if (g->split < 0 || g->split > JSGX_KNN_MAX_SPLIT) return fail(JSGX_ERR_INVALID, who, "split must be in 0..16");
    i128 x_bytes, y_bytes, out_bytes[2];
    int rc = check_xy(g, who, &x_bytes, &y_bytes);
    if (rc == JSGX_OK) rc = check_plane(who, "index", "", "k", g->n, g->k, g->index_pitch, g->index_pair_pitch, g->pairs, &out_bytes[0]);
    if (rc == JSGX_OK) rc = check_plane(who, "dist", "", "k", g->n, g->k, g->dist_pitch, g->dist_pair_pitch, g->pairs, &out_bytes[1]);
    if (rc != JSGX_OK) return rc;
    const i128 out[2] = {addr(g->nn_index), addr(g->nn_dist)};
    for (int i = 0; i < 2; ++i)
        if (overlap(out[i], out_bytes[i], addr(g->x), x_bytes)) return fail(JSGX_ERR_INVALID, who, "an output overlaps x");
    for (int i = 0; i < 2; ++i)
        if (overlap(out[i], out_bytes[i], addr(g->y), y_bytes)) return fail(JSGX_ERR_INVALID, who, "an output overlaps y");
    if (overlap(out[0], out_bytes[0], out[1], out_bytes[1])) return fail(JSGX_ERR_INVALID, who, "nn_index overlaps nn_dist");
    return JSGX_OK;
}

// the smallest S in {1, 2, 4, 8, 16} that gives every compute unit a workgroup, stopping where a workgroup would be left without a tile
int knn_auto_split(const jsgx_knn_args* g, int tiles, long long n_cu) {
    const long long strips = (long long)g->pairs * ((g->n + JSGX_KNN_STRIP - 1) / JSGX_KNN_STRIP);
    int S = 1;
    while (S < JSGX_KNN_MAX_SPLIT && strips * S < n_cu && 2 * S <= tiles) S *= 2;
    return S;
}

KnnPlan knn_plan(const jsgx_knn_args* g, int n_cu) {
    KnnPlan p;
    p.tiles = (g->m + JSGX_KNN_TILE - 1) / JSGX_KNN_TILE;
    // n_cu = 0: the largest answer of the automatic rule, that of a device without end
    p.S = g->split == 0 ? knn_auto_split(g, p.tiles, n_cu > 0 ? n_cu : (1ll << 40)) : (g->split < p.tiles ? g->split : p.tiles);
    p.lds_dynamic = 6 * JSGX_KNN_STRIP * g->k;
    p.scratch_bytes = p.S > 1 ? 8ll * g->pairs * g->n * g->k * p.S : 0;
    return p;
}

int recurrence_check(const jsgx_recurrence_args* g, const char* who) {
    if (!g) return fail(JSGX_ERR_INVALID, who, "null argument");
    if (!g->nn_index) return fail(JSGX_ERR_INVALID, who, "null nn_index");
    if (!g->out) return fail(JSGX_ERR_INVALID, who, "null out");
    if (!jsg::aligned4(g->nn_index, g->nn_dist, g->bandwidth, g->out)) return fail(JSGX_ERR_INVALID, who, "pointers must be 4-byte aligned");
    if (g->pairs < 1 || g->pairs > 65535) return fail(JSGX_ERR_INVALID, who, "pairs must be in 1..65535");
    if (g->n < 1 || g->n > JSGX_DTW_MAX_LEN) return fail(JSGX_ERR_INVALID, who, "n must be in 1..65536");
    if (g->m < 1 || g->m > JSGX_DTW_MAX_LEN) return fail(JSGX_ERR_INVALID, who, "m must be in 1..65536");
    if (g->k < 1 || g->k > JSGX_KNN_MAX_K) return fail(JSGX_ERR_INVALID, who, "k must be in 1..256");
    if (g->mode < JSGX_REC_CONNECTIVITY || g->mode > JSGX_REC_AFFINITY) return fail(JSGX_ERR_INVALID, who, "mode must be in 0..2");
    if (g->sym != 0 && g->sym != 1) return fail(JSGX_ERR_INVALID, who, "sym must be 0 or 1");
    if (g->diag != 0 && g->diag != 1) return fail(JSGX_ERR_INVALID, who, "diag must be 0 or 1");
    if (g->reserved0 != 0) return fail(JSGX_ERR_INVALID, who, "reserved0 must be 0");
    if (g->sym && g->n != g->m) return fail(JSGX_ERR_INVALID, who, "sym needs n == m");
    if (g->mode != JSGX_REC_CONNECTIVITY && !g->nn_dist) return fail(JSGX_ERR_INVALID, who, "null nn_dist");
    if (g->mode == JSGX_REC_AFFINITY && !g->bandwidth) return fail(JSGX_ERR_INVALID, who, "null bandwidth");
    const long long N = g->n, P = g->pairs;
    i128 index_bytes, dist_bytes = 0, out_bytes;
    int rc = check_plane(who, "index", "", "k", N, g->k, g->index_pitch, g->index_pair_pitch, P, &index_bytes);
    if (rc == JSGX_OK && g->nn_dist) rc = check_plane(who, "dist", "", "k", N, g->k, g->dist_pitch, g->dist_pair_pitch, P, &dist_bytes);
    if (rc == JSGX_OK) rc = check_plane(who, "out", "", "m", N, g->m, g->out_pitch, g->out_pair_pitch, P, &out_bytes);
    if (rc != JSGX_OK) return rc;
    const i128 out0 = addr(g->out);
    if (overlap(out0, out_bytes, addr(g->nn_index), index_bytes)) return fail(JSGX_ERR_INVALID, who, "out overlaps nn_index");
    if (g->nn_dist && overlap(out0, out_bytes, addr(g->nn_dist), dist_bytes)) return fail(JSGX_ERR_INVALID, who, "out overlaps nn_dist");
    if (g->mode == JSGX_REC_AFFINITY && overlap(out0, out_bytes, addr(g->bandwidth), 4 * (i128)P)) return fail(JSGX_ERR_INVALID, who, "out overlaps bandwidth");
    return JSGX_OK;
}

int nn_filter_check(const jsgx_nn_filter_args* g, const char* who) {
    if (!g) return fail(JSGX_ERR_INVALID, who, "null argument");
    if (!g->s) return fail(JSGX_ERR_INVALID, who, "null s");
    if (!g->nn_index) return fail(JSGX_ERR_INVALID, who, "null nn_index");
    if (!g->out) return fail(JSGX_ERR_INVALID, who, "null out");
    if (!jsg::aligned4(g->s, g->nn_index, g->weights, g->out)) return fail(JSGX_ERR_INVALID, who, "pointers must be 4-byte aligned");
    if (g->pairs < 1 || g->pairs > 65535) return fail(JSGX_ERR_INVALID, who, "pairs must be in 1..65535");
    if (g->n < 1 || g->n > JSGX_DTW_MAX_LEN) return fail(JSGX_ERR_INVALID, who, "n must be in 1..65536");
    if (g->n_features < 1 || g->n_features > JSGX_NNF_MAX_FEATURES) return fail(JSGX_ERR_INVALID, who, "n_features must be in 1..65536");
    if (g->k < 1 || g->k > JSGX_KNN_MAX_K) return fail(JSGX_ERR_INVALID, who, "k must be in 1..256");
    const long long N = g->n, F = g->n_features, P = g->pairs;
    i128 s_bytes, index_bytes, weights_bytes = 0, out_bytes;
    int rc = check_plane(who, "s", "_frame", "n_features", N, F, g->s_frame_pitch, g->s_pair_pitch, P, &s_bytes);
    if (rc == JSGX_OK) rc = check_plane(who, "index", "", "k", N, g->k, g->index_pitch, g->index_pair_pitch, P, &index_bytes);
    if (rc == JSGX_OK && g->weights) rc = check_plane(who, "weights", "", "k", N, g->k, g->weights_pitch, g->weights_pair_pitch, P, &weights_bytes);
    if (rc == JSGX_OK) rc = check_plane(who, "out", "_frame", "n_features", N, F, g->out_frame_pitch, g->out_pair_pitch, P, &out_bytes);
    if (rc != JSGX_OK) return rc;
    const i128 out0 = addr(g->out);
    if (overlap(out0, out_bytes, addr(g->s), s_bytes)) return fail(JSGX_ERR_INVALID, who, "out overlaps s");
    if (overlap(out0, out_bytes, addr(g->nn_index), index_bytes)) return fail(JSGX_ERR_INVALID, who, "out overlaps nn_index");
    if (g->weights && overlap(out0, out_bytes, addr(g->weights), weights_bytes)) return fail(JSGX_ERR_INVALID, who, "out overlaps weights");
    return JSGX_OK;
}

}  // namespace jsgx

using namespace jsgx;

extern "C" {

int64_t jsgx_knn_scratch_bytes(const jsgx_knn_args* g) {
    const int rc = knn_check(g, "jsgx_knn_scratch_bytes");
    return rc != JSGX_OK ? rc : knn_plan(g, 0).scratch_bytes;
}

int jsgx_knn_plan(const jsgx_knn_args* g, int32_t n_cu, char* name, int name_len, int32_t* strip_rows, int32_t* split, int32_t* threads, int32_t* lds_bytes) {
    static const char* who = "jsgx_knn_plan";
    int rc = check_name_buffer(who, name, name_len, 16);
    if (rc == JSGX_OK) rc = knn_check(g, who);
    if (rc != JSGX_OK) return rc;
    if (n_cu < 1) return fail(JSGX_ERR_INVALID, who, "n_cu must be >= 1");
    const KnnPlan p = knn_plan(g, n_cu);
    put_name(name, name_len, "knn_64");
    if (strip_rows) *strip_rows = JSGX_KNN_STRIP;
    if (split) *split = p.S;
    if (threads) *threads = JSGX_KNN_THREADS;
    if (lds_bytes) *lds_bytes = JSGX_KNN_LDS_STATIC + p.lds_dynamic;
    return JSGX_OK;
}

}  // extern "C"
