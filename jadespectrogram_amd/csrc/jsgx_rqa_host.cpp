// libjsgx.so, recurrence quantification alignment (include/jsgx.h section 9): the refusals, the scratch size and the plan, on the host
// and without a device.  The kernels and their launcher are in jsgx_rqa.hip; the error text (jsgx::fail) is in jsgx_beat_host.cpp.
#include <cmath>
#include <cstdint>

#include "jsgx_internal.h"

namespace jsgx {

namespace {
using jsg::addr;
using jsg::i128;
using jsg::overlap;
}  // namespace

int rqa_check(const jsgx_rqa_args* g, const char* who) {
    if (!g) return fail(JSGX_ERR_INVALID, who, "null argument");
    if (!g->sim) return fail(JSGX_ERR_INVALID, who, "null sim");
    if (!g->score) return fail(JSGX_ERR_INVALID, who, "null score");
    int rc = check_path_pointers(g, who);
    if (rc != JSGX_OK) return rc;
    if (!jsg::aligned4(g->sim, g->score, g->path_i, g->path_j, g->path_len, g->end, g->total))
        return fail(JSGX_ERR_INVALID, who, "pointers must be 4-byte aligned");
    if (g->pairs < 1 || g->pairs > 65535) return fail(JSGX_ERR_INVALID, who, "pairs must be in 1..65535");
    if (g->n < 1 || g->n > JSGX_DTW_MAX_LEN) return fail(JSGX_ERR_INVALID, who, "n must be in 1..65536");
    if (g->m < 1 || g->m > JSGX_DTW_MAX_LEN) return fail(JSGX_ERR_INVALID, who, "m must be in 1..65536");
    if (g->knight != 0 && g->knight != 1) return fail(JSGX_ERR_INVALID, who, "knight must be 0 or 1");
    if (!std::isfinite(g->gap_onset) || !(g->gap_onset >= 0.f)) return fail(JSGX_ERR_INVALID, who, "gap_onset must be finite and >= 0");
    if (!std::isfinite(g->gap_extend) || !(g->gap_extend >= 0.f)) return fail(JSGX_ERR_INVALID, who, "gap_extend must be finite and >= 0");
    if (g->reserved0 != 0) return fail(JSGX_ERR_INVALID, who, "reserved0 must be 0");
    const long long N = g->n, M = g->m, P = g->pairs;
    if ((rc = check_max_path(g, who, N < M ? N : M, "max_path smaller than min(n, m)")) != JSGX_OK) return rc;
    i128 sim_bytes, score_bytes, step_bytes = 0, path_bytes;
    rc = check_plane(who, "sim", "", "m", N, M, g->sim_pitch, g->sim_pair_pitch, P, &sim_bytes);
    if (rc == JSGX_OK) rc = check_plane(who, "score", "", "m", N, M, g->score_pitch, g->score_pair_pitch, P, &score_bytes);
    if (rc == JSGX_OK && g->step) {
        rc = check_plane(who, "step", "", "m", N, M, g->step_pitch, g->step_pair_pitch, P, &step_bytes);
        step_bytes /= 4;            // a plane of bytes
    }
    if (rc == JSGX_OK) rc = check_path_pitch(g, who, &path_bytes);
    if (rc != JSGX_OK) return rc;
    const i128 sim0 = addr(g->sim);
    const i128 out[7] = {addr(g->score), addr(g->step), addr(g->path_i), addr(g->path_j), addr(g->path_len), addr(g->end), addr(g->total)};
    const i128 out_bytes[7] = {score_bytes, step_bytes, path_bytes, path_bytes, 4 * (i128)P, 8 * (i128)P, 4 * (i128)P};
    if (overlap(out[0], out_bytes[0], sim0, sim_bytes)) return fail(JSGX_ERR_INVALID, who, "score overlaps sim");
    for (int i = 1; i < 7; ++i)
        if (overlap(out[i], out_bytes[i], sim0, sim_bytes)) return fail(JSGX_ERR_INVALID, who, "an output overlaps sim");
    for (int i = 0; i < 7; ++i)
        for (int j = i + 1; j < 7; ++j)
            if (overlap(out[i], out_bytes[i], out[j], out_bytes[j])) return fail(JSGX_ERR_INVALID, who, "two outputs overlap");
    return JSGX_OK;
}

RqaScratch rqa_scratch(const jsgx_rqa_args* g) {
    const DtwTiles t = dtw_tiles(g->n, g->m);
    RqaScratch s;
    s.tiles = (long long)t.i * t.j;
    s.off_paths = (g->path_len || g->end || g->total) ? 8ll * g->pairs * s.tiles : 0;
    s.bytes = s.off_paths + (g->path_i ? 8ll * g->pairs * (g->n < g->m ? g->n : g->m) : 0);
    return s;
}

}  // namespace jsgx

using namespace jsgx;

extern "C" {

int64_t jsgx_rqa_scratch_bytes(const jsgx_rqa_args* g) {
    const int rc = rqa_check(g, "jsgx_rqa_scratch_bytes");
    return rc != JSGX_OK ? rc : rqa_scratch(g).bytes;
}

int jsgx_rqa_plan(const jsgx_rqa_args* g, char* name, int name_len, int32_t* tile_rows, int32_t* tile_cols, int32_t* n_launches, int32_t* threads,
                  int32_t* lds_bytes) {
    static const char* who = "jsgx_rqa_plan";
    int rc = check_name_buffer(who, name, name_len, 16);
    if (rc == JSGX_OK) rc = rqa_check(g, who);
    if (rc != JSGX_OK) return rc;
    put_name(name, name_len, "rqa_tiles");
    put_tiles_plan(tile_rows, tile_cols, n_launches, threads, lds_bytes, tile_launches(g->n, g->m, g->path_len || g->end || g->total), JSGX_RQA_THREADS, JSGX_RQA_LDS_BYTES);
    return JSGX_OK;
}

}  // extern "C"
