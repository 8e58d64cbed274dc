// libjsgx.so, temporally constrained agglomerative segmentation (include/jsgx.h section 17): the refusals, the scratch and the plan, on
// the host and without a device.  The kernels and their launcher are in jsgx_agglo.hip; the error text (jsgx::fail) is in
// jsgx_beat_host.cpp.
#include <cstdint>

#include "jsgx_internal.h"

namespace jsgx {

namespace {
using jsg::addr;
using jsg::i128;
using jsg::overlap;

struct Named {
    const char* name;
    const void* p;
    i128 bytes;
};

int overlaps(const char* who, const Named& a, const Named& b) {
    if (!overlap(addr(a.p), a.bytes, addr(b.p), b.bytes)) return JSGX_OK;
    char what[96];
    std::snprintf(what, sizeof what, "%s overlaps %s", a.name, b.name);
    return fail(JSGX_ERR_INVALID, who, what);
}
}  // namespace

int agglo_check(const jsgx_agglomerative_args* g, const char* who, AggloSpans* spans) {
    if (!g) return fail(JSGX_ERR_INVALID, who, "null argument");
    if (!g->x) return fail(JSGX_ERR_INVALID, who, "null x");
    if (!g->segments) return fail(JSGX_ERR_INVALID, who, "null segments");
    if (!g->n_segments) return fail(JSGX_ERR_INVALID, who, "null n_segments");
    if (!g->out_bounds) return fail(JSGX_ERR_INVALID, who, "null out_bounds");
    if (!g->n_out) return fail(JSGX_ERR_INVALID, who, "null n_out");
    if (!g->bounds && g->max_bounds > 0) return fail(JSGX_ERR_INVALID, who, "null bounds with max_bounds > 0");
    if (!g->order != !g->height) return fail(JSGX_ERR_INVALID, who, "order and height go together");
    if (!jsg::aligned4(g->x, g->bounds, g->n_bounds, g->segments, g->n_segments) || !jsg::aligned4(g->out_bounds, g->n_out, g->order, g->height))
        return fail(JSGX_ERR_INVALID, who, "pointers must be 4-byte aligned");
    if (g->pairs < 1 || g->pairs > 65535) return fail(JSGX_ERR_INVALID, who, "pairs must be in 1..65535");
    if (g->n_frames < 1 || g->n_frames > JSGX_SYNC_MAX_FRAMES) return fail(JSGX_ERR_INVALID, who, "n_frames must be in 1..16777216");
    if (g->n_features < 1 || g->n_features > JSGX_SYNC_MAX_FEATURES) return fail(JSGX_ERR_INVALID, who, "n_features must be in 1..65536");
    if (g->max_bounds < 0 || g->max_bounds > JSGX_SYNC_MAX_BOUNDS) return fail(JSGX_ERR_INVALID, who, "max_bounds must be in 0..1048576");
    if (!g->n_bounds && (g->bounds_all < 0 || g->bounds_all > g->max_bounds)) return fail(JSGX_ERR_INVALID, who, "bounds_all must be in 0..max_bounds");
    if (g->max_segments < 1 || g->max_segments > JSGX_SYNC_MAX_SEGMENTS) return fail(JSGX_ERR_INVALID, who, "max_segments must be in 1..1048577");
    if (g->max_out < 1 || g->max_out > JSGX_AGGLO_MAX_OUT) return fail(JSGX_ERR_INVALID, who, "max_out must be in 1..16777216");
    if (g->n_clusters < 1) return fail(JSGX_ERR_INVALID, who, "n_clusters must be at least 1");
    if (g->pad != 0 && g->pad != 1) return fail(JSGX_ERR_INVALID, who, "pad must be 0 or 1");
    if (g->reserved0 != 0) return fail(JSGX_ERR_INVALID, who, "reserved0 must be 0");
    const AggloPlan plan = agglo_plan(g);
    if (g->max_segments < plan.stretches) return fail(JSGX_ERR_INVALID, who, "max_segments smaller than the stretches the list can give");
    if ((g->n_bounds ? g->max_bounds : g->bounds_all) == 0 && g->pad == 1 && g->n_frames > JSGX_AGGLO_MAX_STRETCH)
        return fail(JSGX_ERR_INVALID, who, "n_frames above 16384 without boundaries");
    const long long P = g->pairs, N = g->n_frames, S = g->max_segments;
    AggloSpans s;
    int rc = check_plane(who, "x", "_frame", "n_features", N, g->n_features, g->x_frame_pitch, g->x_pair_pitch, P, &s.x);
    if (rc != JSGX_OK) return rc;
    if (P > 1 && g->bounds && g->bounds_pitch != 0 && g->bounds_pitch < g->max_bounds) return fail(JSGX_ERR_INVALID, who, "bounds_pitch neither 0 nor >= max_bounds");
    if (P > 1 && g->segments_pitch < S + 1) return fail(JSGX_ERR_INVALID, who, "segments_pitch smaller than max_segments + 1");
    if (P > 1 && g->out_pitch < g->max_out) return fail(JSGX_ERR_INVALID, who, "out_pitch smaller than max_out");
    if (P > 1 && g->order && g->tree_pitch < N) return fail(JSGX_ERR_INVALID, who, "tree_pitch smaller than n_frames");
    s.bounds = g->bounds ? jsg::span_bytes(P, g->bounds_pitch, g->max_bounds, 4) : 0;
    s.n_bounds = g->n_bounds ? 4 * P : 0;
    s.out_bounds = jsg::span_bytes(P, g->out_pitch, g->max_out, 4);
    s.n_out = s.n_segments = 4 * P;
    s.segments = jsg::span_bytes(P, g->segments_pitch, S + 1, 4);
    s.order = s.height = g->order ? jsg::span_bytes(P, g->tree_pitch, N, 4) : 0;
    const Named outs[6] = {{"out_bounds", g->out_bounds, s.out_bounds}, {"n_out", g->n_out, s.n_out}, {"segments", g->segments, s.segments},
                           {"n_segments", g->n_segments, s.n_segments}, {"order", g->order, s.order},  {"height", g->height, s.height}},
                ins[3] = {{"x", g->x, s.x}, {"bounds", g->bounds, s.bounds}, {"n_bounds", g->n_bounds, s.n_bounds}};
    for (const auto& o : outs)
        for (const auto& i : ins)
            if ((rc = overlaps(who, o, i)) != JSGX_OK) return rc;
    for (int a = 0; a < 6; ++a)
        for (int b = a + 1; b < 6; ++b)
            if ((rc = overlaps(who, outs[a], outs[b])) != JSGX_OK) return rc;
    if (spans) *spans = s;
    return JSGX_OK;
}

int agglo_check_scratch(const jsgx_agglomerative_args* g, const char* who, const AggloSpans& s, const void* scratch, int64_t scratch_bytes) {
    const long long need = agglo_plan(g).scratch_bytes;
    int rc = check_scratch(who, scratch, scratch_bytes, need, "jsgx_agglomerative_scratch_bytes");
    if (rc != JSGX_OK) return rc;
    const Named mine{"scratch", scratch, need};
    const Named all[9] = {{"x", g->x, s.x},           {"bounds", g->bounds, s.bounds},       {"n_bounds", g->n_bounds, s.n_bounds},
                          {"out_bounds", g->out_bounds, s.out_bounds}, {"n_out", g->n_out, s.n_out}, {"segments", g->segments, s.segments},
                          {"n_segments", g->n_segments, s.n_segments}, {"order", g->order, s.order}, {"height", g->height, s.height}};
    for (const auto& x : all)
        if ((rc = overlaps(who, mine, x)) != JSGX_OK) return rc;
    return JSGX_OK;
}

}  // namespace jsgx

using namespace jsgx;

extern "C" {

int64_t jsgx_agglomerative_scratch_bytes(const jsgx_agglomerative_args* g) {
    const int rc = agglo_check(g, "jsgx_agglomerative_scratch_bytes", nullptr);
    return rc != JSGX_OK ? rc : agglo_plan(g).scratch_bytes;
}

int jsgx_agglomerative_plan(const jsgx_agglomerative_args* g, char* name, int name_len, int32_t* threads, int32_t* lds_bytes, int32_t* n_launches) {
    static const char* who = "jsgx_agglomerative_plan";
    int rc = check_name_buffer(who, name, name_len, 16);
    if (rc == JSGX_OK) rc = agglo_check(g, who, nullptr);
    if (rc != JSGX_OK) return rc;
    const AggloPlan p = agglo_plan(g);
    put_name(name, name_len, p.name);
    if (threads) *threads = p.threads;
    if (lds_bytes) *lds_bytes = p.lds_bytes;
    if (n_launches) *n_launches = p.launches;
    return JSGX_OK;
}

}  // extern "C"
