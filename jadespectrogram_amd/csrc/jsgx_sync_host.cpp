// libjsgx.so, aggregation over segments and time-delay embedding (include/jsgx.h sections 15 and 16): the refusals and the plan, on the
// host and without a device.  The kernels and their launchers are in jsgx_sync.hip; the error text (jsgx::fail) is in jsgx_beat_host.cpp.
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

int sync_check(const jsgx_sync_args* g, const char* who) {
    if (!g) return fail(JSGX_ERR_INVALID, who, "null argument");
    if (!g->x) return fail(JSGX_ERR_INVALID, who, "null x");
    if (!g->out) return fail(JSGX_ERR_INVALID, who, "null out");
    if (!g->segments) return fail(JSGX_ERR_INVALID, who, "null segments");
    if (!g->n_segments) return fail(JSGX_ERR_INVALID, who, "null n_segments");
    if (!g->bounds && g->max_bounds > 0) return fail(JSGX_ERR_INVALID, who, "null bounds with max_bounds > 0");
    if (!jsg::aligned4(g->x, g->out) || !jsg::aligned4(g->bounds, g->n_bounds, g->segments, g->n_segments))
        return fail(JSGX_ERR_INVALID, who, "pointers must be 4-byte aligned");
    if (g->pairs < 1 || g->pairs > 65535) return fail(JSGX_ERR_INVALID, who, "pairs must be in 1..65535");
    if (g->n_frames < 1 || g->n_frames > JSGX_SYNC_MAX_FRAMES) return fail(JSGX_ERR_INVALID, who, "n_frames must be in 1..16777216");
    if (g->n_features < 1 || g->n_features > JSGX_SYNC_MAX_FEATURES) return fail(JSGX_ERR_INVALID, who, "n_features must be in 1..65536");
    if (g->max_bounds < 0 || g->max_bounds > JSGX_SYNC_MAX_BOUNDS) return fail(JSGX_ERR_INVALID, who, "max_bounds must be in 0..1048576");
    if (!g->n_bounds && (g->bounds_all < 0 || g->bounds_all > g->max_bounds)) return fail(JSGX_ERR_INVALID, who, "bounds_all must be in 0..max_bounds");
    if (g->max_segments < 1 || g->max_segments > JSGX_SYNC_MAX_SEGMENTS) return fail(JSGX_ERR_INVALID, who, "max_segments must be in 1..1048577");
    if (g->aggregate < JSGX_SYNC_MEAN || g->aggregate > JSGX_SYNC_MEDIAN) return fail(JSGX_ERR_INVALID, who, "aggregate must be in 0..3");
    if (g->pad != 0 && g->pad != 1) return fail(JSGX_ERR_INVALID, who, "pad must be 0 or 1");
    if (g->reserved0 != 0 || g->reserved1 != 0) return fail(JSGX_ERR_INVALID, who, "reserved0 and reserved1 must be 0");
    const long long P = g->pairs, F = g->n_features, S = g->max_segments;
    i128 x_bytes, out_bytes;
    int rc = check_plane(who, "x", "_frame", "n_features", g->n_frames, F, g->x_frame_pitch, g->x_pair_pitch, P, &x_bytes);
    if (rc == JSGX_OK) rc = check_plane(who, "out", "_frame", "n_features", S, F, g->out_frame_pitch, g->out_pair_pitch, P, &out_bytes);
    if (rc != JSGX_OK) return rc;
    if (P > 1 && g->bounds && g->bounds_pitch != 0 && g->bounds_pitch < g->max_bounds) return fail(JSGX_ERR_INVALID, who, "bounds_pitch neither 0 nor >= max_bounds");
    if (P > 1 && g->segments_pitch < S + 1) return fail(JSGX_ERR_INVALID, who, "segments_pitch smaller than max_segments + 1");
    const Named outs[3] = {{"out", g->out, out_bytes}, {"segments", g->segments, jsg::span_bytes(P, g->segments_pitch, S + 1, 4)}, {"n_segments", g->n_segments, 4 * P}},
                ins[3] = {{"x", g->x, x_bytes}, {"bounds", g->bounds, jsg::span_bytes(P, g->bounds_pitch, g->max_bounds, 4)}, {"n_bounds", g->n_bounds, 4 * P}};
    for (const auto& o : outs)
        for (const auto& i : ins)
            if ((rc = overlaps(who, o, i)) != JSGX_OK) return rc;
    for (int a = 0; a < 3; ++a)
        for (int b = a + 1; b < 3; ++b)
            if ((rc = overlaps(who, outs[a], outs[b])) != JSGX_OK) return rc;
    return JSGX_OK;
}

int stack_memory_check(const jsgx_stack_memory_args* g, const char* who) {
    if (!g) return fail(JSGX_ERR_INVALID, who, "null argument");
    if (!g->x) return fail(JSGX_ERR_INVALID, who, "null x");
    if (!g->out) return fail(JSGX_ERR_INVALID, who, "null out");
    if (!jsg::aligned4(g->x, g->out)) return fail(JSGX_ERR_INVALID, who, "pointers must be 4-byte aligned");
    if (g->pairs < 1 || g->pairs > 65535) return fail(JSGX_ERR_INVALID, who, "pairs must be in 1..65535");
    if (g->n_frames < 1 || g->n_frames > JSGX_SYNC_MAX_FRAMES) return fail(JSGX_ERR_INVALID, who, "n_frames must be in 1..16777216");
    if (g->n_features < 1 || g->n_features > JSGX_SYNC_MAX_FEATURES) return fail(JSGX_ERR_INVALID, who, "n_features must be in 1..65536");
    if (g->n_steps < 1 || g->n_steps > JSGX_STACK_MAX_STEPS) return fail(JSGX_ERR_INVALID, who, "n_steps must be in 1..256");
    const long long W = (long long)g->n_steps * g->n_features;
    if (W > JSGX_STACK_MAX_WIDTH) return fail(JSGX_ERR_INVALID, who, "n_steps * n_features must be at most 1048576");
    if (g->delay == 0 || g->delay > JSGX_STACK_MAX_DELAY || g->delay < -JSGX_STACK_MAX_DELAY) return fail(JSGX_ERR_INVALID, who, "delay must be non-zero and within +-16777216");
    if (g->mode != JSGX_STACK_CONSTANT && g->mode != JSGX_STACK_EDGE) return fail(JSGX_ERR_INVALID, who, "mode must be 0 or 1");
    if (g->reserved0 != 0) return fail(JSGX_ERR_INVALID, who, "reserved0 must be 0");
    i128 x_bytes, out_bytes;
    int rc = check_plane(who, "x", "_frame", "n_features", g->n_frames, g->n_features, g->x_frame_pitch, g->x_pair_pitch, g->pairs, &x_bytes);
    if (rc == JSGX_OK) rc = check_plane(who, "out", "_frame", "n_steps * n_features", g->n_frames, W, g->out_frame_pitch, g->out_pair_pitch, g->pairs, &out_bytes);
    if (rc != JSGX_OK) return rc;
    return overlaps(who, {"out", g->out, out_bytes}, {"x", g->x, x_bytes});
}

}  // namespace jsgx

using namespace jsgx;

extern "C" {

int jsgx_sync_plan(const jsgx_sync_args* g, char* name, int name_len, int32_t* threads, int32_t* lds_bytes, int32_t* n_launches) {
    static const char* who = "jsgx_sync_plan";
    int rc = check_name_buffer(who, name, name_len, 16);
    if (rc == JSGX_OK) rc = sync_check(g, who);
    if (rc != JSGX_OK) return rc;
    const SyncPlan p = sync_plan(g);
    put_name(name, name_len, p.name);
    if (threads) *threads = JSGX_SYNC_THREADS;
    if (lds_bytes) *lds_bytes = JSGX_SYNC_LDS_BYTES + p.lds_dynamic;
    if (n_launches) *n_launches = p.launches;
    return JSGX_OK;
}

}  // extern "C"
