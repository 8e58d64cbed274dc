// libjsgx.so, non-negative matrix factorisation (include/jsgx.h section 12): the refusals, the layout of the scratch and the plan, on the
// host and without a device.  The kernels and their launcher are in jsgx_nmf.hip; the error text (jsgx::fail) is in jsgx_beat_host.cpp.
#include <cstdint>

#include "jsgx_internal.h"

namespace jsgx {

namespace {
using jsg::addr;
using jsg::i128;
using jsg::overlap;

// One plane per problem: "<name>_pitch smaller than <cols_name>", then "<name>_problem_pitch does not cover a plane", and its bytes.
int check_problem_plane(const char* who, const char* name, const char* cols_name, long long rows, long long cols, long long pitch, long long problem_pitch,
                        long long problems, i128* bytes) {
    char what[96];
    const i128 one = jsg::plane(rows, pitch, cols);
    *bytes = jsg::span_bytes(problems, problem_pitch, one, 4);
    if (pitch < cols)
        std::snprintf(what, sizeof what, "%s_pitch smaller than %s", name, cols_name);
    else if (problems > 1 && problem_pitch < one)
        std::snprintf(what, sizeof what, "%s_problem_pitch does not cover a plane", name);
    else
        return JSGX_OK;
    return fail(JSGX_ERR_INVALID, who, what);
}
}  // namespace

int nmf_check(const jsgx_nmf_args* g, const char* who, NmfSpans* spans) {
    if (!g) return fail(JSGX_ERR_INVALID, who, "null argument");
    if (!g->v) return fail(JSGX_ERR_INVALID, who, "null v");
    if (!g->a) return fail(JSGX_ERR_INVALID, who, "null a");
    if (!g->c) return fail(JSGX_ERR_INVALID, who, "null c");
    if (!jsg::aligned4(g->v, g->a, g->c)) return fail(JSGX_ERR_INVALID, who, "pointers must be 4-byte aligned");
    if (g->problems < 1 || g->problems > 65535) return fail(JSGX_ERR_INVALID, who, "problems must be in 1..65535");
    if (g->n_frames < 1 || g->n_frames > JSGX_NMF_MAX_FRAMES) return fail(JSGX_ERR_INVALID, who, "n_frames must be in 1..16777216");
    if (g->n_bins < 1 || g->n_bins > JSGX_NMF_MAX_BINS) return fail(JSGX_ERR_INVALID, who, "n_bins must be in 1..16384");
    if (g->n_components < 1 || g->n_components > JSGX_NMF_MAX_COMPONENTS) return fail(JSGX_ERR_INVALID, who, "n_components must be in 1..64");
    if (g->n_iter < 1 || g->n_iter > JSGX_NMF_MAX_ITER) return fail(JSGX_ERR_INVALID, who, "n_iter must be in 1..65536");
    if (g->update_components != 0 && g->update_components != 1) return fail(JSGX_ERR_INVALID, who, "update_components must be 0 or 1");
    if (g->loss != JSGX_NMF_FROBENIUS) return fail(JSGX_ERR_INVALID, who, "loss must be JSGX_NMF_FROBENIUS");
    if (g->reserved0 != 0) return fail(JSGX_ERR_INVALID, who, "reserved0 must be 0");
    NmfSpans s;
    int rc = check_problem_plane(who, "v", "n_bins", g->n_frames, g->n_bins, g->v_pitch, g->v_problem_pitch, g->problems, &s.v);
    if (rc == JSGX_OK) rc = check_problem_plane(who, "a", "n_components", g->n_frames, g->n_components, g->a_pitch, g->a_problem_pitch, g->problems, &s.a);
    if (rc == JSGX_OK) rc = check_problem_plane(who, "c", "n_bins", g->n_components, g->n_bins, g->c_pitch, g->c_problem_pitch, g->problems, &s.c);
    if (rc != JSGX_OK) return rc;
    if (overlap(addr(g->a), s.a, addr(g->v), s.v)) return fail(JSGX_ERR_INVALID, who, "a overlaps v");
    if (overlap(addr(g->c), s.c, addr(g->v), s.v)) return fail(JSGX_ERR_INVALID, who, "c overlaps v");
    if (overlap(addr(g->a), s.a, addr(g->c), s.c)) return fail(JSGX_ERR_INVALID, who, "a overlaps c");
    if (spans) *spans = s;
    return JSGX_OK;
}

int nmf_check_scratch(const jsgx_nmf_args* g, const char* who, const NmfSpans& s, const void* scratch, int64_t scratch_bytes) {
    const NmfScratch lay = nmf_scratch(g);
    const int rc = check_scratch(who, scratch, scratch_bytes, lay.bytes, "jsgx_nmf_scratch_bytes");
    if (rc != JSGX_OK) return rc;
    if (overlap(addr(scratch), lay.bytes, addr(g->v), s.v)) return fail(JSGX_ERR_INVALID, who, "scratch overlaps v");
    if (overlap(addr(scratch), lay.bytes, addr(g->a), s.a)) return fail(JSGX_ERR_INVALID, who, "scratch overlaps a");
    if (overlap(addr(scratch), lay.bytes, addr(g->c), s.c)) return fail(JSGX_ERR_INVALID, who, "scratch overlaps c");
    return JSGX_OK;
}

}  // namespace jsgx

using namespace jsgx;

extern "C" {

int64_t jsgx_nmf_scratch_bytes(const jsgx_nmf_args* g) {
    const int rc = nmf_check(g, "jsgx_nmf_scratch_bytes", nullptr);
    return rc != JSGX_OK ? rc : nmf_scratch(g).bytes;
}

int jsgx_nmf_plan(const jsgx_nmf_args* g, char* name, int name_len, int32_t* threads, int32_t* lds_bytes, int32_t* launches_per_iter, int32_t* t_chunks) {
    static const char* who = "jsgx_nmf_plan";
    int rc = check_name_buffer(who, name, name_len, 16);
    if (rc == JSGX_OK) rc = nmf_check(g, who, nullptr);
    if (rc != JSGX_OK) return rc;
    put_name(name, name_len, "nmf_update_a");
    if (threads) *threads = JSGX_NMF_THREADS;
    if (lds_bytes) *lds_bytes = JSGX_NMF_LDS_BYTES;
    if (launches_per_iter) *launches_per_iter = g->update_components ? 8 : 1;
    if (t_chunks) *t_chunks = (int32_t)nmf_scratch(g).chunks_t;
    return JSGX_OK;
}

}  // extern "C"
