// libjsgx.so, per-channel energy normalisation (include/jsgx.h section 13): the decay table, the refusals, the scratch and the plan, on
// the host and without a device.  The kernels and their launcher are in jsgx_pcen.hip; the error text (jsgx::fail) is in jsgx_beat_host.cpp.
#include <cmath>
#include <cstdint>

#include "jsgx_internal.h"

namespace jsgx {

namespace {
using jsg::addr;
using jsg::i128;
using jsg::overlap;

// [rows][n_bands] at a row pitch: "<name>_pitch smaller than n_bands" (rows > 1), and its bytes; a null pointer has none
int check_state(const char* who, const char* name, const void* p, long long rows, long long bands, long long pitch, i128* bytes) {
    *bytes = p ? jsg::span_bytes(rows, pitch, bands, 4) : 0;
    if (!p || rows == 1 || pitch >= bands) return JSGX_OK;
    char what[96];
    std::snprintf(what, sizeof what, "%s_pitch smaller than n_bands", name);
    return fail(JSGX_ERR_INVALID, who, what);
}

// a plane of the argument block: "<name>_frame_pitch smaller than n_bands", then "<name>_row_pitch does not cover a plane" (rows > 1)
int check_rows_plane(const char* who, const char* name, const jsgx_pcen_args* g, long long frame_pitch, long long row_pitch, i128* bytes) {
    char what[96];
    const i128 one = jsg::plane(g->n_frames, frame_pitch, g->n_bands);
    *bytes = jsg::span_bytes(g->rows, row_pitch, one, 4);
    if (frame_pitch < g->n_bands)
        std::snprintf(what, sizeof what, "%sframe_pitch smaller than n_bands", name);
    else if (g->rows > 1 && row_pitch < one)
        std::snprintf(what, sizeof what, "%srow_pitch does not cover a plane", name);
    else
        return JSGX_OK;
    return fail(JSGX_ERR_INVALID, who, what);
}
}  // namespace

int pcen_check(const jsgx_pcen_args* g, const char* who, PcenSpans* spans) {
    if (!g) return fail(JSGX_ERR_INVALID, who, "null argument");
    if (!g->in) return fail(JSGX_ERR_INVALID, who, "null in");
    if (!g->decay) return fail(JSGX_ERR_INVALID, who, "null decay");
    if (!g->out) return fail(JSGX_ERR_INVALID, who, "null out");
    if (!jsg::aligned4(g->in, g->decay, g->state_in, g->state_out, g->smooth_out, g->out)) return fail(JSGX_ERR_INVALID, who, "pointers must be 4-byte aligned");
    if (g->rows < 1 || g->rows > 65535) return fail(JSGX_ERR_INVALID, who, "rows must be in 1..65535");
    if (g->n_bands < 1 || g->n_bands > JSGX_PCEN_MAX_BANDS) return fail(JSGX_ERR_INVALID, who, "n_bands must be in 1..65536");
    if (g->n_frames < 1) return fail(JSGX_ERR_INVALID, who, "n_frames must be in 1..2147483647");
    if (pcen_plan(g).chains > JSGX_PCEN_MAX_CHAINS) return fail(JSGX_ERR_INVALID, who, "rows * chunks * n_bands must be at most 2^36");
    PcenSpans s;
    s.decay = 4 * JSGX_PCEN_CHUNK;
    int rc = check_rows_plane(who, "", g, g->frame_pitch, g->row_pitch, &s.in);
    if (rc == JSGX_OK) rc = check_state(who, "state_in", g->state_in, g->rows, g->n_bands, g->state_in_pitch, &s.state_in);
    if (rc == JSGX_OK) rc = check_state(who, "state_out", g->state_out, g->rows, g->n_bands, g->state_out_pitch, &s.state_out);
    if (rc == JSGX_OK && g->smooth_out) rc = check_rows_plane(who, "smooth_", g, g->smooth_frame_pitch, g->smooth_row_pitch, &s.smooth);
    if (!g->smooth_out) s.smooth = 0;
    if (rc == JSGX_OK) rc = check_rows_plane(who, "out_", g, g->out_frame_pitch, g->out_row_pitch, &s.out);
    if (rc != JSGX_OK) return rc;
    if (!std::isfinite(g->b) || !(g->b > 0.f) || g->b > 1.f) return fail(JSGX_ERR_INVALID, who, "b must be in (0, 1]");
    if (!std::isfinite(g->gain) || g->gain < 0.f) return fail(JSGX_ERR_INVALID, who, "gain must be finite and not negative");
    if (!std::isfinite(g->bias) || g->bias < 0.f) return fail(JSGX_ERR_INVALID, who, "bias must be finite and not negative");
    if (!std::isfinite(g->power) || !(g->power > 0.f)) return fail(JSGX_ERR_INVALID, who, "power must be finite and positive");
    if (!std::isfinite(g->eps) || !(g->eps > 0.f)) return fail(JSGX_ERR_INVALID, who, "eps must be finite and positive");
    // every output against every input, then the outputs against each other
    const struct {
        const char* name;
        const void* p;
        i128 bytes;
    } outs[3] = {{"out", g->out, s.out}, {"smooth_out", g->smooth_out, s.smooth}, {"state_out", g->state_out, s.state_out}},
      ins[3] = {{"in", g->in, s.in}, {"decay", g->decay, s.decay}, {"state_in", g->state_in, s.state_in}};
    char what[96];
    for (const auto& o : outs)
        for (const auto& i : ins)
            if (overlap(addr(o.p), o.bytes, addr(i.p), i.bytes)) {
                std::snprintf(what, sizeof what, "%s overlaps %s", o.name, i.name);
                return fail(JSGX_ERR_INVALID, who, what);
            }
    for (int x = 0; x < 3; ++x)
        for (int y = x + 1; y < 3; ++y)
            if (overlap(addr(outs[x].p), outs[x].bytes, addr(outs[y].p), outs[y].bytes)) {
                std::snprintf(what, sizeof what, "%s overlaps %s", outs[x].name, outs[y].name);
                return fail(JSGX_ERR_INVALID, who, what);
            }
    if (spans) *spans = s;
    return JSGX_OK;
}

int pcen_check_scratch(const jsgx_pcen_args* g, const char* who, const PcenSpans& s, const void* scratch, int64_t scratch_bytes) {
    const long long need = pcen_plan(g).scratch_bytes;
    if (need == 0) return JSGX_OK;          // a row is one chunk: the scratch is not looked at
    const int rc = check_scratch(who, scratch, scratch_bytes, need, "jsgx_pcen_scratch_bytes");
    if (rc != JSGX_OK) return rc;
    const struct {
        const char* name;
        const void* p;
        i128 bytes;
    } all[6] = {{"in", g->in, s.in},    {"decay", g->decay, s.decay},          {"state_in", g->state_in, s.state_in},
                {"out", g->out, s.out}, {"smooth_out", g->smooth_out, s.smooth}, {"state_out", g->state_out, s.state_out}};
    for (const auto& x : all)
        if (overlap(addr(scratch), need, addr(x.p), x.bytes)) {
            char what[96];
            std::snprintf(what, sizeof what, "scratch overlaps %s", x.name);
            return fail(JSGX_ERR_INVALID, who, what);
        }
    return JSGX_OK;
}

}  // namespace jsgx

using namespace jsgx;

extern "C" {

int jsgx_pcen_decay_build(float b, float* out) {
    static const char* who = "jsgx_pcen_decay_build";
    if (!out) return fail(JSGX_ERR_INVALID, who, "null out");
    if (!std::isfinite(b) || !(b > 0.f) || b > 1.f) return fail(JSGX_ERR_INVALID, who, "b must be in (0, 1]");
    const float a = 1.0f - b;
    for (int j = 0; j < JSGX_PCEN_CHUNK; ++j) out[j] = (float)std::pow((double)a, (double)(j + 1));
    return JSGX_OK;
}

int64_t jsgx_pcen_scratch_bytes(const jsgx_pcen_args* g) {
    const int rc = pcen_check(g, "jsgx_pcen_scratch_bytes", nullptr);
    return rc != JSGX_OK ? rc : pcen_plan(g).scratch_bytes;
}

int jsgx_pcen_plan(const jsgx_pcen_args* g, char* name, int name_len, int32_t* threads, int32_t* lds_bytes, int32_t* n_launches, int32_t* chunks) {
    static const char* who = "jsgx_pcen_plan";
    int rc = check_name_buffer(who, name, name_len, 16);
    if (rc == JSGX_OK) rc = pcen_check(g, who, nullptr);
    if (rc != JSGX_OK) return rc;
    const PcenPlan p = pcen_plan(g);
    put_name(name, name_len, p.name);
    if (threads) *threads = JSGX_PCEN_THREADS;
    if (lds_bytes) *lds_bytes = 0;
    if (n_launches) *n_launches = p.launches;
    if (chunks) *chunks = (int32_t)p.chunks;
    return JSGX_OK;
}

}  // extern "C"
