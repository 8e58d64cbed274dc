// libjsgx.so, peak picking and onset backtracking (include/jsgx.h section 14): the refusals, the scratch and the plan, on the host and
// without a device.  The kernels and their launcher are in jsgx_peak.hip; the error text (jsgx::fail) is in jsgx_beat_host.cpp.
#include <cmath>
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

int range(const char* who, const char* name, long long v, long long most) {
    if (v >= 0 && v <= most) return JSGX_OK;
    char what[96];
    std::snprintf(what, sizeof what, "%s must be in 0..%lld", name, most);
    return fail(JSGX_ERR_INVALID, who, what);
}

// [rows][width] at a row pitch: "<name>_pitch smaller than <width_name>" (rows > 1)
int pitch(const char* who, const char* name, const char* width_name, const void* p, long long rows, long long width, long long row_pitch) {
    if (!p || rows == 1 || row_pitch >= width) return JSGX_OK;
    char what[96];
    std::snprintf(what, sizeof what, "%s_pitch smaller than %s", name, width_name);
    return fail(JSGX_ERR_INVALID, who, what);
}

int overlaps(const char* who, const Named& a, const Named& b) {
    if (!overlap(addr(a.p), a.bytes, addr(b.p), b.bytes)) return JSGX_OK;
    char what[96];
    std::snprintf(what, sizeof what, "%s overlaps %s", a.name, b.name);
    return fail(JSGX_ERR_INVALID, who, what);
}
}  // namespace

int peak_check(const jsgx_peak_args* g, const char* who, PeakSpans* spans) {
    if (!g) return fail(JSGX_ERR_INVALID, who, "null argument");
    if (!g->in) return fail(JSGX_ERR_INVALID, who, "null in");
    if (!g->peaks) return fail(JSGX_ERR_INVALID, who, "null peaks");
    if (!g->n_peaks) return fail(JSGX_ERR_INVALID, who, "null n_peaks");
    if (!jsg::aligned4(g->in, g->energy) || !jsg::aligned4(g->peaks, g->backtracked, g->n_peaks)) return fail(JSGX_ERR_INVALID, who, "pointers must be 4-byte aligned");
    if (g->rows < 1 || g->rows > 65535) return fail(JSGX_ERR_INVALID, who, "rows must be in 1..65535");
    if (g->n_frames < 1 || g->n_frames > JSGX_PEAK_MAX_FRAMES) return fail(JSGX_ERR_INVALID, who, "n_frames must be in 1..16777216");
    int rc = range(who, "pre_max", g->pre_max, JSGX_PEAK_MAX_REACH);
    if (rc == JSGX_OK) rc = range(who, "post_max", g->post_max, JSGX_PEAK_MAX_REACH);
    if (rc == JSGX_OK) rc = range(who, "pre_avg", g->pre_avg, JSGX_PEAK_MAX_REACH);
    if (rc == JSGX_OK) rc = range(who, "post_avg", g->post_avg, JSGX_PEAK_MAX_REACH);
    if (rc != JSGX_OK) return rc;
    if (!std::isfinite(g->delta)) return fail(JSGX_ERR_INVALID, who, "delta must be finite");
    if ((rc = range(who, "wait", g->wait, JSGX_PEAK_MAX_FRAMES)) != JSGX_OK) return rc;
    if (g->normalise != 0 && g->normalise != 1) return fail(JSGX_ERR_INVALID, who, "normalise must be 0 or 1");
    if (g->max_peaks < 1 || g->max_peaks > JSGX_PEAK_MAX_FRAMES) return fail(JSGX_ERR_INVALID, who, "max_peaks must be in 1..16777216");
    if (!g->energy != !g->backtracked) return fail(JSGX_ERR_INVALID, who, "energy and backtracked go together");
    const long long R = g->rows, T = g->n_frames;
    rc = pitch(who, "in", "n_frames", g->in, R, T, g->in_pitch);
    if (rc == JSGX_OK) rc = pitch(who, "energy", "n_frames", g->energy, R, T, g->energy_pitch);
    if (rc == JSGX_OK) rc = pitch(who, "candidate", "n_frames", g->candidate, R, T, g->candidate_pitch);
    if (rc == JSGX_OK) rc = pitch(who, "peaks", "max_peaks", g->peaks, R, g->max_peaks, g->peaks_pitch);
    if (rc != JSGX_OK) return rc;
    PeakSpans s;
    s.in = jsg::span_bytes(R, g->in_pitch, T, 4);
    s.energy = g->energy ? jsg::span_bytes(R, g->energy_pitch, T, 4) : 0;
    s.peaks = jsg::span_bytes(R, g->peaks_pitch, g->max_peaks, 4);
    s.backtracked = g->backtracked ? s.peaks : 0;
    s.n_peaks = 4 * R;
    s.candidate = g->candidate ? jsg::span_bytes(R, g->candidate_pitch, T, 1) : 0;
    // every output against every input, then the outputs against each other
    const Named outs[4] = {{"peaks", g->peaks, s.peaks}, {"backtracked", g->backtracked, s.backtracked}, {"n_peaks", g->n_peaks, s.n_peaks},
                           {"candidate", g->candidate, s.candidate}},
                ins[2] = {{"in", g->in, s.in}, {"energy", g->energy, s.energy}};
    for (const auto& o : outs)
        for (const auto& i : ins)
            if ((rc = overlaps(who, o, i)) != JSGX_OK) return rc;
    for (int x = 0; x < 4; ++x)
        for (int y = x + 1; y < 4; ++y)
            if ((rc = overlaps(who, outs[x], outs[y])) != JSGX_OK) return rc;
    if (spans) *spans = s;
    return JSGX_OK;
}

int peak_check_scratch(const jsgx_peak_args* g, const char* who, const PeakSpans& s, const void* scratch, int64_t scratch_bytes) {
    const long long need = peak_plan(g).scratch_bytes;
    if (need == 0) return JSGX_OK;          // a row is one block: the scratch is not looked at
    int rc = check_scratch(who, scratch, scratch_bytes, need, "jsgx_peak_scratch_bytes");
    if (rc != JSGX_OK) return rc;
    const Named mine{"scratch", scratch, need};
    const Named all[6] = {{"in", g->in, s.in},           {"energy", g->energy, s.energy},    {"peaks", g->peaks, s.peaks}, {"backtracked", g->backtracked, s.backtracked},
                          {"n_peaks", g->n_peaks, s.n_peaks}, {"candidate", g->candidate, s.candidate}};
    for (const auto& x : all)
        if ((rc = overlaps(who, mine, x)) != JSGX_OK) return rc;
    return JSGX_OK;
}

}  // namespace jsgx

using namespace jsgx;

extern "C" {

int64_t jsgx_peak_scratch_bytes(const jsgx_peak_args* g) {
    const int rc = peak_check(g, "jsgx_peak_scratch_bytes", nullptr);
    return rc != JSGX_OK ? rc : peak_plan(g).scratch_bytes;
}

int jsgx_peak_plan(const jsgx_peak_args* g, char* name, int name_len, int32_t* threads, int32_t* lds_bytes, int32_t* n_launches, int32_t* blocks) {
    static const char* who = "jsgx_peak_plan";
    int rc = check_name_buffer(who, name, name_len, 16);
    if (rc == JSGX_OK) rc = peak_check(g, who, nullptr);
    if (rc != JSGX_OK) return rc;
    const PeakPlan p = peak_plan(g);
    put_name(name, name_len, p.name);
    if (threads) *threads = JSGX_PEAK_THREADS;
    if (lds_bytes) *lds_bytes = JSGX_PEAK_LDS_BYTES;
    if (n_launches) *n_launches = p.launches;
    if (blocks) *blocks = (int32_t)p.blocks;
    return JSGX_OK;
}

}  // extern "C"
