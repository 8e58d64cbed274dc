// libjsg.so, spectral shape descriptors (include/jsg.h section 2l): the refusals and the plan, on the host and without a device.  The
// kernels and their launcher are in jsg_spectral.hip.
#include <algorithm>
#include <cstdint>

#include "jsg_internal.h"

namespace jsg {

int spectral_check(const jsg_spectral_args* g, const char* who) {
    if (!g) return jsg_fail_who(JSG_ERR_INVALID, who, "null argument");
    if (!g->in) return jsg_fail_who(JSG_ERR_INVALID, who, "null in");
    if (!g->freqs) return jsg_fail_who(JSG_ERR_INVALID, who, "null freqs");
    const void* outs[7] = {g->energy, g->centroid, g->spread, g->rolloff, g->rolloff_bin, g->flatness_db, g->crest};
    if (std::all_of(outs, outs + 7, [](const void* o) { return !o; })) return jsg_fail_who(JSG_ERR_INVALID, who, "all outputs null");
    int rc = check_aligned4(who, g->in, g->freqs, g->energy, g->centroid, g->spread, g->rolloff, g->rolloff_bin, g->flatness_db, g->crest);
    if (rc == JSG_OK) rc = check_rows(g->rows, who);
    if (rc != JSG_OK) return rc;
    if (g->n_bins < 1 || g->n_bins > JSG_SPECTRAL_MAX_BINS) return jsg_fail_who(JSG_ERR_INVALID, who, "n_bins must be in 1..65536");
    if (g->n_frames < 1 || g->n_frames >= (1ll << 31)) return jsg_fail_who(JSG_ERR_INVALID, who, "n_frames must be in 1..2^31-1");
    if (!(g->roll_percent > 0.f && g->roll_percent <= 1.f)) return jsg_fail_who(JSG_ERR_INVALID, who, "roll_percent must be in (0, 1]");
    if (g->frame_pitch < g->n_bins) return jsg_fail_who(JSG_ERR_INVALID, who, "frame_pitch smaller than n_bins");
    const bool multi = g->rows > 1;
    const i128 in_plane = plane(g->n_frames, g->frame_pitch, g->n_bins);
    if (multi && (i128)g->row_pitch < in_plane) return jsg_fail_who(JSG_ERR_INVALID, who, "row_pitch smaller than (n_frames-1)*frame_pitch + n_bins");
    if (multi && g->out_pitch < g->n_frames) return jsg_fail_who(JSG_ERR_INVALID, who, "out_pitch smaller than n_frames");
    const i128 in_bytes = span_bytes(g->rows, g->row_pitch, in_plane, 4), out_bytes = span_bytes(g->rows, g->out_pitch, g->n_frames, 4);
    for (const void* o : outs)
        if (overlap(addr(g->in), in_bytes, addr(o), out_bytes)) return jsg_fail_who(JSG_ERR_INVALID, who, "an output overlaps in");
    for (const void* o : outs)
        if (overlap(addr(g->freqs), 4 * (i128)g->n_bins, addr(o), out_bytes)) return jsg_fail_who(JSG_ERR_INVALID, who, "an output overlaps freqs");
    return JSG_OK;
}

// By K alone.  The register paths are cut where the engine's transforms fall: 257, 513, 1025, 2049 and 4097 bins are 5, 9, 17, 33 and
// 65 values per lane.  The frames in flight keep 8 to 65 loads of a lane under way.
void spectral_resolve(const jsg_spectral_args* g, SpectralPlan* p) {
    const int K = g->n_bins;
    int W = 64;
    if (K <= 32)
        for (W = 1; W < K;) W <<= 1;
    static const int nc_of[] = {1, 2, 4, 9, 17, 33, kSpMaxRegs}, fk_of[] = {8, 8, 4, 2, 2, 1, 1};
    const int nc = (K + W - 1) / W;
    p->NC = 0, p->FK = 1, p->W = W;
    for (int i = 0; i < 7; ++i)
        if (nc <= nc_of[i]) {
            p->NC = nc_of[i], p->FK = fk_of[i];
            break;
        }
    const long long per_item = (long long)p->FK * (kSpThreads / W);
    p->groups = (g->n_frames + per_item - 1) / per_item;
}

const char* spectral_path_name(const SpectralPlan& p) {
    switch (p.NC) {
        case 1: return "spectral_regs1";
        case 2: return "spectral_regs2";
        case 4: return "spectral_regs4";
        case 9: return "spectral_regs9";
        case 17: return "spectral_regs17";
        case 33: return "spectral_regs33";
        case kSpMaxRegs: return "spectral_regs65";
        default: return "spectral_stream";
    }
}

}  // namespace jsg

using namespace jsg;

namespace {
// jsg_spectral_shape_plan (the name is optional) and jsg_spectral_shape_kernel_name (the name is all it gives)
int spectral_plan_call(const char* who, const jsg_spectral_args* g, char* name, int name_len, bool need_name, int32_t* lanes_per_frame, int32_t* frames_per_group,
                       int32_t* lds_bytes) {
    int rc = check_name_buffer(who, name, name_len, need_name);
    if (rc == JSG_OK) rc = spectral_check(g, who);
    if (rc != JSG_OK) return rc;
    SpectralPlan p{};
    spectral_resolve(g, &p);
    put_path_name(name, name_len, spectral_path_name(p));
    if (lanes_per_frame) *lanes_per_frame = p.W;
    if (frames_per_group) *frames_per_group = p.FK;
    if (lds_bytes) *lds_bytes = 0;
    return JSG_OK;
}
}  // namespace

extern "C" {

int jsg_spectral_shape_plan(const jsg_spectral_args* g, char* name, int name_len, int32_t* lanes_per_frame, int32_t* frames_per_group, int32_t* lds_bytes) {
    return spectral_plan_call("jsg_spectral_shape_plan", g, name, name_len, false, lanes_per_frame, frames_per_group, lds_bytes);
}

int jsg_spectral_shape_kernel_name(const jsg_spectral_args* g, char* out, int out_len) {
    return spectral_plan_call("jsg_spectral_shape_kernel_name", g, out, out_len, true, nullptr, nullptr, nullptr);
}

}  // extern "C"
