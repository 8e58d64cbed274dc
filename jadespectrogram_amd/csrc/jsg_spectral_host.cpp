// libjsg.so, spectral shape descriptors (include/jsg.h section 2l): the refusals and the plan, on the host and without a device.  The
// kernels and their launcher are in jsg_spectral.hip.
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "jsg_internal.h"

namespace jsg {

namespace {
typedef __int128 i128;

i128 addr(const void* p) { return (i128)reinterpret_cast<uintptr_t>(p); }
bool overlap(i128 a0, i128 a_bytes, i128 b0, i128 b_bytes) { return a0 && b0 && a0 < b0 + b_bytes && b0 < a0 + a_bytes; }
}  // namespace

int spectral_check(const jsg_spectral_args* g, const char* who) {
    if (!g) return jsg_fail_who(JSG_ERR_INVALID, who, "null argument");
    if (!g->in) return jsg_fail_who(JSG_ERR_INVALID, who, "null in");
    if (!g->freqs) return jsg_fail_who(JSG_ERR_INVALID, who, "null freqs");
    const void* outs[7] = {g->energy, g->centroid, g->spread, g->rolloff, g->rolloff_bin, g->flatness_db, g->crest};
    uintptr_t bits = reinterpret_cast<uintptr_t>(g->in) | reinterpret_cast<uintptr_t>(g->freqs), any = 0;
    for (const void* o : outs) any |= reinterpret_cast<uintptr_t>(o);
    if (!any) return jsg_fail_who(JSG_ERR_INVALID, who, "all outputs null");
    if (((bits | any) & 3) != 0) return jsg_fail_who(JSG_ERR_INVALID, who, "pointers must be 4-byte aligned");
    if (g->rows < 1 || g->rows > 65535) return jsg_fail_who(JSG_ERR_INVALID, who, "rows must be in 1..65535");
    if (g->n_bins < 1 || g->n_bins > JSG_SPECTRAL_MAX_BINS) return jsg_fail_who(JSG_ERR_INVALID, who, "n_bins must be in 1..65536");
    if (g->n_frames < 1 || g->n_frames >= (1ll << 31)) return jsg_fail_who(JSG_ERR_INVALID, who, "n_frames must be in 1..2^31-1");
    if (!(g->roll_percent > 0.f && g->roll_percent <= 1.f)) return jsg_fail_who(JSG_ERR_INVALID, who, "roll_percent must be in (0, 1]");
    if (g->frame_pitch < g->n_bins) return jsg_fail_who(JSG_ERR_INVALID, who, "frame_pitch smaller than n_bins");
    const bool multi = g->rows > 1;
    const i128 plane = (i128)(g->n_frames - 1) * g->frame_pitch + g->n_bins;
    if (multi && (i128)g->row_pitch < plane) return jsg_fail_who(JSG_ERR_INVALID, who, "row_pitch smaller than (n_frames-1)*frame_pitch + n_bins");
    if (multi && g->out_pitch < g->n_frames) return jsg_fail_who(JSG_ERR_INVALID, who, "out_pitch smaller than n_frames");
    const i128 rows1 = g->rows - 1;
    const i128 in_bytes = 4 * (rows1 * (multi ? g->row_pitch : 0) + plane);
    const i128 out_bytes = 4 * (rows1 * (multi ? g->out_pitch : 0) + g->n_frames);
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

extern "C" {

int jsg_spectral_shape_plan(const jsg_spectral_args* g, char* name, int name_len, int32_t* lanes_per_frame, int32_t* frames_per_group, int32_t* lds_bytes) {
    static const char* who = "jsg_spectral_shape_plan";
    if (name && name_len < 24) return jsg_fail_who(JSG_ERR_INVALID, who, "bad argument");
    const int rc = spectral_check(g, who);
    if (rc != JSG_OK) return rc;
    SpectralPlan p{};
    spectral_resolve(g, &p);
    if (name) std::strncpy(name, spectral_path_name(p), name_len);
    if (lanes_per_frame) *lanes_per_frame = p.W;
    if (frames_per_group) *frames_per_group = p.FK;
    if (lds_bytes) *lds_bytes = 0;
    return JSG_OK;
}

int jsg_spectral_shape_kernel_name(const jsg_spectral_args* g, char* out, int out_len) {
    static const char* who = "jsg_spectral_shape_kernel_name";
    if (!out || out_len < 24) return jsg_fail_who(JSG_ERR_INVALID, who, "bad argument");
    const int rc = spectral_check(g, who);
    if (rc != JSG_OK) return rc;
    SpectralPlan p{};
    spectral_resolve(g, &p);
    std::strncpy(out, spectral_path_name(p), out_len);
    return JSG_OK;
}

}  // extern "C"
