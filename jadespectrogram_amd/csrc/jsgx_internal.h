// libjsgx.so, what its units share (include/jsgx.h): the error text, the argument checks, the refusals that every unit words alike, the
// launchers' two ends and the float32 routines whose every operation the header states.  Of libjsg.so it takes two headers without
// state, jsg_spans.h (spans, overlap, alignment) and jsg_launch.h (OncePerDevice, launch_large_lds): the two libraries share that
// text, no object code and no state.  The first part needs no HIP header: plain g++ builds the host units for the sanitizer drivers.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>

#include "jsg_spans.h"
#include "jsgx.h"

#if defined(__HIPCC__)      // hipcc compiles the host unit as HIP too
#include <hip/hip_runtime.h>

#include "jsg_launch.h"
#define JSGX_HD __host__ __device__ __forceinline__
#else
#define JSGX_HD static inline
#include <cmath>
#endif

namespace jsgx {

// sets the calling thread's error text to "<who>: <what>" and returns code
int fail(int code, const char* who, const char* what);
// every refusal of jsgx_beat_launch that does not look at the scratch, in the header's order
int beat_check(const jsgx_beat_args* g, const char* who);
int64_t beat_scratch_bytes(const jsgx_beat_args* g);
// sections 2 and 3 (jsgx_dtw_host.cpp): every refusal that does not look at the scratch, in the header's order
int cdist_check(const jsgx_cdist_args* g, const char* who);
int dtw_check(const jsgx_dtw_args* g, const char* who);
int64_t dtw_scratch_bytes(const jsgx_dtw_args* g);
int dtw_launches(const jsgx_dtw_args* g);          // the kernels jsgx_dtw_launch enqueues
// section 4 (jsgx_viterbi_host.cpp): every refusal that does not look at the scratch, in the header's order
int viterbi_check(const jsgx_viterbi_args* g, const char* who);

// How the forward kernel of section 4 serves a shape (include/jsgx.h, "The kernels"), and where the parts of the scratch lie.
struct ViterbiPlan {
    const char* name;
    bool band, table_in_lds;
    int G, threads, lds_bytes;
    int n_blocks, n_launches;
    long long off_end, off_psi, off_jump;          // byte offsets in the scratch; V[T-1] is at 0
    long long scratch_bytes;
};
ViterbiPlan viterbi_plan(const jsgx_viterbi_args* g);

// The three refusals of a launch's scratch buffer, in this order; `sizer` names the call that states `need`.
inline int check_scratch(const char* who, const void* scratch, int64_t scratch_bytes, int64_t need, const char* sizer) {
    if (!scratch) return fail(JSGX_ERR_INVALID, who, "null scratch");
    if (!jsg::aligned4(scratch)) return fail(JSGX_ERR_INVALID, who, "scratch must be 4-byte aligned");
    if (scratch_bytes >= need) return JSGX_OK;
    char what[96];
    std::snprintf(what, sizeof what, "scratch smaller than %s", sizer);
    return fail(JSGX_ERR_INVALID, who, what);
}

// The two ends of a ..._plan call's name buffer: the refusal of one below min_len bytes, before any other (a call may pass none), and
// the kernel's name into it once the call has passed.
inline int check_name_buffer(const char* who, const char* buf, int len, int min_len) {
    return buf && len < min_len ? fail(JSGX_ERR_INVALID, who, "bad argument") : JSGX_OK;
}
inline void put_name(char* buf, int len, const char* name) {
    if (buf) std::strncpy(buf, name, len);
}

// The tiles of an n x m plane of section 3, down and across.  A launch takes one anti-diagonal of them.
struct DtwTiles {
    int i, j;
    int diagonals() const { return i + j - 1; }
};
inline DtwTiles dtw_tiles(int n, int m) { return {(n + JSGX_DTW_TILE_ROWS - 1) / JSGX_DTW_TILE_ROWS, (m + JSGX_DTW_TILE_COLS - 1) / JSGX_DTW_TILE_COLS}; }

#if defined(__HIPCC__)
// the device a launch goes to
inline int current_device(int* dev, const char* who) {
    return hipGetDevice(dev) == hipSuccess ? JSGX_OK : fail(JSGX_ERR_NO_DEVICE, who, "no HIP device");
}
// after the last launch of a call: what the launches left (hipGetLastError(), or what launch_large_lds returned), as the call's return code
inline int finish_launch(const char* who, hipError_t err) {
    if (err == hipSuccess) return JSGX_OK;
    char what[160];
    std::snprintf(what, sizeof what, "HIP error %d (%s)", (int)err, hipGetErrorString(err));
    return fail(JSGX_ERR_HIP, who, what);
}
#endif

constexpr int kBeatRing = 4096;                                 // >= 2 * JSGX_BEAT_MAX_PERIOD + JSGX_BEAT_THREADS, a power of two
constexpr int kBeatPen = 2 * JSGX_BEAT_MAX_PERIOD + 4;           // pen[tau], tau <= 2P
constexpr int kBeatG = JSGX_BEAT_MAX_PERIOD + 4;                 // g[k], k <= P

// a = (P + 1) / 2; G lanes per frame, F frames per step (include/jsgx.h, "The kernel")
struct BeatForm {
    int a, G, F;
};
JSGX_HD BeatForm beat_form(int P) {
    BeatForm f;
    f.a = (P + 1) / 2;
    f.G = 1;
    while (f.G < 64 && JSGX_BEAT_THREADS / f.G > f.a) f.G *= 2;
    f.F = JSGX_BEAT_THREADS / f.G < f.a ? JSGX_BEAT_THREADS / f.G : f.a;
    return f;
}

JSGX_HD float float_of_bits(unsigned b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(b);
#else
    float v;
    memcpy(&v, &b, 4);
    return v;
#endif
}

// exp(x) for x <= 0 as include/jsgx.h states it, operation by operation
JSGX_HD float exp_neg(float x) {
    if (x < -87.0f) return 0.f;
    const float n = __builtin_floorf(__builtin_fmaf(x, 1.44269502162933349609375f, 0.5f));
    float r = __builtin_fmaf(n, -0.693145751953125f, x);
    r = __builtin_fmaf(n, -1.42860676533018704503775e-06f, r);
    float p = 1.984127011382952332496643e-04f;
    p = __builtin_fmaf(p, r, 1.388888922519981861114502e-03f);
    p = __builtin_fmaf(p, r, 8.333333767950534820556641e-03f);
    p = __builtin_fmaf(p, r, 4.166666790843009948730469e-02f);
    p = __builtin_fmaf(p, r, 1.666666716337203979492188e-01f);
    p = __builtin_fmaf(p, r, 0.5f);
    p = __builtin_fmaf(p, r, 1.0f);
    p = __builtin_fmaf(p, r, 1.0f);
    return p * float_of_bits((unsigned)((int)n + 127) << 23);
}

}  // namespace jsgx
