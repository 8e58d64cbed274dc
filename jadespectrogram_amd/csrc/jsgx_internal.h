// libjsgx.so, what its units share (include/jsgx.h): the error text, the argument check and the float32 routines whose every
// operation the header states.  Nothing of libjsg.so is used here.
#pragma once

#include <cstdint>

#include "jsgx.h"

#if defined(__HIPCC__)      // hipcc compiles the host unit as HIP too
#include <hip/hip_runtime.h>

#include <atomic>
#define JSGX_HD __host__ __device__ __forceinline__
#else
#define JSGX_HD static inline
#include <cmath>
#include <cstring>
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

#if defined(__HIPCC__)
// Launches a kernel that may ask for more than 64 KiB of dynamic LDS, up to lds_max bytes.  The runtime has to be told once per
// device and kernel before the first such launch; *told keeps a bit per device (a device index outside 0..63 is told every time).
// Telling is no stream operation, so a first launch under capture works.  The bit is set after the launch has succeeded.
template <class Args>
hipError_t launch_large_lds(std::atomic<unsigned long long>* told, int dev, void (*kernel)(Args), int lds_max, dim3 grid, dim3 block, size_t lds_bytes,
                            hipStream_t s, const Args& k) {
    const unsigned long long bit = dev >= 0 && dev < 64 ? 1ull << dev : 0;
    const bool first = !(told->load(std::memory_order_acquire) & bit);
    if (first) {
        const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
        if (err != hipSuccess) return err;
    }
    void* args[] = {const_cast<Args*>(&k)};
    (void)hipLaunchKernel(reinterpret_cast<const void*>(kernel), grid, block, args, lds_bytes, s);
    const hipError_t err = hipGetLastError();
    if (err == hipSuccess && first) told->fetch_or(bit, std::memory_order_release);
    return err;
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
