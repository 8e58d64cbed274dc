// The host entry points of sections 15 and 16 of libjsgx.so (include/jsgx.h) from C++: the plan over shapes up to the limits (the 64-bit
// pitch arithmetic included: planes more than 2^31 elements apart) and the refusals with their texts in their order.  No launch that
// passes, so no device: built against libjsgx.so (CMake, jsg::jsgx; JSGX_SYNC_TEST_LAUNCHES: the refusals through the launches too) or, for
// the sanitizers, together with csrc/jsgx_beat_host.cpp and csrc/jsgx_sync_host.cpp themselves (tests/test_sync_host.py:
// -fsanitize=address,undefined), where section 16, which has no plan call, is reached through its check.  Exit code 0 and "ok" on success.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "jsgx.h"

static int failures = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("line %d: %s\n", __LINE__, #cond);               \
            ++failures;                                                  \
        }                                                                \
    } while (0)

template <class T>
static T* device(int k, int64_t bytes = 0) {       // device pointers that are never dereferenced: every call below is refused or planned
    return reinterpret_cast<T*>((uintptr_t(k) << 44) + bytes);
}

static const int kN = 1000, kF = 65, kM = 40, kS = 30;

static jsgx_sync_args good() {                 // 3 planes of 1000 frames of 65 features, 40 boundaries, 30 segments taken
    jsgx_sync_args a{};
    a.x = device<const float>(1), a.x_frame_pitch = kF + 3, a.x_pair_pitch = int64_t(kN) * (kF + 3) + 7;
    a.bounds = device<const int32_t>(2), a.bounds_pitch = kM + 2, a.n_bounds = device<const int32_t>(3);
    a.segments = device<int32_t>(4), a.segments_pitch = kS + 3, a.n_segments = device<int32_t>(5);
    a.out = device<float>(6), a.out_frame_pitch = kF + 1, a.out_pair_pitch = int64_t(kS) * (kF + 1) + 5;
    a.pairs = 3, a.n_frames = kN, a.n_features = kF, a.max_bounds = kM, a.bounds_all = 0, a.max_segments = kS, a.aggregate = JSGX_SYNC_MEDIAN, a.pad = 1;
    return a;
}

static jsgx_stack_memory_args good_stack() {
    jsgx_stack_memory_args a{};
    a.x = device<const float>(1), a.x_frame_pitch = kF + 3, a.x_pair_pitch = int64_t(kN) * (kF + 3) + 7;
    a.out = device<float>(6), a.out_frame_pitch = 5 * kF + 1, a.out_pair_pitch = int64_t(kN) * (5 * kF + 1) + 5;
    a.pairs = 3, a.n_frames = kN, a.n_features = kF, a.n_steps = 5, a.delay = -3, a.mode = JSGX_STACK_EDGE, a.fill = 1.5f;
    return a;
}

static bool passes(const jsgx_sync_args& a) { return jsgx_sync_plan(&a, nullptr, 0, nullptr, nullptr, nullptr) == JSGX_OK; }

static bool refused(const jsgx_sync_args& a, const char* text) {
    char want[192];
    std::snprintf(want, sizeof want, "jsgx_sync_plan: %s", text);
    if (!(jsgx_sync_plan(&a, nullptr, 0, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0)) return false;
#if defined(JSGX_SYNC_TEST_LAUNCHES)
    std::snprintf(want, sizeof want, "jsgx_sync_launch: %s", text);
    return jsgx_sync_launch(&a, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0;
#else
    return true;
#endif
}

#if defined(JSGX_SYNC_TEST_LAUNCHES)
static int stack_call(const jsgx_stack_memory_args* a) { return jsgx_stack_memory_launch(a, nullptr); }
static bool stack_passes(const jsgx_stack_memory_args&) { return true; }          // a launch that passes would run: not made here
#else
namespace jsgx {
int stack_memory_check(const jsgx_stack_memory_args* g, const char* who);
}
static int stack_call(const jsgx_stack_memory_args* a) { return jsgx::stack_memory_check(a, "jsgx_stack_memory_launch"); }
static bool stack_passes(const jsgx_stack_memory_args& a) { return stack_call(&a) == JSGX_OK; }
#endif

static bool stack_refused(const jsgx_stack_memory_args& a, const char* text) {
    char want[192];
    std::snprintf(want, sizeof want, "jsgx_stack_memory_launch: %s", text);
    return stack_call(&a) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0;
}

int main() {
    static_assert(sizeof(jsgx_sync_args) == 136 && sizeof(jsgx_stack_memory_args) == 80, "include/jsgx.h states the sizes");
    static_assert(JSGX_SYNC_MEAN == 0 && JSGX_SYNC_MIN == 1 && JSGX_SYNC_MAX == 2 && JSGX_SYNC_MEDIAN == 3, "include/jsgx.h");
    static_assert(4 * JSGX_SYNC_WAVE_MAX <= JSGX_SYNC_STAGE && JSGX_SYNC_LDS_TILE == 4 * 64 * JSGX_SYNC_STAGE && JSGX_SYNC_STAGE == 256 && JSGX_SYNC_THREADS == 256, "include/jsgx.h");
    static_assert(JSGX_SYNC_MAX_SEGMENTS == JSGX_SYNC_MAX_BOUNDS + 1 && JSGX_SYNC_MAX_FRAMES == (1 << 24), "include/jsgx.h");
    EXPECT(jsgx_abi_version() == 1);

    // the plan over shapes, dense planes
    static const char* const names[4] = {"sync_mean", "sync_min", "sync_max", "sync_median"};
    char name[16];
    for (int N : {1, 64, 1025, JSGX_SYNC_MAX_FRAMES})
        for (int F : {1, 65, JSGX_SYNC_MAX_FEATURES})
            for (int P : {1, 3, 65535})
                for (int M : {0, 1, 700, JSGX_SYNC_MAX_BOUNDS})
                    for (int pad : {0, 1})
                        for (int agg = 0; agg < 4; ++agg) {
                            jsgx_sync_args d{};
                            const int S = M + 2 * pad > 1 ? M + 2 * pad - 1 : 1;
                            // x spans up to 2^58 bytes, out up to 2^54: far apart, the two lists behind them
                            d.x = reinterpret_cast<const float*>(uintptr_t(1) << 40), d.x_frame_pitch = F, d.x_pair_pitch = int64_t(N) * F;
                            d.bounds = M ? device<const int32_t>(2) : nullptr, d.bounds_pitch = M, d.n_bounds = device<const int32_t>(3);
                            d.segments = reinterpret_cast<int32_t*>(uintptr_t(5) << 60), d.segments_pitch = S + 1, d.n_segments = reinterpret_cast<int32_t*>(uintptr_t(6) << 60);
                            d.out = reinterpret_cast<float*>(uintptr_t(1) << 62), d.out_frame_pitch = F, d.out_pair_pitch = int64_t(S) * F;
                            d.pairs = P, d.n_frames = N, d.n_features = F, d.max_bounds = M, d.max_segments = S, d.aggregate = agg, d.pad = pad;
                            int32_t threads = -1, lds = -1, launches = -1;
                            EXPECT(jsgx_sync_plan(&d, name, (int)sizeof name, &threads, &lds, &launches) == JSGX_OK);
                            EXPECT(std::strcmp(name, names[agg]) == 0 && threads == JSGX_SYNC_THREADS);
                            EXPECT(lds == JSGX_SYNC_LDS_BYTES + (agg == JSGX_SYNC_MEDIAN ? JSGX_SYNC_LDS_TILE : 0));
                            EXPECT(launches == (M + 2 * pad >= 2 ? 2 : 1));
                        }
    // planes more than 2^31 elements apart: the spans are 64-bit and more
    jsgx_sync_args d = good();
    d.x_pair_pitch = d.out_pair_pitch = d.segments_pitch = d.bounds_pitch = (int64_t(1) << 40) + 7;
    d.x = reinterpret_cast<const float*>(uintptr_t(1) << 50), d.out = reinterpret_cast<float*>(uintptr_t(1) << 58);
    EXPECT(passes(d));
    d.n_segments = reinterpret_cast<int32_t*>(const_cast<float*>(d.x) + 2 * d.x_pair_pitch + int64_t(kN - 1) * d.x_frame_pitch + kF - 1);
    EXPECT(refused(d, "n_segments overlaps x"));          // the last element of the third plane
    d.n_segments += 1;
    EXPECT(passes(d));

    d = good();
    EXPECT(passes(d));
    EXPECT(jsgx_sync_plan(&d, name, 15, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_sync_plan: bad argument") == 0);
    EXPECT(jsgx_sync_plan(nullptr, nullptr, 0, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_sync_plan: null argument") == 0);

    // one refusal of every kind, in the header's order
    d = good(); d.x = nullptr; EXPECT(refused(d, "null x"));
    d = good(); d.out = nullptr; EXPECT(refused(d, "null out"));
    d = good(); d.segments = nullptr; EXPECT(refused(d, "null segments"));
    d = good(); d.n_segments = nullptr; EXPECT(refused(d, "null n_segments"));
    d = good(); d.bounds = nullptr; EXPECT(refused(d, "null bounds with max_bounds > 0"));
    d = good(); d.bounds = nullptr; d.max_bounds = 0; EXPECT(passes(d));
    d = good(); d.x = device<const float>(1, 2); EXPECT(refused(d, "pointers must be 4-byte aligned"));
    d = good(); d.n_bounds = device<const int32_t>(3, 1); EXPECT(refused(d, "pointers must be 4-byte aligned"));
    d = good(); d.segments = device<int32_t>(4, 3); EXPECT(refused(d, "pointers must be 4-byte aligned"));
    for (int v : {0, -1, 65536}) { d = good(); d.pairs = v; EXPECT(refused(d, "pairs must be in 1..65535")); }
    for (int v : {0, -1, JSGX_SYNC_MAX_FRAMES + 1}) { d = good(); d.n_frames = v; EXPECT(refused(d, "n_frames must be in 1..16777216")); }
    for (int v : {0, -1, JSGX_SYNC_MAX_FEATURES + 1}) { d = good(); d.n_features = v; EXPECT(refused(d, "n_features must be in 1..65536")); }
    for (int v : {-1, JSGX_SYNC_MAX_BOUNDS + 1}) { d = good(); d.max_bounds = v; EXPECT(refused(d, "max_bounds must be in 0..1048576")); }
    for (int v : {-1, kM + 1}) { d = good(); d.n_bounds = nullptr; d.bounds_all = v; EXPECT(refused(d, "bounds_all must be in 0..max_bounds")); }
    d = good(); d.bounds_all = -5; EXPECT(passes(d));          // not looked at with n_bounds
    d = good(); d.n_bounds = nullptr; d.bounds_all = kM; EXPECT(passes(d));
    for (int v : {0, -1, JSGX_SYNC_MAX_SEGMENTS + 1}) { d = good(); d.max_segments = v; EXPECT(refused(d, "max_segments must be in 1..1048577")); }
    for (int v : {-1, 4}) { d = good(); d.aggregate = v; EXPECT(refused(d, "aggregate must be in 0..3")); }
    for (int v : {-1, 2}) { d = good(); d.pad = v; EXPECT(refused(d, "pad must be 0 or 1")); }
    d = good(); d.reserved0 = 1; EXPECT(refused(d, "reserved0 and reserved1 must be 0"));
    d = good(); d.reserved1 = -1; EXPECT(refused(d, "reserved0 and reserved1 must be 0"));
    d = good(); d.x_frame_pitch = kF - 1; EXPECT(refused(d, "x_frame_pitch smaller than n_features"));
    d = good(); d.x_pair_pitch -= 11; EXPECT(refused(d, "x_pair_pitch does not cover a plane"));
    d = good(); d.out_frame_pitch = kF - 1; EXPECT(refused(d, "out_frame_pitch smaller than n_features"));
    d = good(); d.out_pair_pitch = int64_t(kS - 1) * (kF + 1) + kF - 1; EXPECT(refused(d, "out_pair_pitch does not cover a plane"));
    d = good(); d.out_pair_pitch = int64_t(kS - 1) * (kF + 1) + kF; EXPECT(passes(d));
    d = good(); d.bounds_pitch = kM - 1; EXPECT(refused(d, "bounds_pitch neither 0 nor >= max_bounds"));
    d = good(); d.bounds_pitch = 0; EXPECT(passes(d));          // one list for every pair
    d = good(); d.segments_pitch = kS; EXPECT(refused(d, "segments_pitch smaller than max_segments + 1"));
    d = good(); d.segments_pitch = kS + 1; EXPECT(passes(d));
    const int64_t x_span = 2 * d.x_pair_pitch + int64_t(kN - 1) * (kF + 3) + kF, out_span = 2 * d.out_pair_pitch + int64_t(kS - 1) * (kF + 1) + kF;
    const int64_t b_span = 2 * (kM + 2) + kM, seg_span = 2 * (kS + 3) + kS + 1;
    d = good(); d.out = const_cast<float*>(d.x) + x_span - 1; EXPECT(refused(d, "out overlaps x"));
    d = good(); d.out = const_cast<float*>(d.x) + x_span; EXPECT(passes(d));
    d = good(); d.out = reinterpret_cast<float*>(const_cast<int32_t*>(d.bounds)) - out_span + 1; EXPECT(refused(d, "out overlaps bounds"));
    d = good(); d.out = reinterpret_cast<float*>(const_cast<int32_t*>(d.n_bounds)) + 2; EXPECT(refused(d, "out overlaps n_bounds"));
    d = good(); d.out = reinterpret_cast<float*>(const_cast<int32_t*>(d.n_bounds)) + 3; EXPECT(passes(d));
    d = good(); d.segments = reinterpret_cast<int32_t*>(const_cast<float*>(d.x)) + 11; EXPECT(refused(d, "segments overlaps x"));
    d = good(); d.segments = const_cast<int32_t*>(d.bounds) + b_span - 1; EXPECT(refused(d, "segments overlaps bounds"));
    d = good(); d.segments = const_cast<int32_t*>(d.bounds) + b_span; EXPECT(passes(d));
    d = good(); d.segments = const_cast<int32_t*>(d.n_bounds) - seg_span + 1; EXPECT(refused(d, "segments overlaps n_bounds"));
    d = good(); d.n_segments = reinterpret_cast<int32_t*>(const_cast<float*>(d.x)) - 2; EXPECT(refused(d, "n_segments overlaps x"));
    d = good(); d.n_segments = reinterpret_cast<int32_t*>(const_cast<float*>(d.x)) - 3; EXPECT(passes(d));
    d = good(); d.n_segments = const_cast<int32_t*>(d.bounds) + 5; EXPECT(refused(d, "n_segments overlaps bounds"));
    d = good(); d.n_segments = const_cast<int32_t*>(d.n_bounds); EXPECT(refused(d, "n_segments overlaps n_bounds"));
    d = good(); d.segments = reinterpret_cast<int32_t*>(d.out) + out_span - 1; EXPECT(refused(d, "out overlaps segments"));
    d = good(); d.n_segments = reinterpret_cast<int32_t*>(d.out) + 100; EXPECT(refused(d, "out overlaps n_segments"));
    d = good(); d.n_segments = d.segments + seg_span - 1; EXPECT(refused(d, "segments overlaps n_segments"));
    d = good(); d.n_segments = d.segments + seg_span; EXPECT(passes(d));
    // an earlier defect is the one reported
    d = good(); d.x = nullptr; d.pairs = 0; d.aggregate = 9; EXPECT(refused(d, "null x"));
    d = good(); d.bounds = nullptr; d.n_frames = 0; d.segments = device<int32_t>(4, 1); EXPECT(refused(d, "null bounds with max_bounds > 0"));
    d = good(); d.max_segments = 0; d.pad = 7; d.out_frame_pitch = 1; EXPECT(refused(d, "max_segments must be in 1..1048577"));
    d = good(); d.aggregate = 4; d.pad = 2; d.reserved0 = 1; EXPECT(refused(d, "aggregate must be in 0..3"));
    d = good(); d.x_pair_pitch = 1; d.segments_pitch = 1; d.n_segments = d.segments; EXPECT(refused(d, "x_pair_pitch does not cover a plane"));
    // one pair: the pair pitches are not looked at; the ends of the ranges
    d = good(); d.pairs = 1; d.x_pair_pitch = d.out_pair_pitch = d.bounds_pitch = d.segments_pitch = 0; EXPECT(passes(d));
    d = good(); d.max_bounds = JSGX_SYNC_MAX_BOUNDS; d.bounds_pitch = JSGX_SYNC_MAX_BOUNDS; d.max_segments = JSGX_SYNC_MAX_SEGMENTS; d.segments_pitch = JSGX_SYNC_MAX_SEGMENTS + 1;
    d.out_pair_pitch = int64_t(JSGX_SYNC_MAX_SEGMENTS) * (kF + 1); d.out = reinterpret_cast<float*>(uintptr_t(1) << 58); EXPECT(passes(d));

    // section 16
    jsgx_stack_memory_args k = good_stack();
    EXPECT(stack_passes(k));
    EXPECT(stack_call(nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_stack_memory_launch: null argument") == 0);
    k = good_stack(); k.x = nullptr; EXPECT(stack_refused(k, "null x"));
    k = good_stack(); k.out = nullptr; EXPECT(stack_refused(k, "null out"));
    k = good_stack(); k.out = device<float>(6, 2); EXPECT(stack_refused(k, "pointers must be 4-byte aligned"));
    for (int v : {0, 65536}) { k = good_stack(); k.pairs = v; EXPECT(stack_refused(k, "pairs must be in 1..65535")); }
    for (int v : {0, (1 << 24) + 1}) { k = good_stack(); k.n_frames = v; EXPECT(stack_refused(k, "n_frames must be in 1..16777216")); }
    for (int v : {0, 65537}) { k = good_stack(); k.n_features = v; EXPECT(stack_refused(k, "n_features must be in 1..65536")); }
    for (int v : {0, -1, JSGX_STACK_MAX_STEPS + 1}) { k = good_stack(); k.n_steps = v; EXPECT(stack_refused(k, "n_steps must be in 1..256")); }
    k = good_stack(); k.n_features = 65536; k.n_steps = 17; EXPECT(stack_refused(k, "n_steps * n_features must be at most 1048576"));
    for (int v : {0, JSGX_STACK_MAX_DELAY + 1, -JSGX_STACK_MAX_DELAY - 1}) { k = good_stack(); k.delay = v; EXPECT(stack_refused(k, "delay must be non-zero and within +-16777216")); }
    for (int v : {-1, 2}) { k = good_stack(); k.mode = v; EXPECT(stack_refused(k, "mode must be 0 or 1")); }
    k = good_stack(); k.reserved0 = 3; EXPECT(stack_refused(k, "reserved0 must be 0"));
    k = good_stack(); k.x_frame_pitch = kF - 1; EXPECT(stack_refused(k, "x_frame_pitch smaller than n_features"));
    k = good_stack(); k.x_pair_pitch = 5; EXPECT(stack_refused(k, "x_pair_pitch does not cover a plane"));
    k = good_stack(); k.out_frame_pitch = 5 * kF - 1; EXPECT(stack_refused(k, "out_frame_pitch smaller than n_steps * n_features"));
    k = good_stack(); k.out_pair_pitch = int64_t(kN - 1) * (5 * kF + 1) + 5 * kF - 1; EXPECT(stack_refused(k, "out_pair_pitch does not cover a plane"));
    k = good_stack(); k.out = const_cast<float*>(k.x) + x_span - 1; EXPECT(stack_refused(k, "out overlaps x"));
    k = good_stack(); k.out = const_cast<float*>(k.x) + x_span; EXPECT(stack_passes(k));
    k = good_stack(); k.x = nullptr; k.n_steps = 0; k.mode = 5; EXPECT(stack_refused(k, "null x"));
    k = good_stack(); k.delay = 0; k.mode = 5; k.out = const_cast<float*>(k.x); EXPECT(stack_refused(k, "delay must be non-zero and within +-16777216"));
    k = good_stack(); k.delay = JSGX_STACK_MAX_DELAY; k.n_steps = 256; k.n_features = 4096; k.x_frame_pitch = 4096; k.x_pair_pitch = int64_t(kN) * 4096;
    k.out_frame_pitch = 1 << 20; k.out_pair_pitch = int64_t(kN) << 20; k.out = reinterpret_cast<float*>(uintptr_t(1) << 58); EXPECT(stack_passes(k));

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
