// The host entry points of section 17 of libjsgx.so (include/jsgx.h) from C++: the plan and the scratch size over shapes up to the limits
// (the 64-bit arithmetic included: a scratch of 2^58 bytes, planes more than 2^31 elements apart) and the refusals with their texts in
// their order.  No launch that passes, so no device: built against libjsgx.so (CMake, jsg::jsgx; JSGX_AGGLO_TEST_LAUNCHES: the refusals
// through the launch too, and those of its scratch) or, for the sanitizers, together with csrc/jsgx_beat_host.cpp and
// csrc/jsgx_agglo_host.cpp themselves (tests/test_agglo_host.py: -fsanitize=address,undefined).  Exit code 0 and "ok" on success.
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

static const int kN = 1000, kF = 65, kM = 40, kS = 41, kOut = 90;

static jsgx_agglomerative_args good() {         // 3 planes of 1000 frames of 65 features, 40 boundaries and the two ends, 90 results taken
    jsgx_agglomerative_args a{};
    a.x = device<const float>(1), a.x_frame_pitch = kF + 3, a.x_pair_pitch = int64_t(kN) * (kF + 3) + 7;
    a.bounds = device<const int32_t>(2), a.bounds_pitch = kM + 2, a.n_bounds = device<const int32_t>(3);
    a.segments = device<int32_t>(4), a.segments_pitch = kS + 3, a.n_segments = device<int32_t>(5);
    a.out_bounds = device<int32_t>(6), a.out_pitch = kOut + 1, a.n_out = device<int32_t>(7);
    a.order = device<int32_t>(8), a.height = device<float>(9), a.tree_pitch = kN + 5;
    a.pairs = 3, a.n_frames = kN, a.n_features = kF, a.max_bounds = kM, a.bounds_all = 0, a.max_segments = kS, a.max_out = kOut, a.n_clusters = 4, a.pad = 1;
    return a;
}

static bool passes(const jsgx_agglomerative_args& a) { return jsgx_agglomerative_plan(&a, nullptr, 0, nullptr, nullptr, nullptr) == JSGX_OK; }

static bool refused(const jsgx_agglomerative_args& a, const char* text) {
    char want[192];
    std::snprintf(want, sizeof want, "jsgx_agglomerative_plan: %s", text);
    if (!(jsgx_agglomerative_plan(&a, nullptr, 0, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0)) return false;
    std::snprintf(want, sizeof want, "jsgx_agglomerative_scratch_bytes: %s", text);
    if (!(jsgx_agglomerative_scratch_bytes(&a) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0)) return false;
#if defined(JSGX_AGGLO_TEST_LAUNCHES)
    std::snprintf(want, sizeof want, "jsgx_agglomerative_launch: %s", text);
    return jsgx_agglomerative_launch(&a, device<void>(10), int64_t(1) << 40, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0;
#else
    return true;
#endif
}

#if defined(JSGX_AGGLO_TEST_LAUNCHES)
static bool scratch_refused(const jsgx_agglomerative_args& a, void* scratch, int64_t bytes, const char* text) {
    char want[192];
    std::snprintf(want, sizeof want, "jsgx_agglomerative_launch: %s", text);
    return jsgx_agglomerative_launch(&a, scratch, bytes, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0;
}
#endif

int main() {
    static_assert(sizeof(jsgx_agglomerative_args) == 160, "include/jsgx.h states the size");
    static_assert(JSGX_AGGLO_MAX_STRETCH == 16384 && JSGX_AGGLO_SHORT == 64 && JSGX_AGGLO_THREADS == 256 && JSGX_AGGLO_GROUP_THREADS == 64, "include/jsgx.h");
    static_assert(JSGX_AGGLO_LDS_LIMIT == 8 * JSGX_AGGLO_MAX_STRETCH + 8 * (JSGX_AGGLO_MAX_STRETCH / 64) && JSGX_AGGLO_LDS_LIMIT <= 163840, "include/jsgx.h");
    static_assert(JSGX_AGGLO_LDS_BYTES == 4 * 8 * JSGX_AGGLO_SHORT, "include/jsgx.h");
    EXPECT(jsgx_abi_version() == 1);

    // the plan and the scratch over shapes, dense planes
    char name[16];
    for (int N : {1, 64, 65, 1025, JSGX_AGGLO_MAX_STRETCH, JSGX_AGGLO_MAX_STRETCH + 1, JSGX_SYNC_MAX_FRAMES})
        for (int F : {1, 65, JSGX_SYNC_MAX_FEATURES})
            for (int P : {1, 3, 65535})
                for (int M : {0, 1, 700, JSGX_SYNC_MAX_BOUNDS})
                    for (int pad : {0, 1}) {
                        jsgx_agglomerative_args d{};
                        const int64_t most = M + 2 * pad - 1 < N ? M + 2 * pad - 1 : N;
                        const int S = most > 1 ? (int)most : 1;
                        d.x = reinterpret_cast<const float*>(uintptr_t(1) << 40), d.x_frame_pitch = F, d.x_pair_pitch = int64_t(N) * F;
                        d.bounds = M ? device<const int32_t>(2) : nullptr, d.bounds_pitch = M, d.n_bounds = M ? device<const int32_t>(3) : nullptr;
                        d.segments = reinterpret_cast<int32_t*>(uintptr_t(5) << 60), d.segments_pitch = S + 1, d.n_segments = reinterpret_cast<int32_t*>(uintptr_t(6) << 60);
                        d.out_bounds = reinterpret_cast<int32_t*>(uintptr_t(7) << 60), d.out_pitch = N, d.n_out = reinterpret_cast<int32_t*>(uintptr_t(9) << 60);
                        d.pairs = P, d.n_frames = N, d.n_features = F, d.max_bounds = M, d.max_segments = S, d.max_out = N, d.n_clusters = 3, d.pad = pad;
                        int32_t threads = -1, lds = -1, launches = -1;
                        const int rc = jsgx_agglomerative_plan(&d, name, (int)sizeof name, &threads, &lds, &launches);
                        if (M == 0 && pad == 1 && N > JSGX_AGGLO_MAX_STRETCH) {
                            EXPECT(rc == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_agglomerative_plan: n_frames above 16384 without boundaries") == 0);
                            continue;
                        }
                        EXPECT(rc == JSGX_OK);
                        const int64_t L = N < JSGX_AGGLO_MAX_STRETCH ? N : JSGX_AGGLO_MAX_STRETCH, stretches = most > 0 ? most : 0;
                        if (N <= JSGX_AGGLO_SHORT)
                            EXPECT(std::strcmp(name, "agglo_wave") == 0 && threads == JSGX_AGGLO_THREADS && lds == JSGX_AGGLO_LDS_BYTES && launches == (stretches ? 4 : 2));
                        else
                            EXPECT(std::strcmp(name, "agglo_group") == 0 && threads == JSGX_AGGLO_GROUP_THREADS && lds == 8 * L + 8 * ((L + 63) / 64) &&
                                   launches == (stretches ? 5 : 2));
                        EXPECT(lds <= JSGX_AGGLO_LDS_LIMIT);
                        const int64_t votes = (int64_t(N) + JSGX_AGGLO_COPY_FRAMES - 1) / JSGX_AGGLO_COPY_FRAMES;
                        EXPECT(jsgx_agglomerative_scratch_bytes(&d) == 4 * int64_t(P) * (int64_t(N) * F + N + votes + stretches + 1));
                    }
    // planes more than 2^31 elements apart: the spans are 64-bit and more
    jsgx_agglomerative_args d = good();
    d.x_pair_pitch = d.out_pitch = d.segments_pitch = d.bounds_pitch = d.tree_pitch = (int64_t(1) << 40) + 7;
    d.x = reinterpret_cast<const float*>(uintptr_t(1) << 50), d.out_bounds = reinterpret_cast<int32_t*>(uintptr_t(1) << 58);
    d.order = reinterpret_cast<int32_t*>(uintptr_t(1) << 59), d.height = reinterpret_cast<float*>(uintptr_t(1) << 60);
    EXPECT(passes(d));
    d.n_segments = reinterpret_cast<int32_t*>(const_cast<float*>(d.x) + 2 * d.x_pair_pitch + int64_t(kN - 1) * d.x_frame_pitch + kF - 1);
    EXPECT(refused(d, "n_segments overlaps x"));          // the last element of the third plane
    d.n_segments += 1;
    EXPECT(passes(d));

    d = good();
    EXPECT(passes(d));
    EXPECT(jsgx_agglomerative_plan(&d, name, 15, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_agglomerative_plan: bad argument") == 0);
    EXPECT(jsgx_agglomerative_plan(nullptr, nullptr, 0, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID &&
           std::strcmp(jsgx_last_error(), "jsgx_agglomerative_plan: null argument") == 0);
    EXPECT(jsgx_agglomerative_scratch_bytes(nullptr) == JSGX_ERR_INVALID);

    // one refusal of every kind, in the header's order
    d = good(); d.x = nullptr; EXPECT(refused(d, "null x"));
    d = good(); d.segments = nullptr; EXPECT(refused(d, "null segments"));
    d = good(); d.n_segments = nullptr; EXPECT(refused(d, "null n_segments"));
    d = good(); d.out_bounds = nullptr; EXPECT(refused(d, "null out_bounds"));
    d = good(); d.n_out = nullptr; EXPECT(refused(d, "null n_out"));
    d = good(); d.bounds = nullptr; EXPECT(refused(d, "null bounds with max_bounds > 0"));
    d = good(); d.order = nullptr; EXPECT(refused(d, "order and height go together"));
    d = good(); d.height = nullptr; EXPECT(refused(d, "order and height go together"));
    d = good(); d.order = nullptr; d.height = nullptr; EXPECT(passes(d));
    d = good(); d.x = device<const float>(1, 2); EXPECT(refused(d, "pointers must be 4-byte aligned"));
    d = good(); d.n_bounds = device<const int32_t>(3, 1); EXPECT(refused(d, "pointers must be 4-byte aligned"));
    d = good(); d.height = device<float>(9, 3); EXPECT(refused(d, "pointers must be 4-byte aligned"));
    for (int v : {0, -1, 65536}) { d = good(); d.pairs = v; EXPECT(refused(d, "pairs must be in 1..65535")); }
    for (int v : {0, -1, JSGX_SYNC_MAX_FRAMES + 1}) { d = good(); d.n_frames = v; EXPECT(refused(d, "n_frames must be in 1..16777216")); }
    for (int v : {0, -1, JSGX_SYNC_MAX_FEATURES + 1}) { d = good(); d.n_features = v; EXPECT(refused(d, "n_features must be in 1..65536")); }
    for (int v : {-1, JSGX_SYNC_MAX_BOUNDS + 1}) { d = good(); d.max_bounds = v; EXPECT(refused(d, "max_bounds must be in 0..1048576")); }
    for (int v : {-1, kM + 1}) { d = good(); d.n_bounds = nullptr; d.bounds_all = v; EXPECT(refused(d, "bounds_all must be in 0..max_bounds")); }
    d = good(); d.bounds_all = -5; EXPECT(passes(d));          // not looked at with n_bounds
    d = good(); d.n_bounds = nullptr; d.bounds_all = kM; EXPECT(passes(d));
    for (int v : {0, -1, JSGX_SYNC_MAX_SEGMENTS + 1}) { d = good(); d.max_segments = v; EXPECT(refused(d, "max_segments must be in 1..1048577")); }
    for (int v : {0, -1, JSGX_AGGLO_MAX_OUT + 1}) { d = good(); d.max_out = v; EXPECT(refused(d, "max_out must be in 1..16777216")); }
    for (int v : {0, -1}) { d = good(); d.n_clusters = v; EXPECT(refused(d, "n_clusters must be at least 1")); }
    d = good(); d.n_clusters = 2147483647; EXPECT(passes(d));
    for (int v : {-1, 2}) { d = good(); d.pad = v; EXPECT(refused(d, "pad must be 0 or 1")); }
    d = good(); d.reserved0 = 1; EXPECT(refused(d, "reserved0 must be 0"));
    d = good(); d.max_segments = kS - 1; EXPECT(refused(d, "max_segments smaller than the stretches the list can give"));
    d = good(); d.pad = 0; d.max_segments = kM - 1; EXPECT(passes(d));
    d = good(); d.n_bounds = nullptr; d.bounds_all = 3; d.max_segments = 4; EXPECT(passes(d));          // the count on the host decides
    d = good(); d.n_bounds = nullptr; d.bounds_all = 0; d.n_frames = JSGX_AGGLO_MAX_STRETCH + 1; d.x_pair_pitch = int64_t(d.n_frames) * (kF + 3); d.tree_pitch = d.n_frames;
    EXPECT(refused(d, "n_frames above 16384 without boundaries"));
    d.pad = 0; EXPECT(passes(d));          // no stretch at all
    d.pad = 1; d.n_frames = JSGX_AGGLO_MAX_STRETCH; EXPECT(passes(d));
    d = good(); d.x_frame_pitch = kF - 1; EXPECT(refused(d, "x_frame_pitch smaller than n_features"));
    d = good(); d.x_pair_pitch -= 11; EXPECT(refused(d, "x_pair_pitch does not cover a plane"));
    d = good(); d.bounds_pitch = kM - 1; EXPECT(refused(d, "bounds_pitch neither 0 nor >= max_bounds"));
    d = good(); d.bounds_pitch = 0; EXPECT(passes(d));          // one list for every pair
    d = good(); d.segments_pitch = kS; EXPECT(refused(d, "segments_pitch smaller than max_segments + 1"));
    d = good(); d.segments_pitch = kS + 1; EXPECT(passes(d));
    d = good(); d.out_pitch = kOut - 1; EXPECT(refused(d, "out_pitch smaller than max_out"));
    d = good(); d.out_pitch = kOut; EXPECT(passes(d));
    d = good(); d.tree_pitch = kN - 1; EXPECT(refused(d, "tree_pitch smaller than n_frames"));
    d = good(); d.tree_pitch = 0; d.order = nullptr; d.height = nullptr; EXPECT(passes(d));
    const int64_t x_span = 2 * d.x_pair_pitch + int64_t(kN - 1) * (kF + 3) + kF, out_span = 2 * (kOut + 1) + kOut, tree_span = 2 * (kN + 5) + kN;
    const int64_t b_span = 2 * (kM + 2) + kM, seg_span = 2 * (kS + 3) + kS + 1;
    d = good(); d.out_bounds = reinterpret_cast<int32_t*>(const_cast<float*>(d.x)) + x_span - 1; EXPECT(refused(d, "out_bounds overlaps x"));
    d = good(); d.out_bounds = reinterpret_cast<int32_t*>(const_cast<float*>(d.x)) + x_span; EXPECT(passes(d));
    d = good(); d.out_bounds = const_cast<int32_t*>(d.bounds) - out_span + 1; EXPECT(refused(d, "out_bounds overlaps bounds"));
    d = good(); d.out_bounds = const_cast<int32_t*>(d.n_bounds) + 2; EXPECT(refused(d, "out_bounds overlaps n_bounds"));
    d = good(); d.out_bounds = const_cast<int32_t*>(d.n_bounds) + 3; EXPECT(passes(d));
    d = good(); d.n_out = const_cast<int32_t*>(d.bounds) + b_span - 1; EXPECT(refused(d, "n_out overlaps bounds"));
    d = good(); d.n_out = const_cast<int32_t*>(d.bounds) + b_span; EXPECT(passes(d));
    d = good(); d.segments = reinterpret_cast<int32_t*>(const_cast<float*>(d.x)) + 11; EXPECT(refused(d, "segments overlaps x"));
    d = good(); d.segments = const_cast<int32_t*>(d.n_bounds) - seg_span + 1; EXPECT(refused(d, "segments overlaps n_bounds"));
    d = good(); d.n_segments = const_cast<int32_t*>(d.n_bounds); EXPECT(refused(d, "n_segments overlaps n_bounds"));
    d = good(); d.order = reinterpret_cast<int32_t*>(const_cast<float*>(d.x)) - tree_span + 1; EXPECT(refused(d, "order overlaps x"));
    d = good(); d.order = reinterpret_cast<int32_t*>(const_cast<float*>(d.x)) - tree_span; EXPECT(passes(d));
    d = good(); d.height = reinterpret_cast<float*>(const_cast<int32_t*>(d.bounds)) + 5; EXPECT(refused(d, "height overlaps bounds"));
    d = good(); d.n_out = d.out_bounds + out_span - 1; EXPECT(refused(d, "out_bounds overlaps n_out"));
    d = good(); d.n_out = d.out_bounds + out_span; EXPECT(passes(d));
    d = good(); d.segments = d.out_bounds + 7; EXPECT(refused(d, "out_bounds overlaps segments"));
    d = good(); d.n_segments = d.n_out + 2; EXPECT(refused(d, "n_out overlaps n_segments"));
    d = good(); d.n_segments = d.n_out + 3; EXPECT(passes(d));
    d = good(); d.n_segments = d.segments + seg_span - 1; EXPECT(refused(d, "segments overlaps n_segments"));
    d = good(); d.order = d.segments - tree_span + 1; EXPECT(refused(d, "segments overlaps order"));
    d = good(); d.height = reinterpret_cast<float*>(d.n_segments) + 1; EXPECT(refused(d, "n_segments overlaps height"));
    d = good(); d.height = reinterpret_cast<float*>(d.order) + tree_span - 1; EXPECT(refused(d, "order overlaps height"));
    d = good(); d.height = reinterpret_cast<float*>(d.order) + tree_span; EXPECT(passes(d));
    // an earlier defect is the one reported
    d = good(); d.x = nullptr; d.pairs = 0; d.n_clusters = 0; EXPECT(refused(d, "null x"));
    d = good(); d.order = nullptr; d.n_frames = 0; d.segments = device<int32_t>(4, 1); EXPECT(refused(d, "order and height go together"));
    d = good(); d.max_out = 0; d.pad = 7; d.x_frame_pitch = 1; EXPECT(refused(d, "max_out must be in 1..16777216"));
    d = good(); d.n_clusters = 0; d.pad = 2; d.reserved0 = 1; d.max_segments = 1; EXPECT(refused(d, "n_clusters must be at least 1"));
    d = good(); d.max_segments = 1; d.x_pair_pitch = 1; EXPECT(refused(d, "max_segments smaller than the stretches the list can give"));
    d = good(); d.x_pair_pitch = 1; d.segments_pitch = 1; d.n_segments = d.segments; EXPECT(refused(d, "x_pair_pitch does not cover a plane"));
    // one pair: the pair pitches are not looked at; the ends of the ranges
    d = good(); d.pairs = 1; d.x_pair_pitch = d.out_pitch = d.bounds_pitch = d.segments_pitch = d.tree_pitch = 0; EXPECT(passes(d));
    d = good(); d.max_bounds = JSGX_SYNC_MAX_BOUNDS; d.bounds_pitch = JSGX_SYNC_MAX_BOUNDS; d.max_segments = JSGX_SYNC_MAX_SEGMENTS; d.segments_pitch = JSGX_SYNC_MAX_SEGMENTS + 1;
    d.segments = reinterpret_cast<int32_t*>(uintptr_t(1) << 58); d.max_out = JSGX_AGGLO_MAX_OUT; d.out_pitch = JSGX_AGGLO_MAX_OUT; d.out_bounds = reinterpret_cast<int32_t*>(uintptr_t(1) << 59);
    EXPECT(passes(d));

#if defined(JSGX_AGGLO_TEST_LAUNCHES)
    // the scratch, behind every other refusal
    d = good();
    const int64_t need = jsgx_agglomerative_scratch_bytes(&d);
    EXPECT(need == 4 * int64_t(3) * (int64_t(kN) * kF + kN + (kN + 63) / 64 + kS + 1));
    EXPECT(scratch_refused(d, nullptr, need, "null scratch"));
    EXPECT(scratch_refused(d, device<void>(10, 2), need, "scratch must be 4-byte aligned"));
    EXPECT(scratch_refused(d, device<void>(10), need - 1, "scratch smaller than jsgx_agglomerative_scratch_bytes"));
    EXPECT(scratch_refused(d, const_cast<float*>(d.x) + x_span - 1, need, "scratch overlaps x"));
    EXPECT(scratch_refused(d, reinterpret_cast<char*>(const_cast<int32_t*>(d.bounds)) - need + 4, need, "scratch overlaps bounds"));
    EXPECT(scratch_refused(d, d.n_out + 2, need, "scratch overlaps n_out"));
    EXPECT(scratch_refused(d, d.segments + seg_span - 1, need, "scratch overlaps segments"));
    EXPECT(scratch_refused(d, reinterpret_cast<char*>(d.height) - need + 4, need, "scratch overlaps height"));
    d.x = nullptr;
    EXPECT(scratch_refused(d, nullptr, 0, "null x"));
#endif

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
