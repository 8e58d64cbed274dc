// The host entry points of section 12 of libjsgx.so (include/jsgx.h) from C++: the plan, the scratch arithmetic and the refusals with
// their texts in their order.  No launch that passes, so no device: built against libjsgx.so (CMake, jsg::jsgx) or, for the sanitizers,
// together with csrc/jsgx_beat_host.cpp and csrc/jsgx_nmf_host.cpp themselves (tests/test_nmf_host.py: -fsanitize=address,undefined).
// Exit code 0 and "ok" on success.
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
static T* device(int k, int bytes = 0) {       // device pointers that are never dereferenced: every call below is refused or planned
    return reinterpret_cast<T*>((uintptr_t(k) << 44) + bytes);
}

static jsgx_nmf_args good() {                  // 3 problems of 100 frames x 300 bins, 7 components
    jsgx_nmf_args a{};
    a.v = device<const float>(1);
    a.v_pitch = 300;
    a.v_problem_pitch = 100 * 300;
    a.a = device<float>(2);
    a.a_pitch = 8;
    a.a_problem_pitch = 100 * 8;
    a.c = device<float>(3);
    a.c_pitch = 304;
    a.c_problem_pitch = 7 * 304;
    a.problems = 3;
    a.n_frames = 100;
    a.n_bins = 300;
    a.n_components = 7;
    a.n_iter = 5;
    a.update_components = 1;
    a.loss = JSGX_NMF_FROBENIUS;
    return a;
}

static bool refused(const jsgx_nmf_args& a, const char* text) {
    char want[192];
    std::snprintf(want, sizeof want, "jsgx_nmf_plan: %s", text);
    if (!(jsgx_nmf_plan(&a, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0)) return false;
    std::snprintf(want, sizeof want, "jsgx_nmf_scratch_bytes: %s", text);
    return jsgx_nmf_scratch_bytes(&a) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0;
}

static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

#if defined(JSGX_NMF_TEST_LAUNCHES)
static bool launch_refused(const jsgx_nmf_args& a, void* scratch, int64_t bytes, const char* text) {
    char want[192];
    std::snprintf(want, sizeof want, "jsgx_nmf_launch: %s", text);
    return jsgx_nmf_launch(&a, scratch, bytes, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0;
}
#endif

int main() {
    static_assert(sizeof(jsgx_nmf_args) == 104, "include/jsgx.h states the size");
    static_assert(JSGX_NMF_CHUNK_K % 4 == 0 && JSGX_NMF_CHUNK_T % 4 == 0, "include/jsgx.h: multiples of 4");
    EXPECT(jsgx_abi_version() == 1);

    // the plan and the scratch over shapes
    char name[16];
    for (int T : {1, 100, JSGX_NMF_CHUNK_T, JSGX_NMF_CHUNK_T + 1, 16384, JSGX_NMF_MAX_FRAMES})
        for (int K : {1, 300, JSGX_NMF_CHUNK_K, JSGX_NMF_CHUNK_K + 1, JSGX_NMF_MAX_BINS})
            for (int r : {1, 7, 64})
                for (int P : {1, 3, 65535})
                    for (int update : {0, 1}) {
                        jsgx_nmf_args d = good();
                        d.n_frames = T, d.n_bins = K, d.n_components = r, d.problems = P, d.update_components = update;
                        // the largest planes span 2^56, 2^48 and 2^38 bytes: far apart
                        d.v = reinterpret_cast<const float*>(uintptr_t(1) << 58), d.a = reinterpret_cast<float*>(uintptr_t(1) << 50), d.c = reinterpret_cast<float*>(uintptr_t(1) << 40);
                        d.v_pitch = K, d.v_problem_pitch = (int64_t)T * K, d.a_pitch = r, d.a_problem_pitch = (int64_t)T * r, d.c_pitch = K, d.c_problem_pitch = (int64_t)r * K;
                        int32_t threads = 0, lds = 0, launches = 0, chunks = 0;
                        EXPECT(jsgx_nmf_plan(&d, name, (int)sizeof name, &threads, &lds, &launches, &chunks) == JSGX_OK);
                        const int64_t cK = ceil_div(K, JSGX_NMF_CHUNK_K), cT = ceil_div(T, JSGX_NMF_CHUNK_T);
                        EXPECT(std::strcmp(name, "nmf_update_a") == 0 && threads == JSGX_NMF_THREADS && lds == JSGX_NMF_LDS_BYTES);
                        EXPECT(launches == (update ? 8 : 1) && chunks == cT);
                        const int64_t want = update ? 4 * (int64_t)P * r * (r * (2 + (cK > cT ? cK : cT)) + cT * K) : 4 * (int64_t)P * r * r * (2 + cK);
                        EXPECT(jsgx_nmf_scratch_bytes(&d) == want && want > 0);
                    }
    jsgx_nmf_args d = good();
    EXPECT(jsgx_nmf_scratch_bytes(&d) == 27552);
    EXPECT(jsgx_nmf_plan(&d, name, 15, nullptr, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_nmf_plan: bad argument") == 0);
    EXPECT(jsgx_nmf_plan(nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_nmf_plan: null argument") == 0);
    EXPECT(jsgx_nmf_scratch_bytes(nullptr) == JSGX_ERR_INVALID);

    // one refusal of every kind, in the header's order
    d = good(); d.v = nullptr; EXPECT(refused(d, "null v"));
    d = good(); d.a = nullptr; EXPECT(refused(d, "null a"));
    d = good(); d.c = nullptr; EXPECT(refused(d, "null c"));
    d = good(); d.v = device<const float>(1, 2); EXPECT(refused(d, "pointers must be 4-byte aligned"));
    d = good(); d.c = device<float>(3, 1); EXPECT(refused(d, "pointers must be 4-byte aligned"));
    d = good(); d.problems = 0; EXPECT(refused(d, "problems must be in 1..65535"));
    d = good(); d.problems = 65536; EXPECT(refused(d, "problems must be in 1..65535"));
    d = good(); d.n_frames = 0; EXPECT(refused(d, "n_frames must be in 1..16777216"));
    d = good(); d.n_frames = JSGX_NMF_MAX_FRAMES + 1; EXPECT(refused(d, "n_frames must be in 1..16777216"));
    d = good(); d.n_bins = 0; EXPECT(refused(d, "n_bins must be in 1..16384"));
    d = good(); d.n_bins = JSGX_NMF_MAX_BINS + 1; EXPECT(refused(d, "n_bins must be in 1..16384"));
    d = good(); d.n_components = 0; EXPECT(refused(d, "n_components must be in 1..64"));
    d = good(); d.n_components = 65; EXPECT(refused(d, "n_components must be in 1..64"));
    d = good(); d.n_iter = 0; EXPECT(refused(d, "n_iter must be in 1..65536"));
    d = good(); d.n_iter = 65537; EXPECT(refused(d, "n_iter must be in 1..65536"));
    d = good(); d.update_components = 2; EXPECT(refused(d, "update_components must be 0 or 1"));
    d = good(); d.loss = 1; EXPECT(refused(d, "loss must be JSGX_NMF_FROBENIUS"));
    d = good(); d.reserved0 = 1; EXPECT(refused(d, "reserved0 must be 0"));
    d = good(); d.v_pitch = 299; EXPECT(refused(d, "v_pitch smaller than n_bins"));
    d = good(); d.v_problem_pitch = 29999; EXPECT(refused(d, "v_problem_pitch does not cover a plane"));
    d = good(); d.a_pitch = 6; EXPECT(refused(d, "a_pitch smaller than n_components"));
    d = good(); d.a_problem_pitch = 99 * 8 + 6; EXPECT(refused(d, "a_problem_pitch does not cover a plane"));
    d = good(); d.c_pitch = 299; EXPECT(refused(d, "c_pitch smaller than n_bins"));
    d = good(); d.c_problem_pitch = 6 * 304 + 299; EXPECT(refused(d, "c_problem_pitch does not cover a plane"));
    d = good(); d.a = const_cast<float*>(d.v) + 89999; EXPECT(refused(d, "a overlaps v"));
    d = good(); d.a = const_cast<float*>(d.v) + 90000; EXPECT(jsgx_nmf_scratch_bytes(&d) == 27552);
    d = good(); d.c = const_cast<float*>(d.v) - (2 * 7 * 304 + 6 * 304 + 300) + 1; EXPECT(refused(d, "c overlaps v"));
    d = good(); d.c = const_cast<float*>(d.v) - (2 * 7 * 304 + 6 * 304 + 300); EXPECT(jsgx_nmf_scratch_bytes(&d) == 27552);
    d = good(); d.a = d.c + 10; EXPECT(refused(d, "a overlaps c"));
    // an earlier defect is the one reported
    d = good(); d.v = nullptr; d.problems = 0; d.loss = 7; EXPECT(refused(d, "null v"));
    d = good(); d.n_bins = 0; d.n_iter = 0; d.v_pitch = -1; EXPECT(refused(d, "n_bins must be in 1..16384"));
    d = good(); d.loss = 3; d.c_pitch = 1; d.a = d.c; EXPECT(refused(d, "loss must be JSGX_NMF_FROBENIUS"));
    // one problem: the problem pitches are not looked at
    d = good(); d.problems = 1; d.v_problem_pitch = d.a_problem_pitch = d.c_problem_pitch = 0; EXPECT(jsgx_nmf_scratch_bytes(&d) == 27552 / 3);

#if defined(JSGX_NMF_TEST_LAUNCHES)
    // the launch's refusals, decided before any device call (the shipped library only: the launcher is a HIP unit)
    float* scratch = device<float>(4);
    EXPECT(jsgx_nmf_launch(nullptr, scratch, 27552, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_nmf_launch: null argument") == 0);
    d = good(); d.c = nullptr; EXPECT(launch_refused(d, scratch, 27552, "null c"));
    d = good(); d.a = d.c + 10; EXPECT(launch_refused(d, nullptr, 0, "a overlaps c"));
    d = good();
    EXPECT(launch_refused(d, nullptr, 27552, "null scratch"));
    EXPECT(launch_refused(d, device<float>(4, 2), 27552, "scratch must be 4-byte aligned"));
    EXPECT(launch_refused(d, scratch, 27551, "scratch smaller than jsgx_nmf_scratch_bytes"));
    EXPECT(launch_refused(d, const_cast<float*>(d.v) + 89999, 27552, "scratch overlaps v"));
    EXPECT(launch_refused(d, d.a - 27552 / 4 + 1, 1 << 20, "scratch overlaps a"));
    EXPECT(launch_refused(d, d.c + 2 * 7 * 304 + 6 * 304 + 299, 27552, "scratch overlaps c"));
    EXPECT(launch_refused(d, device<float>(4, 1), 0, "scratch must be 4-byte aligned"));        // the earlier defect
#endif

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
