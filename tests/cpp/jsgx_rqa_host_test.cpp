// The host entry points of section 9 of libjsgx.so (include/jsgx.h) from C++: the plan, the scratch size and the refusals with their texts,
// in their order.  No launch, so no device: built against libjsgx.so (CMake, jsg::jsgx) or, for the sanitizers, together with
// csrc/jsgx_beat_host.cpp and csrc/jsgx_rqa_host.cpp themselves (tests/test_rqa_host.py: -fsanitize=address,undefined).  Exit code 0 and
// "ok" on success.
#include <cmath>
#include <cstdint>
#include <cstdio>
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
static T* device(int k, int bytes = 0) {       // device pointers that are never dereferenced: every call below is refused, sized or planned
    return reinterpret_cast<T*>((uintptr_t(k) << 44) + bytes);
}

static jsgx_rqa_args good() {                  // 3 pairs of 100 x 300, every output
    jsgx_rqa_args a{};
    a.sim = device<const float>(1);
    a.sim_pitch = 300;
    a.sim_pair_pitch = 100 * 300;
    a.pairs = 3;
    a.n = 100;
    a.m = 300;
    a.knight = 1;
    a.gap_onset = 1.f;
    a.gap_extend = 0.5f;
    a.max_path = 100;
    a.score = device<float>(2);
    a.score_pitch = 304;
    a.score_pair_pitch = 100 * 304;
    a.step = device<int8_t>(3);
    a.step_pitch = 301;
    a.step_pair_pitch = 100 * 301;
    a.path_i = device<int32_t>(4);
    a.path_j = device<int32_t>(5);
    a.path_pitch = 100;
    a.path_len = device<int32_t>(6);
    a.end = device<int32_t>(7);
    a.total = device<float>(8);
    return a;
}

static bool refused(const jsgx_rqa_args& a, const char* text) {
    char want[192];
    std::snprintf(want, sizeof want, "jsgx_rqa_scratch_bytes: %s", text);
    if (jsgx_rqa_scratch_bytes(&a) != JSGX_ERR_INVALID || std::strcmp(jsgx_last_error(), want) != 0) return false;
    std::snprintf(want, sizeof want, "jsgx_rqa_plan: %s", text);
    return jsgx_rqa_plan(&a, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0;
}

int main() {
    static_assert(sizeof(jsgx_rqa_args) == 152, "include/jsgx.h states the size");
    EXPECT(jsgx_abi_version() == 1);

    // the plan and the scratch over shapes
    jsgx_rqa_args d = good();
    char name[16];
    int32_t rows = 0, cols = 0, launches = 0, threads = 0, lds = 0;
    EXPECT(jsgx_rqa_plan(&d, name, (int)sizeof name, &rows, &cols, &launches, &threads, &lds) == JSGX_OK);
    EXPECT(std::strcmp(name, "rqa_tiles") == 0 && rows == JSGX_DTW_TILE_ROWS && cols == JSGX_DTW_TILE_COLS && threads == JSGX_RQA_THREADS);
    EXPECT(lds == JSGX_RQA_LDS_BYTES && lds <= 163840 && launches == 2 + 5 - 1 + 1);
    EXPECT(jsgx_rqa_scratch_bytes(&d) == 8 * 3 * (2 * 5) + 8 * 3 * 100);
    for (int n : {1, 63, 64, 65, 4096, JSGX_DTW_MAX_LEN})
        for (int m : {1, 63, 64, 65, 4096, JSGX_DTW_MAX_LEN}) {
            const int64_t ti = (n + 63) / 64, tj = (m + 63) / 64, shortest = n < m ? n : m;
            d = good();
            d.n = n, d.m = m, d.pairs = 1, d.sim_pitch = d.score_pitch = d.step_pitch = m, d.max_path = (int32_t)shortest;
            EXPECT(jsgx_rqa_plan(&d, nullptr, 0, nullptr, nullptr, &launches, nullptr, nullptr) == JSGX_OK && launches == ti + tj);
            EXPECT(jsgx_rqa_scratch_bytes(&d) == 8 * ti * tj + 8 * shortest);
            d.path_i = d.path_j = nullptr, d.max_path = 0;                     // the end cell without paths: the tiles' entries alone
            EXPECT(jsgx_rqa_scratch_bytes(&d) == 8 * ti * tj);
            d.path_len = nullptr, d.total = nullptr;                           // ... asked for by any of path_len, end and total
            EXPECT(jsgx_rqa_scratch_bytes(&d) == 8 * ti * tj);
            d.end = nullptr;                                                   // the score (and the steps) alone
            EXPECT(jsgx_rqa_plan(&d, nullptr, 0, nullptr, nullptr, &launches, nullptr, nullptr) == JSGX_OK && launches == ti + tj - 1);
            EXPECT(jsgx_rqa_scratch_bytes(&d) == 0);
        }
    d = good();
    EXPECT(jsgx_rqa_plan(&d, name, 15, nullptr, nullptr, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_rqa_plan: bad argument") == 0);
    EXPECT(jsgx_rqa_scratch_bytes(nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_rqa_scratch_bytes: null argument") == 0);

    // one refusal of every kind, in the header's order
    d = good(); d.sim = nullptr; EXPECT(refused(d, "null sim"));
    d = good(); d.score = nullptr; EXPECT(refused(d, "null score"));
    d = good(); d.path_j = nullptr; EXPECT(refused(d, "path_i and path_j go together"));
    d = good(); d.path_len = nullptr; EXPECT(refused(d, "null path_len with paths"));
    d = good(); d.end = device<int32_t>(7, 2); EXPECT(refused(d, "pointers must be 4-byte aligned"));
    d = good(); d.step = device<int8_t>(3, 1); EXPECT(jsgx_rqa_scratch_bytes(&d) > 0);        // a plane of bytes
    d = good(); d.pairs = 0; EXPECT(refused(d, "pairs must be in 1..65535"));
    d = good(); d.n = 65537; EXPECT(refused(d, "n must be in 1..65536"));
    d = good(); d.m = 0; EXPECT(refused(d, "m must be in 1..65536"));
    d = good(); d.knight = 2; EXPECT(refused(d, "knight must be 0 or 1"));
    d = good(); d.gap_onset = -0.5f; EXPECT(refused(d, "gap_onset must be finite and >= 0"));
    d = good(); d.gap_onset = NAN; EXPECT(refused(d, "gap_onset must be finite and >= 0"));
    d = good(); d.gap_extend = INFINITY; EXPECT(refused(d, "gap_extend must be finite and >= 0"));
    d = good(); d.gap_onset = d.gap_extend = 0.f; EXPECT(jsgx_rqa_scratch_bytes(&d) > 0);
    d = good(); d.reserved0 = 1; EXPECT(refused(d, "reserved0 must be 0"));
    d = good(); d.max_path = 99; d.path_pitch = 99; EXPECT(refused(d, "max_path smaller than min(n, m)"));
    d = good(); d.sim_pitch = 299; EXPECT(refused(d, "sim_pitch smaller than m"));
    d = good(); d.sim_pair_pitch = 29999; EXPECT(refused(d, "sim_pair_pitch does not cover a plane"));
    d = good(); d.score_pitch = 1; EXPECT(refused(d, "score_pitch smaller than m"));
    d = good(); d.score_pair_pitch = 99 * 304 + 299; EXPECT(refused(d, "score_pair_pitch does not cover a plane"));
    d = good(); d.step_pitch = 299; EXPECT(refused(d, "step_pitch smaller than m"));
    d = good(); d.step_pair_pitch = 99 * 301 + 299; EXPECT(refused(d, "step_pair_pitch does not cover a plane"));
    d = good(); d.step = nullptr; d.step_pitch = d.step_pair_pitch = 0; EXPECT(jsgx_rqa_scratch_bytes(&d) > 0);
    d = good(); d.path_pitch = 99; EXPECT(refused(d, "path_pitch smaller than max_path"));
    d = good(); d.score = const_cast<float*>(d.sim) + 89999; EXPECT(refused(d, "score overlaps sim"));
    d = good(); d.score = const_cast<float*>(d.sim) + 90000; EXPECT(jsgx_rqa_scratch_bytes(&d) > 0);
    d = good(); d.step = reinterpret_cast<int8_t*>(const_cast<float*>(d.sim)) + 4 * 89999 + 3; EXPECT(refused(d, "an output overlaps sim"));
    d = good(); d.step = reinterpret_cast<int8_t*>(const_cast<float*>(d.sim)) + 4 * 90000; EXPECT(jsgx_rqa_scratch_bytes(&d) > 0);
    d = good(); d.end = reinterpret_cast<int32_t*>(const_cast<float*>(d.sim)) - 5; EXPECT(refused(d, "an output overlaps sim"));
    d = good(); d.end = reinterpret_cast<int32_t*>(const_cast<float*>(d.sim)) - 6; EXPECT(jsgx_rqa_scratch_bytes(&d) > 0);
    d = good(); d.total = d.score + 2 * 100 * 304 + 99 * 304 + 299; EXPECT(refused(d, "two outputs overlap"));
    d = good(); d.total = d.score + 2 * 100 * 304 + 99 * 304 + 300; EXPECT(jsgx_rqa_scratch_bytes(&d) > 0);
    d = good(); d.path_len = reinterpret_cast<int32_t*>(d.step + 2 * 100 * 301 + 99 * 301 + 297); EXPECT(refused(d, "two outputs overlap"));
    d = good(); d.path_len = reinterpret_cast<int32_t*>(d.step + 2 * 100 * 301 + 99 * 301 + 301); EXPECT(jsgx_rqa_scratch_bytes(&d) > 0);
    d = good(); d.path_j = d.path_i + 299; EXPECT(refused(d, "two outputs overlap"));
    d = good(); d.path_j = d.path_i + 300; EXPECT(jsgx_rqa_scratch_bytes(&d) > 0);
    d = good(); d.end = d.path_len + 2; EXPECT(refused(d, "two outputs overlap"));
    // an earlier defect is the one reported
    d = good(); d.sim = nullptr; d.pairs = 0; d.knight = 7; EXPECT(refused(d, "null sim"));
    d = good(); d.knight = 7; d.gap_extend = -1.f; d.sim_pitch = 1; EXPECT(refused(d, "knight must be 0 or 1"));
    d = good(); d.reserved0 = 7; d.max_path = 1; EXPECT(refused(d, "reserved0 must be 0"));
    d = good(); d.max_path = 1; d.sim_pitch = 1; EXPECT(refused(d, "max_path smaller than min(n, m)"));
    d = good(); d.step_pitch = 1; d.score = const_cast<float*>(d.sim); EXPECT(refused(d, "step_pitch smaller than m"));
    // one pair: the pair pitches are not looked at
    d = good(); d.pairs = 1; d.sim_pair_pitch = d.score_pair_pitch = d.step_pair_pitch = d.path_pitch = 0; EXPECT(jsgx_rqa_scratch_bytes(&d) == 8 * 10 + 8 * 100);
#if defined(JSGX_RQA_TEST_LAUNCHES)
    // what only the launch refuses, decided before any device call
    d = good();
    const int64_t need = jsgx_rqa_scratch_bytes(&d);
    EXPECT(jsgx_rqa_launch(&d, nullptr, need, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_rqa_launch: null scratch") == 0);
    EXPECT(jsgx_rqa_launch(&d, device<char>(9, 2), need, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_rqa_launch: scratch must be 4-byte aligned") == 0);
    EXPECT(jsgx_rqa_launch(&d, device<char>(9), need - 1, nullptr) == JSGX_ERR_INVALID &&
           std::strcmp(jsgx_last_error(), "jsgx_rqa_launch: scratch smaller than jsgx_rqa_scratch_bytes") == 0);
    d.sim = nullptr;
    EXPECT(jsgx_rqa_launch(&d, nullptr, 0, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_rqa_launch: null sim") == 0);
#endif

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
