// The host entry points of section 14 of libjsgx.so (include/jsgx.h) from C++: the plan, the scratch arithmetic up to the limits (the
// 64-bit pitch arithmetic included: rows more than 2^31 elements apart) and the refusals with their texts in their order.  No launch
// that passes, so no device: built against libjsgx.so (CMake, jsg::jsgx) or, for the sanitizers, together with csrc/jsgx_beat_host.cpp
// and csrc/jsgx_peak_host.cpp themselves (tests/test_peak_host.py: -fsanitize=address,undefined).  Exit code 0 and "ok" on success.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

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

static const int kB = JSGX_PEAK_BLOCK;
static const int kT = 2 * JSGX_PEAK_BLOCK + 5;          // three blocks a row

static jsgx_peak_args good() {                 // 3 rows of 2B + 5 frames, every optional buffer given
    jsgx_peak_args a{};
    a.in = device<const float>(1);
    a.in_pitch = kT + 3;
    a.energy = device<const float>(2);
    a.energy_pitch = kT + 1;
    a.candidate = device<uint8_t>(3);
    a.candidate_pitch = kT + 2;
    a.peaks = device<int32_t>(4);
    a.backtracked = device<int32_t>(5);
    a.peaks_pitch = 104;
    a.n_peaks = device<int32_t>(6);
    a.rows = 3;
    a.n_frames = kT;
    a.pre_max = 3, a.post_max = 1, a.pre_avg = 5, a.post_avg = 5;
    a.delta = 0.07f;
    a.wait = 3;
    a.normalise = 1;
    a.max_peaks = 100;
    return a;
}
static const int64_t kNeed = 3 * 3 * (32 + 4 * 4 + int64_t(kB));

static bool refused(const jsgx_peak_args& a, const char* text) {
    char want[192];
    std::snprintf(want, sizeof want, "jsgx_peak_plan: %s", text);
    if (!(jsgx_peak_plan(&a, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0)) return false;
    std::snprintf(want, sizeof want, "jsgx_peak_scratch_bytes: %s", text);
    return jsgx_peak_scratch_bytes(&a) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0;
}

#if defined(JSGX_PEAK_TEST_LAUNCHES)
static bool launch_refused(const jsgx_peak_args& a, void* scratch, int64_t bytes, const char* text) {
    char want[192];
    std::snprintf(want, sizeof want, "jsgx_peak_launch: %s", text);
    return jsgx_peak_launch(&a, scratch, bytes, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0;
}
#endif

int main() {
    static_assert(sizeof(jsgx_peak_args) == 120, "include/jsgx.h states the size");
    static_assert(JSGX_PEAK_MAX_REACH == 256 && JSGX_PEAK_MAX_FRAMES == (1 << 24) && JSGX_PEAK_LDS_BYTES <= JSGX_PEAK_LDS_LIMIT, "include/jsgx.h");
    static_assert((JSGX_PEAK_BLOCK & (JSGX_PEAK_BLOCK - 1)) == 0 && (1 << JSGX_PEAK_LOG2_BLOCK) == JSGX_PEAK_BLOCK, "include/jsgx.h");
    EXPECT(jsgx_abi_version() == 1);

    // the plan and the scratch over shapes, dense rows far apart
    char name[16];
    for (int T : {1, 2, 64, 65, kB - 1, kB, kB + 1, 2 * kB, 3 * kB + 7, JSGX_PEAK_MAX_FRAMES})
        for (int R : {1, 3, 65535})
            for (int wait : {0, 1, kB - 2, kB - 1, kB, JSGX_PEAK_MAX_FRAMES}) {
                jsgx_peak_args d{};
                d.in = reinterpret_cast<const float*>(uintptr_t(1) << 50), d.peaks = reinterpret_cast<int32_t*>(uintptr_t(1) << 58);
                d.n_peaks = reinterpret_cast<int32_t*>(uintptr_t(1) << 40);
                d.in_pitch = T, d.peaks_pitch = 7, d.rows = R, d.n_frames = T, d.wait = wait, d.max_peaks = 7;
                const int64_t blocks = (int64_t(T) + kB - 1) / kB, offsets = wait + 1 < kB ? wait + 1 : kB;
                int32_t threads = -1, lds = -1, launches = -1, got_blocks = -1;
                EXPECT(jsgx_peak_plan(&d, name, (int)sizeof name, &threads, &lds, &launches, &got_blocks) == JSGX_OK);
                EXPECT(std::strcmp(name, T <= kB ? "peak_single" : "peak_blocked") == 0 && threads == JSGX_PEAK_THREADS && lds == JSGX_PEAK_LDS_BYTES);
                EXPECT(launches == (T <= kB ? 1 : 5) && got_blocks == blocks);
                const int64_t need = jsgx_peak_scratch_bytes(&d);
                EXPECT(need == (T <= kB ? 0 : R * blocks * (32 + 4 * offsets + kB)));
                EXPECT(need <= int64_t(R) * (16 * int64_t(T) + 32 * blocks));          // what the header promises
            }
    // rows more than 2^31 elements apart, in every buffer: the spans are 64-bit and more
    jsgx_peak_args d = good();
    d.in_pitch = d.energy_pitch = d.candidate_pitch = d.peaks_pitch = (int64_t(1) << 40) + 7;
    d.in = reinterpret_cast<const float*>(uintptr_t(1) << 50), d.energy = reinterpret_cast<const float*>(uintptr_t(1) << 54);
    d.peaks = reinterpret_cast<int32_t*>(uintptr_t(1) << 58), d.backtracked = reinterpret_cast<int32_t*>(uintptr_t(1) << 60);
    d.candidate = reinterpret_cast<uint8_t*>(uintptr_t(1) << 62);
    EXPECT(jsgx_peak_scratch_bytes(&d) == kNeed);
    d.n_peaks = reinterpret_cast<int32_t*>(const_cast<float*>(d.in) + 2 * d.in_pitch + kT - 1); EXPECT(refused(d, "n_peaks overlaps in"));          // the last element of the third row
    d.n_peaks = reinterpret_cast<int32_t*>(const_cast<float*>(d.in) + 2 * d.in_pitch + kT); EXPECT(jsgx_peak_scratch_bytes(&d) == kNeed);

    d = good();
    EXPECT(jsgx_peak_scratch_bytes(&d) == kNeed);
    EXPECT(jsgx_peak_plan(&d, name, 15, nullptr, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_peak_plan: bad argument") == 0);
    EXPECT(jsgx_peak_plan(nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_peak_plan: null argument") == 0);
    EXPECT(jsgx_peak_scratch_bytes(nullptr) == JSGX_ERR_INVALID);

    // one refusal of every kind, in the header's order
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    d = good(); d.in = nullptr; EXPECT(refused(d, "null in"));
    d = good(); d.peaks = nullptr; EXPECT(refused(d, "null peaks"));
    d = good(); d.n_peaks = nullptr; EXPECT(refused(d, "null n_peaks"));
    d = good(); d.in = device<const float>(1, 2); EXPECT(refused(d, "pointers must be 4-byte aligned"));
    d = good(); d.energy = device<const float>(2, 1); EXPECT(refused(d, "pointers must be 4-byte aligned"));
    d = good(); d.backtracked = device<int32_t>(5, 3); EXPECT(refused(d, "pointers must be 4-byte aligned"));
    d = good(); d.n_peaks = device<int32_t>(6, 2); EXPECT(refused(d, "pointers must be 4-byte aligned"));
    d = good(); d.candidate = device<uint8_t>(3, 1); EXPECT(jsgx_peak_scratch_bytes(&d) == kNeed);          // bytes
    for (int v : {0, -1, 65536}) { d = good(); d.rows = v; EXPECT(refused(d, "rows must be in 1..65535")); }
    for (int v : {0, -1, JSGX_PEAK_MAX_FRAMES + 1}) { d = good(); d.n_frames = v; EXPECT(refused(d, "n_frames must be in 1..16777216")); }
    for (int v : {-1, 257}) {
        d = good(); d.pre_max = v; EXPECT(refused(d, "pre_max must be in 0..256"));
        d = good(); d.post_max = v; EXPECT(refused(d, "post_max must be in 0..256"));
        d = good(); d.pre_avg = v; EXPECT(refused(d, "pre_avg must be in 0..256"));
        d = good(); d.post_avg = v; EXPECT(refused(d, "post_avg must be in 0..256"));
    }
    for (float v : {nan, inf, -inf}) { d = good(); d.delta = v; EXPECT(refused(d, "delta must be finite")); }
    for (int v : {-1, JSGX_PEAK_MAX_FRAMES + 1}) { d = good(); d.wait = v; EXPECT(refused(d, "wait must be in 0..16777216")); }
    for (int v : {-1, 2}) { d = good(); d.normalise = v; EXPECT(refused(d, "normalise must be 0 or 1")); }
    for (int v : {0, -1, JSGX_PEAK_MAX_FRAMES + 1}) { d = good(); d.max_peaks = v; EXPECT(refused(d, "max_peaks must be in 1..16777216")); }
    d = good(); d.energy = nullptr; EXPECT(refused(d, "energy and backtracked go together"));
    d = good(); d.backtracked = nullptr; EXPECT(refused(d, "energy and backtracked go together"));
    d = good(); d.in_pitch = kT - 1; EXPECT(refused(d, "in_pitch smaller than n_frames"));
    d = good(); d.energy_pitch = kT - 1; EXPECT(refused(d, "energy_pitch smaller than n_frames"));
    d = good(); d.candidate_pitch = kT - 1; EXPECT(refused(d, "candidate_pitch smaller than n_frames"));
    d = good(); d.peaks_pitch = 99; EXPECT(refused(d, "peaks_pitch smaller than max_peaks"));
    const int64_t in_span = 2 * (kT + 3) + kT, energy_span = 2 * (kT + 1) + kT, peaks_span = 2 * 104 + 100, cand_span = 2 * (kT + 2) + kT;
    d = good(); d.peaks = reinterpret_cast<int32_t*>(const_cast<float*>(d.in) + in_span - 1); EXPECT(refused(d, "peaks overlaps in"));
    d = good(); d.peaks = reinterpret_cast<int32_t*>(const_cast<float*>(d.in) + in_span); EXPECT(jsgx_peak_scratch_bytes(&d) == kNeed);
    d = good(); d.peaks = reinterpret_cast<int32_t*>(const_cast<float*>(d.energy)) - peaks_span + 1; EXPECT(refused(d, "peaks overlaps energy"));
    d = good(); d.backtracked = reinterpret_cast<int32_t*>(const_cast<float*>(d.in)) + 10; EXPECT(refused(d, "backtracked overlaps in"));
    d = good(); d.backtracked = reinterpret_cast<int32_t*>(const_cast<float*>(d.energy)) + energy_span - 1; EXPECT(refused(d, "backtracked overlaps energy"));
    d = good(); d.n_peaks = reinterpret_cast<int32_t*>(const_cast<float*>(d.in)) - 2; EXPECT(refused(d, "n_peaks overlaps in"));
    d = good(); d.n_peaks = reinterpret_cast<int32_t*>(const_cast<float*>(d.in)) - 3; EXPECT(jsgx_peak_scratch_bytes(&d) == kNeed);
    d = good(); d.n_peaks = reinterpret_cast<int32_t*>(const_cast<float*>(d.energy)) + 1; EXPECT(refused(d, "n_peaks overlaps energy"));
    d = good(); d.candidate = reinterpret_cast<uint8_t*>(const_cast<float*>(d.in)) + 4 * in_span - 1; EXPECT(refused(d, "candidate overlaps in"));
    d = good(); d.candidate = reinterpret_cast<uint8_t*>(const_cast<float*>(d.in)) + 4 * in_span; EXPECT(jsgx_peak_scratch_bytes(&d) == kNeed);
    d = good(); d.candidate = reinterpret_cast<uint8_t*>(const_cast<float*>(d.energy)) - cand_span + 1; EXPECT(refused(d, "candidate overlaps energy"));
    d = good(); d.backtracked = d.peaks + peaks_span - 1; EXPECT(refused(d, "peaks overlaps backtracked"));
    d = good(); d.backtracked = d.peaks + peaks_span; EXPECT(jsgx_peak_scratch_bytes(&d) == kNeed);
    d = good(); d.n_peaks = d.peaks + 5; EXPECT(refused(d, "peaks overlaps n_peaks"));
    d = good(); d.candidate = reinterpret_cast<uint8_t*>(d.peaks) - cand_span + 1; EXPECT(refused(d, "peaks overlaps candidate"));
    d = good(); d.n_peaks = d.backtracked - 2; EXPECT(refused(d, "backtracked overlaps n_peaks"));
    d = good(); d.candidate = reinterpret_cast<uint8_t*>(d.backtracked + peaks_span) - 1; EXPECT(refused(d, "backtracked overlaps candidate"));
    d = good(); d.candidate = reinterpret_cast<uint8_t*>(d.n_peaks + 3) - 1; EXPECT(refused(d, "n_peaks overlaps candidate"));
    d = good(); d.candidate = reinterpret_cast<uint8_t*>(d.n_peaks + 3); EXPECT(jsgx_peak_scratch_bytes(&d) == kNeed);
    // the optional buffers absent: their pitches are not looked at, they overlap nothing
    d = good(); d.energy = nullptr; d.backtracked = nullptr; d.candidate = nullptr; d.energy_pitch = d.candidate_pitch = 0; EXPECT(jsgx_peak_scratch_bytes(&d) == kNeed);
    // an earlier defect is the one reported
    d = good(); d.in = nullptr; d.rows = 0; d.delta = nan; EXPECT(refused(d, "null in"));
    d = good(); d.post_max = 300; d.pre_avg = -1; d.wait = -1; EXPECT(refused(d, "post_max must be in 0..256"));
    d = good(); d.normalise = 5; d.energy = nullptr; d.in_pitch = 1; EXPECT(refused(d, "normalise must be 0 or 1"));
    d = good(); d.peaks_pitch = 1; d.n_peaks = d.peaks; EXPECT(refused(d, "peaks_pitch smaller than max_peaks"));
    // one row: the pitches are not looked at; up to B frames: no scratch; the ends of the ranges
    d = good(); d.rows = 1; d.in_pitch = d.energy_pitch = d.candidate_pitch = d.peaks_pitch = 0; EXPECT(jsgx_peak_scratch_bytes(&d) == kNeed / 3);
    d = good(); d.n_frames = kB; EXPECT(jsgx_peak_scratch_bytes(&d) == 0);
    d = good(); d.pre_max = d.post_max = d.pre_avg = d.post_avg = 256; d.wait = JSGX_PEAK_MAX_FRAMES; d.delta = -3e38f; d.normalise = 0;
    EXPECT(jsgx_peak_scratch_bytes(&d) == 3 * 3 * (32 + 4 * int64_t(kB) + kB));

#if defined(JSGX_PEAK_TEST_LAUNCHES)
    // the launch's refusals, decided before any device call (the shipped library only: the launcher is a HIP unit)
    char* scratch = device<char>(7);
    EXPECT(jsgx_peak_launch(nullptr, scratch, kNeed, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_peak_launch: null argument") == 0);
    d = good(); d.peaks = nullptr; EXPECT(launch_refused(d, scratch, kNeed, "null peaks"));
    d = good(); d.n_peaks = d.peaks + 5; EXPECT(launch_refused(d, nullptr, 0, "peaks overlaps n_peaks"));
    d = good();
    EXPECT(launch_refused(d, nullptr, kNeed, "null scratch"));
    EXPECT(launch_refused(d, device<char>(7, 2), kNeed, "scratch must be 4-byte aligned"));
    EXPECT(launch_refused(d, scratch, kNeed - 1, "scratch smaller than jsgx_peak_scratch_bytes"));
    EXPECT(launch_refused(d, const_cast<float*>(d.in) + in_span - 1, kNeed, "scratch overlaps in"));
    EXPECT(launch_refused(d, reinterpret_cast<char*>(const_cast<float*>(d.energy)) - kNeed + 4, 1 << 20, "scratch overlaps energy"));
    EXPECT(launch_refused(d, d.peaks + 7, kNeed, "scratch overlaps peaks"));
    EXPECT(launch_refused(d, d.backtracked + peaks_span - 1, kNeed, "scratch overlaps backtracked"));
    EXPECT(launch_refused(d, d.n_peaks + 2, kNeed, "scratch overlaps n_peaks"));
    EXPECT(launch_refused(d, d.candidate + cand_span - 4 + (4 - cand_span % 4) % 4, kNeed, "scratch overlaps candidate"));
    EXPECT(launch_refused(d, device<char>(7, 1), 0, "scratch must be 4-byte aligned"));        // the earlier defect
#endif

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
