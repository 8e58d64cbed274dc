// The host entry points of libjsgx.so (include/jsgx.h) from C++: the logarithm table, the plan of every period, the scratch size and the
// refusals with their texts.  No launch, so no device: built against libjsgx.so (CMake, jsg::jsgx) or, for the sanitizers, together with
// csrc/jsgx_beat_host.cpp itself (tests/test_beat_host.py: -fsanitize=address,undefined).  Exit code 0 and "ok" on success.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "jsgx.h"

static int failures = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("line %d: %s\n", __LINE__, #cond);               \
            ++failures;                                                  \
        }                                                                \
    } while (0)

static jsgx_beat_args good() {
    // device pointers that are never dereferenced: every call below is refused, sized or planned
    jsgx_beat_args a{};
    a.in = reinterpret_cast<const float*>(uintptr_t(1) << 44);
    a.in_pitch = 600;
    a.rows = 2;
    a.n_frames = 600;
    a.period = nullptr;
    a.period_all = 47;
    a.smooth = 1;
    a.log_table = reinterpret_cast<const float*>(uintptr_t(2) << 44);
    a.tightness = 100.f;
    a.normalise = 1;
    a.beats = reinterpret_cast<int32_t*>(uintptr_t(3) << 44);
    a.beats_pitch = 600;
    a.max_beats = 600;
    a.n_beats = reinterpret_cast<int32_t*>(uintptr_t(4) << 44);
    return a;
}

static bool refused(const jsgx_beat_args& a, const char* text) {
    char want[192];
    std::snprintf(want, sizeof want, "jsgx_beat_scratch_bytes: %s", text);
    return jsgx_beat_scratch_bytes(&a) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0;
}

int main() {
    EXPECT(jsgx_abi_version() == JSGX_ABI_VERSION && JSGX_ABI_VERSION == 1);
    EXPECT(std::strcmp(jsgx_last_error(), "") == 0);

    // the table: exactly its n entries are written
    const int full = 2 * JSGX_BEAT_MAX_PERIOD + 1;
    for (int n : {1, 2, 100, full}) {
        std::vector<float> t(n);
        EXPECT(jsgx_log_table_build(n, t.data()) == JSGX_OK);
        EXPECT(t[0] == 0.f);
        for (int k = 1; k < n; ++k) EXPECT(t[k] == (float)std::log((double)k));
    }
    float one = -1.f;
    EXPECT(jsgx_log_table_build(0, &one) == JSGX_ERR_INVALID && one == -1.f);
    EXPECT(jsgx_log_table_build(full + 1, &one) == JSGX_ERR_INVALID && one == -1.f);
    EXPECT(jsgx_log_table_build(4, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_log_table_build: null out") == 0);

    // the plan of every period; short and missing outputs
    jsgx_beat_args a = good();
    for (int P = 1; P <= JSGX_BEAT_MAX_PERIOD; ++P) {
        char name[16];
        int32_t threads = 0, lds = 0;
        EXPECT(jsgx_beat_plan(&a, P, name, (int)sizeof name, &threads, &lds) == JSGX_OK);
        EXPECT(std::strcmp(name, P >= 511 ? "beat_frames" : "beat_split") == 0 && threads == JSGX_BEAT_THREADS && lds == JSGX_BEAT_LDS_BYTES && lds <= 163840);
    }
    char name[16];
    EXPECT(jsgx_beat_plan(&a, 47, nullptr, 0, nullptr, nullptr) == JSGX_OK);
    EXPECT(jsgx_beat_plan(&a, 47, name, 15, nullptr, nullptr) == JSGX_ERR_INVALID);
    EXPECT(jsgx_beat_plan(&a, 0, name, 16, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_beat_plan: period must be in 1..1024") == 0);
    EXPECT(jsgx_beat_plan(&a, 1025, name, 16, nullptr, nullptr) == JSGX_ERR_INVALID);
    EXPECT(jsgx_beat_plan(nullptr, 47, name, 16, nullptr, nullptr) == JSGX_ERR_INVALID);

    // the scratch: link, and s where smooth
    EXPECT(jsgx_beat_scratch_bytes(&a) == 2 * 4 * 2 * 600);
    a.smooth = 0;
    EXPECT(jsgx_beat_scratch_bytes(&a) == 4 * 2 * 600);
    a = good();
    a.rows = 65535;
    a.n_frames = JSGX_BEAT_MAX_FRAMES;
    a.in_pitch = a.beats_pitch = JSGX_BEAT_MAX_FRAMES;
    a.max_beats = 1;
    EXPECT(jsgx_beat_scratch_bytes(&a) == 2ll * 4 * 65535 * JSGX_BEAT_MAX_FRAMES);

    // one refusal of every kind, with its text
    EXPECT(jsgx_beat_scratch_bytes(nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_beat_scratch_bytes: null argument") == 0);
    a = good(); a.in = nullptr; EXPECT(refused(a, "null in"));
    a = good(); a.log_table = nullptr; EXPECT(refused(a, "null log_table"));
    a = good(); a.beats = nullptr; EXPECT(refused(a, "null beats"));
    a = good(); a.n_beats = nullptr; EXPECT(refused(a, "null n_beats"));
    a = good(); a.period = reinterpret_cast<const int32_t*>((uintptr_t(5) << 44) + 2); EXPECT(refused(a, "pointers must be 4-byte aligned"));
    a = good(); a.rows = 0; EXPECT(refused(a, "rows must be in 1..65535"));
    a = good(); a.n_frames = JSGX_BEAT_MAX_FRAMES + 1; EXPECT(refused(a, "n_frames must be in 1..2^24"));
    a = good(); a.period_all = 1025; EXPECT(refused(a, "period_all must be in 1..1024 (period is null)"));
    a = good(); a.tightness = NAN; EXPECT(refused(a, "tightness must be finite and > 0"));
    a = good(); a.smooth = 2; EXPECT(refused(a, "smooth must be 0 or 1"));
    a = good(); a.normalise = -1; EXPECT(refused(a, "normalise must be 0 or 1"));
    a = good(); a.max_beats = 0; EXPECT(refused(a, "max_beats must be in 1..2^24"));
    a = good(); a.reserved0 = 1; EXPECT(refused(a, "reserved0 must be 0"));
    a = good(); a.in_pitch = 599; EXPECT(refused(a, "in_pitch smaller than n_frames"));
    a = good(); a.beats_pitch = 599; EXPECT(refused(a, "beats_pitch smaller than max_beats"));
    a = good(); a.local_score = reinterpret_cast<float*>(uintptr_t(6) << 44); a.local_pitch = 599; EXPECT(refused(a, "local_pitch smaller than n_frames"));
    a = good(); a.cum_score = reinterpret_cast<float*>(uintptr_t(7) << 44); a.cum_pitch = 1; EXPECT(refused(a, "cum_pitch smaller than n_frames"));
    a = good(); a.n_beats = reinterpret_cast<int32_t*>(const_cast<float*>(a.in) + 1199); EXPECT(refused(a, "an output overlaps in"));
    a = good(); a.beats = reinterpret_cast<int32_t*>(const_cast<float*>(a.log_table) + 2048); EXPECT(refused(a, "an output overlaps log_table"));
    a = good(); a.beats = reinterpret_cast<int32_t*>(const_cast<float*>(a.log_table) + 2049); EXPECT(jsgx_beat_scratch_bytes(&a) > 0);
    // a period in device memory is not read by the host: any period_all goes with it
    a = good(); a.period = reinterpret_cast<const int32_t*>(uintptr_t(5) << 44); a.period_all = -7; EXPECT(jsgx_beat_scratch_bytes(&a) > 0);

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
