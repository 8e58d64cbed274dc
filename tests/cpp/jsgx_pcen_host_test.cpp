// The host entry points of section 13 of libjsgx.so (include/jsgx.h) from C++: the decay table, the plan, the scratch arithmetic up to
// the limits (the 64-bit pitch arithmetic included: rows more than 2^31 elements apart) and the refusals with their texts in their
// order.  No launch that passes, so no device: built against libjsgx.so (CMake, jsg::jsgx) or, for the sanitizers, together with
// csrc/jsgx_beat_host.cpp and csrc/jsgx_pcen_host.cpp themselves (tests/test_pcen_host.py: -fsanitize=address,undefined).
// Exit code 0 and "ok" on success.
#include <cmath>
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

static jsgx_pcen_args good() {                 // 3 rows of 600 frames x 40 bands, every optional buffer given
    jsgx_pcen_args a{};
    a.in = device<const float>(1);
    a.frame_pitch = 44;
    a.row_pitch = 600 * 44;
    a.decay = device<const float>(2);
    a.state_in = device<const float>(3);
    a.state_in_pitch = 40;
    a.state_out = device<float>(4);
    a.state_out_pitch = 48;
    a.smooth_out = device<float>(5);
    a.smooth_frame_pitch = 40;
    a.smooth_row_pitch = 600 * 40;
    a.out = device<float>(6);
    a.out_frame_pitch = 41;
    a.out_row_pitch = 600 * 41;
    a.rows = 3;
    a.n_bands = 40;
    a.n_frames = 600;
    a.b = 0.05f;
    a.gain = 0.98f;
    a.bias = 2.0f;
    a.power = 0.5f;
    a.eps = 1e-6f;
    return a;
}
static const int64_t kNeed = 4 * 3 * 3 * 40;          // three chunks a row

static bool refused(const jsgx_pcen_args& a, const char* text) {
    char want[192];
    std::snprintf(want, sizeof want, "jsgx_pcen_plan: %s", text);
    if (!(jsgx_pcen_plan(&a, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0)) return false;
    std::snprintf(want, sizeof want, "jsgx_pcen_scratch_bytes: %s", text);
    return jsgx_pcen_scratch_bytes(&a) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0;
}

#if defined(JSGX_PCEN_TEST_LAUNCHES)
static bool launch_refused(const jsgx_pcen_args& a, void* scratch, int64_t bytes, const char* text) {
    char want[192];
    std::snprintf(want, sizeof want, "jsgx_pcen_launch: %s", text);
    return jsgx_pcen_launch(&a, scratch, bytes, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0;
}
#endif

int main() {
    static_assert(sizeof(jsgx_pcen_args) == 144, "include/jsgx.h states the size");
    static_assert(JSGX_PCEN_CHUNK == 256 && JSGX_PCEN_MAX_CHAINS == (1LL << 36), "include/jsgx.h");
    EXPECT(jsgx_abi_version() == 1);

    // the table: pow in double of the float a, rounded once
    float q[JSGX_PCEN_CHUNK + 1];
    q[JSGX_PCEN_CHUNK] = -1.f;
    for (float b : {0.025f, 0.0563894f, 0.5f, 1.0f, 1e-4f}) {
        EXPECT(jsgx_pcen_decay_build(b, q) == JSGX_OK);
        const float a = 1.0f - b;
        for (int j = 0; j < JSGX_PCEN_CHUNK; ++j) EXPECT(q[j] == (float)std::pow((double)a, (double)(j + 1)));
        EXPECT(q[0] == a && q[JSGX_PCEN_CHUNK] == -1.f);
    }
    for (float b : {0.0f, -0.5f, 1.5f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()})
        EXPECT(jsgx_pcen_decay_build(b, q) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_pcen_decay_build: b must be in (0, 1]") == 0);
    EXPECT(jsgx_pcen_decay_build(0.5f, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_pcen_decay_build: null out") == 0);

    // the plan and the scratch over shapes, dense planes far apart; the chains decide where a shape is refused
    char name[16];
    const int32_t most = std::numeric_limits<int32_t>::max();
    for (int T : {1, 2, 255, 256, 257, 1000, 1 << 24, most})
        for (int B : {1, 40, 64, 65, JSGX_PCEN_MAX_BANDS})
            for (int R : {1, 3, 65535}) {
                jsgx_pcen_args d{};
                d.in = reinterpret_cast<const float*>(uintptr_t(1) << 50), d.decay = reinterpret_cast<const float*>(uintptr_t(1) << 40);
                d.out = reinterpret_cast<float*>(uintptr_t(1) << 58);
                d.frame_pitch = d.out_frame_pitch = B, d.row_pitch = d.out_row_pitch = (int64_t)T * B;
                d.rows = R, d.n_bands = B, d.n_frames = T, d.b = 0.05f, d.gain = 0.98f, d.bias = 2.0f, d.power = 0.5f, d.eps = 1e-6f;
                const int64_t chunks = ((int64_t)T + 255) / 256, chains = (int64_t)R * chunks * B;
                int32_t threads = -1, lds = -1, launches = -1, got_chunks = -1;
                if (chains > JSGX_PCEN_MAX_CHAINS) {
                    EXPECT(refused(d, "rows * chunks * n_bands must be at most 2^36"));
                    continue;
                }
                EXPECT(jsgx_pcen_plan(&d, name, (int)sizeof name, &threads, &lds, &launches, &got_chunks) == JSGX_OK);
                EXPECT(std::strcmp(name, T <= 256 ? "pcen_single" : "pcen_chunked") == 0 && threads == JSGX_PCEN_THREADS && lds == 0);
                EXPECT(launches == (T <= 256 ? 1 : 3) && got_chunks == chunks);
                EXPECT(jsgx_pcen_scratch_bytes(&d) == (T <= 256 ? 0 : 4 * chains));
            }
    // rows more than 2^31 elements apart, in every plane: the spans are 64-bit and more
    jsgx_pcen_args d = good();
    d.row_pitch = d.smooth_row_pitch = d.out_row_pitch = (int64_t(1) << 40) + 7;
    d.state_in_pitch = d.state_out_pitch = (int64_t(1) << 33) + 1;
    d.in = reinterpret_cast<const float*>(uintptr_t(1) << 50), d.smooth_out = reinterpret_cast<float*>(uintptr_t(1) << 54), d.out = reinterpret_cast<float*>(uintptr_t(1) << 58);
    EXPECT(jsgx_pcen_scratch_bytes(&d) == kNeed);
    d.out = const_cast<float*>(d.in) + 2 * d.row_pitch + 599 * 44 + 39; EXPECT(refused(d, "out overlaps in"));          // the last element of the third row
    d.out = const_cast<float*>(d.in) + 2 * d.row_pitch + 599 * 44 + 40; EXPECT(jsgx_pcen_scratch_bytes(&d) == kNeed);

    d = good();
    EXPECT(jsgx_pcen_scratch_bytes(&d) == kNeed);
    EXPECT(jsgx_pcen_plan(&d, name, 15, nullptr, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_pcen_plan: bad argument") == 0);
    EXPECT(jsgx_pcen_plan(nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_pcen_plan: null argument") == 0);
    EXPECT(jsgx_pcen_scratch_bytes(nullptr) == JSGX_ERR_INVALID);

    // one refusal of every kind, in the header's order
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    d = good(); d.in = nullptr; EXPECT(refused(d, "null in"));
    d = good(); d.decay = nullptr; EXPECT(refused(d, "null decay"));
    d = good(); d.out = nullptr; EXPECT(refused(d, "null out"));
    d = good(); d.in = device<const float>(1, 2); EXPECT(refused(d, "pointers must be 4-byte aligned"));
    d = good(); d.state_out = device<float>(4, 1); EXPECT(refused(d, "pointers must be 4-byte aligned"));
    d = good(); d.rows = 0; EXPECT(refused(d, "rows must be in 1..65535"));
    d = good(); d.rows = 65536; EXPECT(refused(d, "rows must be in 1..65535"));
    d = good(); d.n_bands = 0; EXPECT(refused(d, "n_bands must be in 1..65536"));
    d = good(); d.n_bands = 65537; EXPECT(refused(d, "n_bands must be in 1..65536"));
    d = good(); d.n_frames = 0; EXPECT(refused(d, "n_frames must be in 1..2147483647"));
    d = good(); d.n_frames = -5; EXPECT(refused(d, "n_frames must be in 1..2147483647"));
    d = good(); d.rows = 65535; d.n_bands = 65536; d.n_frames = most; EXPECT(refused(d, "rows * chunks * n_bands must be at most 2^36"));
    d = good(); d.frame_pitch = 39; EXPECT(refused(d, "frame_pitch smaller than n_bands"));
    d = good(); d.row_pitch = 599 * 44 + 39; EXPECT(refused(d, "row_pitch does not cover a plane"));
    d = good(); d.state_in_pitch = 39; EXPECT(refused(d, "state_in_pitch smaller than n_bands"));
    d = good(); d.state_out_pitch = 39; EXPECT(refused(d, "state_out_pitch smaller than n_bands"));
    d = good(); d.smooth_frame_pitch = 39; EXPECT(refused(d, "smooth_frame_pitch smaller than n_bands"));
    d = good(); d.smooth_row_pitch = 599 * 40 + 39; EXPECT(refused(d, "smooth_row_pitch does not cover a plane"));
    d = good(); d.out_frame_pitch = 39; EXPECT(refused(d, "out_frame_pitch smaller than n_bands"));
    d = good(); d.out_row_pitch = 599 * 41 + 39; EXPECT(refused(d, "out_row_pitch does not cover a plane"));
    for (float b : {0.0f, -0.1f, 1.0001f, nan, inf}) { d = good(); d.b = b; EXPECT(refused(d, "b must be in (0, 1]")); }
    for (float v : {-0.1f, nan, inf}) { d = good(); d.gain = v; EXPECT(refused(d, "gain must be finite and not negative")); }
    for (float v : {-0.1f, nan, inf}) { d = good(); d.bias = v; EXPECT(refused(d, "bias must be finite and not negative")); }
    for (float v : {0.0f, -1.0f, nan, inf}) { d = good(); d.power = v; EXPECT(refused(d, "power must be finite and positive")); }
    for (float v : {0.0f, -1.0f, nan, inf}) { d = good(); d.eps = v; EXPECT(refused(d, "eps must be finite and positive")); }
    d = good(); d.b = 1.0f; d.gain = 0.f; d.bias = 0.f; EXPECT(jsgx_pcen_scratch_bytes(&d) == kNeed);
    const int64_t in_span = 2 * 600 * 44 + 599 * 44 + 40, out_span = 2 * 600 * 41 + 599 * 41 + 40, smooth_span = 3 * 600 * 40, so_span = 2 * 48 + 40;
    d = good(); d.out = const_cast<float*>(d.in) + in_span - 1; EXPECT(refused(d, "out overlaps in"));
    d = good(); d.out = const_cast<float*>(d.in) + in_span; EXPECT(jsgx_pcen_scratch_bytes(&d) == kNeed);
    d = good(); d.out = const_cast<float*>(d.decay) - out_span + 1; EXPECT(refused(d, "out overlaps decay"));
    d = good(); d.out = const_cast<float*>(d.decay) - out_span; EXPECT(jsgx_pcen_scratch_bytes(&d) == kNeed);
    d = good(); d.out = const_cast<float*>(d.state_in) + 2 * 40 + 39; EXPECT(refused(d, "out overlaps state_in"));
    d = good(); d.smooth_out = const_cast<float*>(d.in) + 100; EXPECT(refused(d, "smooth_out overlaps in"));
    d = good(); d.smooth_out = const_cast<float*>(d.decay) + 255; EXPECT(refused(d, "smooth_out overlaps decay"));
    d = good(); d.smooth_out = const_cast<float*>(d.decay) + 256; EXPECT(jsgx_pcen_scratch_bytes(&d) == kNeed);
    d = good(); d.smooth_out = const_cast<float*>(d.state_in) - smooth_span + 1; EXPECT(refused(d, "smooth_out overlaps state_in"));
    d = good(); d.state_out = const_cast<float*>(d.in) - so_span + 1; EXPECT(refused(d, "state_out overlaps in"));
    d = good(); d.state_out = const_cast<float*>(d.decay) + 3; EXPECT(refused(d, "state_out overlaps decay"));
    d = good(); d.state_out = const_cast<float*>(d.state_in); EXPECT(refused(d, "state_out overlaps state_in"));
    d = good(); d.smooth_out = d.out + out_span - 1; EXPECT(refused(d, "out overlaps smooth_out"));
    d = good(); d.state_out = d.out + 5; EXPECT(refused(d, "out overlaps state_out"));
    d = good(); d.state_out = d.smooth_out + smooth_span - 1; EXPECT(refused(d, "smooth_out overlaps state_out"));
    d = good(); d.state_out = d.smooth_out + smooth_span; EXPECT(jsgx_pcen_scratch_bytes(&d) == kNeed);
    // the optional buffers absent: their pitches are not looked at, they overlap nothing
    d = good(); d.state_in = nullptr; d.state_out = nullptr; d.smooth_out = nullptr; d.state_in_pitch = d.state_out_pitch = d.smooth_frame_pitch = d.smooth_row_pitch = 0;
    EXPECT(jsgx_pcen_scratch_bytes(&d) == kNeed);
    // an earlier defect is the one reported
    d = good(); d.in = nullptr; d.rows = 0; d.b = 7.f; EXPECT(refused(d, "null in"));
    d = good(); d.n_bands = 0; d.frame_pitch = -1; d.eps = 0.f; EXPECT(refused(d, "n_bands must be in 1..65536"));
    d = good(); d.out_frame_pitch = 1; d.gain = -1.f; d.state_out = d.out; EXPECT(refused(d, "out_frame_pitch smaller than n_bands"));
    d = good(); d.power = 0.f; d.state_out = d.out; EXPECT(refused(d, "power must be finite and positive"));
    // one row: the row pitches are not looked at; up to 256 frames: no scratch
    d = good(); d.rows = 1; d.row_pitch = d.out_row_pitch = d.smooth_row_pitch = d.state_in_pitch = d.state_out_pitch = 0; EXPECT(jsgx_pcen_scratch_bytes(&d) == kNeed / 3);
    d = good(); d.n_frames = 256; EXPECT(jsgx_pcen_scratch_bytes(&d) == 0);

#if defined(JSGX_PCEN_TEST_LAUNCHES)
    // the launch's refusals, decided before any device call (the shipped library only: the launcher is a HIP unit)
    float* scratch = device<float>(7);
    EXPECT(jsgx_pcen_launch(nullptr, scratch, kNeed, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_pcen_launch: null argument") == 0);
    d = good(); d.decay = nullptr; EXPECT(launch_refused(d, scratch, kNeed, "null decay"));
    d = good(); d.state_out = d.out + 5; EXPECT(launch_refused(d, nullptr, 0, "out overlaps state_out"));
    d = good();
    EXPECT(launch_refused(d, nullptr, kNeed, "null scratch"));
    EXPECT(launch_refused(d, device<float>(7, 2), kNeed, "scratch must be 4-byte aligned"));
    EXPECT(launch_refused(d, scratch, kNeed - 1, "scratch smaller than jsgx_pcen_scratch_bytes"));
    EXPECT(launch_refused(d, const_cast<float*>(d.in) + in_span - 1, kNeed, "scratch overlaps in"));
    EXPECT(launch_refused(d, const_cast<float*>(d.decay) - kNeed / 4 + 1, 1 << 20, "scratch overlaps decay"));
    EXPECT(launch_refused(d, const_cast<float*>(d.state_in) + 7, kNeed, "scratch overlaps state_in"));
    EXPECT(launch_refused(d, d.out + out_span - 1, kNeed, "scratch overlaps out"));
    EXPECT(launch_refused(d, d.smooth_out + 1000, kNeed, "scratch overlaps smooth_out"));
    EXPECT(launch_refused(d, d.state_out - kNeed / 4 + 1, kNeed, "scratch overlaps state_out"));
    EXPECT(launch_refused(d, device<float>(7, 1), 0, "scratch must be 4-byte aligned"));        // the earlier defect
#endif

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
