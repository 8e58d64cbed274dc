// The host entry points of section 4 of libjsgx.so (include/jsgx.h) from C++: the refusals with their texts, the scratch size, the plan and
// the band transition builder.  No launch, so no device: built against libjsgx.so (CMake, jsg::jsgx) or, for the sanitizers, together with
// csrc/jsgx_beat_host.cpp and csrc/jsgx_viterbi_host.cpp themselves (tests/test_viterbi_host.py: -fsanitize=address,undefined).  Exit code 0
// and "ok" on success.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
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

template <class T>
static T* device(int k, int bytes = 0) {       // device pointers that are never dereferenced: every call below is refused, sized or planned
    return reinterpret_cast<T*>((uintptr_t(k) << 44) + bytes);
}

static jsgx_viterbi_args good() {
    jsgx_viterbi_args a{};
    a.log_emit = device<const float>(1);
    a.emit_frame_pitch = 24;
    a.emit_seq_pitch = 100 * 24;
    a.log_init = device<const float>(2);
    a.trans = device<const float>(3);
    a.trans_pitch = 20;
    a.trans_form = JSGX_TRANS_DENSE;
    a.seqs = 3;
    a.n_states = 20;
    a.n_frames = 100;
    a.states = device<int32_t>(4);
    a.states_pitch = 100;
    a.logp = device<float>(5);
    a.value = device<float>(6);
    a.value_frame_pitch = 20;
    a.value_seq_pitch = 2000;
    return a;
}

static bool refused(const jsgx_viterbi_args& a, const char* text) {
    char want[192];
    std::snprintf(want, sizeof want, "jsgx_viterbi_scratch_bytes: %s", text);
    return jsgx_viterbi_scratch_bytes(&a) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0;
}

static int64_t scratch_formula(int64_t seqs, int64_t S, int64_t T) {
    const int64_t blocks = (T + JSGX_VITERBI_BLOCK - 1) / JSGX_VITERBI_BLOCK;
    return (4 * seqs * S + 4 * seqs * blocks + 2 * seqs * T * S + 2 * seqs * blocks * S + 3) / 4 * 4;
}

int main() {
    EXPECT(jsgx_abi_version() == 1);
    EXPECT(sizeof(jsgx_viterbi_args) == 120);

    // the plan over the forms; short and missing outputs
    jsgx_viterbi_args a = good();
    char name[24];
    int32_t threads = 0, lds = 0, launches = 0;
    EXPECT(jsgx_viterbi_plan(&a, name, (int)sizeof name, &threads, &lds, &launches) == JSGX_OK);
    EXPECT(std::strcmp(name, "viterbi_dense_lds") == 0 && threads == 640 && lds == 4 * (20 * 20 + 40) && launches == 3);
    EXPECT(jsgx_viterbi_plan(&a, nullptr, 0, nullptr, nullptr, nullptr) == JSGX_OK);
    EXPECT(jsgx_viterbi_plan(&a, name, 23, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_viterbi_plan: bad argument") == 0);
    EXPECT(jsgx_viterbi_plan(nullptr, name, 24, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_viterbi_plan: null argument") == 0);
    for (int S : {1, 2, 63, 64, 65, JSGX_VITERBI_LDS_STATES, JSGX_VITERBI_LDS_STATES + 1, 512, 513, 1024, 1025, JSGX_VITERBI_MAX_STATES})
        for (int T : {1, JSGX_VITERBI_BLOCK, JSGX_VITERBI_BLOCK + 1, JSGX_VITERBI_MAX_FRAMES})
            for (int seqs : {1, 7}) {
                a = good();
                a.n_states = S, a.n_frames = T, a.seqs = seqs, a.emit_frame_pitch = a.trans_pitch = a.value_frame_pitch = S;
                a.emit_seq_pitch = a.value_seq_pitch = (int64_t)S * T, a.states_pitch = T;
                EXPECT(jsgx_viterbi_plan(&a, name, 24, &threads, &lds, &launches) == JSGX_OK);
                const bool in_lds = S <= JSGX_VITERBI_LDS_STATES;
                EXPECT(std::strcmp(name, in_lds ? "viterbi_dense_lds" : "viterbi_dense_mem") == 0);
                EXPECT(lds == (in_lds ? 4 * (S * S + 2 * S) : 8 * S) && lds <= JSGX_VITERBI_LDS_LIMIT);
                EXPECT(threads % 64 == 0 && threads >= 64 && threads <= JSGX_VITERBI_THREADS && (threads >= S || threads == JSGX_VITERBI_THREADS));
                EXPECT(launches == (T <= JSGX_VITERBI_BLOCK ? 3 : 4));
                EXPECT(jsgx_viterbi_scratch_bytes(&a) == scratch_formula(seqs, S, T));
            }
    // band shapes on both sides of the LDS fit: 4 ((2W+1) S + 2 S) <= 163840
    struct { int S, W; bool in_lds; } bands[] = {{1, 0, true}, {5, 4, true}, {40, 64, true}, {300, 25, true}, {312, 64, true}, {313, 64, false},
                                                  {1200, 25, false}, {2048, 64, false}, {2048, 8, true}, {2048, 9, false}};
    for (const auto& c : bands) {
        a = good();
        a.trans_form = JSGX_TRANS_BAND, a.band_half = c.W, a.n_states = c.S, a.emit_frame_pitch = a.trans_pitch = a.value_frame_pitch = c.S;
        a.emit_seq_pitch = a.value_seq_pitch = (int64_t)c.S * 100;
        EXPECT(jsgx_viterbi_plan(&a, name, 24, &threads, &lds, &launches) == JSGX_OK);
        EXPECT(std::strcmp(name, c.in_lds ? "viterbi_band_lds" : "viterbi_band_mem") == 0);
        EXPECT(lds == (c.in_lds ? 4 * ((2 * c.W + 1) * c.S + 2 * c.S) : 8 * c.S) && lds <= JSGX_VITERBI_LDS_LIMIT);
    }
    // the largest call
    a = good();
    a.seqs = 65535, a.n_states = JSGX_VITERBI_MAX_STATES, a.n_frames = JSGX_VITERBI_MAX_FRAMES, a.emit_frame_pitch = a.trans_pitch = a.value_frame_pitch = 2048;
    a.emit_seq_pitch = a.value_seq_pitch = (int64_t)2048 << 20, a.states_pitch = 1 << 20;
    a.log_emit = device<const float>(100), a.value = device<float>(200), a.states = device<int32_t>(300);
    EXPECT(jsgx_viterbi_scratch_bytes(&a) == scratch_formula(65535, 2048, 1 << 20));

    // one refusal of every kind, with its text
    a = good(); a.log_emit = nullptr; EXPECT(refused(a, "null log_emit"));
    a = good(); a.log_init = nullptr; EXPECT(refused(a, "null log_init"));
    a = good(); a.trans = nullptr; EXPECT(refused(a, "null trans"));
    a = good(); a.states = nullptr; EXPECT(refused(a, "null states"));
    a = good(); a.logp = device<float>(5, 2); EXPECT(refused(a, "pointers must be 4-byte aligned"));
    a = good(); a.seqs = 65536; EXPECT(refused(a, "seqs must be in 1..65535"));
    a = good(); a.n_states = 2049; a.emit_frame_pitch = a.trans_pitch = a.value_frame_pitch = 4096; EXPECT(refused(a, "n_states must be in 1..2048"));
    a = good(); a.n_frames = 0; EXPECT(refused(a, "n_frames must be in 1..2^20"));
    a = good(); a.n_frames = (1 << 20) + 1; EXPECT(refused(a, "n_frames must be in 1..2^20"));
    a = good(); a.trans_form = 2; EXPECT(refused(a, "trans_form must be 0 (dense) or 1 (band)"));
    a = good(); a.band_half = 1; EXPECT(refused(a, "band_half must be 0 with the dense form"));
    a = good(); a.trans_form = JSGX_TRANS_BAND; a.band_half = 65; EXPECT(refused(a, "band_half must be in 0..64"));
    a = good(); a.trans_form = JSGX_TRANS_BAND; a.band_half = -1; EXPECT(refused(a, "band_half must be in 0..64"));
    a = good(); a.reserved0 = 1; EXPECT(refused(a, "reserved0 must be 0"));
    a = good(); a.emit_frame_pitch = 19; EXPECT(refused(a, "emit_frame_pitch smaller than n_states"));
    a = good(); a.emit_seq_pitch = 99 * 24 + 19; EXPECT(refused(a, "emit_seq_pitch does not cover a sequence"));
    a = good(); a.emit_seq_pitch = 99 * 24 + 20; EXPECT(jsgx_viterbi_scratch_bytes(&a) > 0);
    a = good(); a.trans_pitch = 19; EXPECT(refused(a, "trans_pitch smaller than n_states"));
    a = good(); a.states_pitch = 99; EXPECT(refused(a, "states_pitch smaller than n_frames"));
    a = good(); a.value_frame_pitch = 19; EXPECT(refused(a, "value_frame_pitch smaller than n_states"));
    a = good(); a.value_seq_pitch = 1999; EXPECT(refused(a, "value_seq_pitch does not cover a sequence"));
    a = good(); a.value = nullptr; a.value_frame_pitch = a.value_seq_pitch = 0; EXPECT(jsgx_viterbi_scratch_bytes(&a) == scratch_formula(3, 20, 100));
    a = good(); a.states = reinterpret_cast<int32_t*>(const_cast<float*>(a.log_emit)) + 2 * 2400 + 99 * 24 + 19; EXPECT(refused(a, "an output overlaps log_emit"));
    a = good(); a.states = reinterpret_cast<int32_t*>(const_cast<float*>(a.log_emit)) + 2 * 2400 + 99 * 24 + 20; EXPECT(jsgx_viterbi_scratch_bytes(&a) > 0);
    a = good(); a.logp = const_cast<float*>(a.log_init) + 19; EXPECT(refused(a, "an output overlaps log_init"));
    a = good(); a.value = const_cast<float*>(a.trans) - 5999; EXPECT(refused(a, "an output overlaps trans"));
    a = good(); a.value = const_cast<float*>(a.trans) - 6000; EXPECT(jsgx_viterbi_scratch_bytes(&a) > 0);
    a = good(); a.logp = reinterpret_cast<float*>(a.states) + 299; EXPECT(refused(a, "an output overlaps another output"));
    a = good(); a.logp = reinterpret_cast<float*>(a.states) + 300; EXPECT(jsgx_viterbi_scratch_bytes(&a) > 0);
    // one sequence: the sequence pitches are not looked at
    a = good(); a.seqs = 1; a.emit_seq_pitch = a.value_seq_pitch = a.states_pitch = 0; EXPECT(jsgx_viterbi_scratch_bytes(&a) == scratch_formula(1, 20, 100));
    EXPECT(jsgx_viterbi_scratch_bytes(nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_viterbi_scratch_bytes: null argument") == 0);

    // the band builder: the tables are real host memory here, with a guard row behind them
    for (int S : {1, 2, 7, 40}) {
        for (int W : {0, 1, 3, 64}) {
            std::vector<double> window(2 * W + 1);
            for (int k = 0; k <= 2 * W; ++k) window[k] = k % 5 == 4 && k != W ? 0.0 : 1.0 + 0.25 * k;
            const int pitch = S + 3;
            std::vector<float> out((size_t)(2 * W + 2) * pitch, 777.f);
            EXPECT(jsgx_viterbi_band_build(S, W, window.data(), out.data(), pitch) == JSGX_OK);
            for (int i = 0; i < S; ++i) {
                double p = 0.0;
                for (int j = 0; j < S; ++j)
                    if (j - i >= -W && j - i <= W) p += std::exp((double)out[(size_t)(i - j + W) * pitch + j]);
                EXPECT(std::fabs(p - 1.0) <= 4 * 5.9604644775390625e-08);        // 4 u
            }
            for (int r = 0; r <= 2 * W; ++r)
                for (int j = 0; j < pitch; ++j) {
                    const int i = j + r - W;
                    const float v = out[(size_t)r * pitch + j];
                    if (j >= S) EXPECT(v == 777.f);
                    else if (i < 0 || i >= S || window[2 * W - r] == 0.0) EXPECT(std::isinf(v) && v < 0);
                    else EXPECT(std::isfinite(v) && v <= 0);
                }
            for (int j = 0; j < pitch; ++j) EXPECT(out[(size_t)(2 * W + 1) * pitch + j] == 777.f);
        }
    }
    double w3[3] = {1.0, 2.0, 1.0};
    float out3[3 * 4];
    EXPECT(jsgx_viterbi_band_build(4, 1, nullptr, out3, 4) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_viterbi_band_build: null window") == 0);
    EXPECT(jsgx_viterbi_band_build(4, 1, w3, nullptr, 4) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_viterbi_band_build: null out") == 0);
    EXPECT(jsgx_viterbi_band_build(0, 1, w3, out3, 4) == JSGX_ERR_INVALID && jsgx_viterbi_band_build(2049, 1, w3, out3, 4096) == JSGX_ERR_INVALID);
    EXPECT(jsgx_viterbi_band_build(4, -1, w3, out3, 4) == JSGX_ERR_INVALID && jsgx_viterbi_band_build(4, 65, w3, out3, 4) == JSGX_ERR_INVALID);
    w3[0] = -1.0; EXPECT(jsgx_viterbi_band_build(4, 1, w3, out3, 4) == JSGX_ERR_INVALID);
    w3[0] = NAN; EXPECT(jsgx_viterbi_band_build(4, 1, w3, out3, 4) == JSGX_ERR_INVALID);
    w3[0] = INFINITY; EXPECT(jsgx_viterbi_band_build(4, 1, w3, out3, 4) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_viterbi_band_build: window entries must be finite and >= 0") == 0);
    w3[0] = 1.0; w3[1] = 0.0; EXPECT(jsgx_viterbi_band_build(4, 1, w3, out3, 4) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_viterbi_band_build: window[band_half] must be > 0") == 0);
    w3[1] = 2.0; EXPECT(jsgx_viterbi_band_build(4, 1, w3, out3, 3) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_viterbi_band_build: out_pitch smaller than n_states") == 0);
    EXPECT(jsgx_viterbi_band_build(4, 1, w3, out3, 4) == JSGX_OK && out3[4 + 1] == (float)std::log(2.0 / 4.0) && out3[4 + 0] == (float)std::log(2.0 / 3.0));

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
