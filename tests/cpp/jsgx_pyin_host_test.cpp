// The host entry points of section 5 of libjsgx.so (include/jsgx.h) from C++: the four table builders on real host buffers with guards
// behind them, the refusals with their texts, the plans and the scratch size.  No launch, so no device: built against libjsgx.so (CMake,
// jsg::jsgx) or, for the sanitizers, together with csrc/jsgx_beat_host.cpp, csrc/jsgx_viterbi_host.cpp and csrc/jsgx_pyin_host.cpp
// themselves (tests/test_pyin_host.py: -fsanitize=address,undefined).  Exit code 0 and "ok" on success.
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

static bool said(int rc, const char* who, const char* text) {
    char want[192];
    std::snprintf(want, sizeof want, "%s: %s", who, text);
    return rc == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0;
}

static jsgx_pyin_observe_args observe() {
    jsgx_pyin_observe_args a{};
    a.cmnd = device<const float>(1);
    a.cmnd_frame_pitch = 344, a.cmnd_row_pitch = 100 * 344;
    a.rows = 3, a.n_frames = 100, a.tau_min = 10, a.tau_max = 338;
    a.prior = device<const float>(2), a.decay = device<const float>(3), a.norm = device<const float>(4), a.edges = device<const float>(5);
    a.n_thresholds = 100, a.boltz_len = 164, a.n_bins = 601, a.no_trough_prob = 0.01f;
    a.log_emit = device<float>(6);
    a.emit_frame_pitch = 1202, a.emit_row_pitch = 100 * 1202;
    a.obs = device<float>(7);
    a.obs_frame_pitch = 601, a.obs_row_pitch = 100 * 601;
    a.voiced_prob = device<float>(8);
    a.voiced_pitch = 100;
    return a;
}

static jsgx_pyin_decode_args decode() {
    jsgx_pyin_decode_args a{};
    a.log_emit = device<const float>(1);
    a.emit_frame_pitch = 1202, a.emit_seq_pitch = 100 * 1202;
    a.log_init = device<const float>(2), a.log_window = device<const float>(3), a.src_offset = device<const float>(4), a.log_switch = device<const float>(5);
    a.n_bins = 601, a.band_half = 50, a.seqs = 3, a.n_frames = 100;
    a.states = device<int32_t>(6);
    a.states_pitch = 100;
    a.logp = device<float>(7);
    a.value = device<float>(8);
    a.value_frame_pitch = 1202, a.value_seq_pitch = 100 * 1202;
    return a;
}

static int64_t scratch_formula(int64_t seqs, int64_t S, int64_t T) {
    const int64_t blocks = (T + JSGX_VITERBI_BLOCK - 1) / JSGX_VITERBI_BLOCK;
    return (4 * seqs * S + 4 * seqs * blocks + 2 * seqs * T * S + 2 * seqs * blocks * S + 3) / 4 * 4;
}

int main() {
    EXPECT(jsgx_abi_version() == 1);
    EXPECT(sizeof(jsgx_pyin_observe_args) == 152 && sizeof(jsgx_pyin_decode_args) == 120);
    const float guard = 777.f;

    // the prior: sums to one, every size, a guard behind it
    for (int N : {1, 7, 100, JSGX_PYIN_MAX_THRESHOLDS}) {
        std::vector<float> out(N + 1, guard);
        EXPECT(jsgx_pyin_prior_build(N, 2.0, 18.0, out.data()) == JSGX_OK && out[N] == guard);
        double sum = 0.0;
        for (int k = 0; k < N; ++k) {
            sum += out[k];
            EXPECT(out[k] >= 0.f);
        }
        EXPECT(std::fabs(sum - 1.0) <= N * 5.9604644775390625e-08);
    }
    float one = 0.f;
    EXPECT(jsgx_pyin_prior_build(1, 0.5, 0.5, &one) == JSGX_OK && one == 1.0f);
    EXPECT(said(jsgx_pyin_prior_build(1, 2.0, 18.0, nullptr), "jsgx_pyin_prior_build", "null out"));
    EXPECT(said(jsgx_pyin_prior_build(0, 2.0, 18.0, &one), "jsgx_pyin_prior_build", "n_thresholds must be in 1..256"));
    EXPECT(said(jsgx_pyin_prior_build(257, 2.0, 18.0, &one), "jsgx_pyin_prior_build", "n_thresholds must be in 1..256"));
    EXPECT(said(jsgx_pyin_prior_build(1, 0.0, 18.0, &one), "jsgx_pyin_prior_build", "a and b must be finite and > 0"));
    EXPECT(said(jsgx_pyin_prior_build(1, 2.0, INFINITY, &one), "jsgx_pyin_prior_build", "a and b must be finite and > 0"));
    EXPECT(said(jsgx_pyin_prior_build(1, NAN, 1.0, &one), "jsgx_pyin_prior_build", "a and b must be finite and > 0"));

    // the Boltzmann tables: the pmf of m troughs sums to one
    for (int n : {1, 2, 164, JSGX_PYIN_MAX_LAG}) {
        std::vector<float> decay(n + 1, guard), norm(n + 2, guard);
        EXPECT(jsgx_pyin_boltzmann_build(2.0, n, decay.data(), norm.data()) == JSGX_OK && decay[n] == guard && norm[n + 1] == guard);
        EXPECT(decay[0] == 1.0f && norm[0] == 0.f && norm[1] == 1.0f);
        for (int m : {1, 2, n}) {
            if (m > n) continue;
            double sum = 0.0;
            for (int i = 0; i < m; ++i) sum += (double)norm[m] * decay[i];
            EXPECT(std::fabs(sum - 1.0) <= 4 * 5.9604644775390625e-08);
        }
    }
    float d1[2], n1[2];
    EXPECT(said(jsgx_pyin_boltzmann_build(2.0, 1, nullptr, n1), "jsgx_pyin_boltzmann_build", "null decay"));
    EXPECT(said(jsgx_pyin_boltzmann_build(2.0, 1, d1, nullptr), "jsgx_pyin_boltzmann_build", "null norm"));
    EXPECT(said(jsgx_pyin_boltzmann_build(0.0, 1, d1, n1), "jsgx_pyin_boltzmann_build", "lambda must be finite and > 0"));
    EXPECT(said(jsgx_pyin_boltzmann_build(NAN, 1, d1, n1), "jsgx_pyin_boltzmann_build", "lambda must be finite and > 0"));
    EXPECT(said(jsgx_pyin_boltzmann_build(2.0, 0, d1, n1), "jsgx_pyin_boltzmann_build", "n must be in 1..4096"));
    EXPECT(said(jsgx_pyin_boltzmann_build(2.0, 4097, d1, n1), "jsgx_pyin_boltzmann_build", "n must be in 1..4096"));

    // the bins: descending periods around the frequencies
    for (int P : {1, 2, 601, JSGX_PYIN_MAX_BINS}) {
        std::vector<float> edges(P + 2, guard), freqs(P + 1, guard);
        EXPECT(jsgx_pyin_bins_build(22050.0, 65.40639132514966, 10, P, edges.data(), freqs.data()) == JSGX_OK && edges[P + 1] == guard && freqs[P] == guard);
        for (int b = 0; b < P; ++b) EXPECT(edges[b] > 22050.0f / freqs[b] && 22050.0f / freqs[b] > edges[b + 1]);
    }
    float e2[2], f1[1];
    EXPECT(said(jsgx_pyin_bins_build(22050.0, 65.4, 10, 1, nullptr, f1), "jsgx_pyin_bins_build", "null edges"));
    EXPECT(said(jsgx_pyin_bins_build(22050.0, 65.4, 10, 1, e2, nullptr), "jsgx_pyin_bins_build", "null freqs"));
    EXPECT(said(jsgx_pyin_bins_build(0.0, 65.4, 10, 1, e2, f1), "jsgx_pyin_bins_build", "sample_rate must be finite and > 0"));
    EXPECT(said(jsgx_pyin_bins_build(22050.0, -1.0, 10, 1, e2, f1), "jsgx_pyin_bins_build", "fmin must be finite and > 0"));
    EXPECT(said(jsgx_pyin_bins_build(22050.0, 65.4, 0, 1, e2, f1), "jsgx_pyin_bins_build", "bins_per_semitone must be in 1..1024"));
    EXPECT(said(jsgx_pyin_bins_build(22050.0, 65.4, 10, 0, e2, f1), "jsgx_pyin_bins_build", "n_bins must be in 1..1024"));
    EXPECT(said(jsgx_pyin_bins_build(22050.0, 65.4, 10, 1025, e2, f1), "jsgx_pyin_bins_build", "n_bins must be in 1..1024"));

    // the transition: every source's row of exp(src_offset + log_window) sums to one
    for (int P : {1, 2, 40, 601})
        for (int W : {0, 1, 50, JSGX_PYIN_MAX_BAND_HALF}) {
            std::vector<double> window(2 * W + 1);
            for (int k = 0; k <= 2 * W; ++k) window[k] = k % 5 == 4 && k != W ? 0.0 : 1.0 + 0.25 * k;
            std::vector<float> lw(2 * W + 2, guard), off(P + 1, guard), sw(5, guard);
            EXPECT(jsgx_pyin_transition_build(P, W, window.data(), 0.01, lw.data(), off.data(), sw.data()) == JSGX_OK);
            EXPECT(lw[2 * W + 1] == guard && off[P] == guard && sw[4] == guard);
            for (int p = 0; p < P; ++p) {
                // a table entry x carries |x| 2^-24 from its one rounding, and so does its term of the sum, relatively
                double sum = 0.0, largest = 0.0;
                for (int d = 0; d < P; ++d)
                    if (d - p >= -W && d - p <= W && window[d - p + W] > 0.0) {
                        sum += std::exp((double)off[p] + lw[d - p + W]);
                        largest = std::fmax(largest, std::fabs((double)lw[d - p + W]));
                    }
                EXPECT(std::fabs(sum - 1.0) <= (std::fabs((double)off[p]) + largest + 1.0) * 5.9604644775390625e-08);
            }
            EXPECT(sw[0] == sw[3] && sw[1] == sw[2] && sw[0] == (float)std::log(0.99) && sw[1] == (float)std::log(0.01));
        }
    double w3[3] = {1.0, 2.0, 1.0};
    float lw3[3], off4[4], sw4[4];
    const char* tb = "jsgx_pyin_transition_build";
    EXPECT(said(jsgx_pyin_transition_build(4, 1, nullptr, 0.01, lw3, off4, sw4), tb, "null window"));
    EXPECT(said(jsgx_pyin_transition_build(4, 1, w3, 0.01, nullptr, off4, sw4), tb, "null log_window"));
    EXPECT(said(jsgx_pyin_transition_build(4, 1, w3, 0.01, lw3, nullptr, sw4), tb, "null src_offset"));
    EXPECT(said(jsgx_pyin_transition_build(4, 1, w3, 0.01, lw3, off4, nullptr), tb, "null log_switch"));
    EXPECT(said(jsgx_pyin_transition_build(0, 1, w3, 0.01, lw3, off4, sw4), tb, "n_bins must be in 1..1024"));
    EXPECT(said(jsgx_pyin_transition_build(4, 129, w3, 0.01, lw3, off4, sw4), tb, "band_half must be in 0..128"));
    EXPECT(said(jsgx_pyin_transition_build(4, -1, w3, 0.01, lw3, off4, sw4), tb, "band_half must be in 0..128"));
    w3[0] = -1.0; EXPECT(said(jsgx_pyin_transition_build(4, 1, w3, 0.01, lw3, off4, sw4), tb, "window entries must be finite and >= 0"));
    w3[0] = NAN; EXPECT(said(jsgx_pyin_transition_build(4, 1, w3, 0.01, lw3, off4, sw4), tb, "window entries must be finite and >= 0"));
    w3[0] = 1.0; w3[1] = 0.0; EXPECT(said(jsgx_pyin_transition_build(4, 1, w3, 0.01, lw3, off4, sw4), tb, "window[band_half] must be > 0"));
    w3[1] = 2.0; EXPECT(said(jsgx_pyin_transition_build(4, 1, w3, 1.5, lw3, off4, sw4), tb, "switch_prob must be in [0, 1]"));
    EXPECT(said(jsgx_pyin_transition_build(4, 1, w3, NAN, lw3, off4, sw4), tb, "switch_prob must be in [0, 1]"));
    EXPECT(jsgx_pyin_transition_build(4, 1, w3, 0.0, lw3, off4, sw4) == JSGX_OK && sw4[0] == 0.f && std::isinf(sw4[1]) && sw4[1] < 0);
    EXPECT(lw3[1] == (float)std::log(2.0) && off4[0] == (float)-std::log(3.0) && off4[1] == (float)-std::log(4.0));

    // the plans
    char name[16];
    int32_t threads = 0, lds = 0, frames = 0, G = 0, launches = 0;
    jsgx_pyin_observe_args o = observe();
    EXPECT(jsgx_pyin_observe_plan(&o, name, 16, &threads, &lds, &frames) == JSGX_OK && std::strcmp(name, "pyin_observe") == 0);
    EXPECT(threads == JSGX_PYIN_OBSERVE_THREADS && frames == 1 && lds == 4 * (339 + 3 * 165 + 601));
    EXPECT(jsgx_pyin_observe_plan(&o, nullptr, 0, nullptr, nullptr, nullptr) == JSGX_OK);
    EXPECT(said(jsgx_pyin_observe_plan(&o, name, 15, nullptr, nullptr, nullptr), "jsgx_pyin_observe_plan", "bad argument"));
    EXPECT(said(jsgx_pyin_observe_plan(nullptr, name, 16, nullptr, nullptr, nullptr), "jsgx_pyin_observe_plan", "null argument"));
    o.tau_min = 1, o.tau_max = JSGX_PYIN_MAX_LAG, o.boltz_len = JSGX_PYIN_MAX_LAG / 2, o.n_bins = JSGX_PYIN_MAX_BINS, o.cmnd_frame_pitch = 4097, o.cmnd_row_pitch = 409700;
    o.emit_frame_pitch = 2048, o.emit_row_pitch = 204800, o.obs_frame_pitch = 1024, o.obs_row_pitch = 102400;
    EXPECT(jsgx_pyin_observe_plan(&o, name, 16, &threads, &lds, &frames) == JSGX_OK && lds == 4 * (4097 + 3 * 2049 + 1024) && lds <= 65536);
    jsgx_pyin_decode_args d = decode();
    EXPECT(jsgx_pyin_decode_plan(&d, name, 16, &G, &threads, &lds, &launches) == JSGX_OK && std::strcmp(name, "pyin_decode") == 0);
    EXPECT(G == 1 && threads == 640 && lds == 4 * (4 * 701 + 101) && launches == 3);
    EXPECT(jsgx_pyin_decode_scratch_bytes(&d) == scratch_formula(3, 1202, 100));
    for (int P : {1, 16, 17, 512, 513, JSGX_PYIN_MAX_BINS})
        for (int W : {0, JSGX_PYIN_MAX_BAND_HALF})
            for (int T : {1, JSGX_VITERBI_BLOCK, JSGX_VITERBI_BLOCK + 1, JSGX_VITERBI_MAX_FRAMES}) {
                d = decode();
                d.n_bins = P, d.band_half = W, d.n_frames = T, d.emit_frame_pitch = d.value_frame_pitch = 2 * P, d.emit_seq_pitch = d.value_seq_pitch = (int64_t)2 * P * T;
                d.states_pitch = T;
                d.log_emit = device<const float>(100), d.value = device<float>(200), d.states = device<int32_t>(300);
                EXPECT(jsgx_pyin_decode_plan(&d, name, 16, &G, &threads, &lds, &launches) == JSGX_OK);
                EXPECT(G >= 1 && G <= 64 && (G & (G - 1)) == 0 && (G == 1 || (P * G <= 512 && 8 * G <= 2 * W + 1)) && (G == 64 || P * G * 2 > 512 || 16 * G > 2 * W + 1));
                EXPECT(threads % 64 == 0 && threads >= P * G && threads < P * G + 64 && lds == 4 * (4 * (P + 2 * W) + 2 * W + 1) && lds <= 65536);
                EXPECT(launches == (T <= JSGX_VITERBI_BLOCK ? 3 : 4) && jsgx_pyin_decode_scratch_bytes(&d) == scratch_formula(3, 2 * P, T));
            }
    EXPECT(said(jsgx_pyin_decode_plan(&d, name, 15, nullptr, nullptr, nullptr, nullptr), "jsgx_pyin_decode_plan", "bad argument"));

    // one refusal of every kind of the observation, with its text
    const char* ol = "jsgx_pyin_observe_plan";      // the plan refuses what the launch refuses, and lives in a host unit
    auto orc = [&](const jsgx_pyin_observe_args& a) { return jsgx_pyin_observe_plan(&a, nullptr, 0, nullptr, nullptr, nullptr); };
    o = observe(); o.cmnd = nullptr; EXPECT(said(orc(o), ol, "null cmnd"));
    o = observe(); o.prior = nullptr; EXPECT(said(orc(o), ol, "null prior"));
    o = observe(); o.decay = nullptr; EXPECT(said(orc(o), ol, "null decay"));
    o = observe(); o.norm = nullptr; EXPECT(said(orc(o), ol, "null norm"));
    o = observe(); o.edges = nullptr; EXPECT(said(orc(o), ol, "null edges"));
    o = observe(); o.log_emit = nullptr; EXPECT(said(orc(o), ol, "null log_emit"));
    o = observe(); o.obs = device<float>(7, 2); EXPECT(said(orc(o), ol, "pointers must be 4-byte aligned"));
    o = observe(); o.rows = 0; EXPECT(said(orc(o), ol, "rows must be in 1..65535"));
    o = observe(); o.n_frames = (1 << 20) + 1; EXPECT(said(orc(o), ol, "n_frames must be in 1..2^20"));
    o = observe(); o.tau_max = 4097; EXPECT(said(orc(o), ol, "tau_max must be in 1..4096"));
    o = observe(); o.tau_min = 0; EXPECT(said(orc(o), ol, "tau_min must be in 1..tau_max"));
    o = observe(); o.tau_min = 339; EXPECT(said(orc(o), ol, "tau_min must be in 1..tau_max"));
    o = observe(); o.n_thresholds = 257; EXPECT(said(orc(o), ol, "n_thresholds must be in 1..256"));
    o = observe(); o.n_bins = 1025; EXPECT(said(orc(o), ol, "n_bins must be in 1..1024"));
    o = observe(); o.boltz_len = 163; EXPECT(said(orc(o), ol, "boltz_len must be in max(1, (tau_max - tau_min + 1) / 2)..4096"));
    o = observe(); o.no_trough_prob = 1.5f; EXPECT(said(orc(o), ol, "no_trough_prob must be in [0, 1]"));
    o = observe(); o.no_trough_prob = NAN; EXPECT(said(orc(o), ol, "no_trough_prob must be in [0, 1]"));
    o = observe(); o.cmnd_frame_pitch = 338; EXPECT(said(orc(o), ol, "cmnd_frame_pitch smaller than tau_max + 1"));
    o = observe(); o.cmnd_row_pitch = 99 * 344 + 338; EXPECT(said(orc(o), ol, "cmnd_row_pitch does not cover a row"));
    o = observe(); o.emit_frame_pitch = 1201; EXPECT(said(orc(o), ol, "emit_frame_pitch smaller than 2 * n_bins"));
    o = observe(); o.emit_row_pitch = 100 * 1202 - 1; EXPECT(said(orc(o), ol, "emit_row_pitch does not cover a row"));
    o = observe(); o.obs_frame_pitch = 600; EXPECT(said(orc(o), ol, "obs_frame_pitch smaller than n_bins"));
    o = observe(); o.obs_row_pitch = 100 * 601 - 1; EXPECT(said(orc(o), ol, "obs_row_pitch does not cover a row"));
    o = observe(); o.voiced_pitch = 99; EXPECT(said(orc(o), ol, "voiced_pitch smaller than n_frames"));
    o = observe(); o.voiced_prob = const_cast<float*>(o.cmnd) + 5; EXPECT(said(orc(o), ol, "an output overlaps cmnd"));
    o = observe(); o.voiced_prob = const_cast<float*>(o.prior) + 99; EXPECT(said(orc(o), ol, "an output overlaps prior"));
    o = observe(); o.voiced_prob = const_cast<float*>(o.decay) + 163; EXPECT(said(orc(o), ol, "an output overlaps decay"));
    o = observe(); o.voiced_prob = const_cast<float*>(o.norm) + 164; EXPECT(said(orc(o), ol, "an output overlaps norm"));
    o = observe(); o.voiced_prob = const_cast<float*>(o.edges) + 601; EXPECT(said(orc(o), ol, "an output overlaps edges"));
    o = observe(); o.voiced_prob = o.log_emit + 7; EXPECT(said(orc(o), ol, "an output overlaps another output"));
    // what lies next to an input passes every refusal: the plan says so without a device
    o = observe(); o.voiced_prob = const_cast<float*>(o.edges) + 602; EXPECT(jsgx_pyin_observe_plan(&o, nullptr, 0, nullptr, nullptr, nullptr) == JSGX_OK);
    o = observe(); o.rows = 1; o.cmnd_row_pitch = o.emit_row_pitch = o.obs_row_pitch = o.voiced_pitch = 0; EXPECT(jsgx_pyin_observe_plan(&o, nullptr, 0, nullptr, nullptr, nullptr) == JSGX_OK);
    o = observe(); o.obs = nullptr; o.voiced_prob = nullptr; o.obs_frame_pitch = o.obs_row_pitch = o.voiced_pitch = 0; EXPECT(jsgx_pyin_observe_plan(&o, nullptr, 0, nullptr, nullptr, nullptr) == JSGX_OK);

    // ... and of the decoder
    const char* ds = "jsgx_pyin_decode_scratch_bytes";
    auto drc = [&](const jsgx_pyin_decode_args& a) { return (int)jsgx_pyin_decode_scratch_bytes(&a); };
    EXPECT(said((int)jsgx_pyin_decode_scratch_bytes(nullptr), ds, "null argument"));
    d = decode(); d.log_emit = nullptr; EXPECT(said(drc(d), ds, "null log_emit"));
    d = decode(); d.log_init = nullptr; EXPECT(said(drc(d), ds, "null log_init"));
    d = decode(); d.log_window = nullptr; EXPECT(said(drc(d), ds, "null log_window"));
    d = decode(); d.src_offset = nullptr; EXPECT(said(drc(d), ds, "null src_offset"));
    d = decode(); d.log_switch = nullptr; EXPECT(said(drc(d), ds, "null log_switch"));
    d = decode(); d.states = nullptr; EXPECT(said(drc(d), ds, "null states"));
    d = decode(); d.logp = device<float>(7, 1); EXPECT(said(drc(d), ds, "pointers must be 4-byte aligned"));
    d = decode(); d.seqs = 65536; EXPECT(said(drc(d), ds, "seqs must be in 1..65535"));
    d = decode(); d.n_bins = 0; EXPECT(said(drc(d), ds, "n_bins must be in 1..1024"));
    d = decode(); d.band_half = 129; EXPECT(said(drc(d), ds, "band_half must be in 0..128"));
    d = decode(); d.n_frames = 0; EXPECT(said(drc(d), ds, "n_frames must be in 1..2^20"));
    d = decode(); d.emit_frame_pitch = 1201; EXPECT(said(drc(d), ds, "emit_frame_pitch smaller than 2 * n_bins"));
    d = decode(); d.emit_seq_pitch = 100 * 1202 - 1; EXPECT(said(drc(d), ds, "emit_seq_pitch does not cover a sequence"));
    d = decode(); d.states_pitch = 99; EXPECT(said(drc(d), ds, "states_pitch smaller than n_frames"));
    d = decode(); d.value_frame_pitch = 1201; EXPECT(said(drc(d), ds, "value_frame_pitch smaller than 2 * n_bins"));
    d = decode(); d.value_seq_pitch = 100 * 1202 - 1; EXPECT(said(drc(d), ds, "value_seq_pitch does not cover a sequence"));
    d = decode(); d.logp = const_cast<float*>(d.log_emit) + 9; EXPECT(said(drc(d), ds, "an output overlaps log_emit"));
    d = decode(); d.logp = const_cast<float*>(d.log_init) + 1201; EXPECT(said(drc(d), ds, "an output overlaps log_init"));
    d = decode(); d.logp = const_cast<float*>(d.log_window) + 100; EXPECT(said(drc(d), ds, "an output overlaps log_window"));
    d = decode(); d.logp = const_cast<float*>(d.src_offset) + 600; EXPECT(said(drc(d), ds, "an output overlaps src_offset"));
    d = decode(); d.logp = const_cast<float*>(d.log_switch) + 3; EXPECT(said(drc(d), ds, "an output overlaps log_switch"));
    d = decode(); d.logp = const_cast<float*>(d.log_switch) + 4; EXPECT(jsgx_pyin_decode_scratch_bytes(&d) == scratch_formula(3, 1202, 100));
    d = decode(); d.logp = reinterpret_cast<float*>(d.states) + 299; EXPECT(said(drc(d), ds, "an output overlaps another output"));
    d = decode(); d.seqs = 1; d.emit_seq_pitch = d.value_seq_pitch = d.states_pitch = 0; EXPECT(jsgx_pyin_decode_scratch_bytes(&d) == scratch_formula(1, 1202, 100));

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
