// The host entry points of sections 6 to 8 of libjsgx.so (include/jsgx.h) from C++: the refusals with their texts, the scratch size and the
// plan of the neighbour search, and the refusals of the recurrence plane and of nn_filter up to the device question.  No kernel runs, so no
// device is needed: built against libjsgx.so (CMake, jsg::jsgx) or, for the sanitizers, together with csrc/jsgx_beat_host.cpp and
// csrc/jsgx_knn_host.cpp themselves (tests/test_knn_host.py: -fsanitize=address,undefined); the launches live in the HIP unit and are called
// only where JSGX_KNN_TEST_LAUNCHES is defined (the build against the library).  Exit code 0 and "ok" on success.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <utility>

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
static T* device(int k, int64_t elements = 0) {       // device pointers that are never dereferenced: every call below is refused, sized or planned
    return reinterpret_cast<T*>((uintptr_t(k) << 44) + 4 * elements);
}

static jsgx_knn_args good() {       // 3 pairs of 100 x 300 frames of 20 features, k = 10
    jsgx_knn_args a{};
    a.x = device<const float>(1);
    a.x_frame_pitch = 24;
    a.x_pair_pitch = 100 * 24;
    a.y = device<const float>(2);
    a.y_frame_pitch = 20;
    a.y_pair_pitch = 300 * 20;
    a.pairs = 3;
    a.n_features = 20;
    a.n = 100;
    a.m = 300;
    a.metric = JSGX_METRIC_EUCLIDEAN;
    a.k = 10;
    a.width = 1;
    a.split = 0;
    a.nn_index = device<int32_t>(3);
    a.index_pitch = 12;
    a.index_pair_pitch = 1200;
    a.nn_dist = device<float>(4);
    a.dist_pitch = 10;
    a.dist_pair_pitch = 1000;
    return a;
}

static bool refused(const jsgx_knn_args& a, const char* text) {
    char want[192];
    std::snprintf(want, sizeof want, "jsgx_knn_scratch_bytes: %s", text);
    const bool sized = jsgx_knn_scratch_bytes(&a) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0;
    std::snprintf(want, sizeof want, "jsgx_knn_plan: %s", text);
    return sized && jsgx_knn_plan(&a, 256, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0;
}

static int auto_split(int64_t pairs, int n, int m, int n_cu) {
    const int64_t strips = pairs * ((n + JSGX_KNN_STRIP - 1) / JSGX_KNN_STRIP);
    const int tiles = (m + JSGX_KNN_TILE - 1) / JSGX_KNN_TILE;
    int S = 1;
    while (S < 16 && strips * S < n_cu && 2 * S <= tiles) S *= 2;
    return S;
}

int main() {
    EXPECT(jsgx_abi_version() == 1);
    EXPECT(sizeof(jsgx_knn_args) == 128 && sizeof(jsgx_recurrence_args) == 112 && sizeof(jsgx_nn_filter_args) == 112);

    jsgx_knn_args a = good();
    char name[16];
    int32_t strip = 0, S = 0, threads = 0, lds = 0;
    EXPECT(jsgx_knn_plan(&a, 256, name, (int)sizeof name, &strip, &S, &threads, &lds) == JSGX_OK);
    EXPECT(std::strcmp(name, "knn_64") == 0 && strip == 64 && S == 4 && threads == 256 && lds == JSGX_KNN_LDS_STATIC + 384 * 10);
    EXPECT(jsgx_knn_plan(&a, 256, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == JSGX_OK);
    EXPECT(jsgx_knn_plan(&a, 256, name, 15, nullptr, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_knn_plan: bad argument") == 0);
    EXPECT(jsgx_knn_plan(&a, 0, name, 16, nullptr, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_knn_plan: n_cu must be >= 1") == 0);
    EXPECT(jsgx_knn_plan(nullptr, 256, name, 16, nullptr, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_knn_plan: null argument") == 0);
    // the automatic split against the compute units, the strips and the tiles; the scratch is sized for the largest answer
    for (int pairs : {1, 2, 3, 65535})
        for (int n : {1, 64, 65, 128, 129, 4096, 16384, 65536})
            for (int m : {1, 64, 65, 128, 129, 1024, 1025, 65536})
                for (int k : {1, 64, 65, 256}) {
                    a = good();
                    a.pairs = pairs, a.n = n, a.m = m, a.k = k, a.index_pitch = a.dist_pitch = k, a.index_pair_pitch = a.dist_pair_pitch = (int64_t)n * k;
                    a.x_pair_pitch = (int64_t)n * 24, a.y_pair_pitch = (int64_t)m * 20;
                    a.x = device<const float>(100), a.y = device<const float>(200), a.nn_index = device<int32_t>(300), a.nn_dist = device<float>(400);
                    const int tiles = (m + 63) / 64;
                    int largest = 1;
                    while (largest < 16 && 2 * largest <= tiles) largest *= 2;
                    for (int n_cu : {1, 4, 255, 256, 257, 304}) {
                        EXPECT(jsgx_knn_plan(&a, n_cu, name, 16, &strip, &S, &threads, &lds) == JSGX_OK);
                        EXPECT(S == auto_split(pairs, n, m, n_cu) && S <= largest && S <= tiles && strip == 64 && threads == 256);
                        EXPECT(lds == JSGX_KNN_LDS_STATIC + 384 * k && lds <= JSGX_KNN_LDS_LIMIT);
                    }
                    EXPECT(jsgx_knn_scratch_bytes(&a) == (largest > 1 ? 8ll * pairs * n * k * largest : 0));
                    for (int split : {1, 2, 3, 5, 16}) {
                        a.split = split;
                        const int want = split < tiles ? split : tiles;
                        EXPECT(jsgx_knn_plan(&a, 256, nullptr, 0, nullptr, &S, nullptr, nullptr) == JSGX_OK && S == want);
                        EXPECT(jsgx_knn_scratch_bytes(&a) == (want > 1 ? 8ll * pairs * n * k * want : 0));
                    }
                }
    // both sides of one workgroup per compute unit: 4 strips of one pair
    a = good(); a.pairs = 1; a.n = 256; a.m = 65536; a.x_pair_pitch = a.y_pair_pitch = 0;
    for (const auto& c : {std::pair<int, int>{4, 1}, {5, 2}, {8, 2}, {9, 4}, {32, 8}, {33, 16}, {64, 16}, {65, 16}, {1000, 16}}) {
        EXPECT(jsgx_knn_plan(&a, c.first, nullptr, 0, nullptr, &S, nullptr, nullptr) == JSGX_OK && S == c.second);
    }

    // one refusal of every kind, with its text, and the neighbour that passes
    a = good(); a.x = nullptr; EXPECT(refused(a, "null x"));
    a = good(); a.y = nullptr; EXPECT(refused(a, "null y"));
    a = good(); a.nn_index = nullptr; EXPECT(refused(a, "null nn_index"));
    a = good(); a.nn_dist = nullptr; EXPECT(refused(a, "null nn_dist"));
    a = good(); a.nn_dist = reinterpret_cast<float*>(reinterpret_cast<char*>(a.nn_dist) + 2); EXPECT(refused(a, "pointers must be 4-byte aligned"));
    a = good(); a.pairs = 0; EXPECT(refused(a, "pairs must be in 1..65535"));
    a = good(); a.pairs = 65536; EXPECT(refused(a, "pairs must be in 1..65535"));
    a = good(); a.n_features = 0; EXPECT(refused(a, "n_features must be in 1..1024"));
    a = good(); a.n_features = 1025; a.x_frame_pitch = a.y_frame_pitch = 2048; EXPECT(refused(a, "n_features must be in 1..1024"));
    a = good(); a.n = 0; EXPECT(refused(a, "n must be in 1..65536"));
    a = good(); a.n = 65537; EXPECT(refused(a, "n must be in 1..65536"));
    a = good(); a.m = 0; EXPECT(refused(a, "m must be in 1..65536"));
    a = good(); a.m = 65537; EXPECT(refused(a, "m must be in 1..65536"));
    a = good(); a.metric = 3; EXPECT(refused(a, "metric must be in 0..2"));
    a = good(); a.metric = -1; EXPECT(refused(a, "metric must be in 0..2"));
    a = good(); a.k = 0; EXPECT(refused(a, "k must be in 1..256"));
    a = good(); a.k = 257; a.index_pitch = a.dist_pitch = 512; a.index_pair_pitch = a.dist_pair_pitch = 51200; EXPECT(refused(a, "k must be in 1..256"));
    a = good(); a.k = 256; a.index_pitch = a.dist_pitch = 256; a.index_pair_pitch = a.dist_pair_pitch = 25600; EXPECT(jsgx_knn_scratch_bytes(&a) == 8ll * 3 * 100 * 256 * 4);
    a = good(); a.width = -1; EXPECT(refused(a, "width must be >= 0"));
    a = good(); a.width = 1 << 30; EXPECT(jsgx_knn_scratch_bytes(&a) > 0);
    a = good(); a.split = -1; EXPECT(refused(a, "split must be in 0..16"));
    a = good(); a.split = 17; EXPECT(refused(a, "split must be in 0..16"));
    a = good(); a.x_frame_pitch = 19; EXPECT(refused(a, "x_frame_pitch smaller than n_features"));
    a = good(); a.y_frame_pitch = 19; EXPECT(refused(a, "y_frame_pitch smaller than n_features"));
    a = good(); a.x_pair_pitch = 99 * 24 + 19; EXPECT(refused(a, "x_pair_pitch does not cover a sequence"));
    a = good(); a.x_pair_pitch = 99 * 24 + 20; EXPECT(jsgx_knn_scratch_bytes(&a) > 0);
    a = good(); a.x_pair_pitch = 0; EXPECT(jsgx_knn_scratch_bytes(&a) > 0);
    a = good(); a.y_pair_pitch = 299 * 20 + 19; EXPECT(refused(a, "y_pair_pitch does not cover a sequence"));
    a = good(); a.y_pair_pitch = 0; EXPECT(jsgx_knn_scratch_bytes(&a) > 0);
    a = good(); a.index_pitch = 9; EXPECT(refused(a, "index_pitch smaller than k"));
    a = good(); a.index_pair_pitch = 99 * 12 + 9; EXPECT(refused(a, "index_pair_pitch does not cover a plane"));
    a = good(); a.index_pair_pitch = 99 * 12 + 10; EXPECT(jsgx_knn_scratch_bytes(&a) > 0);
    a = good(); a.dist_pitch = 9; EXPECT(refused(a, "dist_pitch smaller than k"));
    a = good(); a.dist_pair_pitch = 999; EXPECT(refused(a, "dist_pair_pitch does not cover a plane"));
    a = good(); a.nn_index = reinterpret_cast<int32_t*>(const_cast<float*>(a.x)) + 2 * 2400 + 99 * 24 + 19; EXPECT(refused(a, "an output overlaps x"));
    a = good(); a.nn_index = reinterpret_cast<int32_t*>(const_cast<float*>(a.x)) + 2 * 2400 + 99 * 24 + 20; EXPECT(jsgx_knn_scratch_bytes(&a) > 0);
    a = good(); a.nn_dist = const_cast<float*>(a.y) - 2999; EXPECT(refused(a, "an output overlaps y"));
    a = good(); a.nn_dist = const_cast<float*>(a.y) - 3000; EXPECT(jsgx_knn_scratch_bytes(&a) > 0);
    a = good(); a.nn_dist = reinterpret_cast<float*>(a.nn_index) + 2 * 1200 + 99 * 12 + 9; EXPECT(refused(a, "nn_index overlaps nn_dist"));
    a = good(); a.nn_dist = reinterpret_cast<float*>(a.nn_index) + 2 * 1200 + 99 * 12 + 10; EXPECT(jsgx_knn_scratch_bytes(&a) > 0);
    // one pair: the pair pitches of the outputs are not looked at
    a = good(); a.pairs = 1; a.index_pair_pitch = a.dist_pair_pitch = 0; EXPECT(jsgx_knn_scratch_bytes(&a) == 8ll * 100 * 10 * 4);
    EXPECT(jsgx_knn_scratch_bytes(nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_knn_scratch_bytes: null argument") == 0);
    // the largest call
    a = good(); a.pairs = 65535; a.n = a.m = 65536; a.k = 256; a.n_features = 1024; a.x_frame_pitch = a.y_frame_pitch = 1024; a.x_pair_pitch = a.y_pair_pitch = 0;
    a.index_pitch = a.dist_pitch = 256; a.index_pair_pitch = a.dist_pair_pitch = 65536ll * 256; a.nn_index = device<int32_t>(1000); a.nn_dist = device<float>(100000);
    EXPECT(jsgx_knn_scratch_bytes(&a) == 8ll * 65535 * 65536 * 256 * 16);

#ifdef JSGX_KNN_TEST_LAUNCHES
    // what only the launches decide, in front of the device question: the scratch, and the refusals of sections 7 and 8
    a = good();
    const int64_t need = jsgx_knn_scratch_bytes(&a);
    EXPECT(jsgx_knn_launch(&a, nullptr, need, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_knn_launch: null scratch") == 0);
    EXPECT(jsgx_knn_launch(&a, device<char>(9, 0) + 2, need, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_knn_launch: scratch must be 4-byte aligned") == 0);
    EXPECT(jsgx_knn_launch(&a, device<char>(9), need - 1, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_knn_launch: scratch smaller than jsgx_knn_scratch_bytes") == 0);
    a.k = 0;
    EXPECT(jsgx_knn_launch(&a, nullptr, 0, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_knn_launch: k must be in 1..256") == 0);
    jsgx_recurrence_args r{};
    r.nn_index = device<const int32_t>(3); r.index_pitch = 12; r.index_pair_pitch = 1200; r.nn_dist = device<const float>(4); r.dist_pitch = 10; r.dist_pair_pitch = 1000;
    r.bandwidth = device<const float>(5); r.pairs = 3; r.n = 100; r.m = 100; r.k = 10; r.mode = JSGX_REC_AFFINITY; r.sym = 1; r.diag = 1;
    r.out = device<float>(6); r.out_pitch = 100; r.out_pair_pitch = 10000;
    jsgx_recurrence_args q = r;
    q.m = 101; q.out_pitch = 101; q.out_pair_pitch = 10100;
    EXPECT(jsgx_recurrence_launch(&q, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_recurrence_launch: sym needs n == m") == 0);
    q = r; q.out = const_cast<float*>(q.bandwidth) - 29999;
    EXPECT(jsgx_recurrence_launch(&q, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_recurrence_launch: out overlaps bandwidth") == 0);
    jsgx_nn_filter_args f{};
    f.s = device<const float>(1); f.s_frame_pitch = 24; f.s_pair_pitch = 2400; f.nn_index = device<const int32_t>(3); f.index_pitch = 12; f.index_pair_pitch = 1200;
    f.pairs = 3; f.n = 100; f.n_features = 20; f.k = 10; f.out = device<float>(1, 2 * 2400 + 99 * 24 + 19); f.out_frame_pitch = 20; f.out_pair_pitch = 2000;
    EXPECT(jsgx_nn_filter_launch(&f, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_nn_filter_launch: out overlaps s") == 0);
    f.n_features = 65537;
    EXPECT(jsgx_nn_filter_launch(&f, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_nn_filter_launch: n_features must be in 1..65536") == 0);
#endif

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
