// The host entry points of sections 2 and 3 of libjsgx.so (include/jsgx.h) from C++: the plans, the scratch size and the refusals with
// their texts.  No launch, so no device: built against libjsgx.so (CMake, jsg::jsgx) or, for the sanitizers, together with
// csrc/jsgx_beat_host.cpp and csrc/jsgx_dtw_host.cpp themselves (tests/test_dtw_host.py: -fsanitize=address,undefined).  Exit code 0 and
// "ok" on success.  It also walks the tile anti-diagonals that the launches of sections 3 and 9 take (csrc/jsgx_internal.h, its host part).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../../jadespectrogram_amd/csrc/jsgx_internal.h"

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

static jsgx_cdist_args good_cost() {
    jsgx_cdist_args a{};
    a.x = device<const float>(1);
    a.x_frame_pitch = 20;
    a.x_pair_pitch = 0;
    a.y = device<const float>(2);
    a.y_frame_pitch = 24;
    a.y_pair_pitch = 300 * 24;
    a.pairs = 3;
    a.n_features = 20;
    a.n = 100;
    a.m = 300;
    a.metric = JSGX_METRIC_COSINE;
    a.cost = device<float>(3);
    a.cost_pitch = 300;
    a.cost_pair_pitch = 100 * 300;
    return a;
}

static jsgx_dtw_args good_dtw() {
    jsgx_dtw_args a{};
    a.cost = device<const float>(3);
    a.cost_pitch = 300;
    a.cost_pair_pitch = 100 * 300;
    a.pairs = 3;
    a.n = 100;
    a.m = 300;
    for (int k = 0; k < 3; ++k) a.weights_mul[k] = 1.f;
    a.acc = device<float>(4);
    a.acc_pitch = 300;
    a.acc_pair_pitch = 100 * 300;
    a.path_i = device<int32_t>(5);
    a.path_j = device<int32_t>(6);
    a.path_pitch = 399;
    a.max_path = 399;
    a.path_len = device<int32_t>(7);
    a.total = device<float>(8);
    return a;
}

static bool refused(const jsgx_cdist_args& a, const char* text) {
    char want[192];
    std::snprintf(want, sizeof want, "jsgx_cdist_plan: %s", text);
    return jsgx_cdist_plan(&a, nullptr, 0, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0;
}

static bool refused(const jsgx_dtw_args& a, const char* text) {
    char want[192];
    std::snprintf(want, sizeof want, "jsgx_dtw_scratch_bytes: %s", text);
    return jsgx_dtw_scratch_bytes(&a) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0;
}

int main() {
    EXPECT(jsgx_abi_version() == 1);

    // the plan of the cost kernel; short and missing outputs
    jsgx_cdist_args c = good_cost();
    char name[16];
    int32_t threads = 0, lds = 0;
    EXPECT(jsgx_cdist_plan(&c, name, (int)sizeof name, &threads, &lds) == JSGX_OK);
    EXPECT(std::strcmp(name, "cdist_64x64") == 0 && threads == JSGX_CDIST_THREADS && lds == JSGX_CDIST_LDS_BYTES && lds <= 163840);
    EXPECT(jsgx_cdist_plan(&c, nullptr, 0, nullptr, nullptr) == JSGX_OK);
    EXPECT(jsgx_cdist_plan(&c, name, 15, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_cdist_plan: bad argument") == 0);
    EXPECT(jsgx_cdist_plan(nullptr, name, 16, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_cdist_plan: null argument") == 0);
    // the largest shape
    c = good_cost();
    c.pairs = 65535, c.n = c.m = JSGX_DTW_MAX_LEN, c.n_features = c.x_frame_pitch = c.y_frame_pitch = JSGX_CDIST_MAX_FEATURES;
    c.y_pair_pitch = 0, c.cost_pitch = JSGX_DTW_MAX_LEN, c.cost_pair_pitch = (int64_t)JSGX_DTW_MAX_LEN * JSGX_DTW_MAX_LEN;
    c.cost = device<float>(1000);
    EXPECT(jsgx_cdist_plan(&c, nullptr, 0, nullptr, nullptr) == JSGX_OK);

    // one refusal of every kind, with its text
    c = good_cost(); c.x = nullptr; EXPECT(refused(c, "null x"));
    c = good_cost(); c.y = nullptr; EXPECT(refused(c, "null y"));
    c = good_cost(); c.cost = nullptr; EXPECT(refused(c, "null cost"));
    c = good_cost(); c.y = device<const float>(2, 2); EXPECT(refused(c, "pointers must be 4-byte aligned"));
    c = good_cost(); c.pairs = 65536; EXPECT(refused(c, "pairs must be in 1..65535"));
    c = good_cost(); c.n_features = 1025; c.x_frame_pitch = c.y_frame_pitch = 2000; EXPECT(refused(c, "n_features must be in 1..1024"));
    c = good_cost(); c.n = 0; EXPECT(refused(c, "n must be in 1..65536"));
    c = good_cost(); c.m = 65537; c.cost_pitch = 70000; EXPECT(refused(c, "m must be in 1..65536"));
    c = good_cost(); c.metric = 3; EXPECT(refused(c, "metric must be in 0..2"));
    c = good_cost(); c.reserved0 = -1; EXPECT(refused(c, "reserved0 must be 0"));
    c = good_cost(); c.x_frame_pitch = 19; EXPECT(refused(c, "x_frame_pitch smaller than n_features"));
    c = good_cost(); c.y_frame_pitch = 0; EXPECT(refused(c, "y_frame_pitch smaller than n_features"));
    c = good_cost(); c.x_pair_pitch = 99 * 20 + 19; EXPECT(refused(c, "x_pair_pitch does not cover a sequence"));
    c = good_cost(); c.x_pair_pitch = 99 * 20 + 20; EXPECT(jsgx_cdist_plan(&c, nullptr, 0, nullptr, nullptr) == JSGX_OK);
    c = good_cost(); c.y_pair_pitch = 299 * 24 + 19; EXPECT(refused(c, "y_pair_pitch does not cover a sequence"));
    c = good_cost(); c.cost_pitch = 299; EXPECT(refused(c, "cost_pitch smaller than m"));
    c = good_cost(); c.cost_pair_pitch = 99 * 300 + 299; EXPECT(refused(c, "cost_pair_pitch does not cover a plane"));
    c = good_cost(); c.pairs = 1; c.cost_pair_pitch = 0; EXPECT(jsgx_cdist_plan(&c, nullptr, 0, nullptr, nullptr) == JSGX_OK);
    c = good_cost(); c.cost = const_cast<float*>(c.x) + 99 * 20 + 19; EXPECT(refused(c, "cost overlaps x"));
    c = good_cost(); c.cost = const_cast<float*>(c.x) + 99 * 20 + 20; EXPECT(jsgx_cdist_plan(&c, nullptr, 0, nullptr, nullptr) == JSGX_OK);
    c = good_cost(); c.cost = const_cast<float*>(c.y) - (2 * 30000 + 99 * 300 + 300) + 1; EXPECT(refused(c, "cost overlaps y"));

    // the plan and the scratch of the time warping over shapes
    jsgx_dtw_args d = good_dtw();
    int32_t rows = 0, cols = 0, launches = 0;
    EXPECT(jsgx_dtw_plan(&d, name, (int)sizeof name, &rows, &cols, &launches, &threads, &lds) == JSGX_OK);
    EXPECT(std::strcmp(name, "dtw_tiles") == 0 && rows == JSGX_DTW_TILE_ROWS && cols == JSGX_DTW_TILE_COLS && threads == JSGX_DTW_THREADS);
    EXPECT(lds == JSGX_DTW_LDS_BYTES && lds <= 163840 && launches == 2 + (300 + JSGX_DTW_TILE_COLS - 1) / JSGX_DTW_TILE_COLS - 1 + 1);
    EXPECT(jsgx_dtw_scratch_bytes(&d) == 8 * 3 * 399);
    for (int n : {1, 63, 64, 65, 4096, JSGX_DTW_MAX_LEN})
        for (int m : {1, JSGX_DTW_TILE_COLS - 1, JSGX_DTW_TILE_COLS, JSGX_DTW_TILE_COLS + 1, 4096, JSGX_DTW_MAX_LEN}) {
            d = good_dtw();
            d.n = n, d.m = m, d.pairs = 1, d.cost_pitch = d.acc_pitch = m, d.max_path = n + m - 1;
            EXPECT(jsgx_dtw_plan(&d, nullptr, 0, nullptr, nullptr, &launches, nullptr, nullptr) == JSGX_OK);
            EXPECT(launches == (n + JSGX_DTW_TILE_ROWS - 1) / JSGX_DTW_TILE_ROWS + (m + JSGX_DTW_TILE_COLS - 1) / JSGX_DTW_TILE_COLS);
            EXPECT(jsgx_dtw_scratch_bytes(&d) == 8ll * (n + m - 1));
            d.path_i = d.path_j = nullptr, d.path_len = nullptr, d.total = nullptr, d.max_path = 0;
            EXPECT(jsgx_dtw_plan(&d, nullptr, 0, nullptr, nullptr, &launches, nullptr, nullptr) == JSGX_OK);
            EXPECT(launches == (n + JSGX_DTW_TILE_ROWS - 1) / JSGX_DTW_TILE_ROWS + (m + JSGX_DTW_TILE_COLS - 1) / JSGX_DTW_TILE_COLS - 1 && jsgx_dtw_scratch_bytes(&d) == 0);
        }
    d = good_dtw();
    EXPECT(jsgx_dtw_plan(&d, name, 15, nullptr, nullptr, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_dtw_plan: bad argument") == 0);
    EXPECT(jsgx_dtw_scratch_bytes(nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_dtw_scratch_bytes: null argument") == 0);

    d = good_dtw(); d.cost = nullptr; EXPECT(refused(d, "null cost"));
    d = good_dtw(); d.acc = nullptr; EXPECT(refused(d, "null acc"));
    d = good_dtw(); d.path_j = nullptr; EXPECT(refused(d, "path_i and path_j go together"));
    d = good_dtw(); d.path_len = nullptr; EXPECT(refused(d, "null path_len with paths"));
    d = good_dtw(); d.total = device<float>(8, 1); EXPECT(refused(d, "pointers must be 4-byte aligned"));
    d = good_dtw(); d.pairs = 0; EXPECT(refused(d, "pairs must be in 1..65535"));
    d = good_dtw(); d.n = 65537; EXPECT(refused(d, "n must be in 1..65536"));
    d = good_dtw(); d.m = 0; EXPECT(refused(d, "m must be in 1..65536"));
    d = good_dtw(); d.subseq = 2; EXPECT(refused(d, "subseq must be 0 or 1"));
    d = good_dtw(); d.band = -1; EXPECT(refused(d, "band must be in 0..65536"));
    d = good_dtw(); d.weights_add[2] = INFINITY; EXPECT(refused(d, "weights must be finite"));
    d = good_dtw(); d.weights_mul[0] = NAN; EXPECT(refused(d, "weights must be finite"));
    d = good_dtw(); d.reserved0 = 7; EXPECT(refused(d, "reserved0 must be 0"));
    d = good_dtw(); d.band = 3; d.subseq = 1; EXPECT(refused(d, "band and subseq exclude each other"));
    d = good_dtw(); d.max_path = 398; d.path_pitch = 398; EXPECT(refused(d, "max_path smaller than n + m - 1"));
    d = good_dtw(); d.cost_pitch = 299; EXPECT(refused(d, "cost_pitch smaller than m"));
    d = good_dtw(); d.cost_pair_pitch = 29999; EXPECT(refused(d, "cost_pair_pitch does not cover a plane"));
    d = good_dtw(); d.acc_pitch = 1; EXPECT(refused(d, "acc_pitch smaller than m"));
    d = good_dtw(); d.acc_pair_pitch = 29999; EXPECT(refused(d, "acc_pair_pitch does not cover a plane"));
    d = good_dtw(); d.path_pitch = 398; EXPECT(refused(d, "path_pitch smaller than max_path"));
    d = good_dtw(); d.acc = const_cast<float*>(d.cost) + 89999; EXPECT(refused(d, "acc overlaps cost"));
    d = good_dtw(); d.acc = const_cast<float*>(d.cost) + 90000; EXPECT(jsgx_dtw_scratch_bytes(&d) > 0);
    d = good_dtw(); d.path_len = reinterpret_cast<int32_t*>(const_cast<float*>(d.cost)) + 5; EXPECT(refused(d, "an output overlaps cost"));
    d = good_dtw(); d.total = d.acc + 89999; EXPECT(refused(d, "an output overlaps acc"));
    d = good_dtw(); d.total = d.acc + 90000; EXPECT(jsgx_dtw_scratch_bytes(&d) > 0);
    // one pair: the pair pitches are not looked at
    d = good_dtw(); d.pairs = 1; d.cost_pair_pitch = d.acc_pair_pitch = d.path_pitch = 0; EXPECT(jsgx_dtw_scratch_bytes(&d) == 8 * 399);

    // the launches of a plane: every anti-diagonal of every tile grid takes tiles inside the grid, and together they take each tile once
    for (int ti = 1; ti <= 6; ++ti)
        for (int tj = 1; tj <= 6; ++tj) {
            const jsgx::DtwTiles tiles = jsgx::dtw_tiles(ti * JSGX_DTW_TILE_ROWS, (tj - 1) * JSGX_DTW_TILE_COLS + 1);
            EXPECT(tiles.i == ti && tiles.j == tj);
            int visits[6][6] = {};
            for (int dg = 0; dg < tiles.diagonals(); ++dg) {
                const jsgx::TileRange on = jsgx::tiles_on_diagonal(tiles, dg);
                EXPECT(0 <= on.first && on.first <= on.last && on.last < ti);
                for (int i = on.first; i <= on.last; ++i) {
                    EXPECT(0 <= dg - i && dg - i < tj);
                    if (0 <= dg - i && dg - i < tj) ++visits[i][dg - i];
                }
            }
            for (int i = 0; i < 6; ++i)
                for (int j = 0; j < 6; ++j) EXPECT(visits[i][j] == (i < ti && j < tj ? 1 : 0));
            // ... and the loop above ran once per launch: no anti-diagonal was empty, so there are ti + tj - 1 of them
            EXPECT(tiles.diagonals() == ti + tj - 1 && jsgx::tile_launches(ti * JSGX_DTW_TILE_ROWS, (tj - 1) * JSGX_DTW_TILE_COLS + 1, false) == ti + tj - 1);
            EXPECT(jsgx::tile_launches(ti * JSGX_DTW_TILE_ROWS, (tj - 1) * JSGX_DTW_TILE_COLS + 1, true) == ti + tj);
        }

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
