// CPU-only: the span, overlap and alignment helpers that the refusals of both libraries' units share (csrc/jsg_spans.h), built alone under
// -fsanitize=address,undefined (tests/test_host_cpp.py).  No pointer here is ever dereferenced: they are addresses only.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../jadespectrogram_amd/csrc/jsg_spans.h"

using namespace jsg;

static int failed = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("line %d: %s\n", __LINE__, #cond);            \
            ++failed;                                                 \
        }                                                             \
    } while (0)

static const void* at(uintptr_t a) { return reinterpret_cast<const void*>(a); }

int main() {
    const i128 two64 = (i128)1 << 64;

    // a null pointer on either side never overlaps, whatever the lengths say
    CHECK(!overlap(addr(nullptr), 4096, addr(at(16)), 4096));
    CHECK(!overlap(addr(at(16)), 4096, addr(nullptr), 4096));
    CHECK(!overlap(addr(nullptr), two64, addr(nullptr), two64));
    CHECK(!overlap(addr(nullptr), two64, addr(at(4096)), 4));

    // end to start: half-open intervals that touch share no byte, in either order
    CHECK(!overlap(addr(at(1000)), 24, addr(at(1024)), 8));
    CHECK(!overlap(addr(at(1024)), 8, addr(at(1000)), 24));
    // one byte in common, at either end and in either order; one inside the other; the same region
    CHECK(overlap(addr(at(1000)), 25, addr(at(1024)), 8));
    CHECK(overlap(addr(at(1024)), 8, addr(at(1000)), 25));
    CHECK(overlap(addr(at(1031)), 100, addr(at(1024)), 8));
    CHECK(!overlap(addr(at(1032)), 100, addr(at(1024)), 8));
    CHECK(overlap(addr(at(1000)), 1000, addr(at(1500)), 4));
    CHECK(overlap(addr(at(1500)), 4, addr(at(1000)), 1000));
    CHECK(overlap(addr(at(1000)), 4, addr(at(1000)), 4));

    // plane: one frame is its width, whatever the frame pitch; more frames add whole pitches in front of the last width
    CHECK(plane(1, 0, 513) == 513);
    CHECK(plane(1, -7, 513) == 513);
    CHECK(plane(1, (long long)1 << 62, 513) == 513);
    CHECK(plane(3, 520, 513) == 2 * 520 + 513);
    CHECK(plane(((long long)1 << 31) - 1, (long long)1 << 62, 1) == (i128)(((long long)1 << 31) - 2) * ((i128)1 << 62) + 1);

    // span_bytes: one row ignores a garbage row pitch
    for (long long pitch : {0ll, -1ll, -((long long)1 << 62), (long long)1 << 62, (long long)INT64_MAX, (long long)INT64_MIN}) {
        CHECK(span_bytes(1, pitch, 100, 4) == 400);
        CHECK(span_bytes(1, pitch, 100, 8) == 800);
    }
    // more rows count it: the last row ends one plane behind (rows - 1) pitches
    CHECK(span_bytes(2, 128, 100, 4) == 4 * (128 + 100));
    CHECK(span_bytes(65535, 1000, 1000, 4) == 4 * (i128)65535 * 1000);
    CHECK(span_bytes(65535, (long long)1 << 62, 5, 8) == 8 * ((i128)65534 * ((i128)1 << 62) + 5));

    // a region that ends above 2^64: nothing wraps, so it overlaps what lies under its first bytes and not what lies below it
    const uintptr_t top = UINTPTR_MAX - 15;                // 16 bytes under 2^64
    const i128 huge = span_bytes(65535, (long long)1 << 62, (i128)1 << 62, 8);
    CHECK(addr(at(top)) + huge > two64);
    CHECK(overlap(addr(at(top)), huge, addr(at(top + 8)), 4));
    CHECK(overlap(addr(at(top + 8)), 4, addr(at(top)), huge));
    CHECK(!overlap(addr(at(top)), huge, addr(at(4096)), 4096));        // a wrapped end would reach these low addresses
    CHECK(!overlap(addr(at(4096)), 4096, addr(at(top)), huge));
    CHECK(!overlap(addr(at(top)), huge, addr(at(top - 64)), 64));
    CHECK(overlap(addr(at(4096)), huge, addr(at(top)), 16));
    CHECK(overlap(addr(at(top)), huge, addr(at(top)), huge));

    // aligned4: no pointer at all; every pointer aligned; one misaligned pointer among several, at each place and by each of 1, 2, 3
    CHECK(aligned4());
    CHECK(aligned4(at(4096)));
    CHECK(aligned4(at(4096), at(8), at(1 << 20)));
    for (uintptr_t off : {1, 2, 3}) {
        CHECK(!aligned4(at(4096 + off)));
        CHECK(!aligned4(at(4096 + off), at(8), at(1 << 20)));
        CHECK(!aligned4(at(4096), at(8 + off), at(1 << 20)));
        CHECK(!aligned4(at(4096), at(8), at((1 << 20) + off)));
    }
    // pointers of different types in one call; null pointers (outputs that were not asked for) count as aligned
    CHECK(aligned4(static_cast<const float*>(nullptr), static_cast<int*>(nullptr), at(64)));
    CHECK(aligned4(static_cast<const void*>(nullptr)));
    CHECK(!aligned4(static_cast<const float*>(nullptr), at(66), static_cast<int*>(nullptr)));
    // an address near 2^64: the low bits decide, nothing is narrowed on the way
    CHECK(aligned4(at(UINTPTR_MAX - 3)));
    CHECK(aligned4(at(UINTPTR_MAX - 3), at(4)));
    CHECK(!aligned4(at(UINTPTR_MAX - 2), at(4)));
    CHECK(!aligned4(at(4), at(UINTPTR_MAX)));
    CHECK(!aligned4(at(((uintptr_t)1 << 63) + 2)));

    // What libjsgx.so wrote out by hand before it took this header, restated as plain arithmetic, against span_bytes(plane(...)).
    // dtw: 4 * extent(P, pp, rows, pitch, cols), extent = (P - 1) * pp + (rows - 1) * pitch + cols, called with pp as the field
    // holds it for x and y (0 = a broadcast sequence) and with "P > 1 ? pp : 0" for the planes.  beat: 4 * (rows1 * (multi ? pitch
    // : 0) + T).  pairs 1 and 3; pair pitch 0, exact and padded; n, m, K at 1 and at their maxima; a pitch near 2^62.
    for (long long P : {1ll, 3ll})
        for (long long rows : {1ll, 65536ll})
            for (long long cols : {1ll, 1024ll, 65536ll})
                for (long long pitch : {cols, cols + 7, ((long long)1 << 62) - 3}) {
                    const i128 one = (i128)(rows - 1) * pitch + cols;        // the floats of one plane, as extent(1, 0, ...) had them
                    CHECK(plane(rows, pitch, cols) == one);
                    const long long exact = one < ((i128)1 << 62) ? (long long)one : (long long)1 << 62;
                    for (long long pp : {0ll, exact, exact + 13, ((long long)1 << 62) - 1}) {
                        const i128 old_as_held = 4 * ((i128)(P - 1) * pp + (i128)(rows - 1) * pitch + cols);
                        const i128 old_guarded = 4 * ((i128)(P - 1) * (P > 1 ? pp : 0) + (i128)(rows - 1) * pitch + cols);
                        CHECK(span_bytes(P, pp, plane(rows, pitch, cols), 4) == old_as_held);
                        CHECK(span_bytes(P, pp, plane(rows, pitch, cols), 4) == old_guarded);
                    }
                }
    for (long long rows : {1ll, 3ll, 65535ll})
        for (long long T : {1ll, 1000ll, (long long)1 << 24})
            for (long long pitch : {0ll, T, T + 5, ((long long)1 << 62) - 3}) {
                const bool multi = rows > 1;
                const i128 rows1 = rows - 1;
                CHECK(span_bytes(rows, pitch, T, 4) == 4 * (rows1 * (multi ? pitch : 0) + T));
            }

    std::printf("spans: %d failed\n", failed);
    return failed ? 1 : 0;
}
