// CPU-only: the span and overlap helpers that the refusals of the feature units share (csrc/jsg_spans.h), built alone under
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

    std::printf("spans: %d failed\n", failed);
    return failed ? 1 : 0;
}
