// The bytes that a pitched buffer spans, the test of two such spans for an overlap and the alignment of a call's pointers: what the
// refusals of the feature units of libjsg.so and of the units of libjsgx.so share (the header has no state; the libraries share no object
// code).  Host only and free of HIP types, so that a CPU build can take the header alone (tests/cpp/spans_test.cpp).  The spans are
// 128-bit: 65535 rows at a pitch near 2^63 behind an address near 2^64 neither wrap nor overflow.
#pragma once
#include <cstdint>

namespace jsg {

typedef __int128 i128;

inline i128 addr(const void* p) { return (i128)reinterpret_cast<uintptr_t>(p); }

// elements from the first of frame 0 to the last of frame n_frames - 1, `width` of them in a frame
inline i128 plane(long long n_frames, long long frame_pitch, long long width) { return (i128)(n_frames - 1) * frame_pitch + width; }

// bytes from the first element of row 0 to the last of row rows - 1; one row has no row pitch, whatever the field holds
inline i128 span_bytes(long long rows, long long row_pitch, i128 plane, int elem_bytes) {
    return elem_bytes * ((i128)(rows - 1) * (rows > 1 ? row_pitch : 0) + plane);
}

// half-open [a0, a0 + a_bytes) against [b0, b0 + b_bytes); a null pointer (an output that was not asked for) overlaps nothing
inline bool overlap(i128 a0, i128 a_bytes, i128 b0, i128 b_bytes) { return a0 && b0 && a0 < b0 + b_bytes && b0 < a0 + a_bytes; }

// all of these pointers are 4-byte aligned; a null pointer counts as aligned, and so does no pointer at all
template <class... P>
bool aligned4(const P*... p) {
    return ((uintptr_t(0) | ... | reinterpret_cast<uintptr_t>(p)) & 3) == 0;
}

}  // namespace jsg
