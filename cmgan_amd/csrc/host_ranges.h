// host_ranges.h - the host arithmetic on workspace offsets and buffer ranges that the feature files' entry points share:
// the 256-byte rounding of every workspace section and the two "do these buffers intersect" tests of the argument checks.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace {

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// do the byte ranges [p, p + pb) and [q, q + qb) intersect?
inline bool bytes_overlap(const void* p, size_t pb, const void* q, size_t qb) {
    const uintptr_t p0 = (uintptr_t)p, q0 = (uintptr_t)q;
    return p0 < q0 + qb && q0 < p0 + pb;
}

// do the spans [p, p + (B-1) ld + L) of two float32 batches with row strides ldp and ldq intersect?
inline bool rows_overlap(const float* p, long long ldp, const float* q, long long ldq, int B, int L) {
    const uintptr_t p0 = (uintptr_t)p, p1 = p0 + ((size_t)(B - 1) * (size_t)ldp + (size_t)L) * sizeof(float);
    const uintptr_t q0 = (uintptr_t)q, q1 = q0 + ((size_t)(B - 1) * (size_t)ldq + (size_t)L) * sizeof(float);
    return p0 < q1 && q0 < p1;
}

}  // namespace
