// arg_rules.hpp -- the vocabulary of the C ABI's argument rules (the *_invalid functions of the vit_*.hip units and of the "host side"
// sections of kernels_*.hpp): whether two byte ranges overlap, the bytes a strided array spans, whether a pointer is aligned.  Plain
// C++ on integers: no HIP, no handle, no memory read, so every rule that uses them runs wherever a compiler does
// (tests/cpp/arg_rules_host_check.cpp and the routes' *_host_check.cpp programs).
// overlap compares differences, not sums: a range may end at the last byte of the address space, and x + a_bytes would wrap to the
// front of memory there.  The copies this header replaced compared sums in all routes but the depuncture; for ranges whose end passes
// 2^64 they could answer "no overlap" where this one answers correctly, and no allocation can reach that: every other input gives the
// answer it gave before.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace vit {

// do [a, a + a_bytes) and [b, b + b_bytes) share a byte?  An absent (NULL) or empty range shares none
inline bool overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && a_bytes && b_bytes && (x >= y ? x - y < b_bytes : y - x < a_bytes);
}

// units from the first item's first to the last item's last: `items` things of `each` units, `stride` units apart (the resolved
// stride: a route whose 0 means "packed" says so at the call)
inline uint64_t extent(uint64_t items, uint64_t stride, uint64_t each) { return items ? (items - 1) * stride + each : 0; }

// is p no multiple of n bytes?  NULL is aligned to everything: an optional pointer needs no test of its own
inline bool misaligned(const void* p, size_t n) { return (uintptr_t)p % n != 0; }

}  // namespace vit
