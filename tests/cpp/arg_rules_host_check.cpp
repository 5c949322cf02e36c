// arg_rules_host_check -- the vocabulary of the C ABI's argument rules (viterbidecodercpp_amd/csrc/arg_rules.hpp) as a program of its
// own for the address and undefined-behaviour sanitizers.  Plain C++: no HIP, no stub.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o arg_rules_host_check arg_rules_host_check.cpp
//   ./arg_rules_host_check
// Pointers are made from integers and never dereferenced.  It checks overlap at touching, sharing, equal and nested ranges, at empty
// and absent ones and at the end of the address space (where it also evaluates the sum form every route but one used to carry, and
// prints that the two differ there: the reason there is one definition now); extent at 0 and 1 items and at rows that overlap; the
// alignment predicate at NULL and at odd addresses.
#include <stdint.h>
#include <stdio.h>

#include "../../viterbidecodercpp_amd/csrc/arg_rules.hpp"

using vit::extent;
using vit::misaligned;
using vit::overlap;

static const void* at(uint64_t address) { return (const void*)(uintptr_t)address; }

// the form the routes carried before: sums, which wrap where a range ends at the top of memory
static bool overlap_by_sums(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}

#define WANT(expr)                                                              \
    do {                                                                        \
        if (!(expr)) { printf("MISMATCH line %d: %s\n", __LINE__, #expr); return 1; } \
    } while (0)

static int overlaps() {
    WANT(!overlap(at(0x1000), 16, at(0x1010), 16) && !overlap(at(0x1010), 16, at(0x1000), 16));        // they touch
    WANT(overlap(at(0x1000), 17, at(0x1010), 16) && overlap(at(0x1010), 16, at(0x1000), 17));          // one byte shared
    WANT(overlap(at(0x1000), 16, at(0x1000), 16) && overlap(at(0x1000), 1, at(0x1000), 1));            // equal
    WANT(overlap(at(0x1000), 64, at(0x1010), 4) && overlap(at(0x1010), 4, at(0x1000), 64));            // one contains the other
    WANT(overlap(at(0x1000), 64, at(0x103F), 1) && !overlap(at(0x1000), 64, at(0x1040), 1));
    WANT(!overlap(at(0x1000), 0, at(0x1000), 16) && !overlap(at(0x1000), 16, at(0x1008), 0));          // an empty range
    WANT(!overlap(nullptr, 16, at(0x1000), 16) && !overlap(at(0x1000), 16, nullptr, 16));              // an absent one
    WANT(!overlap(nullptr, 16, nullptr, 16) && !overlap(nullptr, ~0ull, at(8), 16));
    // a range that ends exactly at UINTPTR_MAX + 1
    const uint64_t top = (uint64_t)UINTPTR_MAX - 0xFFF;                                                 // 4096 bytes to the end
    WANT(overlap(at(top), 0x1000, at(top + 0x800), 16) && overlap(at(top + 0x800), 16, at(top), 0x1000));   // one inside it
    WANT(overlap(at(top), 0x1000, at(UINTPTR_MAX), 1) && overlap(at(top), 0x1000, at(top - 8), 9));
    WANT(!overlap(at(top), 0x1000, at(top - 16), 16) && !overlap(at(top - 16), 16, at(top), 0x1000));       // one just below it
    const bool sums_inside = overlap_by_sums(at(top), 0x1000, at(top + 0x800), 16);
    const bool sums_below = overlap_by_sums(at(top), 0x1000, at(top - 16), 16);
    WANT(!sums_inside && !sums_below);                                  // top + 0x1000 wraps to 0: the sum form never sees this range
    printf("at a range ending at 2^%d the sum form answers %d for a range inside it, the difference form %d: they differ there\n",
           (int)(8 * sizeof(uintptr_t)), (int)sums_inside, (int)overlap(at(top), 0x1000, at(top + 0x800), 16));
    // everywhere else the two agree: every pair of short ranges in a small window, the empty ones included
    for (uint64_t x = 0x1000; x < 0x1008; ++x)
        for (uint64_t a = 0; a < 6; ++a)
            for (uint64_t y = 0x1000; y < 0x1008; ++y)
                for (uint64_t b = 0; b < 6; ++b) {
                    bool shared = false;
                    for (uint64_t i = x; i < x + a; ++i) shared = shared || (i >= y && i < y + b);
                    WANT(overlap(at(x), a, at(y), b) == shared && overlap_by_sums(at(x), a, at(y), b) == shared);
                }
    return 0;
}

static int extents() {
    WANT(extent(0, 100, 7) == 0 && extent(0, 0, 0) == 0);
    WANT(extent(1, 100, 7) == 7 && extent(1, 0, 7) == 7 && extent(1, 3, 7) == 7);                      // one item: the stride never counts
    WANT(extent(5, 7, 7) == 35 && extent(5, 10, 7) == 47);                                              // packed; a pitch
    WANT(extent(5, 3, 7) == 19 && extent(5, 0, 48) == 48);                                              // rows that overlap; one shared row
    WANT(extent(0x7FFFFFFFull, 0xFFFFFFFFull, 4) == 0x7FFFFFFEull * 0xFFFFFFFFull + 4);                 // 64-bit throughout
    return 0;
}

static int alignment() {
    WANT(!misaligned(nullptr, 1) && !misaligned(nullptr, 2) && !misaligned(nullptr, 4) && !misaligned(nullptr, 256));
    WANT(misaligned(at(0x1001), 2) && misaligned(at(0x1001), 4) && misaligned(at(0x1003), 2) && misaligned(at(0x1003), 4));
    WANT(!misaligned(at(0x1001), 1) && !misaligned(at(0x1002), 2) && misaligned(at(0x1002), 4) && !misaligned(at(0x1004), 4));
    WANT(misaligned(at(0x1080), 256) && !misaligned(at(0x1100), 256));
    return 0;
}

int main() {
    if (overlaps() || extents() || alignment()) return 1;
    printf("ok: overlap, extent, misaligned\n");
    return 0;
}
