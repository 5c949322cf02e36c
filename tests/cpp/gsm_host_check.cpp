// gsm_host_check -- the source of the GSM kernels (viterbidecodercpp_amd/csrc/kernels_gsm.hpp) compiled for the HOST with the HIP built-ins
// stubbed (hip_stub/hip/hip_runtime.h), as a program of its own for the address and undefined-behaviour sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Itests/cpp/hip_stub -o gsm_host_check gsm_host_check.cpp
//   ./gsm_host_check [shapes = 60] [seed = 1]
// It checks, with no GPU: the literal values of include/vit_hip.h (j(0..7), the bijection, the Fire code's check values and its table of
// powers); every INVALID_ARG case of the three argument rules and the zero-work cases; and random shapes of both symbol widths whose
// inputs end their heap blocks exactly (a read behind a burst's 116 elements, a frame's 28 or 24 bytes or its 78 class II values is a
// sanitizer report) and whose outputs carry guard bytes: every thread of the grid runs through the kernels' own functions and every byte
// of every output buffer is compared with loops that walk the rule bit by bit -- the forward scatter, long division, the search over
// every shift.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../viterbidecodercpp_amd/csrc/kernels_gsm.hpp"

using namespace vit;

static uint64_t rng_state = 1;
static uint64_t rnd() {                                            // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t below(uint64_t n) { return rnd() % n; }

#define FAIL(...) do { printf("MISMATCH line %d: ", __LINE__); printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

// r mod g of 224 bits, the first the highest power: long division
static uint64_t divide(const uint8_t* bits, int n) {
    uint64_t r = 0;
    for (int t = 0; t < n; ++t) {
        r = (r << 1) | bits[t];
        if (r >> 40) r ^= GSM_FIRE_G;
    }
    return r;
}

static int literals() {
    static const uint32_t first[8] = {0, 98, 82, 66, 51, 35, 19, 3};
    int seen[4][114] = {}, per[8][2] = {};
    for (uint32_t k = 0; k < 456; ++k) {
        const uint32_t j = gsm_j(k);
        if (k < 8 && j != first[k]) FAIL("j(%u) = %u", k, j);
        if (j >= 114 || seen[k % 4][j]++) FAIL("the block map is no bijection at k = %u", k);
        if ((j & 1) != (k % 8 >= 4)) FAIL("parity of j(%u)", k);
        ++per[k % 8][j & 1];
        if (gsm_element(j) != (j < 57 ? j : j + 2)) FAIL("element(%u)", j);
    }
    for (int b = 0; b < 8; ++b)
        if (per[b][b >= 4] != 57 || per[b][b < 4] != 0) FAIL("burst offset %d does not receive 57 bits of one parity", b);
    uint64_t x = 1;
    for (int i = 0; i < 28; ++i) {
        if (GSM_FIRE_POWERS.at[i] != x) FAIL("D^(8 * %d) mod g", i);
        for (int s = 0; s < 8; ++s) x = gsm_fire_times_d(x);
    }
    if (gsm_fire_over_d(gsm_fire_times_d(0x8000000001ull)) != 0x8000000001ull) FAIL("x D / D");
    uint8_t bits[224] = {};
    for (int t = 184; t < 224; ++t) bits[t] = 1;
    if ((divide(bits, 224) ^ GSM_FIRE_MASK) != 0) FAIL("184 zeros carry 40 ones");
    bits[223] ^= 1;
    if ((divide(bits, 224) ^ GSM_FIRE_MASK) != 1) FAIL("u(223)");
    bits[223] ^= 1; bits[183] ^= 1;
    if ((divide(bits, 224) ^ GSM_FIRE_MASK) != 0x0004820009ull) FAIL("u(183)");
    return 0;
}

#define WANT(expr, bad)                                                                     \
    do {                                                                                    \
        const char* why_ = (expr);                                                          \
        if ((why_ != nullptr) != (bad)) { printf("MISMATCH line %d: %s\n", __LINE__, why_ ? why_ : "accepted"); return 1; } \
    } while (0)

static int arguments() {
    uint8_t* far = (uint8_t*)(uintptr_t)0x100000000000ull;                             // addresses only: the rules read no memory
    uint8_t* in = far + 0x10000000000ull;
    uint8_t *hi = far + 0x20000000000ull, *ho = far + 0x21000000000ull;
    uint32_t *fi = (uint32_t*)(far + 0x22000000000ull), *fo = (uint32_t*)(far + 0x23000000000ull), *no = (uint32_t*)(far + 0x24000000000ull);
    uint8_t *full = far, *c1 = far + 0x1000000, *c2 = far + 0x2000000;
    int32_t* st = (int32_t*)(far + 0x3000000);
    const unsigned B = VIT_HIP_GSM_BLOCK, D = VIT_HIP_GSM_DIAGONAL, N = VIT_HIP_GSM_NEGATE;
#define DI(...) gsm_deinterleave_invalid(__VA_ARGS__)
    WANT(DI(true, 2, 2, in, 0, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, st), false);
    WANT(DI(true, 2, 2, in, 0, 0, 3, 8, D, N, hi, fi, ho, fo, no, full, c1, c2, st), false);
    WANT(DI(true, 2, 2, in, 0, 0, 3, 8, D, 0, nullptr, nullptr, nullptr, nullptr, nullptr, full, nullptr, nullptr, nullptr), false);
    WANT(DI(false, 2, 2, in, 0, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, st), true);              // NULL handle
    WANT(DI(true, 2, 2, nullptr, 0, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, st), true);          // NULL input
    WANT(DI(true, 2, 2, in, 0, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, nullptr, nullptr, nullptr, nullptr), true);
    for (int keep = 1; keep < 16; ++keep)                                                                                     // every subset but the empty one
        WANT(DI(true, 2, 2, in, 0, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, nullptr, keep & 1 ? full : nullptr, keep & 2 ? c1 : nullptr,
                keep & 4 ? c2 : nullptr, keep & 8 ? st : nullptr), false);
    WANT(DI(true, 3, 2, in, 0, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, st), true);               // R != 2
    WANT(DI(true, 2, 2, in, 0, 0, 3, 8, 2, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, st), true);               // mode
    WANT(DI(true, 2, 2, in, 0, 0, 3, 8, B, 2, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, st), true);               // flags
    WANT(DI(true, 2, 2, in, 0, 0, 3, 8, B, 0, hi, fi, nullptr, nullptr, no, full, c1, c2, st), true);                         // history in block mode
    WANT(DI(true, 2, 2, in, 0, 0, 3, 8, B, 0, nullptr, nullptr, ho, fo, no, full, c1, c2, st), true);
    WANT(DI(true, 2, 2, in, 0, 0, 3, 8, D, 0, hi, nullptr, ho, fo, no, full, c1, c2, st), true);                              // pairs
    WANT(DI(true, 2, 2, in, 0, 0, 3, 8, D, 0, nullptr, fi, ho, fo, no, full, c1, c2, st), true);
    WANT(DI(true, 2, 2, in, 0, 0, 3, 8, D, 0, hi, fi, ho, nullptr, no, full, c1, c2, st), true);
    WANT(DI(true, 2, 2, in, 0, 0, 3, 8, D, 0, hi, fi, nullptr, fo, no, full, c1, c2, st), true);
    WANT(DI(true, 2, 2, in, 0, 0, 3, 8, D, 0, hi, fi, nullptr, nullptr, no, full, c1, c2, st), false);
    WANT(DI(true, 2, 2, in, 0, 0, 3, 8, D, 0, nullptr, nullptr, ho, fo, no, full, c1, c2, st), false);
    for (size_t bursts : {1, 2, 3, 5, 6, 7, 9}) WANT(DI(true, 2, 2, in, 0, 0, 3, bursts, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, st), true);
    WANT(DI(true, 2, 2, in + 1, 0, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, st), true);           // alignment to soft16
    WANT(DI(true, 2, 1, in + 1, 0, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full + 1, c1 + 1, c2 + 1, st), false);
    WANT(DI(true, 2, 2, in, 0, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full + 1, c1, c2, st), true);
    WANT(DI(true, 2, 2, in, 0, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1 + 1, c2, st), true);
    WANT(DI(true, 2, 2, in, 0, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2 + 1, st), true);
    WANT(DI(true, 2, 2, in, 0, 0, 3, 8, D, 0, hi + 1, fi, ho, fo, no, full, c1, c2, st), true);
    WANT(DI(true, 2, 2, in, 0, 0, 3, 8, D, 0, hi, fi, ho + 1, fo, no, full, c1, c2, st), true);
    WANT(DI(true, 2, 2, in, 0, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, (int32_t*)((uint8_t*)st + 2)), true);
    WANT(DI(true, 2, 2, in, 0, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, (uint32_t*)((uint8_t*)no + 2), full, c1, c2, st), true);
    WANT(DI(true, 2, 1, in, 0, 0, 3, 8, D, 0, hi, (uint32_t*)((uint8_t*)fi + 1), ho, fo, no, full, c1, c2, st), true);
    WANT(DI(true, 2, 1, in, 0, 0, 3, 8, D, 0, hi, fi, ho, (uint32_t*)((uint8_t*)fo + 3), no, full, c1, c2, st), true);
    WANT(DI(true, 2, 2, in, 0, 115, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, st), true);             // strides
    WANT(DI(true, 2, 2, in, 0, 117, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, st), false);
    WANT(DI(true, 2, 2, in, 7 * 116 + 115, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, st), true);
    WANT(DI(true, 2, 2, in, 8 * 116, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, st), false);
    WANT(DI(true, 2, 2, in, 7 * 120 + 115, 120, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, st), true);
    WANT(DI(true, 2, 2, in, 7 * 120 + 116, 120, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, st), false);
    WANT(DI(true, 2, 2, in, 0x7FFFFFFFull, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, st), true);
    WANT(DI(true, 2, 2, in, 0, 0x7FFFFFFFull, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, st), true);
    WANT(DI(true, 2, 2, in, 0, 0, 0x7FFFFFFFull, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, st), true);   // counts
    WANT(DI(true, 2, 2, in, 0, 0, 1, 0x80000000ull, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, st), true);
    WANT(DI(true, 2, 2, in, 0, 0, 0x40000000ull, 8, B, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, st), true);   // rows * m
    {   // overlaps: an output on the input, on the history, on another output; right behind is fine
        const size_t in_b = 3 * 8 * 116 * 2;
        WANT(DI(true, 2, 2, in, 0, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, in + in_b - 2, c1, c2, st), true);
        WANT(DI(true, 2, 2, in, 0, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, in + in_b, c1, c2, st), false);
        WANT(DI(true, 2, 2, in, 0, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, (uint32_t*)(in + 8), full, c1, c2, st), true);
        WANT(DI(true, 2, 2, in, 0, 0, 3, 8, D, 0, hi, fi, ho, fo, no, full, c1, c2, (int32_t*)(hi + 3 * 464 * 2 - 4)), true);
        WANT(DI(true, 2, 2, in, 0, 0, 3, 8, D, 0, hi, fi, ho, fo, no, full, c1, c2, (int32_t*)(hi + 3 * 464 * 2)), false);
        WANT(DI(true, 2, 2, in, 0, 0, 3, 8, D, 0, hi, fi, hi, fo, no, full, c1, c2, st), true);                               // the history in place
        WANT(DI(true, 2, 2, in, 0, 0, 3, 8, D, 0, hi, fi, ho, fi, no, full, c1, c2, st), true);
        WANT(DI(true, 2, 2, in, 0, 0, 3, 8, D, 0, hi, fi, ho, fo, fo, full, c1, c2, st), true);
        WANT(DI(true, 2, 2, in, 0, 0, 3, 8, D, 0, hi, fi, ho, fo, (uint32_t*)((uint8_t*)fi + 8), full, c1, c2, st), true);
        WANT(DI(true, 2, 2, in, 0, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, full + 6 * 456 * 2 - 2, c2, st), true);
        WANT(DI(true, 2, 2, in, 0, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, full + 6 * 456 * 2, c2, st), false);
        WANT(DI(true, 2, 2, in, 0, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c1 + 6 * 378 * 2 - 2, st), true);
        WANT(DI(true, 2, 2, in, 0, 0, 3, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, (int32_t*)(c2 + 6 * 78 * 2 - 4)), true);
    }
    WANT(DI(true, 2, 2, in, 0, 0, 0, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, st), false);              // no work
    WANT(DI(true, 2, 2, in, 0, 0, 3, 0, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, st), false);
    WANT(DI(true, 3, 2, in, 0, 0, 0, 8, B, 0, nullptr, nullptr, nullptr, nullptr, no, full, c1, c2, st), true);               // ... still refuses what needs no shape
#undef DI

    vit_hip_gsm_fire* fs = (vit_hip_gsm_fire*)hi;
    WANT(gsm_fire_invalid(true, in, 0, 9, 12, 0, fs, full, 0), false);
    WANT(gsm_fire_invalid(true, in, 0, 9, 0, VIT_HIP_GSM_LSB_FIRST, fs, full, 0), false);
    WANT(gsm_fire_invalid(false, in, 0, 9, 12, 0, fs, full, 0), true);
    WANT(gsm_fire_invalid(true, nullptr, 0, 9, 12, 0, fs, full, 0), true);
    WANT(gsm_fire_invalid(true, in, 0, 9, 12, 0, nullptr, full, 0), true);
    WANT(gsm_fire_invalid(true, in, 0, 9, 12, 0, fs, nullptr, 0), true);
    WANT(gsm_fire_invalid(true, in, 0, 9, 13, 0, fs, full, 0), true);                                  // max_burst
    WANT(gsm_fire_invalid(true, in, 0, 9, 12, 2, fs, full, 0), true);                                  // flags
    WANT(gsm_fire_invalid(true, in, 0, 9, 12, 0, (vit_hip_gsm_fire*)(hi + 2), full, 0), true);         // alignment
    WANT(gsm_fire_invalid(true, in, 27, 9, 12, 0, fs, full, 0), true);                                 // strides
    WANT(gsm_fire_invalid(true, in, 29, 9, 12, 0, fs, full, 22), true);
    WANT(gsm_fire_invalid(true, in, 29, 9, 12, 0, fs, full, 23), false);
    WANT(gsm_fire_invalid(true, in, 0x7FFFFFFFull, 9, 12, 0, fs, full, 0), true);
    WANT(gsm_fire_invalid(true, in, 0, 9, 12, 0, fs, full, 0x7FFFFFFFull), true);
    WANT(gsm_fire_invalid(true, in, 0, 0x7FFFFFFFull, 12, 0, fs, full, 0), true);
    WANT(gsm_fire_invalid(true, in, 0, 9, 12, 0, (vit_hip_gsm_fire*)(in + 9 * 28 - 4), full, 0), true);      // the status on the input, on the data
    WANT(gsm_fire_invalid(true, in, 0, 9, 12, 0, (vit_hip_gsm_fire*)(in + 9 * 28), full, 0), false);
    WANT(gsm_fire_invalid(true, in, 0, 9, 12, 0, (vit_hip_gsm_fire*)(full + 8 * 23 + 20), full, 0), true);
    WANT(gsm_fire_invalid(true, in, 0, 9, 12, 0, fs, in, 28), false);                                  // in place: the same address and stride
    WANT(gsm_fire_invalid(true, in, 32, 9, 12, 0, fs, in, 32), false);
    WANT(gsm_fire_invalid(true, in, 0, 9, 12, 0, fs, in, 0), true);                                    // ... not at another stride
    WANT(gsm_fire_invalid(true, in, 0, 9, 12, 0, fs, in + 1, 28), true);                               // ... or address
    WANT(gsm_fire_invalid(true, in, 0, 9, 12, 0, fs, in + 9 * 28, 0), false);
    WANT(gsm_fire_invalid(true, in, 0, 0, 12, 0, fs, in + 1, 0), false);                               // no work
    WANT(gsm_fire_invalid(true, in, 0, 0, 13, 0, fs, full, 0), true);

    vit_hip_gsm_tchfs* ts = (vit_hip_gsm_tchfs*)ho;
    WANT(gsm_tchfs_invalid(true, 2, in, 0, c2, 9, full, 0, ts), false);
    WANT(gsm_tchfs_invalid(true, 2, in, 0, c2, 9, full, 0, nullptr), false);                           // the status is optional
    WANT(gsm_tchfs_invalid(false, 2, in, 0, c2, 9, full, 0, ts), true);
    WANT(gsm_tchfs_invalid(true, 2, nullptr, 0, c2, 9, full, 0, ts), true);
    WANT(gsm_tchfs_invalid(true, 2, in, 0, nullptr, 9, full, 0, ts), true);
    WANT(gsm_tchfs_invalid(true, 2, in, 0, c2, 9, nullptr, 0, ts), true);
    WANT(gsm_tchfs_invalid(true, 2, in, 0, c2 + 1, 9, full, 0, ts), true);                             // alignment
    WANT(gsm_tchfs_invalid(true, 1, in, 0, c2 + 1, 9, full, 0, ts), false);
    WANT(gsm_tchfs_invalid(true, 2, in, 0, c2, 9, full, 0, (vit_hip_gsm_tchfs*)(ho + 2)), true);
    WANT(gsm_tchfs_invalid(true, 2, in, 23, c2, 9, full, 0, ts), true);                                // strides
    WANT(gsm_tchfs_invalid(true, 2, in, 25, c2, 9, full, 32, ts), true);
    WANT(gsm_tchfs_invalid(true, 2, in, 25, c2, 9, full, 34, ts), false);
    WANT(gsm_tchfs_invalid(true, 2, in, 0x7FFFFFFFull, c2, 9, full, 0, ts), true);
    WANT(gsm_tchfs_invalid(true, 2, in, 0, c2, 9, full, 0x7FFFFFFFull, ts), true);
    WANT(gsm_tchfs_invalid(true, 2, in, 0, c2, 0x7FFFFFFFull, full, 0, ts), true);
    WANT(gsm_tchfs_invalid(true, 2, in, 0, c2, 9, in + 9 * 24 - 1, 0, ts), true);                      // overlaps
    WANT(gsm_tchfs_invalid(true, 2, in, 0, c2, 9, in + 9 * 24, 0, ts), false);
    WANT(gsm_tchfs_invalid(true, 2, in, 0, c2, 9, c2 + 9 * 78 * 2 - 1, 0, ts), true);
    WANT(gsm_tchfs_invalid(true, 2, in, 0, c2, 9, full, 0, (vit_hip_gsm_tchfs*)(in + 8)), true);
    WANT(gsm_tchfs_invalid(true, 2, in, 0, c2, 9, full, 0, (vit_hip_gsm_tchfs*)(c2 + 8)), true);
    WANT(gsm_tchfs_invalid(true, 2, in, 0, c2, 9, full, 0, (vit_hip_gsm_tchfs*)(full + 8)), true);
    WANT(gsm_tchfs_invalid(true, 2, in, 0, c2, 0, in, 0, ts), false);                                  // no work
    return 0;
}

// ---- the kernels' functions, every thread of the grid ------------------------------------------------------------------------------------

template <class T>
static std::vector<T> guarded(size_t n) { return std::vector<T>(n + 8, (T)0x5A); }
template <class T>
static bool guards_hold(const std::vector<T>& v) {
    for (size_t i = v.size() - 8; i < v.size(); ++i)
        if (v[i] != (T)0x5A) return false;
    return true;
}

template <class soft_t>
static int deinterleave_shape() {
    const uint32_t rows = 1 + below(3), m = 1 + below(6), bursts = 4 * m;
    const bool diagonal = below(2), negate = below(2), carried = diagonal && below(2);
    const size_t bs = below(2) ? 116 : 116 + below(9);
    const size_t rs = (bursts - 1) * bs + 116 + (below(2) ? 0 : below(40));
    const int lo = sizeof(soft_t) == 2 ? -32768 : -128, hi = -lo - 1;
    // the input ends its heap block with the last burst's last element
    soft_t* in = (soft_t*)malloc(((rows - 1) * rs + (bursts - 1) * bs + 116) * sizeof(soft_t));
    for (size_t i = 0; i < (rows - 1) * rs + (bursts - 1) * bs + 116; ++i) in[i] = below(8) == 0 ? (soft_t)lo : (soft_t)(below(hi - lo + 1) + lo);
    std::vector<soft_t> hist((size_t)rows * 464);
    for (auto& v : hist) v = (soft_t)(below(hi - lo + 1) + lo);
    std::vector<uint32_t> fill(rows);
    for (auto& v : fill) v = below(3) ? 4 : below(2) ? 0 : 3;
    const size_t blocks = (size_t)rows * m;
    auto full = guarded<soft_t>(blocks * 456), c1 = guarded<soft_t>(blocks * 378), c2 = guarded<soft_t>(blocks * 78), ho = guarded<soft_t>(rows * 464);
    auto st = guarded<int32_t>(blocks);
    auto fo = guarded<uint32_t>(rows), no = guarded<uint32_t>(rows);
    const unsigned keep = 1 + below(15);
    const GsmArgs a = gsm_args(sizeof(soft_t), in, rs, bs == 116 && below(2) ? 0 : bs, rows, bursts, diagonal, negate, carried ? hist.data() : nullptr,
                               carried ? fill.data() : nullptr, diagonal ? ho.data() : nullptr, diagonal ? fo.data() : nullptr, no.data(),
                               keep & 1 ? full.data() : nullptr, keep & 2 ? c1.data() : nullptr, keep & 4 ? c2.data() : nullptr, keep & 8 ? st.data() : nullptr);
    std::vector<soft_t> lds(GSM_BLOCKS * 8 * GSM_BURST);
    for (uint32_t block = 0; block < gsm_grid(blocks); ++block) {
        for (uint32_t tid = 0; tid < GSM_THREADS; ++tid) gsm_stage<soft_t>(a, lds.data(), block, tid);
        for (uint32_t tid = 0; tid < GSM_THREADS; ++tid) gsm_emit<soft_t>(a, lds.data(), block, tid);
    }
    // the rule by the forward scatter: for every row the sequence of bursts, for every block every k
    for (uint32_t r = 0; r < rows; ++r) {
        const bool with = carried && fill[r] == 4;
        std::vector<std::vector<int>> seq;
        auto sg = [&](int v) { return negate ? (-v > hi ? hi : -v) : v; };
        if (with)
            for (int b = 0; b < 4; ++b) { seq.emplace_back(); for (int e = 0; e < 116; ++e) seq.back().push_back(sg(hist[r * 464 + b * 116 + e])); }
        for (uint32_t b = 0; b < bursts; ++b) { seq.emplace_back(); for (int e = 0; e < 116; ++e) seq.back().push_back(sg(in[r * rs + b * bs + e])); }
        const uint32_t n_out = diagonal ? m - 1 + with : m;
        if (no[r] != n_out) FAIL("n_out[%u] = %u, want %u", r, no[r], n_out);
        for (uint32_t n = 0; n < m; ++n) {
            std::vector<int> coded(456, 0);
            int flags = 0;
            if (n < n_out) {
                for (int k = 0; k < 456; ++k) {
                    const int j = 2 * ((49 * k) % 57) + (k % 8) / 4;
                    coded[k] = seq[4 * n + (diagonal ? k % 8 : k % 4)][j < 57 ? j : j + 2];
                }
                for (int q = 0; q < (diagonal ? 8 : 4); ++q) flags += diagonal ? seq[4 * n + q][q < 4 ? 58 : 57] : seq[4 * n + q][57] + seq[4 * n + q][58];
            }
            const size_t item = (size_t)r * m + n;
            for (int k = 0; k < 456; ++k) {
                if ((keep & 1) && full[item * 456 + k] != (soft_t)coded[k]) FAIL("full[%zu][%d]", item, k);
                if ((keep & 2) && k < 378 && c1[item * 378 + k] != (soft_t)coded[k]) FAIL("class1[%zu][%d]", item, k);
                if ((keep & 4) && k >= 378 && c2[item * 78 + k - 378] != (soft_t)coded[k]) FAIL("class2[%zu][%d]", item, k);
            }
            if ((keep & 8) && st[item] != flags) FAIL("steal[%zu] = %d, want %d", item, st[item], flags);
        }
        if (diagonal) {
            if (fo[r] != 4) FAIL("fill_out[%u]", r);
            for (int e = 0; e < 464; ++e)
                if (ho[r * 464 + e] != in[r * rs + (bursts - 4 + e / 116) * bs + e % 116]) FAIL("hist_out[%u][%d]", r, e);
        }
    }
    for (size_t i = 0; i < blocks * 456 && !(keep & 1); ++i) if (full[i] != (soft_t)0x5A) FAIL("an absent output was written");
    for (size_t i = 0; i < rows && !diagonal; ++i) if (fo[i] != 0x5A5A5A5Au && fo[i] != 0x5Au) FAIL("fill_out in block mode");
    if (!guards_hold(full) || !guards_hold(c1) || !guards_hold(c2) || !guards_hold(st) || !guards_hold(ho) || !guards_hold(fo) || !guards_hold(no)) FAIL("a guard");
    free(in);
    return 0;
}

static int fire_shape() {
    const uint32_t frames = 1 + below(9), max_burst = below(3) ? 12 : below(13), lsb = below(2);
    const size_t is = 28 + (below(2) ? 0 : below(5)), os = 23 + (below(2) ? 0 : below(5));
    const bool in_place = below(4) == 0;
    const size_t in_n = (frames - 1) * is + 28;
    uint8_t* in = (uint8_t*)malloc(in_n);
    std::vector<uint8_t> sent((size_t)frames * 224);
    memset(in, 0xEE, in_n);
    for (uint32_t f = 0; f < frames; ++f) {
        uint8_t* u = &sent[f * 224];
        for (int t = 0; t < 184; ++t) u[t] = below(2);
        for (int t = 184; t < 224; ++t) u[t] = 0;
        const uint64_t parity = divide(u, 224) ^ GSM_FIRE_MASK;
        for (int t = 0; t < 40; ++t) u[184 + t] = (parity >> (39 - t)) & 1;
        const uint32_t kind = below(5);                                  // clean, a burst, two bursts, noise
        if (kind == 1 || kind == 2 || kind == 3) {
            const uint32_t len = 1 + below(kind == 3 ? 16 : 12), t0 = below(224 - len + 1);
            u[t0] ^= 1;
            if (len > 1) u[t0 + len - 1] ^= 1;
            for (uint32_t i = 1; i + 1 < len; ++i) u[t0 + i] ^= below(2);
            if (kind == 2) u[below(224)] ^= 1;
        } else if (kind == 4) {
            for (int t = 0; t < 224; ++t) u[t] ^= below(2);
        }
        for (int t = 0; t < 224; ++t) { if (t % 8 == 0) in[f * is + t / 8] = 0; in[f * is + t / 8] |= u[t] << (7 - t % 8); }
    }
    std::vector<uint8_t> data = guarded<uint8_t>((frames - 1) * os + 23);
    std::vector<vit_hip_gsm_fire> status(frames + 1);
    memset(status.data(), 0x5A, status.size() * sizeof(vit_hip_gsm_fire));
    const GsmFireArgs a = gsm_fire_args(in, is, frames, max_burst, lsb, status.data(), in_place ? in : data.data(), in_place ? is : os);
    for (uint32_t block = 0; block < gsm_grid(frames); ++block) {
        GsmFireLds lds;
        memset(&lds, 0xA5, sizeof(lds));
        for (uint32_t tid = 0; tid < GSM_THREADS; ++tid) gsm_fire_stage(a, lds, block, tid);
        for (uint32_t tid = 0; tid < GSM_THREADS; ++tid) gsm_fire_search(a, lds, block, tid);
        for (uint32_t tid = 0; tid < GSM_THREADS; ++tid) gsm_fire_emit(a, lds, block, tid);
    }
    for (uint32_t f = 0; f < frames; ++f) {
        uint8_t* u = &sent[f * 224];
        const uint64_t s = divide(u, 224) ^ GSM_FIRE_MASK;
        int want = s ? -1 : 0;
        uint32_t first = 0;
        // by the definition: every start, every length, every middle is too many here; every shift of every pattern that trapping can
        // see is the same set: try each first bit and each length, take the pattern the syndrome dictates and test it by division
        for (uint32_t len = 1; s && want < 0 && len <= max_burst; ++len)
            for (uint32_t t0 = 0; want < 0 && t0 + len <= 224; ++t0) {
                // the pattern with ends at t0 and t0 + len - 1 whose remainder is s, if there is one: x = s / D^(223 - t0 - len + 1)
                uint64_t x = s;
                for (uint32_t i = 0; i < 223 - (t0 + len - 1); ++i) x = gsm_fire_over_d(x);
                if (!(x & 1) || (x >> len) != 0 || !((x >> (len - 1)) & 1)) continue;
                uint8_t v[224];
                memcpy(v, u, 224);
                for (uint32_t i = 0; i < len; ++i) v[t0 + len - 1 - i] ^= (x >> i) & 1;
                if ((divide(v, 224) ^ GSM_FIRE_MASK) != 0) FAIL("a trapped pattern does not clear the syndrome");
                memcpy(u, v, 224);
                want = (int)len;
                first = t0;
            }
        const vit_hip_gsm_fire& g = status[f];
        if (g.status != want || g.first_bit != first || g.syndrome_lo != (uint32_t)s || g.syndrome_hi != (uint32_t)(s >> 32))
            FAIL("status[%u] = {%d, %u, %x, %x}, want {%d, %u, %llx}", f, g.status, g.first_bit, g.syndrome_lo, g.syndrome_hi, want, first, (unsigned long long)s);
        const uint8_t* out = in_place ? in + f * is : data.data() + f * os;
        for (int i = 0; i < 23; ++i) {
            uint32_t b = 0;
            for (int c = 0; c < 8; ++c) b |= u[8 * i + c] << (lsb ? c : 7 - c);
            if (out[i] != b) FAIL("data[%u][%d] = %02x, want %02x", f, i, out[i], b);
        }
        if (in_place && f + 1 < frames)
            for (size_t i = 28; i < is; ++i) if (in[f * is + i] != 0xEE) FAIL("a byte between the frames");
    }
    if (!guards_hold(data) || status[frames].status != 0x5A5A5A5A) FAIL("a guard");
    for (size_t i = 0; i < (frames - 1) * os + 23 && in_place; ++i) if (data[i] != 0x5A) FAIL("d_data written in an in-place call");
    for (uint32_t f = 0; f + 1 < frames && !in_place; ++f)
        for (size_t i = 23; i < os; ++i) if (data[f * os + i] != 0x5A) FAIL("a byte between the data rows");
    free(in);
    return 0;
}

template <class soft_t>
static int tchfs_shape() {
    const uint32_t frames = 1 + below(9);
    const size_t is = 24 + (below(2) ? 0 : below(5)), os = 33 + (below(2) ? 0 : below(5));
    const int high = sizeof(soft_t) == 2 ? 127 : below(2) ? 1 : 127, low = below(2) ? -high : 0;
    uint8_t* in = (uint8_t*)malloc((frames - 1) * is + 24);
    soft_t* c2 = (soft_t*)malloc((size_t)frames * 78 * sizeof(soft_t));
    for (size_t i = 0; i < (frames - 1) * is + 24; ++i) in[i] = (uint8_t)below(256);
    for (size_t i = 0; i < (size_t)frames * 78; ++i) c2[i] = (soft_t)((int)below(2 * high + 2) - high - 1);
    auto speech = guarded<uint8_t>((frames - 1) * os + 33);
    std::vector<vit_hip_gsm_tchfs> status(frames + 1);
    memset(status.data(), 0x5A, status.size() * sizeof(vit_hip_gsm_tchfs));
    const bool with = below(4) != 0;
    const GsmTchfsArgs a = gsm_tchfs_args(high, low, in, is, c2, frames, speech.data(), os, with ? status.data() : nullptr);
    for (uint32_t block = 0; block < gsm_grid(frames); ++block) {
        GsmTchfsLds lds;
        memset(&lds, 0xA5, sizeof(lds));
        for (uint32_t tid = 0; tid < GSM_THREADS; ++tid) gsm_tchfs_stage<soft_t>(a, lds, block, tid);
        for (uint32_t tid = 0; tid < GSM_THREADS; ++tid) gsm_tchfs_emit(a, lds, block, tid);
    }
    for (uint32_t f = 0; f < frames; ++f) {
        int u[192], d[264] = {}, erased = 0;
        for (int t = 0; t < 192; ++t) u[t] = (in[f * is + t / 8] >> (7 - t % 8)) & 1;
        for (int k = 0; k < 91; ++k) { d[2 * k] = u[k]; d[2 * k + 1] = u[184 - k]; }
        for (int k = 0; k < 78; ++k) { d[182 + k] = 2 * (int)c2[f * 78 + k] > high + low; erased += 2 * (int)c2[f * 78 + k] == high + low; }
        int r = 0;
        for (int i = 0; i < 53; ++i) { r = (r << 1) | (i < 50 ? d[i] : u[91 + i - 50]); if (r & 8) r ^= 0xB; }
        for (int i = 0; i < 33; ++i) {
            int b = 0;
            for (int c = 0; c < 8; ++c) b |= d[8 * i + c] << (7 - c);
            if (speech[f * os + i] != b) FAIL("speech[%u][%d]", f, i);
        }
        for (size_t i = 33; i < os && f + 1 < frames; ++i) if (speech[f * os + i] != 0x5A) FAIL("a byte between the speech rows");
        if (with && (status[f].parity_syndrome != (uint32_t)(r ^ 7) || status[f].class2_erasures != (uint32_t)erased)) FAIL("status[%u]", f);
        if (!with && status[f].parity_syndrome != 0x5A5A5A5Au) FAIL("an absent status was written");
    }
    if (!guards_hold(speech) || status[frames].parity_syndrome != 0x5A5A5A5Au) FAIL("a guard");
    free(in);
    free(c2);
    return 0;
}

int main(int argc, char** argv) {
    const int shapes = argc > 1 ? atoi(argv[1]) : 60;
    rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    if (literals() || arguments()) return 1;
    for (int s = 0; s < shapes; ++s)
        if (deinterleave_shape<int16_t>() || deinterleave_shape<int8_t>() || fire_shape() || tchfs_shape<int16_t>() || tchfs_shape<int8_t>()) {
            printf("shape %d\n", s);
            return 1;
        }
    printf("ok: %d shapes of each kernel, both symbol widths\n", shapes);
    return 0;
}
