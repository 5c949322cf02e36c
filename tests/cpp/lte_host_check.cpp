// lte_host_check -- the source of lte_dematch_kernel (viterbidecodercpp_amd/csrc/kernels_lte.hpp) compiled for the HOST with the HIP
// built-ins stubbed (hip_stub/hip/hip_runtime.h), as a program of its own for the address and undefined-behaviour sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Itests/cpp/hip_stub -o lte_host_check lte_host_check.cpp
//   ./lte_host_check [shapes = 400] [seed = 1]
// Every random shape puts the received elements, the offsets, the counts, the mask and the output into heap blocks that END with their
// last byte (the elements in front of an output that starts off a dword boundary are poisoned under the address sanitizer), runs every
// thread of the grid through the kernel's own lte_thread with the arguments lte_dematch_args makes, and compares the whole output with a
// literal restatement of the rule -- the interleaver as a matrix with NULLs, the circular buffer walked entry by entry, a scalar loop
// over k -- over a 0x5A fill.  The closed form of lte_position is also compared with that walk for every D in 1 .. 8192.
// In front of them: the argument rule (lte_invalid) at an accepted call, at every INVALID_ARG case tests/test_gpu_lte_dematch.py sends
// through the library, and at the zero-work case.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../viterbidecodercpp_amd/csrc/kernels_lte.hpp"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) __asan_poison_memory_region((p), (n))
#define UNPOISON(p, n) __asan_unpoison_memory_region((p), (n))
#else
#define POISON(p, n) ((void)0)
#define UNPOISON(p, n) ((void)0)
#endif

static uint64_t rng_state = 1;
static uint64_t rnd() {                                            // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t below(uint64_t n) { return rnd() % n; }

static const int PATTERN[32] = {1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31, 0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30};

// map[j] = q of the j-th non-NULL entry of the circular buffer, by the definition
static std::vector<uint32_t> rule_map(uint32_t D) {
    const uint32_t rows = (D + 31) / 32, nd = 32 * rows - D;
    std::vector<uint32_t> map;
    for (uint32_t i = 0; i < 3; ++i) {
        std::vector<int64_t> y(32 * rows, -1);
        for (uint32_t d = 0; d < D; ++d) y[nd + d] = d;
        for (uint32_t c = 0; c < 32; ++c)
            for (uint32_t r = 0; r < rows; ++r)
                if (y[PATTERN[c] + 32 * r] >= 0) map.push_back(3 * (uint32_t)y[PATTERN[c] + 32 * r] + i);
    }
    return map;
}

template <class soft_t>
static void run_kernel(const vit::LteArgs& a) {
    const uint32_t blocks = vit::lte_blocks(a);
    for (uint32_t b = 0; b < blocks; ++b)
        for (uint32_t t = 0; t < vit::LTE_BLOCK; ++t) vit::lte_thread<soft_t>(a, b, t);
}

template <class soft_t>
static int one_shape(int it) {
    const int full = sizeof(soft_t) == 2 ? 32767 : 127;
    static const uint32_t Ds[] = {1, 7, 31, 32, 33, 40, 43, 64, 65, 70, 341};
    const uint32_t D = below(3) ? Ds[below(sizeof(Ds) / sizeof(Ds[0]))] : 1 + (uint32_t)below(400), n3 = 3 * D;
    uint32_t E_max;
    switch (below(5)) {
        case 0: E_max = 1 + (uint32_t)below(n3); break;
        case 1: E_max = n3 + (uint32_t)below(3) - (n3 > 1); break;
        case 2: E_max = (uint32_t[]){72, 144, 288, 576, 1920}[below(5)]; break;
        case 3: E_max = 2 * n3 + 5; break;
        default: E_max = 1 + (uint32_t)below(9 * n3); break;
    }
    const uint64_t frames = 1 + below(below(4) ? 6 : 400);
    const bool with_offset = below(2), with_count = below(2), with_mask = below(3) != 0;
    const uint64_t stride = E_max + (below(2) ? 0 : below(9));
    const uint64_t n = with_offset ? below(4 * (uint64_t)E_max) + (below(4) != 0) : (frames - 1) * stride + E_max;
    const uint32_t shift = below(2) ? 0 : (uint32_t)below(16);
    int lo = -full - 1 + (int)below(full), hi = lo + (int)below((uint64_t)(full - lo) + 1);
    if (below(2)) { lo = -full - 1; hi = full; }
    uint64_t period = with_mask ? (uint64_t[]){0, E_max, stride, 1 + below(100), n + 5}[below(5)] : 0;

    soft_t* in = (soft_t*)malloc(n * sizeof(soft_t) + (n == 0));
    for (uint64_t k = 0; k < n; ++k) in[k] = below(4) ? (soft_t)rnd() : (soft_t)(below(2) ? -full - 1 : full);
    uint32_t *offset = nullptr, *count = nullptr;
    if (with_offset) {
        offset = (uint32_t*)malloc(frames * sizeof(uint32_t));
        for (uint64_t f = 0; f < frames; ++f)
            offset[f] = below(8) == 0 ? (uint32_t)rnd() : below(6) == 0 ? (uint32_t)(n + below(3)) : (uint32_t)below(n + 1);
    }
    if (with_count) {
        count = (uint32_t*)malloc(frames * sizeof(uint32_t));
        for (uint64_t f = 0; f < frames; ++f) count[f] = below(6) == 0 ? (uint32_t)rnd() : below(5) == 0 ? 0u : (uint32_t)below(E_max + 3);
    }
    const uint64_t mask_bits = period ? period : n, mask_bytes = (mask_bits + 7) / 8;
    uint8_t* mask = nullptr;
    if (with_mask) {
        mask = (uint8_t*)malloc(mask_bytes + (mask_bytes == 0));
        for (uint64_t i = 0; i < mask_bytes; ++i) mask[i] = (uint8_t)rnd();
    }
    const uint64_t total = frames * n3, lead = below(4 / sizeof(soft_t));          // elements in front of the output: 4-byte aligned malloc + lead
    soft_t* block = (soft_t*)malloc((lead + total) * sizeof(soft_t));
    soft_t* out = block + lead;
    memset(block, 0x5A, (lead + total) * sizeof(soft_t));
    POISON(block, lead * sizeof(soft_t));

    const vit::LteArgs a = vit::lte_dematch_args(in, n, stride, offset, count, frames, D, E_max, mask, period, shift, lo, hi, out, sizeof(soft_t));
    run_kernel<soft_t>(a);

    const std::vector<uint32_t> map = rule_map(D);
    std::vector<uint32_t> acc(n3);
    for (uint64_t f = 0; f < frames; ++f) {
        const uint64_t base = offset ? offset[f] : f * stride;
        uint64_t E = count ? count[f] : E_max;
        E = E < E_max ? E : E_max;
        E = base >= n ? 0 : (E < n - base ? E : n - base);
        std::fill(acc.begin(), acc.end(), 0u);
        for (uint64_t k = 0; k < E; ++k) {
            uint32_t x = (uint32_t)(int32_t)in[base + k];
            if (mask) {
                const uint64_t g = period ? (base + k) % period : base + k;
                if ((mask[g >> 3] >> (7 - (g & 7))) & 1) x = 0u - x;
            }
            acc[map[k % n3]] += x;
        }
        for (uint32_t q = 0; q < n3; ++q) {
            int32_t v = (int32_t)(acc[q] + ((1u << shift) >> 1)) >> shift;
            v = v < lo ? lo : v > hi ? hi : v;
            if (out[f * n3 + q] != (soft_t)v) {
                printf("MISMATCH shape %d: soft_bytes %zu D %u E_max %u frames %llu n %llu stride %llu offset %d count %d mask %d period %llu shift %u "
                       "clamp %d %d lead %llu: frame %llu q %u got %d want %d\n", it, sizeof(soft_t), D, E_max, (unsigned long long)frames,
                       (unsigned long long)n, (unsigned long long)stride, with_offset, with_count, with_mask, (unsigned long long)period, shift, lo, hi,
                       (unsigned long long)lead, (unsigned long long)f, q, (int)out[f * n3 + q], v);
                return 1;
            }
        }
    }
    UNPOISON(block, lead * sizeof(soft_t));
    free(block); free(in); free(offset); free(count); free(mask);
    return 0;
}

// one call of the argument rule: the accepted base call, which a case changes in a field or two
struct RuleCall {
    bool handle = true;
    int R = 3;
    size_t sb = 2;
    const void* rec;
    size_t n = 4 * 40, stride = 40;
    const uint32_t *off = nullptr, *count = nullptr;
    size_t fr = 4, D = 10, E = 40;
    unsigned shift = 0;
    int lo = -32768, hi = 32767;
    const void* out;
    const char* operator()() const { return vit::lte_invalid(handle, R, sb, rec, n, stride, off, count, fr, D, E, shift, lo, hi, out); }
};

#define WANT(set, bad)                                                                      \
    do {                                                                                    \
        RuleCall k = base;                                                                  \
        set;                                                                                \
        const char* why_ = k();                                                             \
        if ((why_ != nullptr) != (bad)) { printf("MISMATCH line %d: %s\n", __LINE__, why_ ? why_ : "accepted"); return 1; } \
    } while (0)

static int arguments() {
    const size_t frames = 4, D = 10, E = 40;
    std::vector<int16_t> in(frames * E + 3), outs(frames * 3 * D + 8);                  // heap blocks the rule never reads
    std::vector<uint32_t> cnt(frames);
    const uint8_t *a = (const uint8_t*)in.data(), *o = (const uint8_t*)outs.data();
    RuleCall base;
    base.rec = a; base.out = o;
    WANT((void)0, false);
    WANT(k.handle = false, true);
    WANT(k.rec = nullptr, true);
    WANT(k.out = nullptr, true);
    WANT(k.R = 2, true);
    WANT(k.D = 0, true);
    WANT(k.D = 8193, true);
    WANT(k.E = 0, true);
    WANT(k.E = 1u << 24, true);
    WANT(k.n = (size_t)1 << 32, true);
    WANT(k.shift = 16, true);
    WANT((k.lo = 5, k.hi = 4), true);
    WANT(k.lo = -32769, true);
    WANT(k.hi = 32768, true);
    WANT((k.sb = 1, k.hi = 128), true);
    WANT((k.sb = 1, k.lo = -129, k.hi = 0), true);
    WANT(k.stride = E - 1, true);
    WANT(k.n = frames * E - 1, true);
    WANT(k.stride = E + 1, true);
    WANT(k.out = a, true);                                                               // the output on the input
    WANT(k.out = a + 2 * frames * E - 2, true);
    WANT(k.out = (const void*)((uintptr_t)a - 2 * frames * 3 * D + 2), true);
    WANT(k.out = (const void*)((uintptr_t)a - 2 * frames * 3 * D), false);               // right in front of it
    WANT(k.rec = a + 1, true);                                                           // not aligned to soft16
    WANT(k.out = o + 1, true);
    WANT((k.sb = 1, k.lo = -128, k.hi = 127, k.rec = a + 1, k.out = o + 1), false);      // soft8: any address
    WANT((k.off = cnt.data(), k.out = cnt.data()), true);
    WANT((k.count = cnt.data(), k.out = cnt.data() + frames - 1), true);
    WANT((k.fr = ((size_t)1 << 32) / 30 + 1, k.off = cnt.data()), true);
    WANT((k.lo = 7, k.hi = 7), false);                                                   // the edges that pass
    WANT((k.n = frames * E + 3, k.stride = E + 1), false);
    WANT((k.E = (1u << 24) - 1, k.off = cnt.data()), false);
    WANT(k.fr = 0, false);                                                               // no work
    WANT((k.fr = 0, k.stride = 0), false);
    WANT((k.fr = 0, k.shift = 16), true);                                                // ... still refuses what needs no shape
    return 0;
}

int main(int argc, char** argv) {
    const int shapes = argc > 1 ? atoi(argv[1]) : 400;
    rng_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 1;
    if (arguments()) return 1;
    // the closed form against the walk, every D
    for (uint32_t D = 1; D <= vit::LTE_MAX_D; ++D) {
        int16_t dummy = 0;
        const vit::LteArgs a = vit::lte_dematch_args(&dummy, 1, 1, nullptr, nullptr, 1, D, 1, nullptr, 0, 0, 0, 0, &dummy, 2);
        const std::vector<uint32_t> map = rule_map(D);
        if (map.size() != 3 * D) { printf("MISMATCH D %u: the walk met %zu entries\n", D, map.size()); return 1; }
        for (uint32_t j = 0; j < 3 * D; ++j)
            if (vit::lte_position(a, map[j]) != j) { printf("MISMATCH D %u: position of q %u is %u, want %u\n", D, map[j], vit::lte_position(a, map[j]), j); return 1; }
    }
    for (int it = 0; it < shapes; ++it)
        if (it % 2 ? one_shape<int8_t>(it) : one_shape<int16_t>(it)) return 1;
    printf("ok: %d shapes, the closed form at every D in 1 .. %u\n", shapes, vit::LTE_MAX_D);
    return 0;
}
