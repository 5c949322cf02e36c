// depuncture_host_check -- the source of depuncture_kernel (viterbidecodercpp_amd/csrc/kernels_depuncture.hpp) compiled for the HOST with
// the HIP built-ins stubbed (hip_stub/hip/hip_runtime.h), one thread per block, as a program of its own for the address and
// undefined-behaviour sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Itests/cpp/hip_stub -o depuncture_host_check depuncture_host_check.cpp
//   ./depuncture_host_check [shapes = 400] [seed = 1]
// Every random shape, at both symbol widths in turn, puts the input, the map and the output into heap blocks of EXACTLY their size (the
// output behind 0 .. 15 leading elements that are poisoned under the address sanitizer, so that frames meet the vector store and the
// scalar one), draws the map from all of int32 -- in range, negative, just past punctured_per_frame, INT32_MIN / INT32_MAX and anything
// between -- runs every thread of the grid through the kernel and compares the whole output with the rule of include/vit_hip.h in a
// plain loop: out[f][k] = in[f][j] where 0 <= j < punctured_per_frame, else 0.  A kernel that follows an out-of-range entry reads
// outside a heap block here: that is where far indices are proven harmless without a GPU.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../viterbidecodercpp_amd/csrc/kernels_depuncture.hpp"

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

static int32_t map_entry(uint64_t P, int kind) {
    static const int32_t far[] = {INT32_MIN, INT32_MIN + 1, -2, -1, INT32_MAX, INT32_MAX - 1, 1 << 30, 1 << 16, -(1 << 30)};
    switch (kind) {
        case 0: return P ? (int32_t)below(P) : -1;                                  // in range
        case 1: return (int32_t)(P + below(33));                                    // just past the frame: the next frame's symbols
        case 2: return far[below(sizeof(far) / sizeof(far[0]))];
        case 3: return -1 - (int32_t)below(1000);
        default: return (int32_t)(uint32_t)rnd();                                   // all of int32
    }
}

static uint64_t vector_stores = 0, scalar_chunks = 0, out_of_range = 0, in_range = 0;

template <typename T>
static int run_shape(int it) {
    static const uint64_t edges[] = {0, 1, 2, 7, 8, 9, 13, 15, 16, 17, 24, 31, 33, 126, 1001};
    const uint64_t n_out = below(3) ? 1 + below(40) : below(2) ? edges[1 + below(sizeof(edges) / sizeof(edges[0]) - 1)] : 1 + below(1200);
    const uint64_t frames = n_out > 200 ? 1 + below(4) : 1 + below(40);
    const uint64_t P = below(3) == 0 ? edges[below(sizeof(edges) / sizeof(edges[0]))] : below(2) ? below(2 * n_out + 1) : n_out;
    const uint64_t lead = below(2) ? 0 : below(16);                                 // elements in front of the output: its alignment class
    const int mix = (int)below(6);                                                  // 5: every kind in one map

    T* in = (T*)malloc(frames * P * sizeof(T) + (frames * P == 0));
    for (uint64_t i = 0; i < frames * P; ++i) in[i] = (T)(rnd() | 1);               // never 0: a gathered symbol differs from an erasure
    int32_t* idx = (int32_t*)malloc(n_out * sizeof(int32_t));
    for (uint64_t k = 0; k < n_out; ++k) idx[k] = map_entry(P, mix == 5 ? (int)below(5) : below(4) ? mix : 0);
    // aligned_alloc: the block starts on a 16-byte boundary, so `lead` alone decides which store a frame's chunks take
    const uint64_t out_bytes = (lead + frames * n_out) * sizeof(T);
    T* block = (T*)aligned_alloc(16, (out_bytes + 15) / 16 * 16);
    T* out = block + lead;
    memset(block, 0xA5, out_bytes);
    POISON(block, lead * sizeof(T));
    POISON((char*)block + out_bytes, (out_bytes + 15) / 16 * 16 - out_bytes);      // the round-up of aligned_alloc is no part of the output

    const uint64_t chunks = (n_out + 7) / 8, threads = chunks * frames;
    blockDim = dim3(1);
    gridDim = dim3((unsigned)(threads + 3));                                        // a few blocks past the end: they must return at once
    for (uint64_t b = 0; b < threads + 3; ++b) {
        blockIdx = dim3((unsigned)b);
        vit::depuncture_kernel<T>(in, (size_t)P, idx, (size_t)n_out, (size_t)frames, out);
    }
    for (uint64_t f = 0; f < frames; ++f)
        for (uint64_t c = 0; c < chunks; ++c) {
            const bool vec = c * 8 + 8 <= n_out && ((uintptr_t)(out + f * n_out + c * 8) % (8 * sizeof(T))) == 0;
            ++(vec ? vector_stores : scalar_chunks);
        }

    for (uint64_t f = 0; f < frames; ++f)
        for (uint64_t k = 0; k < n_out; ++k) {
            const int32_t j = idx[k];
            const bool ok = j >= 0 && (uint64_t)j < P;
            const T want = ok ? in[f * P + (uint64_t)j] : (T)0;
            ++(ok ? in_range : out_of_range);
            if (out[f * n_out + k] != want) {
                printf("MISMATCH shape %d width %zu: n_out %llu frames %llu P %llu lead %llu: out[%llu][%llu] = %d, want %d (map entry %d)\n", it,
                       sizeof(T), (unsigned long long)n_out, (unsigned long long)frames, (unsigned long long)P, (unsigned long long)lead,
                       (unsigned long long)f, (unsigned long long)k, (int)out[f * n_out + k], (int)want, j);
                return 1;
            }
        }
    UNPOISON(block, (out_bytes + 15) / 16 * 16);
    free(block); free(idx); free(in);
    return 0;
}

int main(int argc, char** argv) {
    const int shapes = argc > 1 ? atoi(argv[1]) : 400;
    rng_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 1;
    for (int it = 0; it < shapes; ++it)
        if (run_shape<int16_t>(it) || run_shape<int8_t>(it)) return 1;
    if (!vector_stores || !scalar_chunks || !out_of_range || !in_range) {
        printf("the shapes never met: vector stores %llu, scalar chunks %llu, out-of-range entries %llu, in-range entries %llu\n",
               (unsigned long long)vector_stores, (unsigned long long)scalar_chunks, (unsigned long long)out_of_range,
               (unsigned long long)in_range);
        return 1;
    }
    printf("ok: %d shapes of both widths, %llu vector stores, %llu scalar chunks, %llu in-range and %llu out-of-range map entries\n", shapes,
           (unsigned long long)vector_stores, (unsigned long long)scalar_chunks, (unsigned long long)in_range,
           (unsigned long long)out_of_range);
    return 0;
}
