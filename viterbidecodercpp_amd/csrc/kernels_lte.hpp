// kernels_lte.hpp -- LTE rate de-matching for the tail-biting code (vit_hip_lte_rate_dematch_batch): the inverse of 3GPP TS 36.212
// 5.1.4.2 -- three sub-block interleavers, a circular buffer read E bits long -- with the descrambling in front, writing the [F][D][3]
// symbols vit_hip_decode_tail_biting_batch reads.
//   lte_dematch_kernel<soft_t>   A gather, not a scatter: every OUTPUT q = 3 d + i knows in closed form where it stands among the non-NULL
//                       entries of the circular buffer, so it sums its own repetitions and nothing is zeroed, added atomically or kept
//                       between launches.  With Rsb = ceil(D / 32) rows and N_D = 32 Rsb - D NULLs in front of stream i, bit d is entry
//                       p = N_D + d of the matrix: row r = p / 32, original column p % 32, which the permutation P puts at column
//                       cc = Pinv[p % 32].  P[c] is the 5-bit reversal of c with its lowest bit flipped (1, 17, 9, 25, ... 30), so
//                       Pinv[x] = bitrev5(x ^ 1): no table.  Read by columns that is entry cc Rsb + r of v(i); the NULLs are the row-0
//                       entries of the columns whose original column lies below N_D -- a 32-bit column mask the host works out --, and
//                       those in front of (cc, r) are the mask's bits 0 .. cc (bit cc itself only counts in a row r > 0, and a data entry
//                       in row 0 never stands in such a column): one popcount.  j = i D + cc Rsb + r - nulls, and the received elements
//                       of output q are k = j, j + 3D, j + 6D, ... below E_f: one element of every wrap, all of a wrap inside one
//                       3D-element window of the frame.
//                       The position costs some twenty integer instructions an output and no LDS: no table is built, so no frame
//                       length is assumed to fit anywhere, and a block needs no barrier.
//                       Stores: the output [F][D][3] is one dense array of F 3D elements.  A thread owns the 4 / sizeof(soft_t)
//                       consecutive elements of one ALIGNED dword of it (they may belong to two frames) and stores them as one
//                       dword: a wave writes 256 contiguous bytes.  The at most 4 / sizeof(soft_t) - 1 elements in front of the first
//                       aligned dword and behind the last are stored one by one by threads of block 0.
//                       Loads: one element each (d_offset may be odd: an element load is always aligned), four wraps in flight.
//                       The sum, the negation and the rounding add run modulo 2^32 (unsigned arithmetic, read back as int32).
// Everything is plain C++ in device functions that take (block, thread): the source also runs on the host (tests/cpp/lte_host_check.cpp).
// Included only from vit_lte.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vit_hip.h"
#include "arg_rules.hpp"

namespace vit {

constexpr uint32_t LTE_BLOCK = 256;            // threads of a block: one aligned output dword each
constexpr uint32_t LTE_MAX_D = 8192;

struct LteArgs {
    const void* in;                  // soft_t [n_received]
    void* out;                       // soft_t [frames][D][3]
    const uint32_t* offset;          // [frames] or null: frame f starts at f * stride
    const uint32_t* count;           // [frames] or null: E_max
    const uint8_t* scramble;         // mask bits, MSB-first, or null
    uint64_t stride;                 // elements; (frames - 1) * stride + E_max <= n_received where it is used
    uint32_t n_received, E_max, period;        // period 0: the mask bit of element g is g
    uint32_t D, n3, Rsb, N_D, nullmask;        // n3 = 3 D; nullmask bit cc: column cc holds a NULL in row 0
    uint32_t shift;
    int32_t lo, hi;
    uint32_t total;                  // frames * n3 < 2^32
    uint32_t head, tail, groups;     // elements in front of the first aligned dword, behind the last; dwords between
};

// 5-bit reversal; P[c] = bitrev5(c) ^ 1 is the column permutation of table 5.1.4-2, Pinv[x] = bitrev5(x ^ 1)
__host__ __device__ inline uint32_t lte_bitrev5(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bitreverse32(x) >> 27;
#else
    return ((x & 1u) << 4) | ((x & 2u) << 2) | (x & 4u) | ((x & 8u) >> 2) | ((x & 16u) >> 4);
#endif
}

// where output q = 3 d + i stands among the 3D non-NULL entries of the circular buffer
__host__ __device__ inline uint32_t lte_position(const LteArgs& a, uint32_t q) {
    const uint32_t d = q / 3u, i = q - 3u * d;
    const uint32_t p = a.N_D + d, cc = lte_bitrev5((p & 31u) ^ 1u), r = p >> 5;
    const uint32_t nulls = (uint32_t)__builtin_popcount(a.nullmask & ((2u << cc) - 1u));       // cc = 31: 2u << 31 is 0, the mask all ones
    return i * a.D + cc * a.Rsb + r - nulls;
}

// where frame f lies in the received elements: nothing outside [0, n_received) whatever the offset and count memory holds
struct LteFrame { uint32_t base, E; };
__device__ inline LteFrame lte_frame(const LteArgs& a, uint32_t f) {
    const uint64_t base = a.offset ? (uint64_t)a.offset[f] : (uint64_t)f * a.stride;
    uint32_t E = a.count ? a.count[f] : a.E_max;
    E = E < a.E_max ? E : a.E_max;
    if (base >= a.n_received) return LteFrame{0u, 0u};
    const uint32_t room = a.n_received - (uint32_t)base;
    return LteFrame{(uint32_t)base, E < room ? E : room};
}

// s(f, k) * received[base + k], modulo 2^32; gb = the mask bit of element base
template <class soft_t>
__device__ inline uint32_t lte_term(const LteArgs& a, const soft_t* in, uint32_t base, uint32_t gb, uint32_t k) {
    const uint32_t x = (uint32_t)(int32_t)in[(size_t)base + k];
    if (!a.scramble) return x;
    const uint64_t g64 = (uint64_t)gb + k;
    uint32_t g = (uint32_t)g64;
    if (a.period && g64 >= a.period) g = (uint32_t)(g64 % a.period);
    return ((a.scramble[g >> 3] >> (7u - (g & 7u))) & 1u) ? 0u - x : x;
}

// out[f][q]
template <class soft_t>
__device__ inline soft_t lte_output(const LteArgs& a, uint32_t f, uint32_t q) {
    const soft_t* in = (const soft_t*)a.in;
    const LteFrame fr = lte_frame(a, f);
    const uint32_t gb = a.scramble && a.period ? fr.base % a.period : fr.base;
    uint32_t k = lte_position(a, q), sum = 0;
    for (; k + 3u * a.n3 < fr.E; k += 4u * a.n3) {                 // k < 2^24 + 3 * 24576: no wrap-around
        const uint32_t x0 = lte_term(a, in, fr.base, gb, k), x1 = lte_term(a, in, fr.base, gb, k + a.n3);
        const uint32_t x2 = lte_term(a, in, fr.base, gb, k + 2u * a.n3), x3 = lte_term(a, in, fr.base, gb, k + 3u * a.n3);
        sum += x0 + x1 + x2 + x3;
    }
    for (; k < fr.E; k += a.n3) sum += lte_term(a, in, fr.base, gb, k);
    int32_t v = (int32_t)(sum + ((1u << a.shift) >> 1)) >> a.shift;
    v = v < a.lo ? a.lo : v;
    v = v > a.hi ? a.hi : v;
    return (soft_t)v;
}

// what thread `tid` of block `block` does
template <class soft_t>
__device__ inline void lte_thread(const LteArgs& a, uint32_t block, uint32_t tid) {
    constexpr uint32_t VEC = 4u / sizeof(soft_t);
    soft_t* out = (soft_t*)a.out;
    const uint32_t G = block * LTE_BLOCK + tid;                    // groups <= 2^32 / VEC: no wrap-around below
    if (G < a.groups) {
        const uint32_t g = a.head + G * VEC;
        uint32_t f = g / a.n3, q = g - f * a.n3, word = 0;
#pragma unroll
        for (uint32_t v = 0; v < VEC; ++v) {
            const soft_t s = lte_output<soft_t>(a, f, q);
            word |= ((uint32_t)s & (0xFFFFFFFFu >> (32u - 8u * sizeof(soft_t)))) << (8u * sizeof(soft_t) * v);
            if (++q == a.n3) { q = 0; ++f; }
        }
        __builtin_memcpy(__builtin_assume_aligned(out + g, 4), &word, 4);
    }
    if (block == 0 && tid < a.head + a.tail) {
        const uint32_t g = tid < a.head ? tid : a.total - a.tail + (tid - a.head);
        const uint32_t f = g / a.n3;
        out[g] = lte_output<soft_t>(a, f, g - f * a.n3);
    }
}

template <class soft_t>
__global__ void __launch_bounds__(LTE_BLOCK) lte_dematch_kernel(LteArgs a) {
    lte_thread<soft_t>(a, blockIdx.x, threadIdx.x);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------

// argument rule (include/vit_hip.h): everything the host can know without reading device memory.  R and sb are the handle's
inline const char* lte_invalid(bool handle, int R, size_t sb, const void* d_received, size_t n_received, size_t stride, const uint32_t* d_offset,
                               const uint32_t* d_count, size_t frames, size_t D, size_t E_max, unsigned shift, int lo, int hi, const void* d_out) {
    if (!handle || !d_received || !d_out) return "NULL handle, d_received or d_symbols_out";
    if (R != 3) return "the handle's code rate must be 1/3";
    if (D == 0 || D > LTE_MAX_D) return "D must be 1 .. 8192";
    if (E_max == 0 || E_max >= (1u << 24)) return "E_max must be 1 .. 2^24 - 1";
    if (n_received >= 0x100000000ull) return "n_received must lie below 2^32";
    if (shift > 15) return "shift must be 0 .. 15";
    const int top = sb == 2 ? 32767 : 127;
    if (lo > hi || lo < -top - 1 || hi > top) return "clamp_lo .. clamp_hi must be a range of the symbol type";
    if (misaligned(d_received, sb) || misaligned(d_out, sb)) return "d_received and d_symbols_out must be aligned to the symbol type";
    if (frames == 0) return nullptr;
    if (!d_offset && (stride < E_max || n_received < E_max || (frames - 1) > (n_received - E_max) / stride))
        return "received_frame_stride below E_max, or (frames - 1) * stride + E_max above n_received";
    if (frames > 0xFFFFFFFFull / (3 * D)) return "frames * 3 D must lie below 2^32";
    const size_t out_b = frames * 3 * D * sb;
    if (overlap(d_out, out_b, d_received, n_received * sb)) return "d_symbols_out overlaps d_received";
    if (overlap(d_out, out_b, d_offset, frames * sizeof(uint32_t)) || overlap(d_out, out_b, d_count, frames * sizeof(uint32_t)))
        return "d_symbols_out overlaps d_offset or d_count";
    return nullptr;
}

// the kernel arguments of a call the argument rule has accepted: frames >= 1, frames * 3 D < 2^32, pointers aligned to soft_t
inline LteArgs lte_dematch_args(const void* d_received, size_t n_received, size_t stride, const uint32_t* d_offset, const uint32_t* d_count,
                                size_t frames, size_t D, size_t E_max, const uint8_t* d_scramble, size_t period, unsigned shift, int lo,
                                int hi, void* d_out, size_t soft_bytes) {
    LteArgs a{};
    a.in = d_received; a.out = d_out; a.offset = d_offset; a.count = d_count; a.scramble = d_scramble;
    a.stride = d_offset || frames < 2 ? 0 : stride;
    a.n_received = (uint32_t)n_received; a.E_max = (uint32_t)E_max;
    a.period = d_scramble && period < n_received ? (uint32_t)period : 0u;           // a period no element index reaches changes nothing
    a.D = (uint32_t)D; a.n3 = 3u * a.D; a.Rsb = (a.D + 31u) / 32u; a.N_D = 32u * a.Rsb - a.D;
    for (uint32_t cc = 0; cc < 32; ++cc)
        if ((lte_bitrev5(cc) ^ 1u) < a.N_D) a.nullmask |= 1u << cc;
    a.shift = shift; a.lo = lo; a.hi = hi;
    a.total = (uint32_t)(frames * a.n3);
    const uint32_t vec = 4u / (uint32_t)soft_bytes;
    const uint32_t mis = (uint32_t)(((uintptr_t)d_out / soft_bytes) % vec);          // elements the output starts behind a dword boundary
    a.head = (vec - mis) % vec;
    a.head = a.head < a.total ? a.head : a.total;
    a.groups = (a.total - a.head) / vec;
    a.tail = a.total - a.head - a.groups * vec;
    return a;
}

inline uint32_t lte_blocks(const LteArgs& a) { return a.groups ? (a.groups + LTE_BLOCK - 1) / LTE_BLOCK : 1u; }

// ---- launcher (hipGetLastError() after it: 0 / -1) ---------------------------------------------------------------------------

inline int lte_launch_dematch(const LteArgs& a, size_t soft_bytes, hipStream_t st) {
    if (soft_bytes == 2) hipLaunchKernelGGL(lte_dematch_kernel<int16_t>, dim3(lte_blocks(a)), dim3(LTE_BLOCK), 0, st, a);
    else hipLaunchKernelGGL(lte_dematch_kernel<int8_t>, dim3(lte_blocks(a)), dim3(LTE_BLOCK), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace vit
