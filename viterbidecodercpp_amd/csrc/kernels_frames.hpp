// kernels_frames.hpp -- frame extraction (vit_hip_frames_extract): the frames of bit-packed, MSB-first rows cut at the marker lock, each
// starting on a byte, complemented under an inverted lock, a pad sequence (the CCSDS randomiser) XORed off, the leading bits
// (the marker) dropped, and the unfinished frame at a row's end handed over as the next call's carry.
//   frames_extract_kernel    one thread per 64 output bits.  The items [0, frame_items) are (row, frame below the capacity, word of
//                            the frame), the items behind them (row, word of the new carry); the thread of carry word 0 also writes
//                            the row's two counts.
//                            Every thread works skip, nf and rem out of the same three inputs (the lock, the carry length, phase0):
//                            nothing passes between threads, so ONE long row spreads over the whole grid.  A thread takes its 64 bits
//                            of the logical stream (the carry's bits, then the row's) from three aligned dwords, byte-swapped (the
//                            stream is big-endian) and funnel-shifted by the bit offset; where fewer than 12 bytes of the source lie
//                            around its position -- the ragged ends of a row or a carry -- it takes them byte by byte, and no byte
//                            at or behind the source's length is touched.  A word that straddles the seam takes a part from either.
//                            Stores are two dwords where the address is a multiple of 4 and the word is whole, bytes elsewhere.
// The loop strides by the grid and there is no barrier, so the source also runs one thread per block (the host build that checks its
// reads).  Included only from vit_frames.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vit_hip.h"

namespace vit {

struct FramesArgs {
    const uint8_t* bytes;            // row r at bytes + r * row_stride
    const vit_hip_marker_lock* lock; // [rows]
    const uint8_t* carry_in;         // row r at carry_in + r * carry_stride, or null (c = 0)
    const uint32_t* carry_bits_in;   // [rows]
    const uint8_t* pad;              // [ceil(Q/8)] or null
    uint8_t* frames;                 // frame f of row r at frames + (r * max_frames + f) * frame_stride
    uint32_t* n_frames;              // [rows]
    uint32_t* marker_errors;         // [rows][max_frames] or null
    uint8_t* carry_out;
    uint32_t* carry_bits_out;        // [rows]
    uint64_t row_stride, carry_stride, frame_stride, max_frames;
    uint64_t marker, mask;           // left-aligned in 64 bits; mask = 0 with m = 0
    uint64_t cap;                    // frames a row can complete: vit_hip_frames_capacity, <= max_frames
    uint64_t frame_items, items;     // rows * cap * wpf, and that + rows * cw
    uint32_t n_bits, row_bytes;
    uint32_t P, phase0, drop, Q, m;
    uint32_t wpf, cw;                // 64-bit words of a frame's output, of a carry row
};

// the high 32 bits of (hi:lo) << sh, 0 <= sh <= 31: v_alignbit_b32 by 32 - sh
__device__ inline uint32_t frames_funnel(uint32_t hi, uint32_t lo, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t v = __builtin_amdgcn_alignbit(hi, lo, 32u - sh);                  // the instruction reads the low 5 bits of its shift
    return sh ? v : hi;
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (32u - sh));
#endif
}

// the 64 bits from bit `pos` on of the `len` bytes at p, MSB-first, left-aligned.  Bytes at or behind len read as 0 and are not touched
__device__ inline uint64_t frames_fetch64(const uint8_t* p, uint64_t len, uint64_t pos) {
    const uint64_t b = pos >> 3;
    const uint32_t bit = (uint32_t)pos & 7u;
    const uint32_t mis = (uint32_t)((uintptr_t)(p + b) & 3u);
    if (b >= mis && b - mis + 12 <= len) {                         // the three aligned dwords around byte b lie inside the source
        const uint32_t* q = (const uint32_t*)(p + (b - mis));
        const uint32_t w0 = __builtin_bswap32(q[0]), w1 = __builtin_bswap32(q[1]), w2 = __builtin_bswap32(q[2]);
        const uint32_t sh = 8u * mis + bit;
        return ((uint64_t)frames_funnel(w0, w1, sh) << 32) | frames_funnel(w1, w2, sh);
    }
    uint64_t hi = 0;
    uint32_t lo = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) hi = (hi << 8) | (b + i < len ? (uint64_t)p[b + i] : 0ull);
    if (bit && b + 8 < len) lo = p[b + 8];
    return bit ? (hi << bit) | (uint64_t)(lo >> (8u - bit)) : hi;
}

// bits [s, s + nb) of the logical stream, 1 <= nb <= 64, left-aligned, 0 behind them: the c carry bits, then the row's
__device__ inline uint64_t frames_gather64(const uint8_t* carry, uint32_t c, const uint8_t* row, uint32_t row_bytes, uint64_t s, uint32_t nb) {
    uint64_t v;
    if (s < c) {
        const uint32_t n1 = c - s < nb ? (uint32_t)(c - s) : nb;     // bits the carry gives
        v = frames_fetch64(carry, (c + 7u) / 8u, s) & (~0ull << (64u - n1));
        if (n1 < nb) v |= frames_fetch64(row, row_bytes, 0) >> n1;
    } else {
        v = frames_fetch64(row, row_bytes, s - c);
    }
    return v & (~0ull << (64u - nb));
}

// the first ceil(nb/8) bytes of v, the highest first
__device__ inline void frames_put(uint8_t* dst, uint64_t v, uint32_t nb) {
    if (nb == 64 && ((uintptr_t)dst & 3u) == 0) {
        ((uint32_t*)dst)[0] = __builtin_bswap32((uint32_t)(v >> 32));
        ((uint32_t*)dst)[1] = __builtin_bswap32((uint32_t)v);
        return;
    }
    const uint32_t n = (nb + 7u) / 8u;
    for (uint32_t i = 0; i < n; ++i) dst[i] = (uint8_t)(v >> (56u - 8u * i));
}

__global__ void __launch_bounds__(256) frames_extract_kernel(FramesArgs a) {
    const uint32_t P = a.P;
    for (uint64_t item = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; item < a.items; item += (uint64_t)gridDim.x * blockDim.x) {
        const bool in_frames = item < a.frame_items;
        uint64_t r, f = 0;
        uint32_t w;
        if (in_frames) {
            const uint64_t fr = item / a.wpf;
            w = (uint32_t)(item - fr * a.wpf);
            r = fr / a.cap;
            f = fr - r * a.cap;
        } else {
            const uint64_t i = item - a.frame_items;
            r = i / a.cw;
            w = (uint32_t)(i - r * a.cw);
        }

        // the row's cut, from the same three inputs in every thread.  Whatever the lock and the carry length hold, phi and c are below P
        uint32_t c = a.carry_in ? a.carry_bits_in[r] : 0u;
        c = c >= P ? 0u : c;
        const uint32_t phi = a.lock[r].phase % P;
        const uint64_t inv = a.lock[r].inverted ? ~0ull : 0ull;
        uint32_t x = phi + c;
        x = x >= P ? x - P : x;
        const uint32_t skip = x >= a.phase0 ? x - a.phase0 : x + (P - a.phase0);
        const uint64_t total = (uint64_t)c + a.n_bits;
        uint64_t nf = 0;
        uint32_t rem = 0;
        if (skip < total) {
            nf = (total - skip) / P;
            rem = (uint32_t)((total - skip) - nf * P);
        }
        const uint8_t* row = a.bytes + r * a.row_stride;
        const uint8_t* carry = c ? a.carry_in + r * a.carry_stride : nullptr;
        const uint32_t k0 = 64u * w;

        if (in_frames) {
            if (f >= nf) continue;
            const uint32_t nb = a.Q - k0 < 64u ? a.Q - k0 : 64u;
            const uint64_t start = skip + f * P;                                        // the frame's bit 0 in the logical stream
            uint64_t v = frames_gather64(carry, c, row, a.row_bytes, start + a.drop + k0, nb) ^ inv;
            if (a.pad) v ^= frames_fetch64(a.pad, (a.Q + 7u) / 8u, k0);
            v &= ~0ull << (64u - nb);
            frames_put(a.frames + (r * a.max_frames + f) * a.frame_stride + 8u * (uint64_t)w, v, nb);
            if (w == 0 && a.marker_errors && a.m) {                                     // frame bits [0, m) lie in front of drop
                const uint64_t head = frames_gather64(carry, c, row, a.row_bytes, start, a.m) ^ inv;
                a.marker_errors[r * a.max_frames + f] = (uint32_t)__builtin_popcountll((head ^ a.marker) & a.mask);
            }
        } else {
            if (w == 0) {
                a.n_frames[r] = (uint32_t)nf;
                a.carry_bits_out[r] = rem;
            }
            if (k0 >= rem) continue;
            const uint32_t nb = rem - k0 < 64u ? rem - k0 : 64u;
            // raw: the lock may change before these bits complete a frame
            const uint64_t v = frames_gather64(carry, c, row, a.row_bytes, skip + nf * P + k0, nb);
            frames_put(a.carry_out + r * a.carry_stride + 8u * (uint64_t)w, v, nb);
        }
    }
}

// the kernel arguments of a call the argument rule has accepted (rows >= 1)
inline FramesArgs frames_extract_args(const uint8_t* d_bytes, size_t row_stride, size_t rows, size_t n_bits, uint32_t P, size_t phase0,
                                      const vit_hip_marker_lock* d_lock, const uint8_t* d_carry_in, const uint32_t* d_carry_bits_in,
                                      size_t carry_stride, uint64_t marker, uint32_t m, uint32_t drop, const uint8_t* d_pad,
                                      uint8_t* d_frames, size_t frame_stride, size_t max_frames, uint32_t* d_n_frames,
                                      uint32_t* d_marker_errors, uint8_t* d_carry_out, uint32_t* d_carry_bits_out) {
    FramesArgs a{};
    a.bytes = d_bytes; a.lock = d_lock; a.carry_in = d_carry_in; a.carry_bits_in = d_carry_in ? d_carry_bits_in : nullptr; a.pad = d_pad;
    a.frames = d_frames; a.n_frames = d_n_frames; a.marker_errors = d_marker_errors; a.carry_out = d_carry_out;
    a.carry_bits_out = d_carry_bits_out;
    a.n_bits = (uint32_t)n_bits; a.row_bytes = (uint32_t)((n_bits + 7) / 8);
    a.P = P; a.phase0 = (uint32_t)phase0; a.drop = drop; a.Q = P - drop; a.m = m;
    a.marker = m ? marker << (64 - m) : 0; a.mask = m ? ~0ull << (64 - m) : 0;
    a.row_stride = row_stride ? row_stride : a.row_bytes;
    a.carry_stride = carry_stride ? carry_stride : (P - 1 + 7) / 8;
    a.frame_stride = frame_stride ? frame_stride : (a.Q + 7) / 8;
    a.max_frames = max_frames;
    a.cap = (n_bits + P - 1) / P;
    a.wpf = (a.Q + 63) / 64;
    a.cw = (P - 1 + 63) / 64;
    a.frame_items = (uint64_t)rows * a.cap * a.wpf;
    a.items = a.frame_items + (uint64_t)rows * a.cw;
    return a;
}

// ---- launcher (hipGetLastError() after it: 0 / -1) ---------------------------------------------------------------------------

inline int frames_launch_extract(const FramesArgs& a, hipStream_t st) {
    const uint64_t want = (a.items + 255) / 256;
    const uint64_t blocks = want < 8192 ? want : 8192;             // grid-stride past that
    hipLaunchKernelGGL(frames_extract_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace vit
