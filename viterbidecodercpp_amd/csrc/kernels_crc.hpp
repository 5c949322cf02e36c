// kernels_crc.hpp -- the frame check (vit_hip_crc_batch): the CRC of a bit range of every frame in the layout vit_hip_frames_extract
// writes, any (width <= 32, poly, init, xorout), not reflected, and its XOR with the transmitted field behind the data.
//   crc_batch_kernel    All widths run as ONE 32-bit code: the register is kept left-aligned, which is the CRC with the generator
//                       P' = P x^(32 - width); its low 32 - width bits stay zero and the result is the register shifted down.
//                       A frame is owned by a group of G lanes (a power of two, 1 .. 64, from the message length: CrcGeometry), a wave
//                       carries 64 / G frames.  The message is right-aligned in G chunks of C bytes, C a multiple of 4: lane j
//                       reduces the message bits [n_bits - (G-j) 8C, n_bits - (G-j-1) 8C) from a zero register; bits in front of
//                       bit 0 are zero and leading zeros leave a zero register as it is, so the words wholly in front are skipped and
//                       the one that straddles bit 0 is masked.  A word is 32 message bits: two aligned dwords, byte-swapped (the
//                       frame is big-endian) and funnel-shifted by the bit offset (v_alignbit_b32), the second kept as the next
//                       word's first: one load a word.  A dword that does not lie wholly inside the bytes the data occupy is put
//                       together from those of its bytes that do; no other byte is touched.
//                       Chunk reduction: slice-by-4 over tables in LDS, tab[k][b] = b(x) x^(8k + 32) mod P': the register XORed with
//                       the word is replaced by the XOR of four INDEPENDENT lookups, so the four LDS latencies of a word overlap
//                       (a single byte table would chain them).  The 4 KiB are built in the prologue by the block itself, entry b
//                       by thread b: eight shift / conditional-xor steps for tab[0], then tab[k+1][b] = tab[k][b] x^8 through tab[0].
//                       LDS banks: the indices are data, a wave's 64 lookups spread over the 64 banks at random (no padding helps).
//                       Combine: crc_0(a || b) = crc_0(a) x^|b| mod P' ^ crc_0(b).  log2 G steps of __shfl_xor; in step s the lane
//                       whose bit s of j is clear holds the earlier part and multiplies it by m[s] = x^(8C 2^s) mod P', a host
//                       constant: 32 steps of "where bit i of the register is set, XOR m x^i in" -- m x^i is uniform, so the
//                       compiler keeps its shift / conditional xor on the scalar unit.  The group's lane 0 ends with the whole.
//                       init enters as the host constant init x^n mod P' (linearity), xorout at the end.
//                       The group's lane 0 reads the field -- the width bits behind the data, by the same guarded loads bounded by
//                       the bytes the field occupies -- and writes the frame's entries.  Lanes of frames at or behind the row's
//                       count, or behind the last frame, load and store nothing; they still take part in the exchanges.
// Everything but the exchange itself is plain C++ in device functions, and the table build strides by blockDim.x between barriers: the
// source also runs one thread per block (the host build that checks its reads).  Included only from vit_crc.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vit_hip.h"
#include "arg_rules.hpp"

namespace vit {

constexpr uint32_t CRC_BLOCK = 256;            // threads of a block: 256 / G frames
constexpr uint32_t CRC_G_MAX = 64;             // lanes of a frame at most: a group never leaves its wave
constexpr uint32_t CRC_CHUNK_BYTES = 16;       // G doubles while a lane's chunk would be longer than this

struct CrcArgs {
    const uint8_t* in;               // frame (r, f) at in + (r * max_frames + f) * stride
    const uint32_t* n_frames;        // [rows] or null
    uint32_t* crc;                   // [rows][max_frames] or null
    uint32_t* syndrome;              // [rows][max_frames] or null
    uint64_t stride, max_frames, frames;       // frames = rows * max_frames
    uint64_t first_bit, n_bits;      // first_bit + n_bits + 32 < 2^32
    uint32_t poly;                   // P' without its x^32 term: poly << shift
    uint32_t fin;                    // (init << shift) x^n_bits mod P'
    uint32_t xorout, shift, width;   // shift = 32 - width
    uint32_t logG, C;                // lanes of a frame = 1 << logG; bytes of a chunk, a multiple of 4
    uint32_t m[6];                   // m[s] = x^(8 C 2^s) mod P', s < logG
};

// lanes of a frame and bytes of a chunk for a message of n_bits: G C covers it
struct CrcGeometry { uint32_t logG, C; };
inline CrcGeometry crc_geometry(uint64_t n_bits) {
    const uint64_t bytes = (n_bits + 7) / 8;
    uint32_t logG = 0;
    while ((1u << logG) < CRC_G_MAX && ((bytes + (1u << logG) - 1) >> logG) > CRC_CHUNK_BYTES) ++logG;
    const uint64_t per = (bytes + (1u << logG) - 1) >> logG;
    return CrcGeometry{logG, per ? (uint32_t)((per + 3) / 4 * 4) : 4u};
}

// a x mod P', and a b mod P' (host and device)
__host__ __device__ inline uint32_t crc_timesx(uint32_t a, uint32_t poly) { return (a << 1) ^ (poly & (0u - (a >> 31))); }
__host__ __device__ inline uint32_t crc_mul(uint32_t a, uint32_t b, uint32_t poly) {
    uint32_t acc = 0;
#pragma unroll
    for (uint32_t i = 0; i < 32; ++i) {
        acc ^= b & (0u - ((a >> i) & 1u));
        b = crc_timesx(b, poly);
    }
    return acc;
}
// x^e mod P'
inline uint32_t crc_xpow(uint64_t e, uint32_t poly) {
    uint32_t r = 1, sq = crc_timesx(1u, poly);
    for (; e; e >>= 1) {
        if (e & 1) r = crc_mul(r, sq, poly);
        sq = crc_mul(sq, sq, poly);
    }
    return r;
}

// the high 32 bits of (hi:lo) << sh, 0 <= sh <= 31: v_alignbit_b32 by 32 - sh
__device__ inline uint32_t crc_funnel(uint32_t hi, uint32_t lo, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t v = __builtin_amdgcn_alignbit(hi, lo, 32u - sh);                  // the instruction reads the low 5 bits of its shift
    return sh ? v : hi;
#else
    return sh ? (uint32_t)((((uint64_t)hi << 32) | lo) >> (32u - sh)) : hi;
#endif
}

// the dword at base + off (a multiple of 4 as an address), its first byte highest.  Bytes outside [lo, hi) read as 0 and are not touched
__device__ inline uint32_t crc_load_be32(const uint8_t* base, int64_t off, int64_t lo, int64_t hi) {
    if (off >= lo && off + 4 <= hi) return __builtin_bswap32(*(const uint32_t*)(base + off));
    uint32_t v = 0;
#pragma unroll
    for (int32_t i = 0; i < 4; ++i)
        if (off + i >= lo && off + i < hi) v |= (uint32_t)base[off + i] << (24 - 8 * i);
    return v;
}

// tab[k][b] = b(x) x^(8k + 32) mod P', entry b by thread b.  The block meets at every barrier
__device__ inline void crc_build_tables(uint32_t* tab, uint32_t poly, uint32_t tid, uint32_t nthreads) {
    for (uint32_t b = tid; b < 256; b += nthreads) {
        uint32_t reg = b << 24;
#pragma unroll
        for (uint32_t i = 0; i < 8; ++i) reg = crc_timesx(reg, poly);
        tab[b] = reg;
    }
    __syncthreads();
    for (uint32_t k = 1; k < 4; ++k) {
        for (uint32_t b = tid; b < 256; b += nthreads) {
            const uint32_t t = tab[256 * (k - 1) + b];
            tab[256 * k + b] = (t << 8) ^ tab[t >> 24];
        }
        __syncthreads();
    }
}

// what global lane t works on
struct CrcLane {
    const uint8_t* base;             // the frame's byte 0
    uint64_t fi;                     // r * max_frames + f
    uint32_t j;                      // the lane's place in its group
    bool active;                     // the frame exists and lies below its row's count
};
__device__ inline CrcLane crc_lane(const CrcArgs& a, uint64_t t) {
    CrcLane L;
    L.fi = t >> a.logG;
    L.j = (uint32_t)t & ((1u << a.logG) - 1u);
    L.active = false;
    L.base = a.in;
    if (L.fi < a.frames) {
        const uint64_t r = L.fi / a.max_frames, f = L.fi - r * a.max_frames;
        uint64_t nf = a.n_frames ? a.n_frames[r] : a.max_frames;
        nf = nf < a.max_frames ? nf : a.max_frames;
        L.active = f < nf;
        L.base = a.in + L.fi * a.stride;
    }
    return L;
}

// lane j's chunk of the frame at base, reduced from a zero register (left-aligned)
__device__ inline uint32_t crc_chunk(const CrcArgs& a, const uint32_t* tab, const uint8_t* base, uint32_t j) {
    const uint32_t G = 1u << a.logG, words = a.C / 4u;
    const int64_t p0 = (int64_t)a.n_bits - (int64_t)(G - j) * 8 * (int64_t)a.C;      // the chunk's first bit in the message
    const uint32_t k0 = p0 < 0 ? (uint32_t)((uint64_t)(-p0) >> 5) : 0u;              // words wholly in front of the message
    if (k0 >= words) return 0u;
    const int64_t lo = (int64_t)(a.first_bit >> 3), hi = (int64_t)((a.first_bit + a.n_bits + 7) >> 3);   // the bytes the data occupy
    const int64_t p = p0 + 32 * (int64_t)k0;                                           // -31 .. : the first word that holds message bits
    const int64_t q = (int64_t)a.first_bit + p;                                        // its first bit in the frame (may lie in front of it)
    const int64_t B = q >> 3;                                                          // floor
    const uint32_t mis = (uint32_t)(((uintptr_t)base + (uintptr_t)B) & 3u);            // no pointer is formed in front of the frame
    const uint32_t sh = 8u * mis + ((uint32_t)q & 7u);
    int64_t off = B - (int64_t)mis;
    uint32_t d0 = crc_load_be32(base, off, lo, hi), reg = 0;
    for (uint32_t k = k0; k < words; ++k) {
        off += 4;
        const uint32_t d1 = crc_load_be32(base, off, lo, hi);
        uint32_t w = crc_funnel(d0, d1, sh);
        d0 = d1;
        if (k == k0 && p < 0) w &= 0xFFFFFFFFu >> (uint32_t)(-p);                      // the bits in front of message bit 0
        reg ^= w;
        reg = tab[768u + (reg >> 24)] ^ tab[512u + ((reg >> 16) & 255u)] ^ tab[256u + ((reg >> 8) & 255u)] ^ tab[reg & 255u];
    }
    return reg;
}

// one step of the combine: `mine` is the earlier part where bit s of j is clear, `theirs` the partner's
__device__ inline uint32_t crc_combine(const CrcArgs& a, uint32_t mine, uint32_t theirs, uint32_t s) {
    return crc_mul(mine, a.m[s], a.poly) ^ theirs;
}

// the group's lane 0: the frame's entries from the register over the whole message
__device__ inline void crc_finish(const CrcArgs& a, const CrcLane& L, uint32_t reg) {
    const uint32_t crc = ((reg ^ a.fin) >> a.shift) ^ a.xorout;
    if (a.crc) a.crc[L.fi] = crc;
    if (a.syndrome) {
        const uint64_t q = a.first_bit + a.n_bits;
        const int64_t lo = (int64_t)(q >> 3), hi = (int64_t)((q + a.width + 7) >> 3);  // the bytes the field occupies
        const uint32_t mis = (uint32_t)((uintptr_t)(L.base + lo) & 3u);
        const int64_t off = lo - (int64_t)mis;
        const uint32_t d0 = crc_load_be32(L.base, off, lo, hi), d1 = crc_load_be32(L.base, off + 4, lo, hi);
        a.syndrome[L.fi] = crc ^ (crc_funnel(d0, d1, 8u * mis + ((uint32_t)q & 7u)) >> a.shift);
    }
}

// kernels_dabplus.hpp reuses the device functions above; a kernel is emitted by the one unit that launches it
#ifndef VIT_CRC_DEVICE_FUNCTIONS_ONLY
__global__ void __launch_bounds__(CRC_BLOCK) crc_batch_kernel(CrcArgs a) {
    __shared__ uint32_t tab[1024];
    crc_build_tables(tab, a.poly, threadIdx.x, blockDim.x);
    const CrcLane L = crc_lane(a, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
    uint32_t reg = L.active ? crc_chunk(a, tab, L.base, L.j) : 0u;
    for (uint32_t s = 0; s < a.logG; ++s) reg = crc_combine(a, reg, __shfl_xor(reg, 1 << s), s);
    if (L.active && L.j == 0) crc_finish(a, L, reg);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------

// argument rule (include/vit_hip.h): everything the host can know without reading device memory
inline const char* crc_invalid(bool handle, const vit_hip_crc_params* c, const uint8_t* d_frames, size_t stride, size_t rows, size_t max_frames,
                               size_t first_bit, size_t n_bits, const uint32_t* d_crc, const uint32_t* d_syndrome) {
    if (!handle || !c || !d_frames) return "NULL handle, crc or d_frames";
    if (!d_crc && !d_syndrome) return "d_crc and d_syndrome are both NULL";
    if (c->width < 1 || c->width > 32) return "width must be 1 .. 32";
    const uint64_t top = 1ull << c->width;
    if (c->poly >= top || c->init >= top || c->xorout >= top) return "poly, init and xorout must lie below 2^width";
    if (first_bit >= 0xFFFFFFFFull || n_bits >= 0xFFFFFFFFull || first_bit + n_bits + 32 >= 0xFFFFFFFFull)
        return "first_bit + n_bits + 32 must lie below 2^32 - 1";
    const size_t need = (first_bit + n_bits + (d_syndrome ? c->width : 0u) + 7) / 8;
    if (stride != 0 && stride < need) return "frame_stride_bytes does not cover first_bit + n_bits (+ width)";
    if (rows == 0 || max_frames == 0) return nullptr;
    if (rows > 0x7FFFFFFFu || max_frames > 0x7FFFFFFFu) return "more than 2^31 - 1 blocks";
    const size_t frames = rows * max_frames;
    if (frames > ((uint64_t)0x7FFFFFFFu * CRC_BLOCK) >> crc_geometry(n_bits).logG) return "more than 2^31 - 1 blocks";
    const size_t in_b = extent(frames, stride ? stride : need, need), out_b = frames * sizeof(uint32_t);
    if (overlap(d_crc, out_b, d_syndrome, out_b)) return "d_crc overlaps d_syndrome";
    if (overlap(d_crc, out_b, d_frames, in_b) || overlap(d_syndrome, out_b, d_frames, in_b)) return "an output overlaps d_frames";
    return nullptr;
}

// the kernel arguments of a call the argument rule has accepted (rows, max_frames >= 1); poly, init, xorout below 2^width
inline CrcArgs crc_batch_args(const vit_hip_crc_params& c, const uint8_t* d_frames, size_t stride, size_t rows, size_t max_frames,
                              const uint32_t* d_n_frames, size_t first_bit, size_t n_bits, uint32_t* d_crc, uint32_t* d_syndrome) {
    CrcArgs a{};
    a.in = d_frames; a.n_frames = d_n_frames; a.crc = d_crc; a.syndrome = d_syndrome;
    a.max_frames = max_frames; a.frames = (uint64_t)rows * max_frames;
    a.first_bit = first_bit; a.n_bits = n_bits;
    a.width = c.width; a.shift = 32u - c.width;
    a.stride = stride ? stride : (first_bit + n_bits + (d_syndrome ? c.width : 0u) + 7) / 8;
    a.poly = c.poly << a.shift;
    a.fin = crc_mul(c.init << a.shift, crc_xpow(n_bits, a.poly), a.poly);
    a.xorout = c.xorout;
    const CrcGeometry g = crc_geometry(n_bits);
    a.logG = g.logG; a.C = g.C;
    uint32_t m = crc_xpow(8ull * g.C, a.poly);
    for (uint32_t s = 0; s < g.logG; ++s, m = crc_mul(m, m, a.poly)) a.m[s] = m;
    return a;
}

inline uint64_t crc_blocks(const CrcArgs& a) { return ((a.frames << a.logG) + CRC_BLOCK - 1) / CRC_BLOCK; }

// ---- launcher (hipGetLastError() after it: 0 / -1) ---------------------------------------------------------------------------

inline int crc_launch_batch(const CrcArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(crc_batch_kernel, dim3((unsigned)crc_blocks(a)), dim3(CRC_BLOCK), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
#endif  // VIT_CRC_DEVICE_FUNCTIONS_ONLY

}  // namespace vit
