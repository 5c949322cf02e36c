// kernels_dabplus.hpp -- DAB+ audio superframes (ETSI TS 102 563) on the logical frames the DAB route returns:
//   dabplus_sync_kernel   vit_hip_dabplus_sync: a thread per logical frame.  The 11 header bytes come in as three big-endian words through
//                         the guarded loads of kernels_crc.hpp (aligned dwords where they lie wholly inside the 11 bytes, single bytes at
//                         the ragged ends: any base alignment, no byte outside the header touched).  The Fire code runs as 72 shift /
//                         conditional-xor steps on a left-aligned register -- no table: a frame costs about 300 vector operations
//                         against four loads, and a table in LDS would add a prologue and a barrier to every block for nothing.  Hits are
//                         rare (one frame in five at best), so a hit is one LDS atomic on the block's five sums; the per-phase counts are a
//                         closed form of the block's span.  Five threads then add the block's sums to the totals with 32-bit atomics.
//   dabplus_zero_kernel   the totals of a call that overwrites them (a kernel, as marker_zero_kernel: the call enqueues kernels only).
//   dabplus_pick_kernel   a thread per row over its five candidates, by the "a beats b" rule of marker_search, the lower phase on a tie.
//   dabplus_au_kernel     vit_hip_dabplus_au_batch: ONE wave per (superframe, AU slot 0 .. 5).  Every wave reads the header itself (11
//                         bytes, the same address in all lanes), so the lengths never leave registers.  The AU is right-aligned in 64
//                         chunks of C bytes, C a host constant from s alone (64 C >= 110 s covers the longest AU): lane j reduces the
//                         message bits [n - (64-j) 8C, n - (63-j) 8C) from a zero register with the slice-by-4 tables of kernels_crc.hpp,
//                         lanes wholly in front of the AU do nothing, and the 6 combine steps use the host constants x^(8C 2^s) -- no
//                         multiplier is worked out on the device.  init = 0xFFFF enters by linearity as an XOR into the first 16 message
//                         bits, which needs no power of x that depends on the length (a one-byte AU: into its 8 bits, and the other 8 into
//                         the result).  Lane 0 writes the slot's entry; slot 0's lane 0 also writes the info word.
// Everything but the exchange is plain C++ in device functions and every loop strides by blockDim.x, so the source also compiles for the
// host (tests/cpp/dabplus_host_check.cpp).  Included only from vit_dabplus.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vit_hip.h"
#define VIT_CRC_DEVICE_FUNCTIONS_ONLY
#include "kernels_crc.hpp"

namespace vit {

constexpr uint32_t DABPLUS_BLOCK = 256;                // threads of a block, both kernels: 256 frames, or 4 (superframe, slot) waves
constexpr uint32_t DABPLUS_PHASES = 5;                 // logical frames of a superframe
constexpr uint32_t DABPLUS_SLOTS = 6;                  // AU entries of a superframe
constexpr uint32_t DABPLUS_FIRE_POLY = 0x782Fu << 16;  // left-aligned, without x^16
constexpr uint32_t DABPLUS_AU_POLY = 0x1021u << 16;

// ---- the header: bytes 0 .. 10 of a frame as three big-endian words (byte 11 reads as 0 and is not touched) ----------------------------

struct DabplusWords { uint32_t w[3]; };
__device__ inline DabplusWords dabplus_load_header(const uint8_t* base) {
    const uint32_t mis = (uint32_t)((uintptr_t)base & 3u), sh = 8u * mis;
    const int64_t off = -(int64_t)mis;
    const uint32_t d0 = crc_load_be32(base, off, 0, 11), d1 = crc_load_be32(base, off + 4, 0, 11), d2 = crc_load_be32(base, off + 8, 0, 11),
                   d3 = crc_load_be32(base, off + 12, 0, 11);
    DabplusWords h;
    h.w[0] = crc_funnel(d0, d1, sh); h.w[1] = crc_funnel(d1, d2, sh); h.w[2] = crc_funnel(d2, d3, sh);
    return h;
}

__device__ inline uint32_t dabplus_shift(uint32_t reg, uint32_t steps) {
    for (uint32_t i = 0; i < steps; ++i) reg = crc_timesx(reg, DABPLUS_FIRE_POLY);
    return reg;
}

// the Fire code over bytes 2 .. 10 equals bytes 0 .. 1, and the 11 bytes are not all zero
__device__ inline bool dabplus_fire_hit(const DabplusWords& h) {
    uint32_t reg = dabplus_shift(h.w[0] << 16, 16);
    reg = dabplus_shift(reg ^ h.w[1], 32);
    reg = dabplus_shift(reg ^ (h.w[2] & 0xFFFFFF00u), 24);
    return (reg >> 16) == (h.w[0] >> 16) && (h.w[0] | h.w[1] | (h.w[2] & 0xFFFFFF00u)) != 0u;
}

// the 12 bits at bit offset t <= 72 of the header
__device__ inline uint32_t dabplus_field12(const DabplusWords& h, uint32_t t) {
    const uint32_t i = t >> 5, r = t & 31u;
    const uint64_t v = ((uint64_t)h.w[i] << 32) | (i < 2 ? h.w[i + 1] : 0u);
    return (uint32_t)(v >> (52u - r)) & 0xFFFu;
}

struct DabplusHeader {
    uint32_t fire_ok, consistent, n_aus, byte2;
    uint32_t start[DABPLUS_SLOTS + 1];                 // start[n_aus] = data_bytes; entries behind it are not set
};
__device__ inline DabplusHeader dabplus_header(const uint8_t* base, uint32_t data_bytes) {
    const DabplusWords h = dabplus_load_header(base);
    DabplusHeader H;
    H.fire_ok = dabplus_fire_hit(h) ? 1u : 0u;
    H.byte2 = (h.w[0] >> 8) & 0xFFu;
    const uint32_t dac = (H.byte2 >> 6) & 1u, sbr = (H.byte2 >> 5) & 1u;
    H.n_aus = sbr ? (dac ? 3u : 2u) : (dac ? 6u : 4u);
    H.start[0] = sbr ? (dac ? 6u : 5u) : (dac ? 11u : 8u);
    H.consistent = 1u;
#pragma unroll
    for (uint32_t k = 1; k <= DABPLUS_SLOTS; ++k) {
        if (k <= H.n_aus) {
            H.start[k] = k < H.n_aus ? dabplus_field12(h, 24u + 12u * (k - 1u)) : data_bytes;
            if (H.start[k] < H.start[k - 1] + 3u) H.consistent = 0u;
        } else {
            H.start[k] = 0u;
        }
    }
    return H;
}

// ---- sync --------------------------------------------------------------------------------------------------------------------------

struct DabplusSyncArgs {
    const uint8_t* frames;           // frame (r, f) at frames + r * row_stride + f * frame_stride
    const uint32_t* n_frames;        // [rows] or null
    uint32_t* hits;                  // [rows][5]
    uint32_t* count;                 // [rows][5]
    uint64_t row_stride, frame_stride;
    uint64_t items;                  // rows * spans_per_row
    uint32_t max_frames, frame0, spans_per_row;
};

// frames f < x of phase p, frame f being of phase (frame0 + f) mod 5
__device__ inline uint32_t dabplus_phase_count(uint32_t x, uint32_t p, uint32_t frame0) {
    const uint32_t first = (p + DABPLUS_PHASES - frame0) % DABPLUS_PHASES;
    return x > first ? (x - first + DABPLUS_PHASES - 1u) / DABPLUS_PHASES : 0u;
}

__global__ void __launch_bounds__(DABPLUS_BLOCK) dabplus_sync_kernel(DabplusSyncArgs a) {
    __shared__ uint32_t acc[DABPLUS_PHASES];
    const uint32_t NT = blockDim.x, tid = threadIdx.x;
    for (uint64_t item = blockIdx.x; item < a.items; item += gridDim.x) {
        for (uint32_t p = tid; p < DABPLUS_PHASES; p += NT) acc[p] = 0;
        __syncthreads();
        const uint64_t r = item / a.spans_per_row;
        const uint32_t span = (uint32_t)(item - r * a.spans_per_row);
        uint32_t nf = a.n_frames ? a.n_frames[r] : a.max_frames;
        nf = nf < a.max_frames ? nf : a.max_frames;
        const uint32_t lo = span * DABPLUS_BLOCK;                                       // below max_frames < 2^31
        uint32_t hi = nf < lo + DABPLUS_BLOCK ? nf : lo + DABPLUS_BLOCK;
        hi = hi < lo ? lo : hi;
        const uint8_t* row = a.frames + r * a.row_stride;
        for (uint32_t f = lo + tid; f < hi; f += NT)
            if (dabplus_fire_hit(dabplus_load_header(row + (uint64_t)f * a.frame_stride))) atomicAdd(&acc[(a.frame0 + f) % DABPLUS_PHASES], 1u);
        __syncthreads();
        for (uint32_t p = tid; p < DABPLUS_PHASES; p += NT) {
            const uint32_t c = dabplus_phase_count(hi, p, a.frame0) - dabplus_phase_count(lo, p, a.frame0);
            if (c) atomicAdd(a.count + r * DABPLUS_PHASES + p, c);
            if (acc[p]) atomicAdd(a.hits + r * DABPLUS_PHASES + p, acc[p]);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(DABPLUS_BLOCK) dabplus_zero_kernel(uint32_t* hits, uint32_t* count, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        hits[i] = 0;
        count[i] = 0;
    }
}

// a beats b iff compared_a > 0 and (compared_b == 0 or errors_a * compared_b < errors_b * compared_a): marker_beats of kernels_marker.hpp
__device__ inline bool dabplus_beats(uint32_t ea, uint32_t ca, uint32_t eb, uint32_t cb) {
    return ca > 0 && (cb == 0 || (uint64_t)ea * cb < (uint64_t)eb * ca);
}

// the lock of one row from its totals: ascending phases and a strict "beats" leave the lower phase on a tie
__device__ inline vit_hip_marker_lock dabplus_pick(const uint32_t* hits, const uint32_t* count, uint32_t frame_bytes) {
    uint32_t best = 0, e = count[0] - hits[0], c = count[0];
    for (uint32_t p = 1; p < DABPLUS_PHASES; ++p) {
        const uint32_t ep = count[p] - hits[p], cp = count[p];
        if (dabplus_beats(ep, cp, e, c)) { best = p; e = ep; c = cp; }
    }
    vit_hip_marker_lock out;
    out.phase = best * 8u * frame_bytes;
    out.inverted = 0;
    out.errors = e;
    out.compared = c;
    return out;
}

__global__ void __launch_bounds__(DABPLUS_BLOCK) dabplus_pick_kernel(const uint32_t* hits, const uint32_t* count, vit_hip_marker_lock* lock,
                                                                     uint64_t rows, uint32_t frame_bytes) {
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (uint64_t)gridDim.x * blockDim.x)
        lock[r] = dabplus_pick(hits + r * DABPLUS_PHASES, count + r * DABPLUS_PHASES, frame_bytes);
}

// the kernel arguments of a call the argument rule has accepted (rows, max_frames >= 1)
inline DabplusSyncArgs dabplus_sync_args(const uint8_t* d_frames, size_t row_stride, size_t frame_stride, size_t rows, size_t max_frames,
                                         const uint32_t* d_n_frames, unsigned frame0, uint32_t* d_hits, uint32_t* d_count) {
    DabplusSyncArgs a{};
    a.frames = d_frames; a.n_frames = d_n_frames; a.hits = d_hits; a.count = d_count;
    a.row_stride = row_stride; a.frame_stride = frame_stride;
    a.max_frames = (uint32_t)max_frames; a.frame0 = frame0;
    a.spans_per_row = (uint32_t)((max_frames + DABPLUS_BLOCK - 1) / DABPLUS_BLOCK);
    a.items = (uint64_t)rows * a.spans_per_row;
    return a;
}

// ---- AU table ------------------------------------------------------------------------------------------------------------------------

struct DabplusAuArgs {
    const uint8_t* in;               // superframe (r, f) at in + (r * max_frames + f) * stride
    const uint32_t* n_frames;        // [rows] or null
    const int32_t* rs_status;        // [frames][s] or null
    uint32_t* info;                  // [frames]
    vit_hip_dabplus_au* au;          // [frames][6]
    uint64_t stride, max_frames, frames;       // frames = rows * max_frames
    uint32_t s, data_bytes;          // data_bytes = 110 s
    uint32_t C;                      // bytes of a lane's chunk, a multiple of 4: 64 C >= data_bytes
    uint32_t m[6];                   // m[t] = x^(8 C 2^t) mod P'
};

inline uint32_t dabplus_chunk_bytes(uint32_t s) { return ((110u * s + 63u) / 64u + 3u) & ~3u; }

// what global thread t works on: lane j of the wave of (superframe fi, slot k)
struct DabplusAuLane {
    const uint8_t* base;
    uint64_t fi;
    uint32_t k, j;
    bool active;                     // the superframe exists and lies below its row's count
    bool has;                        // and is valid with an AU in this slot
    uint32_t start, next;            // then au_start[k] and au_start[k + 1] (picked by comparison: no indexed register array)
    DabplusHeader H;
};
__device__ inline DabplusAuLane dabplus_au_lane(const DabplusAuArgs& a, uint64_t t) {
    DabplusAuLane L;
    const uint64_t w = t >> 6;
    L.j = (uint32_t)t & 63u;
    L.fi = w / DABPLUS_SLOTS;
    L.k = (uint32_t)(w - L.fi * DABPLUS_SLOTS);
    L.active = L.has = false;
    L.base = a.in;
    L.H = DabplusHeader{};
    L.start = L.next = 0;
    if (L.fi < a.frames) {
        const uint64_t r = L.fi / a.max_frames, f = L.fi - r * a.max_frames;
        uint64_t nf = a.n_frames ? a.n_frames[r] : a.max_frames;
        nf = nf < a.max_frames ? nf : a.max_frames;
        L.active = f < nf;
        L.base = a.in + L.fi * a.stride;
    }
    if (L.active) {
        L.H = dabplus_header(L.base, a.data_bytes);
        L.has = L.H.fire_ok && L.H.consistent && L.k < L.H.n_aus;
#pragma unroll
        for (uint32_t i = 0; i < DABPLUS_SLOTS; ++i)
            if (i == L.k) { L.start = L.H.start[i]; L.next = L.H.start[i + 1]; }
    }
    return L;
}

// lane j's chunk of the AU's `bytes` data bytes at base + start, reduced from a zero register (left-aligned), init XORed into the
// message's first 16 bits.  A consistent header keeps [start, start + bytes + 2) inside the superframe's data bytes
__device__ inline uint32_t dabplus_au_chunk(const uint32_t* tab, const uint8_t* base, uint32_t start, uint32_t bytes, uint32_t C, uint32_t j) {
    const uint32_t words = C / 4u;
    const int64_t p0 = 8 * (int64_t)bytes - (int64_t)(64u - j) * 8 * (int64_t)C;       // the chunk's first bit in the message
    const uint32_t k0 = p0 < 0 ? (uint32_t)((uint64_t)(-p0) >> 5) : 0u;                // words wholly in front of the message
    if (k0 >= words) return 0u;
    const int64_t lo = start, hi = (int64_t)start + bytes;
    int64_t p = p0 + 32 * (int64_t)k0;                                                 // -24 .. : the first word that holds message bits
    const int64_t B = (int64_t)start + (p >> 3);                                       // its first byte in the superframe: start >= 5 keeps it >= 2
    const uint32_t mis = (uint32_t)(((uintptr_t)base + (uintptr_t)B) & 3u);
    const uint32_t sh = 8u * mis;
    int64_t off = B - (int64_t)mis;
    uint32_t d0 = crc_load_be32(base, off, lo, hi), reg = 0;
    for (uint32_t k = k0; k < words; ++k, p += 32) {
        off += 4;
        const uint32_t d1 = crc_load_be32(base, off, lo, hi);
        uint32_t w = crc_funnel(d0, d1, sh);
        d0 = d1;
        if (p < 0) w &= 0xFFFFFFFFu >> (uint32_t)(-p);                                 // the bits in front of message bit 0
        if (p < 16) w ^= p < 0 ? 0xFFFF0000u >> (uint32_t)(-p) : 0xFFFFFFFFu << (uint32_t)(16 + p);    // init over message bits 0 .. 15
        reg ^= w;
        reg = tab[768u + (reg >> 24)] ^ tab[512u + ((reg >> 16) & 255u)] ^ tab[256u + ((reg >> 8) & 255u)] ^ tab[reg & 255u];
    }
    return reg;
}

// one step of the combine: `mine` is the earlier part where bit t of j is clear
__device__ inline uint32_t dabplus_au_combine(const DabplusAuArgs& a, uint32_t mine, uint32_t theirs, uint32_t t) {
    return crc_mul(mine, a.m[t], DABPLUS_AU_POLY) ^ theirs;
}

// lane 0 of a wave: the slot's entry, and with slot 0 the info word
__device__ inline void dabplus_au_finish(const DabplusAuArgs& a, const DabplusAuLane& L, uint32_t reg) {
    vit_hip_dabplus_au e;
    e.start = 0; e.bytes = 0; e.syndrome = 0xFFFFFFFFu;
    if (L.has) {
        e.start = L.start;
        e.bytes = L.next - L.start - 2u;
        const uint32_t crc = ((reg >> 16) ^ 0xFFFFu) ^ (e.bytes == 1u ? 0xFF00u : 0u);  // a one-byte AU takes 8 bits of init; the rest falls through
        const uint8_t* field = L.base + e.start + e.bytes;
        e.syndrome = crc ^ ((uint32_t)field[0] << 8 | field[1]);
    }
    a.au[L.fi * DABPLUS_SLOTS + L.k] = e;
    if (L.k == 0) {
        uint32_t rs_failed = 0;
        if (a.rs_status)
            for (uint32_t c = 0; c < a.s; ++c) rs_failed |= a.rs_status[L.fi * a.s + c] < 0 ? 1u : 0u;
        const uint32_t valid = L.H.fire_ok & L.H.consistent;
        a.info[L.fi] = L.H.fire_ok | L.H.consistent << 1 | rs_failed << 2 | (valid ? L.H.n_aus : 0u) << 4 | L.H.byte2 << 8;
    }
}

__global__ void __launch_bounds__(DABPLUS_BLOCK) dabplus_au_kernel(DabplusAuArgs a) {
    __shared__ uint32_t tab[1024];
    crc_build_tables(tab, DABPLUS_AU_POLY, threadIdx.x, blockDim.x);
    const DabplusAuLane L = dabplus_au_lane(a, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
    uint32_t reg = L.has ? dabplus_au_chunk(tab, L.base, L.start, L.next - L.start - 2u, a.C, L.j) : 0u;
    for (uint32_t t = 0; t < 6; ++t) reg = dabplus_au_combine(a, reg, __shfl_xor(reg, 1 << t), t);
    if (L.active && L.j == 0) dabplus_au_finish(a, L, reg);
}

// the kernel arguments of a call the argument rule has accepted (rows, max_frames >= 1, 1 <= s <= 24)
inline DabplusAuArgs dabplus_au_args(const uint8_t* d_in, size_t stride, size_t rows, size_t max_frames, const uint32_t* d_n_frames, unsigned s,
                                     const int32_t* d_rs_status, uint32_t* d_info, vit_hip_dabplus_au* d_au) {
    DabplusAuArgs a{};
    a.in = d_in; a.n_frames = d_n_frames; a.rs_status = d_rs_status; a.info = d_info; a.au = d_au;
    a.stride = stride ? stride : 120u * s;
    a.max_frames = max_frames; a.frames = (uint64_t)rows * max_frames;
    a.s = s; a.data_bytes = 110u * s;
    a.C = dabplus_chunk_bytes(s);
    uint32_t m = crc_xpow(8ull * a.C, DABPLUS_AU_POLY);
    for (uint32_t t = 0; t < 6; ++t, m = crc_mul(m, m, DABPLUS_AU_POLY)) a.m[t] = m;
    return a;
}

inline uint64_t dabplus_au_blocks(const DabplusAuArgs& a) { return (a.frames * DABPLUS_SLOTS * 64u + DABPLUS_BLOCK - 1) / DABPLUS_BLOCK; }

// ---- host side -----------------------------------------------------------------------------------------------------------------------------

// argument rules (include/vit_hip.h): everything the host can know without reading device memory
inline const char* dabplus_sync_invalid(bool handle, const uint8_t* d_frames, size_t row_stride, size_t frame_stride, size_t frame_bytes,
                                        size_t rows, size_t max_frames, const uint32_t* d_n_frames, unsigned frame0, unsigned flags,
                                        const uint32_t* d_hits, const uint32_t* d_count, const vit_hip_marker_lock* d_lock) {
    if (!handle || !d_frames || !d_hits || !d_count) return "NULL handle, d_frames, d_hits or d_count";
    if (flags & ~VIT_HIP_MARKER_ACCUMULATE) return "unknown flag bits";
    if (frame_bytes < 11) return "frame_bytes must be at least 11";
    if (frame_bytes > 0x7FFFFFFFull / 40) return "40 * frame_bytes must lie below 2^31";
    if (frame0 >= DABPLUS_PHASES) return "frame0 must be below 5";
    const size_t fs = frame_stride ? frame_stride : frame_bytes;
    if (fs < frame_bytes) return "frame_stride is below frame_bytes";
    if (rows > 0x7FFFFFFFu || max_frames > 0x7FFFFFFFu) return "more than 2^31 - 1 rows or frames";
    if (fs > 0xFFFFFFFFFFFFull / (max_frames ? max_frames : 1)) return "max_frames * frame_stride is too large";
    if (row_stride != 0 && row_stride < max_frames * fs) return "row_stride is below max_frames * frame_stride";
    if (misaligned(d_n_frames, 4) || misaligned(d_hits, 4) || misaligned(d_count, 4) || misaligned(d_lock, 4))
        return "the count arrays, the totals and d_lock must be aligned to 4 bytes";
    if (rows == 0) return nullptr;
    const size_t rs = row_stride ? row_stride : max_frames * fs;
    const size_t in_b = max_frames ? extent(rows, rs, extent(max_frames, fs, frame_bytes)) : 0, tot_b = rows * DABPLUS_PHASES * sizeof(uint32_t);
    const size_t lock_b = rows * sizeof(vit_hip_marker_lock), cnt_b = rows * sizeof(uint32_t);
    if (overlap(d_hits, tot_b, d_count, tot_b) || overlap(d_hits, tot_b, d_lock, lock_b) || overlap(d_count, tot_b, d_lock, lock_b))
        return "d_hits, d_count and d_lock overlap";
    if (overlap(d_hits, tot_b, d_frames, in_b) || overlap(d_count, tot_b, d_frames, in_b) || overlap(d_lock, lock_b, d_frames, in_b) ||
        overlap(d_hits, tot_b, d_n_frames, cnt_b) || overlap(d_count, tot_b, d_n_frames, cnt_b) || overlap(d_lock, lock_b, d_n_frames, cnt_b))
        return "an output overlaps the frames or d_n_frames";
    return nullptr;
}

inline const char* dabplus_au_invalid(bool handle, const uint8_t* d_in, size_t stride, size_t rows, size_t max_frames, const uint32_t* d_n_frames,
                                      unsigned s, const int32_t* d_rs_status, const uint32_t* d_info, const vit_hip_dabplus_au* d_au) {
    if (!handle || !d_in || !d_info || !d_au) return "NULL handle, d_in, d_info or d_au";
    if (s < 1 || s > 24) return "s must be 1 .. 24";
    if (stride != 0 && stride < 110u * s) return "frame_stride_bytes is below 110 s";
    if (misaligned(d_n_frames, 4) || misaligned(d_rs_status, 4) || misaligned(d_info, 4) || misaligned(d_au, 4))
        return "the count array, d_rs_status, d_info and d_au must be aligned to 4 bytes";
    if (rows == 0 || max_frames == 0) return nullptr;
    if (rows > 0x7FFFFFFFu || max_frames > 0x7FFFFFFFu) return "more than 2^31 - 1 rows or frames";
    const size_t frames = rows * max_frames, st = stride ? stride : 120u * s;
    if (frames > 0x7FFFFFFFull * DABPLUS_BLOCK / (DABPLUS_SLOTS * 64u)) return "more than 2^31 - 1 blocks";
    const size_t in_b = extent(frames, st, 110u * s), info_b = frames * sizeof(uint32_t), au_b = frames * DABPLUS_SLOTS * sizeof(vit_hip_dabplus_au);
    const size_t rs_b = frames * s * sizeof(int32_t), cnt_b = rows * sizeof(uint32_t);
    if (overlap(d_info, info_b, d_au, au_b)) return "d_info overlaps d_au";
    if (overlap(d_info, info_b, d_in, in_b) || overlap(d_au, au_b, d_in, in_b) || overlap(d_info, info_b, d_rs_status, rs_b) ||
        overlap(d_au, au_b, d_rs_status, rs_b) || overlap(d_info, info_b, d_n_frames, cnt_b) || overlap(d_au, au_b, d_n_frames, cnt_b))
        return "an output overlaps the superframes, d_rs_status or d_n_frames";
    return nullptr;
}

// ---- launchers (hipGetLastError() after each: 0 / -1) ----------------------------------------------------------------------------

// blocks of a grid-stride kernel over n items, `most` at the most
inline unsigned dabplus_grid(uint64_t n, uint64_t most) {
    const uint64_t blocks = (n + DABPLUS_BLOCK - 1) / DABPLUS_BLOCK;
    return (unsigned)(blocks < most ? blocks : most);
}

inline int dabplus_launch_zero(uint32_t* hits, uint32_t* count, uint64_t n, hipStream_t st) {
    hipLaunchKernelGGL(dabplus_zero_kernel, dim3(dabplus_grid(n, 2048)), dim3(DABPLUS_BLOCK), 0, st, hits, count, n);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

inline int dabplus_launch_sync(const DabplusSyncArgs& a, hipStream_t st) {
    // at most 65536 blocks: the kernel strides by the grid past that
    hipLaunchKernelGGL(dabplus_sync_kernel, dim3((unsigned)(a.items < 65536 ? a.items : 65536)), dim3(DABPLUS_BLOCK), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

inline int dabplus_launch_pick(const uint32_t* hits, const uint32_t* count, vit_hip_marker_lock* lock, uint64_t rows, uint32_t frame_bytes,
                               hipStream_t st) {
    hipLaunchKernelGGL(dabplus_pick_kernel, dim3(dabplus_grid(rows, 2048)), dim3(DABPLUS_BLOCK), 0, st, hits, count, lock, rows, frame_bytes);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

inline int dabplus_launch_au(const DabplusAuArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(dabplus_au_kernel, dim3((unsigned)dabplus_au_blocks(a)), dim3(DABPLUS_BLOCK), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace vit
