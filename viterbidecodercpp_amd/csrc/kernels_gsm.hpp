// kernels_gsm.hpp -- GSM channel decoding (3GPP TS 45.003) around the K = 5, R = 1/2 decode: vit_hip_gsm_deinterleave_batch (the block and the
// diagonal burst de-interleaver with the stealing flags), vit_hip_gsm_fire_batch (the 40-bit Fire code of the control channels: check and
// correction of one error burst by error trapping) and vit_hip_gsm_tchfs_batch (the TCH/FS frame: class I reorder, the 3 parity bits, the
// hard decisions of class II).
//   gsm_deinterleave_kernel<soft_t>  One wavefront per (row, block), GSM_BLOCKS blocks per workgroup.  The wave STAGES the block's 4 or 8
//                       bursts in LDS: lane l reads elements l and l + 64 of every burst, so a burst is two runs of consecutive
//                       addresses; the optional negation (int32, clamped to soft_t) happens here, once per element.  Behind the barrier
//                       lane l EMITS coded bits k = l, l + 64, .. < 456: j = 2 (49 k mod 57) + (k mod 8) div 4 in arithmetic, no table, one
//                       LDS read at (k mod 8 or 4) * 116 + j (+ 2 behind the flags), and up to two stores (d_full[k]; d_class1[k] or
//                       d_class2[k - 378]) at consecutive addresses across the wave.  A block is read from memory once for its up to
//                       three outputs.  Lane 0 adds the flags; the wave of a row's last slot carries the last four bursts, as received,
//                       to d_hist_out and writes the row's counts.  A slot without a block (diagonal mode, no history) is written as zeros.
//   gsm_fire_kernel     One wavefront per frame, GSM_BLOCKS frames per workgroup.  Lane l < 28 takes byte l of the 224 bits and multiplies
//                       it by D^(8 (27 - l)) mod g (a constant table of 28 remainders, 7 reduction steps in 64-bit registers) into LDS;
//                       behind the barrier every lane XORs the 28 pieces: linearity, as kernels_crc.hpp does it, and every lane holds
//                       the syndrome.  Zero: done.  Otherwise lane l walks the shifts m = l, l + 64, l + 128, l + 192 by dividing the
//                       syndrome by D (if bit 0 is set, XOR g; shift right) and posts the one (m, pattern) with pattern(0) = 1, degree
//                       below max_burst and m + degree <= 223 -- it is unique (include/vit_hip.h) -- to LDS; behind a second barrier
//                       lanes l < 23 flip and write the data bytes.  Only frames that fail the check walk.
//   gsm_tchfs_kernel    One wavefront per frame: stage the 24 decoded bytes and the 78 hard decisions of class II in LDS, then lane
//                       l < 33 composes speech byte l and lane 33 the parity syndrome and the erasure count.
// Everything is plain C++ in device functions that take (block, thread): the source also runs on the host (tests/cpp/gsm_host_check.cpp),
// the argument rules included.  Included only from vit_gsm.hip.
// Out of scope: GPRS CS-2..4 and EGPRS (puncturing tables, USF precoding); TCH/HS, EFR's preliminary CRC-8, AMR; SACCH/TCH multiframe
// scheduling and deciphering (the caller negates with the A5 keystream); burst demodulation; per-row burst counts in one call; a
// transmitter on the card.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vit_hip.h"
#include "arg_rules.hpp"

namespace vit {

constexpr uint32_t GSM_THREADS = 256, GSM_WAVE = 64;
constexpr uint32_t GSM_BLOCKS = GSM_THREADS / GSM_WAVE;            // blocks or frames of a workgroup: one wavefront each
constexpr uint32_t GSM_BURST = 116, GSM_CODED = 456, GSM_CLASS1 = 378, GSM_CLASS2 = 78, GSM_HIST = 4 * GSM_BURST;
constexpr uint32_t GSM_FIRE_IN = 28, GSM_FIRE_OUT = 23, GSM_TCHFS_IN = 24, GSM_TCHFS_OUT = 33;
constexpr uint64_t GSM_FIRE_G = 0x10004820009ull, GSM_FIRE_MASK = (1ull << 40) - 1;

// coded bit k of a block lies at payload position j(k) of burst 4 n + (k mod 4) (block mode) or 4 n + (k mod 8) (diagonal mode)
__host__ __device__ inline uint32_t gsm_j(uint32_t k) { return 2u * ((49u * k) % 57u) + ((k & 7u) >> 2); }
// payload position j as an element of the 116 of a burst: the two stealing flags sit at 57 and 58
__host__ __device__ inline uint32_t gsm_element(uint32_t j) { return j < 57u ? j : j + 2u; }

// ---- the burst de-interleaver --------------------------------------------------------------------------------------------------------------

struct GsmArgs {
    const void* in;                  // soft_t, burst b of row r at r * row_stride + b * burst_stride: 116 elements
    const void* hist_in;             // soft_t [rows][4][116] or null
    const uint32_t* fill_in;         // [rows] or null
    void* hist_out;                  // soft_t [rows][4][116] or null
    uint32_t *fill_out, *n_out;      // [rows] or null
    void *full, *class1, *class2;    // soft_t [rows][blocks][456 / 378 / 78] or null
    int32_t* steal;                  // [rows][blocks] or null
    uint64_t row_stride, burst_stride;
    uint32_t rows, blocks, diagonal, negate;
    int32_t lo, hi;                  // the range of soft_t
};

// the bursts of slot `slot` of row `row`: how many (0: the slot holds no block), and burst q's address
struct GsmSlot {
    uint32_t count;
    uint32_t carried;                // 1: the row's history is in front of the input
};

__device__ inline GsmSlot gsm_slot(const GsmArgs& a, uint32_t row, uint32_t slot) {
    GsmSlot s;
    s.carried = a.diagonal && a.hist_in && a.fill_in && a.fill_in[row] == 4u ? 1u : 0u;
    s.count = !a.diagonal ? 4u : (slot + 1u - s.carried < a.blocks ? 8u : 0u);
    return s;
}

template <class soft_t>
__device__ inline const soft_t* gsm_burst(const GsmArgs& a, const GsmSlot& s, uint32_t row, uint32_t slot, uint32_t q) {
    const uint32_t at = 4u * slot + q;                               // in the sequence history + input
    if (s.carried && at < 4u) return (const soft_t*)a.hist_in + (uint64_t)row * GSM_HIST + at * GSM_BURST;
    return (const soft_t*)a.in + (uint64_t)row * a.row_stride + (uint64_t)(at - 4u * s.carried) * a.burst_stride;
}

// lane `tid % 64` of wavefront `tid / 64`: its two elements of every burst of the slot into LDS, negated where the call says so
template <class soft_t>
__device__ inline void gsm_stage(const GsmArgs& a, soft_t* lds, uint32_t block, uint32_t tid) {
    const uint32_t w = tid / GSM_WAVE, lane = tid % GSM_WAVE;
    const uint64_t item = (uint64_t)block * GSM_BLOCKS + w;
    if (item >= (uint64_t)a.rows * a.blocks) return;
    const uint32_t row = (uint32_t)(item / a.blocks), slot = (uint32_t)(item % a.blocks);
    const GsmSlot s = gsm_slot(a, row, slot);
    soft_t* mine = lds + w * (8u * GSM_BURST);
    for (uint32_t q = 0; q < s.count; ++q) {
        const soft_t* burst = gsm_burst<soft_t>(a, s, row, slot, q);
        for (uint32_t e = lane; e < GSM_BURST; e += GSM_WAVE) {
            int32_t v = (int32_t)burst[e];
            if (a.negate) {
                v = -v;
                v = v > a.hi ? a.hi : v;
            }
            mine[q * GSM_BURST + e] = (soft_t)v;
        }
    }
}

// the same lane behind the barrier: coded bits lane, lane + 64, .. of the slot's block into the outputs; the row's carried state
template <class soft_t>
__device__ inline void gsm_emit(const GsmArgs& a, const soft_t* lds, uint32_t block, uint32_t tid) {
    const uint32_t w = tid / GSM_WAVE, lane = tid % GSM_WAVE;
    const uint64_t item = (uint64_t)block * GSM_BLOCKS + w;
    if (item >= (uint64_t)a.rows * a.blocks) return;
    const uint32_t row = (uint32_t)(item / a.blocks), slot = (uint32_t)(item % a.blocks);
    const GsmSlot s = gsm_slot(a, row, slot);
    const soft_t* mine = lds + w * (8u * GSM_BURST);
    const uint32_t spread = a.diagonal ? 7u : 3u;
    for (uint32_t k = lane; k < GSM_CODED; k += GSM_WAVE) {
        const soft_t v = s.count ? mine[(k & spread) * GSM_BURST + gsm_element(gsm_j(k))] : (soft_t)0;
        if (a.full) ((soft_t*)a.full)[item * GSM_CODED + k] = v;
        if (k < GSM_CLASS1) {
            if (a.class1) ((soft_t*)a.class1)[item * GSM_CLASS1 + k] = v;
        } else if (a.class2) {
            ((soft_t*)a.class2)[item * GSM_CLASS2 + (k - GSM_CLASS1)] = v;
        }
    }
    if (lane == 0 && a.steal) {
        int32_t sum = 0;
        for (uint32_t q = 0; q < s.count; ++q) {
            if (!a.diagonal || q < 4u) sum += (int32_t)mine[q * GSM_BURST + 58u];          // hu
            if (!a.diagonal || q >= 4u) sum += (int32_t)mine[q * GSM_BURST + 57u];         // hl
        }
        a.steal[item] = sum;
    }
    if (slot + 1u != a.blocks) return;
    // the row's last slot: the last four bursts of the input, as received, are the next call's history
    if (a.hist_out) {
        const soft_t* last = (const soft_t*)a.in + (uint64_t)row * a.row_stride + (uint64_t)(4u * a.blocks - 4u) * a.burst_stride;
        soft_t* hist = (soft_t*)a.hist_out + (uint64_t)row * GSM_HIST;
        for (uint32_t e = lane; e < GSM_HIST; e += GSM_WAVE) hist[e] = last[(uint64_t)(e / GSM_BURST) * a.burst_stride + e % GSM_BURST];
    }
    if (lane == 0) {
        if (a.fill_out) a.fill_out[row] = 4u;
        if (a.n_out) a.n_out[row] = a.diagonal ? a.blocks - 1u + s.carried : a.blocks;
    }
}

template <class soft_t>
__global__ void __launch_bounds__(GSM_THREADS) gsm_deinterleave_kernel(GsmArgs a) {
    __shared__ soft_t lds[GSM_BLOCKS * 8 * GSM_BURST];
    gsm_stage<soft_t>(a, lds, blockIdx.x, threadIdx.x);
    __syncthreads();
    gsm_emit<soft_t>(a, lds, blockIdx.x, threadIdx.x);
}

// ---- the Fire code ----------------------------------------------------------------------------------------------------------------------------

// x D mod g, x below 2^40
__host__ __device__ constexpr uint64_t gsm_fire_times_d(uint64_t x) { return ((x << 1) ^ ((x >> 39) & 1 ? GSM_FIRE_G : 0)) & GSM_FIRE_MASK; }
// x / D mod g
__host__ __device__ constexpr uint64_t gsm_fire_over_d(uint64_t x) { return (x ^ (x & 1 ? GSM_FIRE_G : 0)) >> 1; }

struct GsmFirePowers {
    uint64_t at[GSM_FIRE_IN];        // D^(8 i) mod g
    constexpr GsmFirePowers() : at() {
        uint64_t x = 1;
        for (uint32_t i = 0; i < GSM_FIRE_IN; ++i) {
            at[i] = x;
            for (int s = 0; s < 8; ++s) x = gsm_fire_times_d(x);
        }
    }
};
__device__ static constexpr GsmFirePowers GSM_FIRE_POWERS{};

struct GsmFireArgs {
    const uint8_t* bytes;            // frame f at f * bytes_stride: 28 bytes, bit t of a frame is bit 7 - t % 8 of byte t / 8
    vit_hip_gsm_fire* status;
    uint8_t* data;                   // frame f at f * data_stride: 23 bytes
    uint64_t bytes_stride, data_stride;
    uint32_t frames, max_burst, lsb_first;
};

struct GsmFireLds {
    uint64_t piece[GSM_BLOCKS][GSM_FIRE_IN];
    uint64_t pattern[GSM_BLOCKS];
    uint32_t shift[GSM_BLOCKS];
    uint8_t raw[GSM_BLOCKS][GSM_FIRE_IN];
};

// lane l < 28: byte l times D^(8 (27 - l)) mod g
__device__ inline void gsm_fire_stage(const GsmFireArgs& a, GsmFireLds& lds, uint32_t block, uint32_t tid) {
    const uint32_t w = tid / GSM_WAVE, lane = tid % GSM_WAVE;
    const uint64_t f = (uint64_t)block * GSM_BLOCKS + w;
    if (f >= a.frames) return;
    if (lane == 0) lds.shift[w] = 0xFFFFFFFFu;
    if (lane >= GSM_FIRE_IN) return;
    const uint32_t b = a.bytes[f * a.bytes_stride + lane];
    const uint64_t power = GSM_FIRE_POWERS.at[GSM_FIRE_IN - 1u - lane];
    uint64_t x = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i)
        if ((b >> i) & 1u) x ^= power << i;
#pragma unroll
    for (int top = 46; top >= 40; --top)
        if ((x >> top) & 1u) x ^= GSM_FIRE_G << (top - 40);
    lds.piece[w][lane] = x;
    lds.raw[w][lane] = (uint8_t)b;
}

__device__ inline uint64_t gsm_fire_syndrome(const GsmFireLds& lds, uint32_t w) {
    uint64_t x = GSM_FIRE_MASK;
#pragma unroll
    for (uint32_t i = 0; i < GSM_FIRE_IN; ++i) x ^= lds.piece[w][i];
    return x;
}

// every lane: the syndrome; where it is not zero, the lane's four shifts
__device__ inline void gsm_fire_search(const GsmFireArgs& a, GsmFireLds& lds, uint32_t block, uint32_t tid) {
    const uint32_t w = tid / GSM_WAVE, lane = tid % GSM_WAVE;
    const uint64_t f = (uint64_t)block * GSM_BLOCKS + w;
    if (f >= a.frames) return;
    uint64_t x = gsm_fire_syndrome(lds, w);
    if (x == 0 || a.max_burst == 0) return;
    for (uint32_t s = 0; s < lane; ++s) x = gsm_fire_over_d(x);
    for (uint32_t m = lane; m < 224u; m += GSM_WAVE) {
        if ((x & 1u) && (x >> a.max_burst) == 0) {
            const uint32_t degree = 63u - (uint32_t)__builtin_clzll(x);
            if (m + degree <= 223u) {
                lds.pattern[w] = x;
                lds.shift[w] = m;
            }
        }
        if (m + GSM_WAVE >= 224u) break;
        for (uint32_t s = 0; s < GSM_WAVE; ++s) x = gsm_fire_over_d(x);
    }
}

// lane l < 23: data byte l, flipped where the pattern says so; lane 23: the status
__device__ inline void gsm_fire_emit(const GsmFireArgs& a, const GsmFireLds& lds, uint32_t block, uint32_t tid) {
    const uint32_t w = tid / GSM_WAVE, lane = tid % GSM_WAVE;
    const uint64_t f = (uint64_t)block * GSM_BLOCKS + w;
    if (f >= a.frames || lane > GSM_FIRE_OUT) return;
    const uint32_t m = lds.shift[w];
    const bool found = m != 0xFFFFFFFFu;
    const uint64_t p = found ? lds.pattern[w] : 0;
    if (lane == GSM_FIRE_OUT) {
        const uint64_t syndrome = gsm_fire_syndrome(lds, w);
        const uint32_t degree = found ? 63u - (uint32_t)__builtin_clzll(p) : 0u;
        vit_hip_gsm_fire st;
        st.status = syndrome == 0 ? 0 : found ? (int32_t)degree + 1 : -1;
        st.first_bit = found ? 223u - (m + degree) : 0u;
        st.syndrome_lo = (uint32_t)syndrome;
        st.syndrome_hi = (uint32_t)(syndrome >> 32);
        a.status[f] = st;
        return;
    }
    uint32_t b = lds.raw[w][lane];
    if (found) {
#pragma unroll
        for (uint32_t c = 0; c < 8; ++c) {
            const uint32_t power = 223u - (8u * lane + c);             // bit t is the coefficient of D^(223 - t)
            if (power >= m && power - m < 40u && ((p >> (power - m)) & 1u)) b ^= 0x80u >> c;
        }
    }
    if (a.lsb_first) b = ((b & 0x01u) << 7) | ((b & 0x02u) << 5) | ((b & 0x04u) << 3) | ((b & 0x08u) << 1) | ((b & 0x10u) >> 1) | ((b & 0x20u) >> 3) |
                         ((b & 0x40u) >> 5) | ((b & 0x80u) >> 7);
    a.data[f * a.data_stride + lane] = (uint8_t)b;
}

__global__ void __launch_bounds__(GSM_THREADS) gsm_fire_kernel(GsmFireArgs a) {
    __shared__ GsmFireLds lds;
    gsm_fire_stage(a, lds, blockIdx.x, threadIdx.x);
    __syncthreads();
    gsm_fire_search(a, lds, blockIdx.x, threadIdx.x);
    __syncthreads();
    gsm_fire_emit(a, lds, blockIdx.x, threadIdx.x);
}

// ---- the TCH/FS frame --------------------------------------------------------------------------------------------------------------------------

struct GsmTchfsArgs {
    const uint8_t* bytes;            // frame f at f * bytes_stride: 24 bytes, the 185 decoded bits u
    const void* class2;              // soft_t [frames][78]
    uint8_t* speech;                 // frame f at f * speech_stride: 33 bytes
    vit_hip_gsm_tchfs* status;       // or null
    uint64_t bytes_stride, speech_stride;
    uint32_t frames;
    int32_t mid;                     // soft_decision_high + soft_decision_low
};

struct GsmTchfsLds {
    uint8_t raw[GSM_BLOCKS][GSM_TCHFS_IN];
    uint8_t hard[GSM_BLOCKS][GSM_CLASS2 + 2];                         // bit 0: the decision, bit 1: an erasure
};

template <class soft_t>
__device__ inline void gsm_tchfs_stage(const GsmTchfsArgs& a, GsmTchfsLds& lds, uint32_t block, uint32_t tid) {
    const uint32_t w = tid / GSM_WAVE, lane = tid % GSM_WAVE;
    const uint64_t f = (uint64_t)block * GSM_BLOCKS + w;
    if (f >= a.frames) return;
    if (lane < GSM_TCHFS_IN) lds.raw[w][lane] = a.bytes[f * a.bytes_stride + lane];
    for (uint32_t k = lane; k < GSM_CLASS2; k += GSM_WAVE) {
        const int32_t d = 2 * (int32_t)((const soft_t*)a.class2)[f * GSM_CLASS2 + k] - a.mid;
        lds.hard[w][k] = (uint8_t)((d > 0 ? 1u : 0u) | (d == 0 ? 2u : 0u));
    }
}

__device__ inline uint32_t gsm_u(const uint8_t* raw, uint32_t t) { return (raw[t >> 3] >> (7u - (t & 7u))) & 1u; }
// speech bit i < 182 of the decoded bits u
__device__ inline uint32_t gsm_class1(const uint8_t* raw, uint32_t i) { return gsm_u(raw, i & 1u ? 184u - (i >> 1) : i >> 1); }

__device__ inline void gsm_tchfs_emit(const GsmTchfsArgs& a, const GsmTchfsLds& lds, uint32_t block, uint32_t tid) {
    const uint32_t w = tid / GSM_WAVE, lane = tid % GSM_WAVE;
    const uint64_t f = (uint64_t)block * GSM_BLOCKS + w;
    if (f >= a.frames || lane > GSM_TCHFS_OUT) return;
    const uint8_t* raw = lds.raw[w];
    if (lane == GSM_TCHFS_OUT) {
        if (!a.status) return;
        uint32_t reg = 0, erased = 0;                                 // (d(0..49) D^3 + p) mod (D^3 + D + 1)
        for (uint32_t i = 0; i < 53u; ++i) {
            reg = (reg << 1) | (i < 50u ? gsm_class1(raw, i) : gsm_u(raw, 91u + (i - 50u)));
            if (reg & 8u) reg ^= 0xBu;
        }
        for (uint32_t k = 0; k < GSM_CLASS2; ++k) erased += lds.hard[w][k] >> 1;
        vit_hip_gsm_tchfs st;
        st.parity_syndrome = reg ^ 7u;
        st.class2_erasures = erased;
        a.status[f] = st;
        return;
    }
    uint32_t b = 0;
#pragma unroll
    for (uint32_t c = 0; c < 8; ++c) {
        const uint32_t i = 8u * lane + c;
        const uint32_t bit = i < 182u ? gsm_class1(raw, i) : i < 260u ? lds.hard[w][i - 182u] & 1u : 0u;
        b |= bit << (7u - c);
    }
    a.speech[f * a.speech_stride + lane] = (uint8_t)b;
}

template <class soft_t>
__global__ void __launch_bounds__(GSM_THREADS) gsm_tchfs_kernel(GsmTchfsArgs a) {
    __shared__ GsmTchfsLds lds;
    gsm_tchfs_stage<soft_t>(a, lds, blockIdx.x, threadIdx.x);
    __syncthreads();
    gsm_tchfs_emit(a, lds, blockIdx.x, threadIdx.x);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------

struct GsmSpan { const void* at; uint64_t bytes; };

// argument rules (include/vit_hip.h): everything the host can know without reading device memory.  R and sb are the handle's
inline const char* gsm_deinterleave_invalid(bool handle, int R, size_t sb, const void* d_in, size_t in_row_stride, size_t in_burst_stride, size_t rows,
                                            size_t bursts, unsigned mode, unsigned flags, const void* d_hist_in, const uint32_t* d_fill_in,
                                            const void* d_hist_out, const uint32_t* d_fill_out, const uint32_t* d_n_out, const void* d_full,
                                            const void* d_class1, const void* d_class2, const int32_t* d_steal) {
    if (!handle || !d_in) return "NULL handle or d_in";
    if (!d_full && !d_class1 && !d_class2 && !d_steal) return "d_full, d_class1, d_class2 and d_steal are all NULL";
    if (R != 2) return "the handle's code rate must be 1/2";
    if (mode > VIT_HIP_GSM_DIAGONAL) return "mode must be VIT_HIP_GSM_BLOCK or VIT_HIP_GSM_DIAGONAL";
    if (flags & ~(unsigned)VIT_HIP_GSM_NEGATE) return "flags other than VIT_HIP_GSM_NEGATE";
    if (mode == VIT_HIP_GSM_BLOCK && (d_hist_in || d_fill_in || d_hist_out || d_fill_out)) return "the block mode carries no history";
    if ((d_hist_in != nullptr) != (d_fill_in != nullptr)) return "d_hist_in and d_fill_in come together";
    if ((d_hist_out != nullptr) != (d_fill_out != nullptr)) return "d_hist_out and d_fill_out come together";
    if (bursts % 4 != 0) return "bursts must be a multiple of 4";
    if (misaligned(d_in, sb) || misaligned(d_hist_in, sb) || misaligned(d_hist_out, sb) || misaligned(d_full, sb) || misaligned(d_class1, sb) ||
        misaligned(d_class2, sb))
        return "the symbol buffers must be aligned to the symbol type";
    if (misaligned(d_fill_in, 4) || misaligned(d_fill_out, 4) || misaligned(d_n_out, 4) || misaligned(d_steal, 4))
        return "the count arrays and d_steal must be aligned to 4 bytes";
    if (in_burst_stride != 0 && in_burst_stride < GSM_BURST) return "in_burst_stride below 116";
    if (in_row_stride >= 0x7FFFFFFFull || in_burst_stride >= 0x7FFFFFFFull) return "the strides must lie below 2^31 - 1";
    if (rows >= 0x7FFFFFFFull || bursts >= 0x7FFFFFFFull || rows * (bursts / 4) >= 0x7FFFFFFFull) return "rows, bursts and rows * bursts / 4 must lie below 2^31 - 1";
    if (rows == 0 || bursts == 0) return nullptr;
    const uint64_t bs = in_burst_stride ? in_burst_stride : GSM_BURST, row = extent(bursts, bs, GSM_BURST);
    if (in_row_stride != 0 && in_row_stride < row) return "in_row_stride below a row's bursts";
    const uint64_t blocks = rows * (bursts / 4);
    const GsmSpan in[3] = {{d_in, extent(rows, in_row_stride ? in_row_stride : bursts * bs, row) * sb}, {d_hist_in, rows * GSM_HIST * sb}, {d_fill_in, rows * 4}};
    const GsmSpan out[7] = {{d_full, blocks * GSM_CODED * sb}, {d_class1, blocks * GSM_CLASS1 * sb}, {d_class2, blocks * GSM_CLASS2 * sb},
                            {d_steal, blocks * 4},             {d_hist_out, rows * GSM_HIST * sb},   {d_fill_out, rows * 4},
                            {d_n_out, rows * 4}};
    for (int o = 0; o < 7; ++o) {
        for (int i = 0; i < 3; ++i)
            if (overlap(out[o].at, out[o].bytes, in[i].at, in[i].bytes)) return "an output overlaps an input";
        for (int p = o + 1; p < 7; ++p)
            if (overlap(out[o].at, out[o].bytes, out[p].at, out[p].bytes)) return "two outputs overlap";
    }
    return nullptr;
}

// the kernel arguments of a call the argument rule has accepted, rows and bursts at least 1
inline GsmArgs gsm_args(size_t sb, const void* d_in, size_t in_row_stride, size_t in_burst_stride, size_t rows, size_t bursts, unsigned mode,
                        unsigned flags, const void* d_hist_in, const uint32_t* d_fill_in, void* d_hist_out, uint32_t* d_fill_out, uint32_t* d_n_out,
                        void* d_full, void* d_class1, void* d_class2, int32_t* d_steal) {
    GsmArgs a{};
    a.in = d_in; a.hist_in = d_hist_in; a.fill_in = d_fill_in; a.hist_out = d_hist_out; a.fill_out = d_fill_out; a.n_out = d_n_out;
    a.full = d_full; a.class1 = d_class1; a.class2 = d_class2; a.steal = d_steal;
    a.burst_stride = in_burst_stride ? in_burst_stride : GSM_BURST;
    a.row_stride = in_row_stride ? in_row_stride : bursts * a.burst_stride;
    a.rows = (uint32_t)rows; a.blocks = (uint32_t)(bursts / 4);
    a.diagonal = mode == VIT_HIP_GSM_DIAGONAL; a.negate = (flags & VIT_HIP_GSM_NEGATE) != 0;
    a.lo = sb == 2 ? -32768 : -128; a.hi = sb == 2 ? 32767 : 127;
    return a;
}

inline uint32_t gsm_grid(uint64_t items) { return (uint32_t)((items + GSM_BLOCKS - 1) / GSM_BLOCKS); }

inline const char* gsm_fire_invalid(bool handle, const uint8_t* d_bytes, size_t bytes_frame_stride, size_t frames, unsigned max_burst, unsigned flags,
                                    const vit_hip_gsm_fire* d_status, const uint8_t* d_data, size_t data_stride) {
    if (!handle || !d_bytes || !d_status || !d_data) return "NULL handle, d_bytes, d_status or d_data";
    if (max_burst > 12) return "max_burst must be 0 .. 12";
    if (flags & ~(unsigned)VIT_HIP_GSM_LSB_FIRST) return "flags other than VIT_HIP_GSM_LSB_FIRST";
    if (misaligned(d_status, 4)) return "d_status must be aligned to 4 bytes";
    if (bytes_frame_stride != 0 && bytes_frame_stride < GSM_FIRE_IN) return "bytes_frame_stride below 28";
    if (data_stride != 0 && data_stride < GSM_FIRE_OUT) return "data_stride below 23";
    if (bytes_frame_stride >= 0x7FFFFFFFull || data_stride >= 0x7FFFFFFFull) return "the strides must lie below 2^31 - 1";
    if (frames >= 0x7FFFFFFFull) return "frames must lie below 2^31 - 1";
    if (frames == 0) return nullptr;
    const uint64_t is = bytes_frame_stride ? bytes_frame_stride : GSM_FIRE_IN, os = data_stride ? data_stride : GSM_FIRE_OUT;
    const uint64_t in_b = extent(frames, is, GSM_FIRE_IN), out_b = extent(frames, os, GSM_FIRE_OUT), st_b = frames * sizeof(vit_hip_gsm_fire);
    if (overlap(d_status, st_b, d_bytes, in_b) || overlap(d_status, st_b, d_data, out_b)) return "d_status overlaps d_bytes or d_data";
    if (overlap(d_data, out_b, d_bytes, in_b) && !(d_data == d_bytes && is == os)) return "d_data overlaps d_bytes and is not in place: the same address and stride";
    return nullptr;
}

inline GsmFireArgs gsm_fire_args(const uint8_t* d_bytes, size_t bytes_frame_stride, size_t frames, unsigned max_burst, unsigned flags,
                                 vit_hip_gsm_fire* d_status, uint8_t* d_data, size_t data_stride) {
    GsmFireArgs a{};
    a.bytes = d_bytes; a.status = d_status; a.data = d_data;
    a.bytes_stride = bytes_frame_stride ? bytes_frame_stride : GSM_FIRE_IN;
    a.data_stride = data_stride ? data_stride : GSM_FIRE_OUT;
    a.frames = (uint32_t)frames; a.max_burst = max_burst; a.lsb_first = (flags & VIT_HIP_GSM_LSB_FIRST) != 0;
    return a;
}

// sb is the handle's
inline const char* gsm_tchfs_invalid(bool handle, size_t sb, const uint8_t* d_bytes, size_t bytes_frame_stride, const void* d_class2, size_t frames,
                                     const uint8_t* d_speech, size_t speech_stride, const vit_hip_gsm_tchfs* d_status) {
    if (!handle || !d_bytes || !d_class2 || !d_speech) return "NULL handle, d_bytes, d_class2 or d_speech";
    if (misaligned(d_class2, sb)) return "d_class2 must be aligned to the symbol type";
    if (misaligned(d_status, 4)) return "d_status must be aligned to 4 bytes";
    if (bytes_frame_stride != 0 && bytes_frame_stride < GSM_TCHFS_IN) return "bytes_frame_stride below 24";
    if (speech_stride != 0 && speech_stride < GSM_TCHFS_OUT) return "speech_stride below 33";
    if (bytes_frame_stride >= 0x7FFFFFFFull || speech_stride >= 0x7FFFFFFFull) return "the strides must lie below 2^31 - 1";
    if (frames >= 0x7FFFFFFFull) return "frames must lie below 2^31 - 1";
    if (frames == 0) return nullptr;
    const uint64_t in_b = extent(frames, bytes_frame_stride ? bytes_frame_stride : GSM_TCHFS_IN, GSM_TCHFS_IN), c2_b = frames * GSM_CLASS2 * sb;
    const uint64_t out_b = extent(frames, speech_stride ? speech_stride : GSM_TCHFS_OUT, GSM_TCHFS_OUT), st_b = frames * sizeof(vit_hip_gsm_tchfs);
    if (overlap(d_speech, out_b, d_bytes, in_b) || overlap(d_speech, out_b, d_class2, c2_b) || overlap(d_status, st_b, d_bytes, in_b) ||
        overlap(d_status, st_b, d_class2, c2_b))
        return "an output overlaps an input";
    if (overlap(d_speech, out_b, d_status, st_b)) return "d_speech overlaps d_status";
    return nullptr;
}

inline GsmTchfsArgs gsm_tchfs_args(int high, int low, const uint8_t* d_bytes, size_t bytes_frame_stride, const void* d_class2, size_t frames,
                                   uint8_t* d_speech, size_t speech_stride, vit_hip_gsm_tchfs* d_status) {
    GsmTchfsArgs a{};
    a.bytes = d_bytes; a.class2 = d_class2; a.speech = d_speech; a.status = d_status;
    a.bytes_stride = bytes_frame_stride ? bytes_frame_stride : GSM_TCHFS_IN;
    a.speech_stride = speech_stride ? speech_stride : GSM_TCHFS_OUT;
    a.frames = (uint32_t)frames; a.mid = high + low;
    return a;
}

// ---- launchers (hipGetLastError() after them: 0 / -1) -------------------------------------------------------------------------------

inline int gsm_launch_deinterleave(const GsmArgs& a, size_t soft_bytes, hipStream_t st) {
    if (soft_bytes == 2) hipLaunchKernelGGL(gsm_deinterleave_kernel<int16_t>, dim3(gsm_grid((uint64_t)a.rows * a.blocks)), dim3(GSM_THREADS), 0, st, a);
    else hipLaunchKernelGGL(gsm_deinterleave_kernel<int8_t>, dim3(gsm_grid((uint64_t)a.rows * a.blocks)), dim3(GSM_THREADS), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

inline int gsm_launch_fire(const GsmFireArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(gsm_fire_kernel, dim3(gsm_grid(a.frames)), dim3(GSM_THREADS), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

inline int gsm_launch_tchfs(const GsmTchfsArgs& a, size_t soft_bytes, hipStream_t st) {
    if (soft_bytes == 2) hipLaunchKernelGGL(gsm_tchfs_kernel<int16_t>, dim3(gsm_grid(a.frames)), dim3(GSM_THREADS), 0, st, a);
    else hipLaunchKernelGGL(gsm_tchfs_kernel<int8_t>, dim3(gsm_grid(a.frames)), dim3(GSM_THREADS), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace vit
