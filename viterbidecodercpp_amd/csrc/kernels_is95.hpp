// kernels_is95.hpp -- the IS-95A forward traffic channel, rate set 1, around the K = 9, R = 1/2 decode: vit_hip_is95_deinterleave_batch (long-code
// descrambling, the 384-symbol block de-interleaver and the combining of the symbol repetitions under the four rate hypotheses, in one launch)
// and vit_hip_is95_rate_decide_batch (the blind rate decision over the four decodes and the compaction of the winner's info bits).
//   is95_deinterleave_kernel<soft_t>   One wavefront per frame, IS95_FRAMES frames per workgroup.  Lane l < 48 owns the received symbols
//                       8 l .. 8 l + 7 -- one load of 8 elements (16 bytes at soft16) and mask byte l -- negates where the mask says so and
//                       SCATTERS them into the frame's 384 int32 of LDS at their place in the repeated stream, A(i) = 64 (i mod 6) +
//                       BRO6(i div 6), BRO6 a 32-bit reversal and a shift.  int32 because -(-32768) must add as 32768.  Scatter on write,
//                       not gather on read: a ds_write_b32 takes the bank of dword A(i) mod 32 = BRO6(i div 6) mod 32, and over the 32
//                       lanes of a group i div 6 runs through 43 consecutive values, so a bank is hit at most twice -- 32 LDS cycles a
//                       frame for the 8 stores where 16 is conflict-free (no row pitch between 64 and 96 does better); the gather would
//                       read 6 BRO6(a mod 64) + a div 64 for consecutive a, four to a bank, 48 cycles for hypothesis 0 alone, and the
//                       other three hypotheses would gather again.
//                       Behind the barrier lane l reads ITS eight consecutive stream positions 8 l .. 8 l + 7 (two 16-byte LDS reads)
//                       and holds everything the four hypotheses need of them: the 8 values are 8 outputs of hypothesis 0, their 4 pair
//                       sums 4 outputs of hypothesis 1, 2 quad sums, 1 sum of eight.  Each is rounded, clamped and stored as one
//                       contiguous piece of 8 >> h elements: the 48 lanes of a wave write the frame's 384 >> h elements of out[h] as one
//                       contiguous run.  No lane idles in one hypothesis and works in another, nothing is read twice.
//   is95_zero_kernel    One thread per frame zeroes the up to eight counters of vit_hip_is95_channel_errors_batch: that call holds no memset,
//                       because memset nodes of a replayed graph have been seen not to write zeros (HISTORY, the marker search).
//   is95_decide_kernel  One thread per frame: the rule of include/vit_hip.h over at most four (errors, compared, syndrome) triples in
//                       64-bit cross-multiplication, then 22 info bytes from the winner's decoded bytes, zero behind its info bits.
// Everything is plain C++ in device functions that take (block, thread): the source also runs on the host (tests/cpp/is95_host_check.cpp),
// the argument rules included.  Included only from vit_is95.hip.
// Out of scope: rate set 2 (14400 and its puncturing), the long-code generator (the caller supplies the decimated bits), power-control
// bit extraction, sync and paging channels (continuous encoding: vit_hip_decode_stream), the reverse link, cdma2000 radio configurations 3
// and up, any rate-decision policy beyond the stated rule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vit_hip.h"
#include "arg_rules.hpp"

namespace vit {

constexpr uint32_t IS95_BLOCK = 256, IS95_WAVE = 64;
constexpr uint32_t IS95_FRAMES = IS95_BLOCK / IS95_WAVE;           // frames of a workgroup: one wavefront each
constexpr uint32_t IS95_SYMBOLS = 384, IS95_MASK_BYTES = 48;
constexpr uint32_t IS95_LANES = IS95_SYMBOLS / 8;                  // lanes of a wavefront that work: 8 symbols each
constexpr uint32_t IS95_INFO_BYTES = 22;
// hypothesis h: trellis steps S_h = L_h + 8, info bits, decoded bytes ceil(L_h / 8)
__host__ __device__ constexpr uint32_t is95_steps(uint32_t h) { return 192u >> h; }
__host__ __device__ constexpr uint32_t is95_info_bits(uint32_t h) { return h == 0 ? 172u : h == 1 ? 80u : h == 2 ? 40u : 16u; }
__host__ __device__ constexpr uint32_t is95_bytes(uint32_t h) { return h == 0 ? 23u : h == 1 ? 11u : h == 2 ? 5u : 2u; }

__host__ __device__ inline uint32_t is95_bro6(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bitreverse32(x) >> 26;
#else
    return ((x & 1u) << 5) | ((x & 2u) << 3) | ((x & 4u) << 1) | ((x & 8u) >> 1) | ((x & 16u) >> 3) | ((x & 32u) >> 5);
#endif
}
// received symbol i is symbol A(i) of the repeated stream
__host__ __device__ inline uint32_t is95_place(uint32_t i) {
    const uint32_t c = i / 6u;
    return 64u * (i - 6u * c) + is95_bro6(c);
}

// ---- de-interleave and combine ------------------------------------------------------------------------------------------------------------

struct Is95Args {
    const void* in;                  // soft_t, frame f at f * in_stride: 384 elements
    const uint8_t* scramble;         // 48 bytes a frame at f * scramble_stride, MSB-first, or null
    void* out[4];                    // soft_t [frames][S_h][2], or null
    uint64_t in_stride, scramble_stride;       // elements; bytes (0: one mask for the batch)
    uint32_t frames, shift;
    int32_t lo, hi;
};

// lane `tid % 64` of wavefront `tid / 64`: its 8 received symbols into the frame's LDS
template <class soft_t>
__device__ inline void is95_stage(const Is95Args& a, int32_t* lds, uint32_t block, uint32_t tid) {
    const uint32_t w = tid / IS95_WAVE, lane = tid % IS95_WAVE, f = block * IS95_FRAMES + w;
    if (f >= a.frames || lane >= IS95_LANES) return;
    struct Piece { soft_t v[8]; } x;
    const soft_t* in = (const soft_t*)a.in + (uint64_t)f * a.in_stride + 8u * lane;
    __builtin_memcpy(&x, __builtin_assume_aligned(in, sizeof(soft_t)), sizeof(x));
    const uint32_t bits = a.scramble ? a.scramble[(uint64_t)f * a.scramble_stride + lane] : 0u;
    int32_t* frame = lds + w * IS95_SYMBOLS;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        const int32_t v = (int32_t)x.v[j];
        frame[is95_place(8u * lane + j)] = ((bits >> (7u - j)) & 1u) ? -v : v;
    }
}

__device__ inline int32_t is95_round(const Is95Args& a, int32_t sum) {
    int32_t v = (sum + (int32_t)((1u << a.shift) >> 1)) >> a.shift;
    v = v < a.lo ? a.lo : v;
    return v > a.hi ? a.hi : v;
}

// the 8 >> H outputs of hypothesis H a lane holds in v[0 .. 8 >> H), as one contiguous piece
template <class soft_t, uint32_t H>
__device__ inline void is95_store(const Is95Args& a, const int32_t* v, uint32_t f, uint32_t lane) {
    constexpr uint32_t N = 8u >> H, BYTES = N * sizeof(soft_t), ALIGN = BYTES < 4u ? BYTES : 4u;
    if (!a.out[H]) return;
    struct Piece { soft_t v[N]; } x;
#pragma unroll
    for (uint32_t k = 0; k < N; ++k) x.v[k] = (soft_t)is95_round(a, v[k]);
    soft_t* out = (soft_t*)a.out[H] + (uint64_t)f * (2u * is95_steps(H)) + N * lane;
    __builtin_memcpy(__builtin_assume_aligned(out, ALIGN), &x, sizeof(x));
}

// the same lane behind the barrier: stream positions 8 lane .. 8 lane + 7 under the four hypotheses
template <class soft_t>
__device__ inline void is95_emit(const Is95Args& a, const int32_t* lds, uint32_t block, uint32_t tid) {
    const uint32_t w = tid / IS95_WAVE, lane = tid % IS95_WAVE, f = block * IS95_FRAMES + w;
    if (f >= a.frames || lane >= IS95_LANES) return;
    const int32_t* s = lds + w * IS95_SYMBOLS + 8u * lane;
    int32_t v[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) v[j] = s[j];
    is95_store<soft_t, 0>(a, v, f, lane);
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) v[k] = v[2 * k] + v[2 * k + 1];
    is95_store<soft_t, 1>(a, v, f, lane);
    v[0] += v[1]; v[1] = v[2] + v[3];
    is95_store<soft_t, 2>(a, v, f, lane);
    v[0] += v[1];
    is95_store<soft_t, 3>(a, v, f, lane);
}

template <class soft_t>
__global__ void __launch_bounds__(IS95_BLOCK) is95_deinterleave_kernel(Is95Args a) {
    __shared__ int32_t lds[IS95_FRAMES * IS95_SYMBOLS];
    is95_stage<soft_t>(a, lds, blockIdx.x, threadIdx.x);
    __syncthreads();
    is95_emit<soft_t>(a, lds, blockIdx.x, threadIdx.x);
}

// ---- the rate decision ----------------------------------------------------------------------------------------------------------------------

struct Is95DecideArgs {
    const uint8_t* bytes[4];         // decoded bytes of hypothesis h, frame f at f * bytes_stride[h]; null: absent
    const uint32_t* errors[4];
    const uint32_t* compared[4];
    const uint32_t* syndrome[2];
    uint64_t bytes_stride[4], info_stride;
    uint32_t max_num[4], den;
    uint32_t frames;
    vit_hip_is95_decision* decision;
    uint8_t* info;
};

__device__ inline void is95_decide(const Is95DecideArgs& a, uint32_t block, uint32_t tid) {
    const uint64_t f = (uint64_t)block * IS95_BLOCK + tid;
    if (f >= a.frames) return;
    uint32_t best = 4, be = 0, bc = 0;
#pragma unroll
    for (uint32_t h = 0; h < 4; ++h) {
        if (!a.bytes[h]) continue;
        if (h < 2 && a.syndrome[h][f] != 0u) continue;
        const uint32_t e = a.errors[h][f], c = a.compared[h][f];
        if (c == 0u || (uint64_t)e * a.den > (uint64_t)c * a.max_num[h]) continue;
        if (best == 4u || (uint64_t)e * bc < (uint64_t)be * c) { best = h; be = e; bc = c; }
    }
    const uint32_t bits = best < 4u ? is95_info_bits(best) : 0u;
    vit_hip_is95_decision d;
    d.rate = best; d.info_bits = bits; d.errors = be; d.compared = bc;
    a.decision[f] = d;
    const uint8_t* src = best < 4u ? a.bytes[best] + f * a.bytes_stride[best] : nullptr;
    uint8_t* info = a.info + f * a.info_stride;
    for (uint32_t b = 0; b < IS95_INFO_BYTES; ++b) {
        uint32_t x = 0;
        if (8u * b < bits) {
            x = src[b];
            if (bits - 8u * b < 8u) x &= 0xFF00u >> (bits - 8u * b);
        }
        info[b] = (uint8_t)x;
    }
}

__global__ void __launch_bounds__(IS95_BLOCK) is95_decide_kernel(Is95DecideArgs a) {
    is95_decide(a, blockIdx.x, threadIdx.x);
}

// ---- zeroing the counters of the four error counts --------------------------------------------------------------------------------------

struct Is95ZeroArgs {
    uint32_t* counters[8];           // [frames] each, or null
    uint32_t frames;
};

__device__ inline void is95_zero(const Is95ZeroArgs& a, uint32_t block, uint32_t tid) {
    const uint64_t f = (uint64_t)block * IS95_BLOCK + tid;
    if (f >= a.frames) return;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k)
        if (a.counters[k]) a.counters[k][f] = 0u;
}

__global__ void __launch_bounds__(IS95_BLOCK) is95_zero_kernel(Is95ZeroArgs a) {
    is95_zero(a, blockIdx.x, threadIdx.x);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------

// argument rules (include/vit_hip.h): everything the host can know without reading device memory.  R and sb are the handle's
inline const char* is95_deinterleave_invalid(bool handle, int R, size_t sb, const void* d_in, size_t in_frame_stride, size_t frames,
                                             const uint8_t* d_scramble, size_t scramble_frame_stride, unsigned shift, int lo, int hi,
                                             void* const* d_out) {
    if (!handle || !d_in || !d_out) return "NULL handle, d_in or d_out";
    if (!d_out[0] && !d_out[1] && !d_out[2] && !d_out[3]) return "all four outputs are NULL";
    if (R != 2) return "the handle's code rate must be 1/2";
    if (shift > 15) return "shift must be 0 .. 15";
    const int top = sb == 2 ? 32767 : 127;
    if (lo > hi || lo < -top - 1 || hi > top) return "clamp_lo .. clamp_hi must be a range of the symbol type";
    if (misaligned(d_in, sb)) return "d_in must be aligned to the symbol type";
    for (int h = 0; h < 4; ++h)
        if (misaligned(d_out[h], 4)) return "every output must be aligned to 4 bytes";
    if (in_frame_stride != 0 && in_frame_stride < IS95_SYMBOLS) return "in_frame_stride below 384";
    if (d_scramble && scramble_frame_stride != 0 && scramble_frame_stride < IS95_MASK_BYTES) return "scramble_frame_stride below 48";
    if (in_frame_stride >= 0x7FFFFFFFull || scramble_frame_stride >= 0x7FFFFFFFull) return "the strides must lie below 2^31 - 1";
    if (frames >= 0x7FFFFFFFull) return "frames must lie below 2^31 - 1";
    if (frames == 0) return nullptr;
    const uint64_t is = in_frame_stride ? in_frame_stride : IS95_SYMBOLS;
    const uint64_t in_b = extent(frames, is, IS95_SYMBOLS) * sb, mask_b = extent(frames, scramble_frame_stride, IS95_MASK_BYTES);
    for (int h = 0; h < 4; ++h) {
        const uint64_t out_b = frames * 2 * is95_steps(h) * sb;
        if (overlap(d_out[h], out_b, d_in, in_b)) return "an output overlaps d_in";
        if (overlap(d_out[h], out_b, d_scramble, mask_b)) return "an output overlaps d_scramble";
        for (int g = h + 1; g < 4; ++g)
            if (overlap(d_out[h], out_b, d_out[g], frames * 2 * is95_steps(g) * sb)) return "two outputs overlap";
    }
    return nullptr;
}

// the kernel arguments of a call the argument rule has accepted, frames at least 1
inline Is95Args is95_args(const void* d_in, size_t in_frame_stride, size_t frames, const uint8_t* d_scramble, size_t scramble_frame_stride,
                          unsigned shift, int lo, int hi, void* const* d_out) {
    Is95Args a{};
    a.in = d_in; a.scramble = d_scramble;
    for (int h = 0; h < 4; ++h) a.out[h] = d_out[h];
    a.in_stride = in_frame_stride ? in_frame_stride : IS95_SYMBOLS;
    a.scramble_stride = scramble_frame_stride;
    a.frames = (uint32_t)frames; a.shift = shift; a.lo = lo; a.hi = hi;
    return a;
}

inline uint32_t is95_blocks(const Is95Args& a) { return (a.frames + IS95_FRAMES - 1) / IS95_FRAMES; }

inline const char* is95_decide_invalid(bool handle, const uint8_t* const* d_bytes, const size_t* bytes_stride, const uint32_t* const* d_errors,
                                       const uint32_t* const* d_compared, const uint32_t* const* d_syndrome, size_t frames,
                                       const uint32_t* max_ser_num, uint32_t ser_den, const vit_hip_is95_decision* d_decision,
                                       const uint8_t* d_info, size_t info_stride) {
    if (!handle || !d_bytes || !d_errors || !d_compared || !d_syndrome || !max_ser_num || !d_decision || !d_info)
        return "NULL handle, array of pointers, max_ser_num, d_decision or d_info";
    if (!d_bytes[0] && !d_bytes[1] && !d_bytes[2] && !d_bytes[3]) return "all four hypotheses are absent";
    if (ser_den == 0) return "ser_den must be at least 1";
    if (info_stride != 0 && info_stride < IS95_INFO_BYTES) return "info_stride below 22";
    if (info_stride >= 0x7FFFFFFFull) return "the strides must lie below 2^31 - 1";
    if (misaligned(d_decision, 4)) return "d_decision must be aligned to 4 bytes";
    for (int h = 0; h < 4; ++h) {
        if (!d_bytes[h]) continue;
        if (!d_errors[h] || !d_compared[h] || (h < 2 && !d_syndrome[h])) return "a present hypothesis needs d_errors, d_compared and, at h < 2, d_syndrome";
        if (misaligned(d_errors[h], 4) || misaligned(d_compared[h], 4) || (h < 2 && misaligned(d_syndrome[h], 4)))
            return "the count arrays must be aligned to 4 bytes";
        if (bytes_stride && bytes_stride[h] != 0 && bytes_stride[h] < is95_bytes(h)) return "a bytes stride below 23, 11, 5 or 2";
        if (bytes_stride && bytes_stride[h] >= 0x7FFFFFFFull) return "the strides must lie below 2^31 - 1";
    }
    if (frames >= 0x7FFFFFFFull) return "frames must lie below 2^31 - 1";
    if (frames == 0) return nullptr;
    const uint64_t dec_b = frames * sizeof(vit_hip_is95_decision);
    const uint64_t info_b = extent(frames, info_stride ? info_stride : IS95_INFO_BYTES, IS95_INFO_BYTES), cnt_b = frames * 4;
    if (overlap(d_decision, dec_b, d_info, info_b)) return "d_decision overlaps d_info";
    for (int h = 0; h < 4; ++h) {
        if (!d_bytes[h]) continue;
        const uint64_t bs = bytes_stride && bytes_stride[h] ? bytes_stride[h] : is95_bytes(h), in_b = extent(frames, bs, is95_bytes(h));
        const void* outs[2] = {d_decision, d_info};
        const uint64_t out_b[2] = {dec_b, info_b};
        for (int o = 0; o < 2; ++o)
            if (overlap(outs[o], out_b[o], d_bytes[h], in_b) || overlap(outs[o], out_b[o], d_errors[h], cnt_b) ||
                overlap(outs[o], out_b[o], d_compared[h], cnt_b) || (h < 2 && overlap(outs[o], out_b[o], d_syndrome[h], cnt_b)))
                return "an output overlaps an input";
    }
    return nullptr;
}

inline Is95DecideArgs is95_decide_args(const uint8_t* const* d_bytes, const size_t* bytes_stride, const uint32_t* const* d_errors,
                                       const uint32_t* const* d_compared, const uint32_t* const* d_syndrome, size_t frames,
                                       const uint32_t* max_ser_num, uint32_t ser_den, vit_hip_is95_decision* d_decision, uint8_t* d_info,
                                       size_t info_stride) {
    Is95DecideArgs a{};
    for (int h = 0; h < 4; ++h) {
        a.bytes[h] = d_bytes[h];
        a.errors[h] = d_bytes[h] ? d_errors[h] : nullptr;
        a.compared[h] = d_bytes[h] ? d_compared[h] : nullptr;
        if (h < 2) a.syndrome[h] = d_bytes[h] ? d_syndrome[h] : nullptr;
        a.bytes_stride[h] = bytes_stride && bytes_stride[h] ? bytes_stride[h] : is95_bytes(h);
        a.max_num[h] = max_ser_num[h];
    }
    a.den = ser_den; a.frames = (uint32_t)frames; a.decision = d_decision; a.info = d_info;
    a.info_stride = info_stride ? info_stride : IS95_INFO_BYTES;
    return a;
}

// K, R and sb are the handle's
inline const char* is95_errors_invalid(bool handle, int K, int R, size_t sb, const void* const* d_symbols, const uint8_t* const* d_bytes,
                                       const size_t* bytes_stride, size_t frames, uint32_t* const* d_errors, uint32_t* const* d_compared) {
    if (!handle || !d_symbols || !d_bytes || !d_errors || !d_compared) return "NULL handle or array of pointers";
    if (K != 9 || R != 2) return "the handle must be a K = 9, R = 1/2 code";
    if (!d_bytes[0] && !d_bytes[1] && !d_bytes[2] && !d_bytes[3]) return "all four hypotheses are absent";
    for (int h = 0; h < 4; ++h) {
        if (!d_bytes[h]) continue;
        if (!d_symbols[h] || !d_errors[h] || !d_compared[h]) return "a present hypothesis needs d_symbols, d_errors and d_compared";
        if (misaligned(d_symbols[h], sb) || misaligned(d_errors[h], 4) || misaligned(d_compared[h], 4))
            return "d_symbols must be aligned to the symbol type, the count arrays to 4 bytes";
        if (bytes_stride && bytes_stride[h] != 0 && bytes_stride[h] < is95_bytes(h)) return "a bytes stride below 23, 11, 5 or 2";
        if (bytes_stride && bytes_stride[h] >= 0x7FFFFFFFull) return "the strides must lie below 2^31 - 1";
    }
    if (frames >= 0x7FFFFFFFull) return "frames must lie below 2^31 - 1";
    if (frames == 0) return nullptr;
    const uint64_t cnt_b = frames * 4;
    for (int h = 0; h < 4; ++h) {
        if (!d_bytes[h]) continue;
        const void* outs[2] = {d_errors[h], d_compared[h]};
        if (overlap(outs[0], cnt_b, outs[1], cnt_b)) return "two count arrays overlap";
        for (int g = 0; g < 4; ++g) {
            if (!d_bytes[g]) continue;
            const uint64_t gs = bytes_stride && bytes_stride[g] ? bytes_stride[g] : is95_bytes(g);
            for (int o = 0; o < 2; ++o) {
                if (g != h && (overlap(outs[o], cnt_b, d_errors[g], cnt_b) || overlap(outs[o], cnt_b, d_compared[g], cnt_b)))
                    return "two count arrays overlap";
                if (overlap(outs[o], cnt_b, d_bytes[g], extent(frames, gs, is95_bytes(g))) ||
                    overlap(outs[o], cnt_b, d_symbols[g], frames * 2 * is95_steps(g) * sb))
                    return "a count array overlaps an input";
            }
        }
    }
    return nullptr;
}

inline uint32_t is95_decide_blocks(const Is95DecideArgs& a) { return (a.frames + IS95_BLOCK - 1) / IS95_BLOCK; }

// ---- launchers (hipGetLastError() after them: 0 / -1) -------------------------------------------------------------------------------

inline int is95_launch_deinterleave(const Is95Args& a, size_t soft_bytes, hipStream_t st) {
    if (soft_bytes == 2) hipLaunchKernelGGL(is95_deinterleave_kernel<int16_t>, dim3(is95_blocks(a)), dim3(IS95_BLOCK), 0, st, a);
    else hipLaunchKernelGGL(is95_deinterleave_kernel<int8_t>, dim3(is95_blocks(a)), dim3(IS95_BLOCK), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

inline int is95_launch_zero(const Is95ZeroArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(is95_zero_kernel, dim3((a.frames + IS95_BLOCK - 1) / IS95_BLOCK), dim3(IS95_BLOCK), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

inline int is95_launch_decide(const Is95DecideArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(is95_decide_kernel, dim3(is95_decide_blocks(a)), dim3(IS95_BLOCK), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace vit
