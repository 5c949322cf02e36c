// kernels_enc.hpp -- the convolutional encoder on the caller's own bytes, and the re-encoded channel symbol error count.
//
// The encoder is the one synth_kernel (kernels_synth.hpp) runs on its Philox bytes -- shift-register form,
// include/viterbi/convolutional_encoder_shift_register.h:42-62 -- behind an entry point of its own, with what a receiver needs on
// top of the harness: a start state per frame, tail-biting frames, unterminated pieces of a stream, frame strides.
//   encode_kernel          info bits (MSB-first in bytes, as chainback() writes them) -> [steps][R] symbols at exactly high / low
//   channel_errors_kernel  the same bits re-encoded in registers against the received symbols: per frame, how many symbols were
//                          compared (2 r != high + low: a symbol at the midpoint is an erasure) and how many of those have a hard
//                          decision (2 r > high + low) that differs from the re-encoded bit.  No encoded buffer exists.
// State numbering is the decoder's (d_start_state of update, d_end_state of chainback): bit j of a state is the input bit j+1
// steps back, the register at step t is (state << 1 | bit_t) & (2^K - 1), symbol i of step t is parity(reg & G[i]).
//
// One thread makes 8 trellis steps (one info byte) of one frame, as in synth_kernel: 8*R contiguous symbols, 32 bytes at R = 2 /
// int16, moved as 16- or 8-byte vectors when the address allows (a frame stride can misalign a frame: then 4-byte words or single
// symbols).  24 bits of input history per thread (bytes b-2, b-1, b) serve K <= 16; before the frame they come from the start state.
// Counts: a thread packs (compared << 16 | errors) -- at most 8 chunks x 64 symbols per thread, 32768 per wave -- and the wave adds
// them up with __shfl before anything touches memory:
//   - a workgroup whose chunks all lie in one frame (long frames): every thread sums its chunks_per_thread chunks, the waves reduce
//     by __shfl_xor, the four wave sums meet in LDS and ONE lane adds them to the frame's counters (one frame of 2^26 steps: 4096
//     workgroups of 2048 chunks, not 131072 waves, meet on its counter);
//   - otherwise (short frames: a wave spans several): a segmented __shfl_down reduction over the runs of equal frame index, and the
//     first lane of every run adds its run's sum.
// Integer sums: the result does not depend on the order of the atomics.  The counters are zeroed by the call, on its stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vit {

struct EncArgs {
    const uint8_t* bytes;        // frame f at bytes + f * byte_stride: ceil(L/8) info bytes
    void* symbols;               // frame f at symbols + f * sym_stride (soft_t elements): [steps][R]; read by channel_errors_kernel
    const uint32_t* start;       // [frames] or null (=> 0); null under tail_biting
    uint32_t* end_state;         // [frames] or null (encode_kernel)
    uint32_t* errors;            // [frames]           (channel_errors_kernel)
    uint32_t* compared;          // [frames] or null   (channel_errors_kernel)
    uint64_t sym_stride, byte_stride, total_chunks;   // total_chunks = frames * nchunks
    uint32_t L, steps, nchunks;  // nchunks = ceil(steps / 8)
    uint32_t K, tail_biting;
    uint32_t chunks_per_thread;  // channel_errors_kernel: a workgroup covers 256 * this many consecutive chunks (1 .. 8)
    uint32_t G[8];               // masked to K bits
    int32_t high, low;
};

__device__ inline void enc_locate(const EncArgs& a, uint64_t gid, uint32_t& f, uint32_t& b) {
    if (a.total_chunks <= 0xFFFFFFFFull) {
        f = (uint32_t)gid / a.nchunks;
        b = (uint32_t)gid - f * a.nchunks;
    } else {
        f = (uint32_t)(gid / a.nchunks);
        b = (uint32_t)(gid - (uint64_t)f * a.nchunks);
    }
}

// input bits of steps 8b-16 .. 8b+7 of frame f, newest = bit 0: info bytes b-2, b-1, b; pad bits of the last byte and everything
// behind it read as 0 (the zero tail); before the frame, the start state (tail-biting: the frame's own last 16 bits)
__device__ inline uint32_t enc_history(const EncArgs& a, uint32_t f, uint32_t b) {
    const uint8_t* src = a.bytes + (size_t)f * a.byte_stride;
    const uint32_t nbytes = (a.L + 7u) / 8u, pad = 8u * nbytes - a.L;
    uint32_t word = 0;
#pragma unroll
    for (int d = 2; d >= 0; --d) {
        uint32_t v = 0;
        if (b >= (uint32_t)d && b - (uint32_t)d < nbytes) {
            const uint32_t i = b - (uint32_t)d;
            v = src[i];
            if (i == nbytes - 1u) v &= 0xFFu << pad;
        }
        word = (word << 8) | v;
    }
    if (b < 2u) {
        uint32_t before;                 // bit j = the input bit j+1 steps before step 0
        if (a.tail_biting) {
            uint32_t last = 0;
#pragma unroll
            for (int d = 2; d >= 0; --d) last = (last << 8) | (nbytes > (uint32_t)d ? (uint32_t)src[nbytes - 1u - (uint32_t)d] : 0u);
            before = last >> pad;
        } else {
            before = a.start ? a.start[f] : 0u;
        }
        before &= 0xFFFFu;
        word |= b == 0u ? before << 8 : (before & 0xFFu) << 16;
    }
    return word;
}

// 8*R symbols at p: 16-, 8- or 4-byte vectors by what the address allows; a partial chunk and an odd address go symbol by symbol
template <typename soft_t, int R>
__device__ inline void enc_load(const soft_t* p, uint32_t nsteps, soft_t (&val)[8 * R]) {
    constexpr int NV = 8 * R, BYTES = NV * (int)sizeof(soft_t);
    if (nsteps == 8u && ((uintptr_t)p & 3u) == 0) {
        uint32_t pk[BYTES / 4];
        if (BYTES % 16 == 0 && ((uintptr_t)p & 15u) == 0) {
#pragma unroll
            for (int w = 0; w < BYTES / 16; ++w) {
                const uint4 x = ((const uint4*)p)[w];
                pk[4 * w] = x.x; pk[4 * w + 1] = x.y; pk[4 * w + 2] = x.z; pk[4 * w + 3] = x.w;
            }
        } else if (((uintptr_t)p & 7u) == 0) {
#pragma unroll
            for (int w = 0; w < BYTES / 8; ++w) {
                const uint2 x = ((const uint2*)p)[w];
                pk[2 * w] = x.x; pk[2 * w + 1] = x.y;
            }
        } else {
#pragma unroll
            for (int w = 0; w < BYTES / 4; ++w) pk[w] = ((const uint32_t*)p)[w];
        }
        __builtin_memcpy(val, pk, BYTES);
    } else {
#pragma unroll
        for (int k = 0; k < NV; ++k) val[k] = (uint32_t)(k / R) < nsteps ? p[k] : (soft_t)0;
    }
}

template <typename soft_t, int R>
__device__ inline void enc_store(soft_t* p, uint32_t nsteps, const soft_t (&val)[8 * R]) {
    constexpr int NV = 8 * R, BYTES = NV * (int)sizeof(soft_t);
    if (nsteps == 8u && ((uintptr_t)p & 3u) == 0) {
        uint32_t pk[BYTES / 4];
        __builtin_memcpy(pk, val, BYTES);
        if (BYTES % 16 == 0 && ((uintptr_t)p & 15u) == 0) {
#pragma unroll
            for (int w = 0; w < BYTES / 16; ++w) ((uint4*)p)[w] = make_uint4(pk[4 * w], pk[4 * w + 1], pk[4 * w + 2], pk[4 * w + 3]);
        } else if (((uintptr_t)p & 7u) == 0) {
#pragma unroll
            for (int w = 0; w < BYTES / 8; ++w) ((uint2*)p)[w] = make_uint2(pk[2 * w], pk[2 * w + 1]);
        } else {
#pragma unroll
            for (int w = 0; w < BYTES / 4; ++w) ((uint32_t*)p)[w] = pk[w];
        }
    } else {
#pragma unroll
        for (int k = 0; k < NV; ++k)
            if ((uint32_t)(k / R) < nsteps) p[k] = val[k];
    }
}

template <typename soft_t, int R>
__global__ void __launch_bounds__(256) encode_kernel(EncArgs a) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= a.total_chunks) return;
    uint32_t f, b;
    enc_locate(a, gid, f, b);
    const uint32_t word = enc_history(a, f, b);
    const uint32_t t0 = 8u * b;
    const uint32_t nsteps = a.steps - t0 < 8u ? a.steps - t0 : 8u;
    constexpr int NV = 8 * R;
    soft_t val[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const uint32_t reg = word >> (7u - (uint32_t)(k / R));       // bit j = input bit of step t - j; G holds K bits
        val[k] = (soft_t)((__builtin_popcount(reg & a.G[k % R]) & 1) ? a.high : a.low);
    }
    enc_store<soft_t, R>((soft_t*)a.symbols + (size_t)f * a.sym_stride + (size_t)t0 * R, nsteps, val);
    // the state after the frame's last step: its K-1 newest input bits
    if (a.end_state && b == a.nchunks - 1u) a.end_state[f] = (word >> (8u - nsteps)) & ((1u << (a.K - 1u)) - 1u);
}

// compared << 16 | errors of chunk b of frame f
template <typename soft_t, int R>
__device__ inline uint32_t channel_errors_chunk(const EncArgs& a, uint32_t f, uint32_t b) {
    const uint32_t word = enc_history(a, f, b);
    const uint32_t t0 = 8u * b;
    const uint32_t nsteps = a.steps - t0 < 8u ? a.steps - t0 : 8u;
    constexpr int NV = 8 * R;
    soft_t val[NV];
    enc_load<soft_t, R>((const soft_t*)a.symbols + (size_t)f * a.sym_stride + (size_t)t0 * R, nsteps, val);
    const int32_t mid = a.high + a.low;
    uint32_t err = 0, cmp = 0;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const uint32_t reg = word >> (7u - (uint32_t)(k / R));
        const int32_t d = 2 * (int32_t)val[k] - mid;
        const uint32_t live = (d != 0 && (uint32_t)(k / R) < nsteps) ? 1u : 0u;
        const uint32_t hard = d > 0 ? 1u : 0u;
        cmp += live;
        err += ((uint32_t)__builtin_popcount(reg & a.G[k % R]) + hard) & live;    // odd sum: hard decision != re-encoded bit
    }
    return (cmp << 16) | err;
}

template <typename soft_t, int R>
__global__ void __launch_bounds__(256) channel_errors_kernel(EncArgs a) {
    __shared__ uint32_t wave_sum[4];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t tile = 256ull * a.chunks_per_thread;
    const uint64_t first = (uint64_t)blockIdx.x * tile;
    const uint64_t last = first + tile - 1 < a.total_chunks ? first + tile - 1 : a.total_chunks - 1;
    uint32_t f0, b0, f1, b1;
    enc_locate(a, first, f0, b0);
    enc_locate(a, last, f1, b1);
    if (f0 == f1) {
        // the whole workgroup works on one frame: registers -> wave -> LDS -> one pair of atomics
        uint32_t v = 0;
        for (uint32_t u = 0; u < a.chunks_per_thread; ++u) {
            const uint64_t gid = first + 256ull * u + threadIdx.x;
            if (gid <= last) v += channel_errors_chunk<soft_t, R>(a, f0, b0 + 256u * u + threadIdx.x);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) wave_sum[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t err = 0, cmp = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) { err += wave_sum[w] & 0xFFFFu; cmp += wave_sum[w] >> 16; }
            if (err) atomicAdd(a.errors + f0, err);
            if (cmp && a.compared) atomicAdd(a.compared + f0, cmp);
        }
        return;
    }
    for (uint32_t u = 0; u < a.chunks_per_thread; ++u) {
        const uint64_t gid = first + 256ull * u + threadIdx.x;
        uint32_t f = 0xFFFFFFFFu, b = 0, v = 0;            // lanes past the end: a run of their own that adds nothing
        if (gid <= last) {
            enc_locate(a, gid, f, b);
            v = channel_errors_chunk<soft_t, R>(a, f, b);
        }
        // frames are runs of consecutive lanes: after the step of distance `off`, a lane holds the sum of the next 2*off lanes of its run
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t vo = __shfl_down(v, off), fo = __shfl_down(f, off);
            if (lane + (uint32_t)off < 64u && fo == f) v += vo;
        }
        const uint32_t fp = __shfl_up(f, 1);
        if (f != 0xFFFFFFFFu && (lane == 0 || fp != f)) {
            if (v & 0xFFFFu) atomicAdd(a.errors + f, v & 0xFFFFu);
            if ((v >> 16) && a.compared) atomicAdd(a.compared + f, v >> 16);
        }
    }
}

}  // namespace vit
