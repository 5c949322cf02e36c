// kernels_sync.hpp -- the side passes of node synchronisation (vit_hip_sync_build, vit_hip_sync_search), around the unchanged
// windowed decode (vit_hip_decode_streams) and channel symbol error count (vit_hip_channel_errors_batch):
//   1. sync_build_kernel   ONE received buffer -> the [T][R] stream of every alignment hypothesis (offset, pair swap, negation of the
//                          even / odd received symbols), depunctured on the way: the front end of the search, in one launch;
//   2. sync_state_kernel   per hypothesis the encoder state in front of emitted bit `skip`, read from the decoded bytes;
//   3. sync_pick_kernel    the hypothesis no other beats (errors / compared, exact in 64-bit integers; the lower index on a tie).
// 1 is memory-bound and makes one pass over its output; 2 and 3 are a handful of threads.  Not specialised on the polynomials: one
// instantiation per soft width.  Included only from vit_sync.hip (not from the register-plan units, whose kernel sources key the
// precompiled and run-time compiled caches).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vit_hip.h"

namespace vit {

constexpr uint32_t SYNC_MAX_HYPOTHESES = 64;   // they travel by value in the kernel arguments: no copy, nothing to keep alive
constexpr uint32_t SYNC_MAP_LDS = 1024;        // source maps up to this many entries are staged in LDS (4 KiB)

struct SyncBuildArgs {
    const void* received;         // [n_received] soft_t
    const int32_t* source_index;  // [period] or null: the identity (unpunctured, period = kept = R)
    void* out;                    // hypothesis h at out + h * out_stride (soft_t elements): [T][R]; steps behind T are not written
    uint64_t out_stride;          // pitch * R
    uint32_t n_elems;             // T * R
    uint32_t period, kept;        // symbols of one puncturing period: of the mother code, transmitted
    int32_t mid;                  // high + low: a negated symbol is mid - v, clamped to soft_t
    vit_hip_sync_hypothesis hyp[SYNC_MAX_HYPOTHESES];
};

// One thread per 16 bytes of one hypothesis's stream (blockIdx.y), 16-byte stores: a wavefront writes 1 KiB contiguous.  The
// position inside the puncturing period comes from ONE division per thread and then advances with a wrap.  The reads follow the
// output order (the kept symbols of a period are consecutive received symbols), so a wavefront reads one contiguous stretch of
// about kept / period KiB; a pair swap permutes it inside 4 bytes.  A row whose address is not a multiple of 16 (pitch * R *
// sizeof(soft_t) is not, or the caller's buffer) and the last, partial chunk go symbol by symbol.  Grid-strided in x.
template <typename soft_t>
__global__ void __launch_bounds__(256) sync_build_kernel(SyncBuildArgs a) {
    __shared__ int32_t lds_map[SYNC_MAP_LDS];
    constexpr uint32_t E = 16 / sizeof(soft_t);
    constexpr int32_t VMIN = sizeof(soft_t) == 2 ? -32768 : -128, VMAX = sizeof(soft_t) == 2 ? 32767 : 127;
    const bool staged = a.source_index && a.period <= SYNC_MAP_LDS;
    if (staged) {
        for (uint32_t i = threadIdx.x; i < a.period; i += blockDim.x) lds_map[i] = a.source_index[i];
        __syncthreads();
    }
    const vit_hip_sync_hypothesis hyp = a.hyp[blockIdx.y];
    const uint32_t swap = hyp.flags & VIT_HIP_SYNC_SWAP_PAIRS ? 1u : 0u;
    const soft_t* rec = (const soft_t*)a.received;
    soft_t* row = (soft_t*)a.out + (size_t)blockIdx.y * a.out_stride;
    const bool row_aligned = ((uintptr_t)row & 15u) == 0;
    const uint32_t chunks = (a.n_elems + E - 1) / E;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += gridDim.x * blockDim.x) {
        const uint32_t k0 = c * E;
        const uint32_t p = k0 / a.period;
        uint32_t pos = k0 - p * a.period;
        uint64_t base = (uint64_t)hyp.offset + (uint64_t)p * a.kept;      // received index of this period's first kept symbol
        soft_t v[E];
#pragma unroll
        for (uint32_t e = 0; e < E; ++e) {
            int32_t x = 0;
            if (k0 + e < a.n_elems) {
                const int32_t s = !a.source_index ? (int32_t)pos : staged ? lds_map[pos] : a.source_index[pos];
                // s >= kept is no index into a period's transmitted symbols: read as an erasure, never past what the host checked
                if (s >= 0 && (uint32_t)s < a.kept) {
                    const uint64_t j = base + (uint32_t)s;
                    x = rec[j ^ swap];
                    if (hyp.flags & (j & 1u ? VIT_HIP_SYNC_NEGATE_ODD : VIT_HIP_SYNC_NEGATE_EVEN)) {
                        x = a.mid - x;
                        x = x < VMIN ? VMIN : x > VMAX ? VMAX : x;
                    }
                }
            }
            v[e] = (soft_t)x;
            if (++pos == a.period) {
                pos = 0;
                base += a.kept;
            }
        }
        soft_t* dst = row + k0;
        if (row_aligned && k0 + E <= a.n_elems) {
            uint4 w;
            __builtin_memcpy(&w, v, 16);
            *(uint4*)dst = w;
        } else {
#pragma unroll
            for (uint32_t e = 0; e < E; ++e)
                if (k0 + e < a.n_elems) dst[e] = v[e];
        }
    }
}

struct SyncStateArgs {
    const uint8_t* bytes;    // hypothesis h's decoded bytes at bytes + h * byte_stride, MSB-first
    uint32_t* state;         // [n_hyp]
    uint32_t* errors;        // [n_hyp] the counters the count that follows adds into: zeroed here, in place of two memsets
    uint32_t* compared;      // [n_hyp]
    uint64_t byte_stride;
    uint32_t n_hyp, skip_bytes, K;
};

// bit j of the state = emitted bit skip - 1 - j: the last K-1 of the first `skip` bits, the newest in bit 0 (the decoder's numbering)
__global__ void __launch_bounds__(64) sync_state_kernel(SyncStateArgs a) {
    const uint32_t h = threadIdx.x;
    if (h >= a.n_hyp) return;
    const uint8_t* p = a.bytes + (size_t)h * a.byte_stride;
    uint32_t w = 0;
    for (uint32_t i = 0; i < a.skip_bytes; ++i) w = (w << 8) | p[i];
    a.state[h] = w & ((1u << (a.K - 1u)) - 1u);
    a.errors[h] = 0;
    a.compared[h] = 0;
}

struct SyncPickArgs {
    const uint32_t* errors;    // [n_hyp]
    const uint32_t* compared;  // [n_hyp]
    uint32_t* best;            // [1]
    uint32_t n_hyp;            // <= 64: one wavefront, one hypothesis per lane
};

// a beats b iff compared_a > 0 and (compared_b == 0 or errors_a * compared_b < errors_b * compared_a)
__device__ inline bool sync_beats(uint32_t ea, uint32_t ca, uint32_t eb, uint32_t cb) {
    return ca > 0 && (cb == 0 || (uint64_t)ea * cb < (uint64_t)eb * ca);
}

// every lane asks each other hypothesis whether it beats this one; the winner is the lowest lane nobody beats (the relation orders
// the rates, so such a lane exists)
__global__ void __launch_bounds__(64) sync_pick_kernel(SyncPickArgs a) {
    const uint32_t i = threadIdx.x;
    const bool live = i < a.n_hyp;
    const uint32_t e = live ? a.errors[i] : 0u, c = live ? a.compared[i] : 0u;
    bool beaten = !live;
    for (uint32_t j = 0; j < a.n_hyp; ++j) {
        const uint32_t ej = __shfl(e, (int)j), cj = __shfl(c, (int)j);
        beaten = beaten || sync_beats(ej, cj, e, c);
    }
    const uint64_t free_lanes = __ballot(!beaten);
    if (i == 0) a.best[0] = free_lanes ? (uint32_t)__builtin_ctzll(free_lanes) : 0u;
}

// ---- launchers (hipGetLastError() after each: 0 / -1) -----------------------------------------------------------------------

inline int sync_launch_build(int soft_bytes, const SyncBuildArgs& a, uint32_t n_hyp, hipStream_t st) {
    const uint64_t chunks = ((uint64_t)a.n_elems * (uint64_t)soft_bytes + 15) / 16;
    uint64_t blocks = (chunks + 255) / 256;
    const uint64_t cap = 8192 / n_hyp < 1 ? 1 : 8192 / n_hyp;           // memory-bound: grid-stride past 8192 blocks in all
    blocks = blocks < 1 ? 1 : blocks > cap ? cap : blocks;
    if (soft_bytes == 2) hipLaunchKernelGGL(sync_build_kernel<int16_t>, dim3((unsigned)blocks, n_hyp), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(sync_build_kernel<int8_t>, dim3((unsigned)blocks, n_hyp), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

inline int sync_launch_state(const SyncStateArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(sync_state_kernel, dim3(1), dim3(64), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

inline int sync_launch_pick(const SyncPickArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(sync_pick_kernel, dim3(1), dim3(64), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace vit
