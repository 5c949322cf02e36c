// kernels_marker.hpp -- frame synchronisation (vit_hip_marker_search): the Hamming distance of a sync marker of up to 64 bits to every
// bit position of bit-packed, MSB-first rows, summed per phase of the frame period, and the (phase, polarity) no other beats:
//   1. marker_search_kernel  a workgroup owns one row and a contiguous span of positions, tile by tile: the tile's bytes into LDS once
//                            (16-byte loads, bytes at the row's ragged ends, 8 bytes of look-ahead, the history word in front of bit
//                            0), big-endian 64-bit windows by funnel shift, popcount of the xor with the left-aligned marker, the
//                            distances through LDS so that consecutive lanes hold consecutive phases, per-phase sums in registers
//                            (P <= the workgroup) or an LDS table (P <= MARKER_TABLE_MAX), then 32-bit atomics of the partial sums;
//   0. marker_zero_kernel    the totals of a call that overwrites them;
//   2. marker_pick_kernel    one workgroup per row over the 2 P candidates (phase, upright / inverted), the 64-bit rule of
//                            sync_beats, the lower candidate on a tie.
// 1 reads its input once; the per-phase counts are a closed form of the shape, added by the same launch.  Every loop strides by
// blockDim.x and the workgroup meets only at __syncthreads(), so the source also runs one thread per block (the host build that
// checks its reads).  Included only from vit_marker.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vit_hip.h"

namespace vit {

constexpr uint32_t MARKER_TILE = 1024;                           // row bytes of one tile: 8192 positions
constexpr uint32_t MARKER_TILE_LDS = MARKER_TILE + 32;           // 16 bytes in front (history, the bytes before an odd row start), 16 behind
constexpr uint32_t MARKER_DIST_LDS = 8 * MARKER_TILE + 64;       // one distance byte per position from LDS byte 8 on
constexpr uint32_t MARKER_TABLE_MAX = 12288;                     // phases whose sums a workgroup keeps in LDS (48 KiB)

struct MarkerSearchArgs {
    const uint8_t* bytes;      // row r at bytes + r * row_stride
    const uint64_t* history;   // [rows] or null (hb = 0)
    uint32_t* distance;        // [rows][P]
    uint32_t* count;           // [rows][P] or null
    uint64_t row_stride;
    uint64_t marker, mask;     // left-aligned in 64 bits
    uint64_t items;            // rows * spans_per_row
    uint32_t n_bits, row_bytes, m, hb;
    uint32_t P, base;          // base: the phase of the first position, p = -hb
    uint32_t n_pos;            // positions of a row: n_bits + hb - m + 1
    uint32_t count_full, count_rem;        // n_pos / P and n_pos % P: the count of a phase is count_full, +1 for the first count_rem
    uint32_t tiles_per_span, spans_per_row;
    uint32_t table_in_lds;     // P <= MARKER_TABLE_MAX
};

// positions of phase `phase` among n_pos consecutive ones that start at phase `base`
__device__ inline uint32_t marker_phase_count(uint32_t phase, uint32_t base, uint32_t P, uint32_t full, uint32_t rem) {
    const uint32_t first = phase >= base ? phase - base : phase + (P - base);
    return full + (first < rem ? 1u : 0u);
}

__global__ void __launch_bounds__(256) marker_search_kernel(MarkerSearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t marker_lds[];
    uint8_t* tile = marker_lds;                                   // LDS byte 16 + i = byte i behind the tile's 16-byte aligned address
    uint8_t* dist = marker_lds + MARKER_TILE_LDS;                 // dist[i]: the distance at LDS bit 64 + i
    uint32_t* table = (uint32_t*)(marker_lds + MARKER_TILE_LDS + MARKER_DIST_LDS);
    const uint32_t NT = blockDim.x, tid = threadIdx.x;
    const uint32_t P = a.P;

    for (uint64_t item = blockIdx.x; item < a.items; item += gridDim.x) {
        const uint64_t r = item / a.spans_per_row;
        const uint32_t span = (uint32_t)(item - r * a.spans_per_row);
        const uint8_t* row = a.bytes + r * a.row_stride;
        uint32_t* gdist = a.distance + r * P;
        const int64_t mis = (int64_t)((uintptr_t)row & 15u);
        const uint64_t hist = a.hb ? a.history[r] & ((1ull << a.hb) - 1ull) : 0ull;

        // the counts do not depend on the data: the row's spans share the phases
        if (a.count)
            for (uint64_t ph = (uint64_t)span * NT + tid; ph < P; ph += (uint64_t)a.spans_per_row * NT) {
                const uint32_t c = marker_phase_count((uint32_t)ph, a.base, P, a.count_full, a.count_rem);
                if (c) atomicAdd(a.count + r * P + ph, c);
            }

        if (a.table_in_lds) {
            for (uint32_t ph = tid; ph < P; ph += NT) table[ph] = 0;
            __syncthreads();
        }

        const int64_t p_last = (int64_t)a.n_bits - (int64_t)a.m;                     // the last position of the row
        for (uint32_t t = 0; t < a.tiles_per_span; ++t) {
            const int64_t T = (int64_t)span * a.tiles_per_span + t;
            const int64_t rel_tile = T * MARKER_TILE - mis;                             // row byte of LDS byte 16
            const int64_t p_lo = T == 0 ? -(int64_t)a.hb : 8 * rel_tile;
            int64_t p_hi = 8 * (rel_tile + MARKER_TILE) - 1;
            p_hi = p_hi < p_last ? p_hi : p_last;
            if (p_hi < p_lo) continue;                                                  // the whole workgroup: the row ended

            // 1. the tile's bytes, once: row bytes only, 0 for what lies outside the row, the history in the 8 bytes before bit 0
            for (uint32_t c = tid; c < MARKER_TILE_LDS / 16; c += NT) {
                const int64_t rel = rel_tile - 16 + 16 * (int64_t)c;
                uint4 v;
                if (rel >= 0 && rel + 16 <= (int64_t)a.row_bytes) {
                    v = *(const uint4*)(row + rel);
                } else {
                    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (uint32_t i = 0; i < 16; ++i) {
                        const int64_t at = rel + i;
                        uint32_t b = 0;
                        if (at >= 0) {
                            if (at < (int64_t)a.row_bytes) b = row[at];
                        } else if (at >= -8) {
                            b = (uint32_t)(hist >> (8 * (uint32_t)(-1 - at))) & 0xFFu;
                        }
                        w[i >> 2] |= b << (8 * (i & 3u));
                    }
                    v = make_uint4(w[0], w[1], w[2], w[3]);
                }
                *(uint4*)(tile + 16 * c) = v;
            }
            __syncthreads();

            // 2. 32 positions per thread: LDS dwords dd .. dd + 2 as one big-endian 96-bit word
            const uint32_t* tile32 = (const uint32_t*)tile;
            uint32_t* dist32 = (uint32_t*)dist;
            for (uint32_t j = tid; j < MARKER_TILE / 4 + 2; j += NT) {
                const uint32_t dd = 2 + j;
                const uint64_t hi = ((uint64_t)__builtin_bswap32(tile32[dd]) << 32) | __builtin_bswap32(tile32[dd + 1]);
                const uint32_t lo = __builtin_bswap32(tile32[dd + 2]);
#pragma unroll
                for (uint32_t k4 = 0; k4 < 8; ++k4) {
                    uint32_t packed = 0;
#pragma unroll
                    for (uint32_t kk = 0; kk < 4; ++kk) {
                        const uint32_t k = 4 * k4 + kk;
                        const uint64_t win = k ? (hi << k) | (uint64_t)(lo >> (32 - k)) : hi;
                        packed |= (uint32_t)__builtin_popcountll((win ^ a.marker) & a.mask) << (8 * kk);
                    }
                    dist32[8 * j + k4] = packed;
                }
            }
            __syncthreads();

            // 3. consecutive lanes take consecutive positions, so consecutive phases
            const int64_t p_base = 8 * (rel_tile - 8);                                  // the position of dist[0]
            const uint32_t i_lo = (uint32_t)(p_lo - p_base), i_hi = (uint32_t)(p_hi - p_base);
            const uint32_t ph_tile = (uint32_t)(((uint32_t)(p_lo + (int64_t)a.hb) % P + a.base) % P);
            if (P <= NT) {
                // a stride that is a multiple of P keeps a thread on one phase: sum in a register
                const uint32_t Q = NT / P * P;
                if (tid < Q) {
                    uint32_t acc = 0;
                    for (uint32_t i = i_lo + tid; i <= i_hi; i += Q) acc += dist[i];
                    if (acc) atomicAdd(table + (ph_tile + tid) % P, acc);
                }
            } else {
                uint32_t ph = ph_tile + tid;
                ph = ph >= P ? ph - P : ph;
                if (a.table_in_lds) {
                    for (uint32_t i = i_lo + tid; i <= i_hi; i += NT) {
                        atomicAdd(table + ph, (uint32_t)dist[i]);
                        ph += NT;
                        ph = ph >= P ? ph - P : ph;
                    }
                } else {                                                                // more phases than the table holds: few hits each
                    for (uint32_t i = i_lo + tid; i <= i_hi; i += NT) {
                        atomicAdd(gdist + ph, (uint32_t)dist[i]);
                        ph += NT;
                        ph = ph >= P ? ph - P : ph;
                    }
                }
            }
            __syncthreads();
        }

        if (a.table_in_lds) {
            for (uint32_t ph = tid; ph < P; ph += NT) {
                const uint32_t v = table[ph];
                if (v) atomicAdd(gdist + ph, v);
            }
            __syncthreads();
        }
    }
}

// the totals of a call that overwrites them, zeroed on the stream in front of the search (a kernel, as sync_state_kernel zeroes the
// counters of the synchronisation search: the call enqueues kernels only)
__global__ void __launch_bounds__(256) marker_zero_kernel(uint32_t* distance, uint32_t* count, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        distance[i] = 0;
        if (count) count[i] = 0;
    }
}

struct MarkerPickArgs {
    const uint32_t* distance;  // [rows][P]
    const uint32_t* count;     // [rows][P], or null: the counts of this call alone (the closed form)
    vit_hip_marker_lock* lock; // [rows]
    uint32_t P, m, base, count_full, count_rem;
};

// a beats b iff compared_a > 0 and (compared_b == 0 or errors_a * compared_b < errors_b * compared_a): sync_beats of kernels_sync.hpp
__device__ inline bool marker_beats(uint32_t ea, uint32_t ca, uint32_t eb, uint32_t cb) {
    return ca > 0 && (cb == 0 || (uint64_t)ea * cb < (uint64_t)eb * ca);
}

// candidate index = 2 * phase + inverted: the order of the tie-break.  The relation orders the rates, so the winner does not depend
// on the order of the reduction: (e, c, idx) becomes the better of itself and (oe, oc, oidx)
__device__ inline void marker_keep_better(uint32_t& e, uint32_t& c, uint64_t& idx, uint32_t oe, uint32_t oc, uint64_t oidx) {
    const bool other = marker_beats(oe, oc, e, c) || (!marker_beats(e, c, oe, oc) && oidx < idx);
    e = other ? oe : e;
    c = other ? oc : c;
    idx = other ? oidx : idx;
}

__global__ void __launch_bounds__(256) marker_pick_kernel(MarkerPickArgs a) {
    __shared__ uint32_t wave_e[4], wave_c[4];
    __shared__ uint64_t wave_idx[4];
    const uint64_t r = blockIdx.x;
    const uint32_t* d = a.distance + r * a.P;
    const uint32_t* cnt = a.count ? a.count + r * a.P : nullptr;
    uint32_t e = 0, c = 0;
    uint64_t idx = ~0ull;                                        // beats nothing, loses every tie
    for (uint32_t ph = threadIdx.x; ph < a.P; ph += blockDim.x) {
        const uint32_t n = cnt ? cnt[ph] : marker_phase_count(ph, a.base, a.P, a.count_full, a.count_rem);
        const uint32_t compared = a.m * n, dist = d[ph];
        marker_keep_better(e, c, idx, dist, compared, 2ull * ph);
        marker_keep_better(e, c, idx, compared - dist, compared, 2ull * ph + 1);
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t oe = __shfl_down(e, off), oc = __shfl_down(c, off);
        const uint64_t oidx = ((uint64_t)__shfl_down((uint32_t)(idx >> 32), off) << 32) | __shfl_down((uint32_t)idx, off);
        marker_keep_better(e, c, idx, oe, oc, oidx);
    }
    if ((threadIdx.x & 63u) == 0) {
        wave_e[threadIdx.x >> 6] = e;
        wave_c[threadIdx.x >> 6] = c;
        wave_idx[threadIdx.x >> 6] = idx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < blockDim.x / 64; ++w) marker_keep_better(e, c, idx, wave_e[w], wave_c[w], wave_idx[w]);
        vit_hip_marker_lock out;
        out.phase = (uint32_t)(idx >> 1);
        out.inverted = (uint32_t)(idx & 1u);
        out.errors = e;
        out.compared = c;
        a.lock[r] = out;
    }
}

// the kernel arguments of a call the argument rule has accepted (rows >= 1), and the shape of its grid: the grid follows the positions,
// not the phases -- a row's tiles (one more than its bytes fill when it starts off 16 bytes) are cut into spans so that about 1024
// workgroups share the work; a workgroup that keeps P sums in LDS takes enough tiles to pay for zeroing and flushing them
inline MarkerSearchArgs marker_search_args(const uint8_t* d_bytes, size_t stride, size_t rows, size_t n_bits, uint64_t marker, uint32_t m,
                                           const uint64_t* d_history, uint32_t hb, uint32_t P, size_t phase0, uint32_t* d_distance,
                                           uint32_t* d_count) {
    MarkerSearchArgs a{};
    const size_t row_bytes = (n_bits + 7) / 8;
    a.bytes = d_bytes; a.history = hb ? d_history : nullptr; a.distance = d_distance; a.count = d_count;
    a.row_stride = stride ? stride : row_bytes;
    a.marker = marker << (64 - m); a.mask = ~0ull << (64 - m);
    a.n_bits = (uint32_t)n_bits; a.row_bytes = (uint32_t)row_bytes; a.m = m; a.hb = hb;
    a.P = P; a.base = (uint32_t)((phase0 + P - hb % P) % P);
    a.n_pos = (uint32_t)(n_bits + hb - m + 1);
    a.count_full = a.n_pos / P; a.count_rem = a.n_pos % P;
    a.table_in_lds = P <= MARKER_TABLE_MAX;
    const size_t row_tiles = n_bits >= m ? ((n_bits - m) / 8 + 15) / MARKER_TILE + 1 : 1;
    size_t per_span = (rows * row_tiles + 1023) / 1024;
    if (a.table_in_lds && per_span < (P + 2047) / 2048) per_span = (P + 2047) / 2048;
    if (per_span > row_tiles) per_span = row_tiles;
    a.tiles_per_span = (uint32_t)per_span;
    a.spans_per_row = (uint32_t)((row_tiles + per_span - 1) / per_span);
    a.items = (uint64_t)rows * a.spans_per_row;
    return a;
}

// ---- launchers (hipGetLastError() after each: 0 / -1) -----------------------------------------------------------------------

inline int marker_launch_zero(uint32_t* distance, uint32_t* count, uint64_t n, hipStream_t st) {
    const uint64_t blocks = (n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048;
    hipLaunchKernelGGL(marker_zero_kernel, dim3((unsigned)blocks), dim3(256), 0, st, distance, count, n);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

inline int marker_launch_search(const MarkerSearchArgs& a, hipStream_t st) {
    const uint64_t blocks = a.items < 8192 ? a.items : 8192;       // grid-stride past that
    const size_t lds = MARKER_TILE_LDS + MARKER_DIST_LDS + (a.table_in_lds ? (size_t)a.P * sizeof(uint32_t) : 0);
    hipLaunchKernelGGL(marker_search_kernel, dim3((unsigned)blocks), dim3(256), lds, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

inline int marker_launch_pick(const MarkerPickArgs& a, size_t rows, hipStream_t st) {
    hipLaunchKernelGGL(marker_pick_kernel, dim3((unsigned)rows), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace vit
