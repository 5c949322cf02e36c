// kernels_dvb.hpp -- the DVB-S outer chain around Reed-Solomon: the convolutional (Forney) de-interleaver in front of it
// (vit_hip_deinterleave_batch) and the energy-dispersal removal behind it (vit_hip_dvb_derandomize_batch), both on packets in the layout
// vit_hip_frames_extract writes.
//   deinterleave_kernel     a gather: output byte i of a packet rode branch i mod B and comes from (B-1 - i mod B) M B bytes further back
//                           in the byte stream than the byte H packets ahead of it.  The blocks of a row are ob OUTPUT blocks and hb HISTORY
//                           blocks.  An output block owns G consecutive output packets: it stages their G + H source packets ONCE in LDS
//                           as one contiguous piece of the logical byte stream -- each packet from the history or from the input by its
//                           index, aligned dwords where source and LDS offset agree mod 4, bytes at the ragged ends and elsewhere -- so
//                           that the source of an output byte is ONE subtraction away, with no division by the packet length.  Then a wave
//                           takes a packet, a lane an aligned output dword: four LDS byte reads, one store; bytes at a packet's ragged
//                           ends.  Read amplification (G + H) / G: 75 / 64 at DVB-S's (12, 17, 204).
//                           LDS banks: neighbouring lanes read 4 bytes apart on the same branch every B / gcd(B, 4) lanes, and the
//                           branches lie M B bytes apart: at 204 bytes = 51 dwords the three branch families of a byte lane fall on banks
//                           3a, 3a + 13 and 3a + 26, at worst two lanes on a bank.  A cell M B that is a multiple of 128 bytes puts every
//                           branch on one bank (up to B / gcd(B, 4) lanes); the image is not padded against that, the result is the same.
//                           A history block copies up to GH packets of the new history, dwords where source and destination agree mod 4;
//                           the first of a row also writes the row's two counts.
//   dvb_derandomize_kernel  the group phase comes from d_phase_in or, unknown, from a vote over ALL sync bytes of the row, which every
//                           block of the row takes for itself (a thread's packets share f mod 8, so it keeps one sum; eight LDS atomics
//                           per thread) -- nothing passes between blocks.  Then a wave takes a packet, a lane an aligned output dword: the
//                           188 bytes XORed with the sequence, which lies in LDS as dwords and is cut at any byte offset by a 64-bit
//                           shift.  In place the vote would read sync bytes another block has already de-inverted: there a row is ONE
//                           block of 1024 threads that votes, meets at a barrier and only then writes.
// The sequence is a compile-time constant (dvb_prbs_words).  Nothing here names a packet by a 32-bit byte offset into global memory.
// Included only from vit_dvb.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vit_hip.h"

namespace vit {

constexpr uint32_t DVB_LDS_BYTES = 32768;      // staging of one de-interleaver block: (G + H) n bytes at most, G >= 1
constexpr uint32_t DVB_G_MAX = 64;             // output packets of a block at most
constexpr uint32_t DVB_HIST_BLOCK_BYTES = 16384;
constexpr uint32_t DVB_PACKET = 188;           // an MPEG-2 transport packet
constexpr uint32_t DVB_PRBS_BYTES = 1503;      // 8 * 188 - 1: the sequence runs from behind the inverted sync byte to the next one
constexpr uint32_t DVB_PRBS_WORDS = 378;       // the bytes as little-endian dwords, zero-filled, one dword to spare for the 64-bit cut

// 1 + x^14 + x^15, registers 1 .. 15 loaded with 100101010000000, output = reg 14 ^ reg 15 fed back into reg 1, bits MSB-first
struct DvbPrbs { uint32_t w[DVB_PRBS_WORDS]; };
constexpr DvbPrbs dvb_prbs_words() {
    DvbPrbs t{};
    uint32_t reg = 0;                          // bit k-1 = register k
    const char* init = "100101010000000";
    for (uint32_t k = 0; k < 15; ++k) reg |= (uint32_t)(init[k] - '0') << k;
    for (uint32_t i = 0; i < DVB_PRBS_BYTES; ++i) {
        uint32_t byte = 0;
        for (uint32_t b = 0; b < 8; ++b) {
            const uint32_t o = ((reg >> 13) ^ (reg >> 14)) & 1u;
            reg = ((reg << 1) | o) & 0x7FFFu;
            byte = (byte << 1) | o;
        }
        t.w[i / 4] |= byte << (8u * (i % 4));
    }
    return t;
}
__device__ constexpr DvbPrbs DVB_PRBS = dvb_prbs_words();

struct DeintArgs {
    const uint8_t* in;               // packet (r, f) at in + (r * max_frames + f) * stride
    const uint32_t* n_frames;        // [rows] or null
    const uint8_t* hist_in;          // row r at hist_in + r * hist_stride: H packets packed, the newest last; or null
    const uint32_t* fill_in;         // [rows]
    uint8_t* out;
    uint32_t* n_out;                 // [rows]
    uint8_t* hist_out;
    uint32_t* fill_out;              // [rows]
    uint64_t stride, out_stride, hist_stride, max_frames;
    uint32_t B, MB, n, H;            // branches, bytes between two branches' delays (M * B), packet bytes, packets of history
    uint32_t magic;                  // ceil(2^32 / B): i / B = (i * magic) >> 32 for i, B <= 2^15
    uint32_t G, GH, ob, hb;          // output packets per output block, history packets per history block, blocks of either per row
};

// n bytes from src to dst (global): a lane takes the aligned dwords of the DESTINATION; bytes where a dword is not whole
__device__ inline void dvb_copy_packet(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t lane, uint32_t lanes) {
    const uint32_t mis = (uint32_t)((uintptr_t)dst & 3u);
    const uint32_t units = (n + mis + 3u) / 4u;
    for (uint32_t u = lane; u < units; u += lanes) {
        const int32_t lo = (int32_t)(4u * u) - (int32_t)mis;
        if (lo >= 0 && (uint32_t)lo + 4u <= n) {
            const uint8_t* s = src + lo;
            uint32_t w;
            if (((uintptr_t)s & 3u) == 0) w = *(const uint32_t*)s;
            else w = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
            *(uint32_t*)(dst + lo) = w;
        } else {
            for (int32_t i = lo < 0 ? 0 : lo; i < lo + 4 && (uint32_t)i < n; ++i) dst[i] = src[i];
        }
    }
}

__global__ void __launch_bounds__(256) deinterleave_kernel(DeintArgs a) {
    extern __shared__ uint32_t dvb_lds32[];
    uint8_t* lds = (uint8_t*)dvb_lds32;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u, waves = blockDim.x >> 6;
    const uint32_t per_row = a.ob + a.hb;
    const uint64_t r = blockIdx.x / per_row;
    const uint32_t b = blockIdx.x - (uint32_t)r * per_row;
    const uint32_t n = a.n, H = a.H;

    // the row's counts, from the same inputs in every block.  Whatever the memory holds, nf <= max_frames and fill <= H
    uint64_t nf = a.n_frames ? a.n_frames[r] : a.max_frames;
    nf = nf < a.max_frames ? nf : a.max_frames;
    uint32_t fill = a.hist_in ? a.fill_in[r] : 0u;
    fill = fill < H ? fill : H;
    const uint64_t T = fill + nf;
    const uint64_t nout = T > H ? T - H : 0;
    const uint8_t* in_row = a.in + r * a.max_frames * a.stride;
    const uint8_t* hist_row = fill ? a.hist_in + r * a.hist_stride + (uint64_t)(H - fill) * n : a.in;      // packet 0 of S, with fill > 0

    if (b >= a.ob) {                                               // ---- the new history: the last min(H, T) packets of S, right-aligned
        const uint32_t hbk = b - a.ob;
        const uint32_t keep = T < H ? (uint32_t)T : H;
        if (hbk == 0 && tid == 0) {
            a.n_out[r] = (uint32_t)nout;
            a.fill_out[r] = keep;
        }
        uint32_t h0 = hbk * a.GH, h1 = h0 + a.GH < H ? h0 + a.GH : H;
        h0 = h0 > H - keep ? h0 : H - keep;
        for (uint32_t h = h0 + wave; h < h1; h += waves) {
            const uint64_t j = T - (H - h);
            const uint8_t* src = j < fill ? hist_row + j * n : in_row + (j - fill) * a.stride;
            dvb_copy_packet(a.hist_out + r * a.hist_stride + (uint64_t)h * n, src, n, lane, 64u);
        }
        return;
    }

    const uint64_t k0 = (uint64_t)b * a.G;
    if (k0 >= nout) return;
    const uint32_t g = nout - k0 < a.G ? (uint32_t)(nout - k0) : a.G;

    // ---- staging: S packets [k0, k0 + g + H), all of which exist (k0 + g + H <= T), at LDS byte s * n
    for (uint32_t s = wave; s < g + H; s += waves) {
        const uint64_t j = k0 + s;
        const uint8_t* src = j < fill ? hist_row + j * n : in_row + (j - fill) * a.stride;
        const uint32_t mis = (uint32_t)((uintptr_t)src & 3u);
        const uint32_t units = (n + mis + 3u) / 4u;
        const uint32_t at = s * n;
        for (uint32_t u = lane; u < units; u += 64u) {
            const int32_t lo = (int32_t)(4u * u) - (int32_t)mis;
            if (lo >= 0 && (uint32_t)lo + 4u <= n) {
                const uint32_t w = *(const uint32_t*)(src + lo);
                const uint32_t d = at + (uint32_t)lo;
                if ((d & 3u) == 0) {
                    *(uint32_t*)(lds + d) = w;
                } else {
                    lds[d] = (uint8_t)w; lds[d + 1] = (uint8_t)(w >> 8); lds[d + 2] = (uint8_t)(w >> 16); lds[d + 3] = (uint8_t)(w >> 24);
                }
            } else {
                for (int32_t i = lo < 0 ? 0 : lo; i < lo + 4 && (uint32_t)i < n; ++i) lds[at + (uint32_t)i] = src[i];
            }
        }
    }
    __syncthreads();

    // ---- output: byte i of packet k0 + kk lies at LDS byte (H + kk) n + i - (B-1 - i mod B) M B; 0 <= that < (g + H) n
    for (uint32_t kk = wave; kk < g; kk += waves) {
        uint8_t* dst = a.out + (r * a.max_frames + k0 + kk) * a.out_stride;
        const uint32_t mis = (uint32_t)((uintptr_t)dst & 3u);
        const uint32_t units = (n + mis + 3u) / 4u;
        const uint32_t base = (H + kk) * n - (a.B - 1u) * a.MB;
        for (uint32_t u = lane; u < units; u += 64u) {
            const int32_t lo = (int32_t)(4u * u) - (int32_t)mis;
            const uint32_t i0 = lo < 0 ? 0u : (uint32_t)lo;
            uint32_t m = i0 - (uint32_t)(((uint64_t)i0 * a.magic) >> 32) * a.B;          // i0 mod B
            if (lo >= 0 && (uint32_t)lo + 4u <= n) {
                uint32_t w = 0;
#pragma unroll
                for (uint32_t c = 0; c < 4; ++c) {
                    w |= (uint32_t)lds[base + i0 + c + m * a.MB] << (8u * c);
                    m = m + 1u == a.B ? 0u : m + 1u;
                }
                *(uint32_t*)(dst + lo) = w;
            } else {
                for (uint32_t i = i0; (int32_t)i < lo + 4 && i < n; ++i) {
                    dst[i] = lds[base + i + m * a.MB];
                    m = m + 1u == a.B ? 0u : m + 1u;
                }
            }
        }
    }
}

struct DerandArgs {
    const uint8_t* in;               // packet (r, f) at in + (r * max_frames + f) * stride; the first 188 bytes are read
    const uint32_t* n_frames;        // [rows] or null
    const uint32_t* phase_in;        // [rows] or null: all unknown
    const int32_t* rs_status;        // [rows][max_frames] or null
    uint8_t* out;
    uint32_t* phase_out;             // [rows]
    uint32_t* sync_errors;           // [rows][max_frames] or null
    uint64_t stride, out_stride, max_frames;
    uint32_t PB, bpr;                // packets per block, blocks per row
};

// the four sequence bytes from byte idx on, the first in the low byte; idx + 3 < 4 * (DVB_PRBS_WORDS - 1)
__device__ inline uint32_t dvb_prbs4(const uint32_t* tab, uint32_t idx) {
    const uint64_t two = ((uint64_t)tab[idx / 4u + 1u] << 32) | tab[idx / 4u];
    return (uint32_t)(two >> (8u * (idx & 3u)));
}

__global__ void __launch_bounds__(1024) dvb_derandomize_kernel(DerandArgs a) {
    __shared__ uint32_t tab[DVB_PRBS_WORDS];
    __shared__ int32_t cost[8];
    const uint32_t tid = threadIdx.x, nthreads = blockDim.x, wave = tid >> 6, lane = tid & 63u, waves = nthreads >> 6;
    const uint64_t r = blockIdx.x / a.bpr;
    const uint32_t b = blockIdx.x - (uint32_t)r * a.bpr;
    uint64_t nf = a.n_frames ? a.n_frames[r] : a.max_frames;
    nf = nf < a.max_frames ? nf : a.max_frames;
    const uint8_t* in_row = a.in + r * a.max_frames * a.stride;

    for (uint32_t k = tid; k < DVB_PRBS_WORDS; k += nthreads) tab[k] = DVB_PRBS.w[k];
    if (tid < 8) cost[tid] = 0;
    __syncthreads();

    uint32_t g = a.phase_in ? a.phase_in[r] : 8u;
    if (g >= 8u) {
        // cost(g) = sum_f d47(f) + sum over the f with (g + f) mod 8 = 0 of (8 - 2 d47(f)), d47 the distance to 0x47: the first sum is
        // the same for every g.  nthreads is a multiple of 8, so every packet of a thread votes for the same g
        int32_t acc = 0;
        for (uint64_t f = tid; f < nf; f += nthreads) acc += 8 - 2 * (int32_t)__popc((uint32_t)in_row[f * a.stride] ^ 0x47u);
        if (acc) atomicAdd(&cost[(8u - (tid & 7u)) & 7u], acc);
        __syncthreads();                                           // in place: every sync byte is read before one is written
        g = 0;
        for (uint32_t k = 1; k < 8; ++k) g = cost[k] < cost[g] ? k : g;
        if (nf == 0) g = 8u;
    }
    if (b == 0 && tid == 0) a.phase_out[r] = g >= 8u ? 0xFFFFFFFFu : (g + (uint32_t)(nf & 7u)) & 7u;

    const uint64_t f0 = (uint64_t)b * a.PB;
    const uint64_t f1 = f0 + a.PB < nf ? f0 + a.PB : nf;
    for (uint64_t f = f0 + wave; f < f1; f += waves) {
        const uint64_t fi = r * a.max_frames + f;
        const uint8_t* src = a.in + fi * a.stride;
        uint8_t* dst = a.out + fi * a.out_stride;
        const uint32_t q = (g + (uint32_t)(f & 7u)) & 7u;
        const bool tei = a.rs_status && a.rs_status[fi] < 0;
        const uint32_t mis = (uint32_t)((uintptr_t)dst & 3u);
        const uint32_t units = (DVB_PACKET + mis + 3u) / 4u;
        for (uint32_t u = lane; u < units; u += 64u) {
            const int32_t lo = (int32_t)(4u * u) - (int32_t)mis;
            if (lo >= 2 && (uint32_t)lo + 4u <= DVB_PACKET) {
                const uint8_t* s = src + lo;
                uint32_t w;
                if (((uintptr_t)s & 3u) == 0) w = *(const uint32_t*)s;
                else w = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
                *(uint32_t*)(dst + lo) = w ^ dvb_prbs4(tab, q * DVB_PACKET + (uint32_t)lo - 1u);
            } else {
                for (int32_t i = lo < 0 ? 0 : lo; i < lo + 4 && (uint32_t)i < DVB_PACKET; ++i) {
                    const uint32_t x = src[i];
                    uint32_t y;
                    if (i == 0) {
                        y = q == 0 ? x ^ 0xFFu : x;                // de-inverted, not forced
                        if (a.sync_errors) a.sync_errors[fi] = (uint32_t)__popc(x ^ (q == 0 ? 0xB8u : 0x47u));
                    } else {
                        y = x ^ (dvb_prbs4(tab, q * DVB_PACKET + (uint32_t)i - 1u) & 0xFFu);
                        if (i == 1 && tei) y |= 0x80u;             // transport_error_indicator
                    }
                    dst[i] = (uint8_t)y;
                }
            }
        }
    }
}

// ---- launchers (hipGetLastError() after them: 0 / -1) ---------------------------------------------------------------------------

inline int dvb_launch_deinterleave(const DeintArgs& a, uint64_t rows, hipStream_t st) {
    const uint32_t lds = ((a.G + a.H) * a.n + 3u) & ~3u;
    hipLaunchKernelGGL(deinterleave_kernel, dim3((unsigned)(rows * (a.ob + a.hb))), dim3(256), lds, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

inline int dvb_launch_derandomize(const DerandArgs& a, uint64_t rows, bool in_place, hipStream_t st) {
    hipLaunchKernelGGL(dvb_derandomize_kernel, dim3((unsigned)(rows * a.bpr)), dim3(in_place ? 1024 : 256), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace vit
