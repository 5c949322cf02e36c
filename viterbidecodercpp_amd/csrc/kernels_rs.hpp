// kernels_rs.hpp -- Reed-Solomon decoding over GF(256) on frames of interleaved codewords (vit_hip_rs_decode_batch): bounded-distance,
// errors only.  ONE kernel does both stages, so nothing passes through the host or through global memory between them:
//   rs_decode_kernel   one block per (frame, tile of up to 8 codewords), one wavefront per codeword.
//     staging    the block reads the tile's bytes once -- aligned dwords where the tile is the whole frame (interleave <= 8), bytes at
//                the ragged ends and for deeper interleaves -- and writes them de-interleaved, mapped to the conventional basis, into
//                one 256-byte LDS slot per codeword, zero-filled in front: leading zeros change no syndrome.
//     syndromes  a lane owns a (root, segment) pair: with R2 = the power of two at or above nroots the slot is cut into G = 64 / R2
//                segments, so nroots = 32 keeps both halves of the wave busy on one codeword and nroots = 2 all 32 pairs of lanes.
//                The lanes of a segment read the same LDS dword (a broadcast; G addresses per read) and run Horner's rule over its
//                four bytes.  The multiplication by the lane's root is linear over GF(2): three lookups of the state's bits 0-2, 3-5
//                and 6-7 in tables of 8, 8 and 4 products held in five registers, each lookup one v_perm_b32 (the selector is the
//                digit; its upper bytes select entry 0, the product of 0, so the result needs no mask).  Per byte and lane that is
//                v_and (or v_bitop3), v_bfe_u32, v_lshrrev, 3 x v_perm_b32 and 3 x v_xor, one of which takes the byte by SDWA: 9 vector
//                instructions, and one ds_read2_b32 per 8 bytes, against the log/exp form's 5 and TWO dependent LDS reads with 64
//                different addresses inside every Horner step.  A segment's sum is then raised by the power of the root that the segments behind it span, and the segments
//                are folded by __shfl_xor.
//     correction only where a syndrome is non-zero (a wave-uniform branch): Berlekamp-Massey with lane = coefficient (the discrepancy
//                is a cross-lane XOR reduction, B(x) shifts by one lane per step), the root search with lane = position in four rounds
//                of 64, Forney's value on the lanes that found a root.  Field products go through the exp / log tables in LDS here.
//                The decision is complete: locator degree != L, L > t, fewer roots than the degree, a root in the virtual fill, a
//                zero error value or a zero derivative all give status -1 and leave the word as received.
//     output     in place a wave stores only the bytes it corrected.  Out of place the block writes the whole tile back from LDS after a
//                barrier, by the indexing it was read with.
// Included only from vit_rs.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vit_hip.h"
#include "rs_tables.hpp"

namespace vit {

constexpr uint32_t RS_TILE = 8;          // codewords, and so wavefronts, per block at most

struct RsArgs {
    const uint8_t* in;
    uint8_t* out;
    const uint32_t* n_frames;        // [rows] or null
    int32_t* status;                 // [rows * max_frames * I]
    const uint8_t* tables;           // RS_TABLE_BYTES device bytes (rs_tables.hpp)
    uint64_t stride, max_frames;
    uint32_t I, tiles;               // interleave depth, ceil(I / RS_TILE)
    uint32_t n, nroots, t, fcr, prim;
    uint32_t R2, G, seg, base;       // lanes per segment, segments, bytes per segment (a multiple of 4), zero bytes in front: G * seg - n
};

struct RsShared {
    uint8_t tab[RS_TABLE_BYTES];
    alignas(16) uint8_t slot[RS_TILE][256];
    uint8_t syn[RS_TILE][64], lam[RS_TILE][64], om[RS_TILE][64];
};

// entry idx < 8 of the byte table held in (lo, hi)
__device__ inline uint32_t rs_lookup8(uint32_t lo, uint32_t hi, uint32_t idx) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, idx);
#else
    return (uint32_t)(((((uint64_t)hi << 32) | lo) >> (8u * idx)) & 0xFFu);
#endif
}

__device__ inline uint32_t rs_mul(const uint8_t* tab, uint32_t a, uint32_t b) {
    return a && b ? tab[RS_EXP + tab[RS_LOG + a] + tab[RS_LOG + b]] : 0u;
}
// a * alpha^e, e <= 256
__device__ inline uint32_t rs_mul_exp(const uint8_t* tab, uint32_t a, uint32_t e) { return a ? tab[RS_EXP + tab[RS_LOG + a] + e] : 0u; }

__device__ inline uint32_t rs_wave_xor(uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v ^= (uint32_t)__shfl_xor((int)v, off);
    return v;
}

__global__ void __launch_bounds__(64 * RS_TILE) rs_decode_kernel(RsArgs a) {
    __shared__ RsShared sh;
    const uint32_t tid = threadIdx.x, nthreads = blockDim.x;
    const uint64_t fi = blockIdx.x / a.tiles;                     // r * max_frames + f
    const uint32_t tile = blockIdx.x - (uint32_t)fi * a.tiles;
    const uint64_t r = fi / a.max_frames, f = fi - r * a.max_frames;
    if (a.n_frames && f >= a.n_frames[r]) return;                 // the whole block: nothing of this frame is read or written
    const uint32_t c0 = tile * RS_TILE;
    const uint32_t cw = a.I - c0 < RS_TILE ? a.I - c0 : RS_TILE;  // codewords of this tile
    const uint8_t* src = a.in + fi * a.stride;
    uint8_t* dst = a.out + fi * a.stride;
    const uint32_t n = a.n, total = n * cw;

    for (uint32_t k = tid; k < RS_TABLE_BYTES / 4; k += nthreads) ((uint32_t*)sh.tab)[k] = ((const uint32_t*)a.tables)[k];
    for (uint32_t k = tid; k < cw * a.base; k += nthreads) sh.slot[k / a.base][k % a.base] = 0;
    __syncthreads();

    // staging: byte q of the tile is symbol q / cw of codeword c0 + q % cw, frame byte (q / cw) * I + c0 + q % cw
    const uint8_t* to_conv = sh.tab + RS_TO_CONV;
    if (cw == a.I) {                                              // the tile is the frame: q is the frame offset
        const uint32_t head = (uint32_t)((4u - ((uintptr_t)src & 3u)) & 3u) < total ? (uint32_t)((4u - ((uintptr_t)src & 3u)) & 3u) : total;
        const uint32_t words = (total - head) / 4u;
        for (uint32_t k = tid; k < words; k += nthreads) {
            const uint32_t q0 = head + 4u * k;
            const uint32_t w = *(const uint32_t*)(src + q0);
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b) {
                const uint32_t q = q0 + b, i = q / cw, cc = q - i * cw;
                sh.slot[cc][a.base + i] = to_conv[(w >> (8u * b)) & 0xFFu];
            }
        }
        const uint32_t ragged = head + (total - head - 4u * words);          // bytes in front of the first and behind the last dword
        for (uint32_t k = tid; k < ragged; k += nthreads) {
            const uint32_t q = k < head ? k : head + 4u * words + (k - head), i = q / cw, cc = q - i * cw;
            sh.slot[cc][a.base + i] = to_conv[src[q]];
        }
    } else {
        for (uint32_t q = tid; q < total; q += nthreads) {
            const uint32_t i = q / cw, cc = q - i * cw;
            sh.slot[cc][a.base + i] = to_conv[src[(uint64_t)i * a.I + c0 + cc]];
        }
    }
    __syncthreads();

    const uint32_t wave = tid >> 6, lane = tid & 63u;
    const uint8_t* tab = sh.tab;
    if (wave < cw) {
        uint8_t* slot = sh.slot[wave];
        // ---- syndromes: S_j = r(alpha^(prim (fcr + j))), the received word read as a polynomial, first byte the highest power
        const uint32_t j = lane & (a.R2 - 1u), s = lane / a.R2;
        const bool active = j < a.nroots;
        const uint32_t rootlog = a.prim * (a.fcr + j) % 255u;
        uint32_t t0lo = 0, t0hi = 0, t1lo = 0, t1hi = 0, t2 = 0;                // products of the root with k, k << 3, k << 6
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            t0lo |= rs_mul_exp(tab, k, rootlog) << (8u * k);
            t0hi |= rs_mul_exp(tab, k + 4u, rootlog) << (8u * k);
            t1lo |= rs_mul_exp(tab, k << 3, rootlog) << (8u * k);
            t1hi |= rs_mul_exp(tab, (k + 4u) << 3, rootlog) << (8u * k);
            t2 |= rs_mul_exp(tab, k << 6, rootlog) << (8u * k);
        }
        const uint32_t* seg = (const uint32_t*)(slot + s * a.seg);
        uint32_t st = 0;
        for (uint32_t k = 0; k < a.seg / 4u; ++k) {
            const uint32_t w = seg[k];
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b) {
                const uint32_t m = rs_lookup8(t0lo, t0hi, st & 7u) ^ rs_lookup8(t1lo, t1hi, (st >> 3) & 7u) ^ rs_lookup8(t2, t2, st >> 6);
                st = m ^ ((w >> (8u * b)) & 0xFFu);
            }
        }
        // the segments behind segment s span seg * (G - 1 - s) powers
        st = rs_mul_exp(tab, st, rootlog * (a.seg * (a.G - 1u - s)) % 255u);
        for (uint32_t off = a.R2; off < 64u; off <<= 1) st ^= (uint32_t)__shfl_xor((int)st, (int)off);
        const uint32_t S = active ? st : 0u;

        int32_t status = 0;
        if (__ballot(S != 0) != 0) {
            uint8_t* syn = sh.syn[wave];
            uint8_t* lam = sh.lam[wave];
            uint8_t* om = sh.om[wave];
            if (lane < a.R2) syn[lane] = (uint8_t)S;                            // lanes [nroots, R2) hold 0
            __builtin_amdgcn_wave_barrier();
            // ---- Berlekamp-Massey, lane = coefficient.  Coefficient 64 (nroots = 64 only) is dropped: no discrepancy reads it, and a
            // locator that long has L > t
            uint32_t lambda = lane == 0, B = lane == 0, L = 0;
            for (uint32_t rr = 0; rr < a.nroots; ++rr) {
                const uint32_t up = (uint32_t)__shfl_up((int)B, 1);
                B = lane ? up : 0u;
                const uint32_t d = rs_wave_xor(lane <= rr ? rs_mul(tab, lambda, syn[rr - lane]) : 0u);
                if (d) {
                    const uint32_t next = lambda ^ rs_mul(tab, d, B);
                    if (2u * L <= rr) {
                        B = rs_mul_exp(tab, lambda, 255u - tab[RS_LOG + d]);    // lambda / d
                        L = rr + 1u - L;
                    }
                    lambda = next;
                }
            }
            const uint64_t nz = __ballot(lambda != 0);                          // bit 0 is always set
            const uint32_t deg = 63u - (uint32_t)__builtin_clzll(nz);
            bool bad = deg != L || L > a.t;
            uint32_t Y[4] = {0, 0, 0, 0};
            if (!bad) {
                lam[lane] = (uint8_t)lambda;
                __builtin_amdgcn_wave_barrier();
                // Omega = S Lambda mod x^L: with L errors its degree is below L
                uint32_t w = 0;
                for (uint32_t m = 0; m < L; ++m)
                    if (m <= lane && lane < L) w ^= rs_mul(tab, lam[m], syn[lane - m]);
                om[lane] = (uint8_t)w;
                __builtin_amdgcn_wave_barrier();
                // ---- roots: position p is the power of x, X = alpha^(prim p), z = 1 / X
                uint32_t found = 0;
#pragma unroll
                for (uint32_t round = 0; round < 4; ++round) {
                    const uint32_t p = 64u * round + lane;
                    const uint32_t zl = a.prim * ((255u - p) % 255u) % 255u;    // log z; lane p = 255 of the last round idles below
                    uint32_t sum = 0, odd = 0, e = 0;
                    for (uint32_t i = 0; i <= L; ++i) {
                        const uint32_t term = rs_mul_exp(tab, lam[i], e);
                        sum ^= term;
                        odd ^= (i & 1u) ? term : 0u;
                        e += zl;
                        e -= e >= 255u ? 255u : 0u;
                    }
                    const bool root = p < 255u && sum == 0;
                    found += (uint32_t)__builtin_popcountll(__ballot(root));
                    if (root) {
                        uint32_t omega = 0;
                        e = 0;
                        for (uint32_t i = 0; i < L; ++i) {
                            omega ^= rs_mul_exp(tab, om[i], e);
                            e += zl;
                            e -= e >= 255u ? 255u : 0u;
                        }
                        // Forney: Y = X^(-fcr) Omega(z) / (z Lambda'(z)), and z Lambda'(z) is the odd part of Lambda(z)
                        if (p >= a.n || omega == 0 || odd == 0) bad = true;
                        else Y[round] = rs_mul_exp(tab, rs_mul_exp(tab, omega, 255u - tab[RS_LOG + odd]), zl * a.fcr % 255u);
                    }
                }
                bad = __ballot(bad) != 0 || found != L;
            }
            status = bad ? -1 : (int32_t)L;
            if (!bad) {
#pragma unroll
                for (uint32_t round = 0; round < 4; ++round) {
                    if (Y[round]) {                                             // a lane with a root has a non-zero value
                        const uint32_t i = n - 1u - (64u * round + lane);
                        const uint32_t v = slot[a.base + i] ^ Y[round];
                        slot[a.base + i] = (uint8_t)v;
                        if (a.out == a.in) dst[(uint64_t)i * a.I + c0 + wave] = tab[RS_TO_DUAL + v];
                    }
                }
            }
        }
        if (lane == 0) a.status[fi * a.I + c0 + wave] = status;
    }
    if (a.out == a.in) return;
    __syncthreads();
    const uint8_t* to_dual = sh.tab + RS_TO_DUAL;
    for (uint32_t q = tid; q < total; q += nthreads) {
        const uint32_t i = q / cw, cc = q - i * cw;
        dst[(uint64_t)i * a.I + c0 + cc] = to_dual[sh.slot[cc][a.base + i]];
    }
}

// ---- launcher (hipGetLastError() after it: 0 / -1) ---------------------------------------------------------------------------

inline int rs_launch_decode(const RsArgs& a, uint64_t frames, hipStream_t st) {
    const uint32_t waves = a.I < RS_TILE ? a.I : RS_TILE;
    hipLaunchKernelGGL(rs_decode_kernel, dim3((unsigned)(frames * a.tiles)), dim3(64 * waves), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace vit
