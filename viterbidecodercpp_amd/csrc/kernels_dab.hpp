// kernels_dab.hpp -- the DAB receive chain around the decoder (ETSI EN 300 401): the time de-interleaver of clause 12 fused with the
// depuncturing of clause 11 in front of it (vit_hip_dab_deinterleave_batch), and the energy-dispersal removal of clause 10 behind it
// (vit_hip_dab_descramble_batch).
//   dab_deinterleave_kernel<soft_t>   A gather.  Soft bit i of a frame was sent d(i mod 16) frames late, d the 4-bit reversal, so logical
//                       frame k of a row is a_k[i] = S[k + d(i mod 16)][i], S being the row's real history frames followed by its input
//                       frames; output symbol q is a_k[map[q]], or 0 where the map names nothing.  The output [rows][max_frames][spf]
//                       is ONE dense array: a thread owns the 4 / sizeof(soft_t) consecutive elements of one ALIGNED dword of it (they
//                       may belong to two frames, even two rows), finds frame and position by one division each and steps from there,
//                       and stores one dword -- or, where some of its elements belong to a frame at or behind the row's nout, which is
//                       not written, the others one by one.  The elements in front of the first aligned dword and behind the last are
//                       stored by threads of block 0.  Map reads are coalesced; a wave's 64 consecutive sources fall on 16 frames of S,
//                       16 cache lines that the neighbouring output frames read again: there is no LDS and no barrier.
//                       Behind the output blocks come, per row, H * cb HISTORY blocks: block (h, c) copies chunk c of frame h of the new
//                       history, element by element (an element load and store is always aligned); the first of a row also writes the
//                       row's two counts.  Every block works the row's counts out for itself from the same inputs.
//   dab_descramble_kernel   The 511-bit sequence of x^9 + x^5 + 1 is a compile-time constant (dab_prbs_words), doubled and as big-endian
//                       bit words, which every block copies into LDS once.  The frames are cut into units of one aligned dword of the
//                       DESTINATION; unit u of a frame lies 4u - mis bytes into it, its 32 pad bits are the window of the doubled
//                       sequence at (8 (4u - mis)) mod 511, one funnel shift of two LDS words, byte-swapped (the frame is big-endian)
//                       and cut at n_bits.  Units that are not whole inside the frame's bytes go byte by byte.  A thread takes four
//                       units, 256 apart; in place it reads and writes its own bytes alone.
// Everything is plain C++ in device functions that take (block, thread): the source also runs on the host (tests/cpp/dab_host_check.cpp).
// Included only from vit_dab.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vit_hip.h"
#include "arg_rules.hpp"

namespace vit {

constexpr uint32_t DAB_BLOCK = 256;            // threads of a block
constexpr uint32_t DAB_H = 15;                 // frames of history: the longest delay
constexpr uint32_t DAB_HIST_CHUNK = 4096;      // elements of one history block
constexpr uint32_t DAB_PRBS_PERIOD = 511;
constexpr uint32_t DAB_PRBS_WORDS = 33;        // 2 * 511 = 1022 bits and the word behind the last window's
constexpr uint32_t DAB_UNITS_PER_THREAD = 4;

struct DabDeintArgs {
    const void* in;                  // soft_t: frame (r, f) at r * row_stride + f * frame_stride
    const uint32_t* n_frames;        // [rows] or null
    const int32_t* map;              // [spf] or null: the identity
    const void* hist_in;             // row r at r * hist_stride: H frames of n packed, the newest last; or null
    const uint32_t* fill_in;         // [rows]
    void* out;                       // soft_t [rows][max_frames][spf]
    uint32_t* n_out;                 // [rows]
    void* hist_out;
    uint32_t* fill_out;              // [rows]
    uint64_t row_stride, frame_stride, hist_stride;      // elements
    uint32_t rows, max_frames, n, spf;
    uint32_t total;                  // rows * max_frames * spf < 2^32
    uint32_t head, tail, groups;     // elements in front of the first aligned dword, behind the last; dwords between
    uint32_t ob, cb;                 // output blocks; history blocks per history frame
};

// the delay of soft bit i in frames: the 4-bit reversal of i mod 16
__host__ __device__ inline uint32_t dab_delay(uint32_t i) {
    return ((i & 1u) << 3) | ((i & 2u) << 1) | ((i & 4u) >> 1) | ((i & 8u) >> 3);
}

// what a block knows of row r.  Whatever the memory holds: nf <= max_frames, fill <= H
struct DabRow { uint32_t nf, fill, T, nout; };
__device__ inline DabRow dab_row(const DabDeintArgs& a, uint32_t r) {
    DabRow w;
    w.nf = a.n_frames ? a.n_frames[r] : a.max_frames;
    w.nf = w.nf < a.max_frames ? w.nf : a.max_frames;
    w.fill = a.hist_in ? a.fill_in[r] : 0u;
    w.fill = w.fill < DAB_H ? w.fill : DAB_H;
    w.T = w.fill + w.nf;                                           // max_frames < 2^31: no wrap-around
    w.nout = w.T > DAB_H ? w.T - DAB_H : 0u;
    return w;
}

// S[s][i] of row r, s < T, i < n
template <class soft_t>
__device__ inline soft_t dab_source(const DabDeintArgs& a, uint32_t r, const DabRow& w, uint32_t s, uint32_t i) {
    if (s < w.fill) return ((const soft_t*)a.hist_in)[(uint64_t)r * a.hist_stride + (uint64_t)(DAB_H - w.fill + s) * a.n + i];
    return ((const soft_t*)a.in)[(uint64_t)r * a.row_stride + (uint64_t)(s - w.fill) * a.frame_stride + i];
}

// out[r][k][q], k < nout: k + delay <= nout - 1 + 15 = T - 1
template <class soft_t>
__device__ inline soft_t dab_output(const DabDeintArgs& a, uint32_t r, const DabRow& w, uint32_t k, uint32_t q) {
    const uint32_t p = a.map ? (uint32_t)a.map[q] : q;
    if (p >= a.n) return (soft_t)0;
    return dab_source<soft_t>(a, r, w, k + dab_delay(p), p);
}

// what thread `tid` of output block `block` does
template <class soft_t>
__device__ inline void dab_output_thread(const DabDeintArgs& a, uint32_t block, uint32_t tid) {
    constexpr uint32_t VEC = 4u / sizeof(soft_t);
    soft_t* out = (soft_t*)a.out;
    const uint32_t G = block * DAB_BLOCK + tid;                    // groups <= 2^32 / VEC: no wrap-around below
    if (G < a.groups) {
        const uint32_t g = a.head + G * VEC;
        const uint32_t fr = g / a.spf;
        uint32_t q = g - fr * a.spf, r = fr / a.max_frames, k = fr - r * a.max_frames, word = 0, written = 0;
        DabRow w = dab_row(a, r);
#pragma unroll
        for (uint32_t v = 0; v < VEC; ++v) {
            if (k < w.nout) {
                const soft_t s = dab_output<soft_t>(a, r, w, k, q);
                word |= ((uint32_t)s & (0xFFFFFFFFu >> (32u - 8u * sizeof(soft_t)))) << (8u * sizeof(soft_t) * v);
                written |= 1u << v;
            }
            if (++q == a.spf) {
                q = 0;
                if (++k == a.max_frames) {
                    k = 0;
                    ++r;
                    if (v + 1 < VEC) w = dab_row(a, r);            // g + v + 1 < total: the row exists
                }
            }
        }
        if (written == (1u << VEC) - 1u) {
            __builtin_memcpy(__builtin_assume_aligned(out + g, 4), &word, 4);
        } else {
#pragma unroll
            for (uint32_t v = 0; v < VEC; ++v)
                if (written & (1u << v)) out[g + v] = (soft_t)(word >> (8u * sizeof(soft_t) * v));
        }
    }
    if (block == 0 && tid < a.head + a.tail) {
        const uint32_t g = tid < a.head ? tid : a.total - a.tail + (tid - a.head);
        const uint32_t fr = g / a.spf, q = g - fr * a.spf, r = fr / a.max_frames, k = fr - r * a.max_frames;
        const DabRow w = dab_row(a, r);
        if (k < w.nout) out[g] = dab_output<soft_t>(a, r, w, k, q);
    }
}

// what thread `tid` of history block `hbk` (0 .. rows * H * cb) does
template <class soft_t>
__device__ inline void dab_history_thread(const DabDeintArgs& a, uint32_t hbk, uint32_t tid, uint32_t nthreads) {
    const uint32_t per_row = DAB_H * a.cb;
    const uint32_t r = hbk / per_row, b = hbk - r * per_row, h = b / a.cb, c = b - h * a.cb;
    const DabRow w = dab_row(a, r);
    const uint32_t keep = w.T < DAB_H ? w.T : DAB_H;
    if (b == 0 && tid == 0) {
        a.n_out[r] = w.nout;
        a.fill_out[r] = keep;
    }
    if (h < DAB_H - keep) return;                                  // the frames in front of the real ones are not written
    const uint32_t s = w.T - (DAB_H - h);                          // < T
    soft_t* dst = (soft_t*)a.hist_out + (uint64_t)r * a.hist_stride + (uint64_t)h * a.n;
    const uint32_t i0 = c * DAB_HIST_CHUNK;                        // cb * DAB_HIST_CHUNK < n + DAB_HIST_CHUNK: no wrap-around
    const uint32_t i1 = a.n - i0 < DAB_HIST_CHUNK ? a.n : i0 + DAB_HIST_CHUNK;
    for (uint32_t i = i0 + tid; i < i1; i += nthreads) dst[i] = dab_source<soft_t>(a, r, w, s, i);
}

template <class soft_t>
__global__ void __launch_bounds__(DAB_BLOCK) dab_deinterleave_kernel(DabDeintArgs a) {
    if (blockIdx.x < a.ob) dab_output_thread<soft_t>(a, blockIdx.x, threadIdx.x);
    else dab_history_thread<soft_t>(a, blockIdx.x - a.ob, threadIdx.x, DAB_BLOCK);
}

// the head / groups / tail of a call the argument rule has accepted
inline void dab_deinterleave_split(DabDeintArgs& a, size_t soft_bytes) {
    const uint32_t vec = 4u / (uint32_t)soft_bytes;
    const uint32_t mis = (uint32_t)(((uintptr_t)a.out / soft_bytes) % vec);            // elements the output starts behind a dword boundary
    a.head = (vec - mis) % vec;
    a.head = a.head < a.total ? a.head : a.total;
    a.groups = (a.total - a.head) / vec;
    a.tail = a.total - a.head - a.groups * vec;
    a.ob = a.groups ? (a.groups + DAB_BLOCK - 1) / DAB_BLOCK : 1u;
    a.cb = (a.n + DAB_HIST_CHUNK - 1) / DAB_HIST_CHUNK;
}

inline uint64_t dab_deinterleave_blocks(const DabDeintArgs& a) { return (uint64_t)a.ob + (uint64_t)a.rows * DAB_H * a.cb; }

// ---- energy dispersal ---------------------------------------------------------------------------------------------------------------

// p[n] = p[n-5] ^ p[n-9], p[-9 .. -1] = 1; bit t of the doubled sequence is bit 31 - t%32 of word t/32
struct DabPrbs { uint32_t w[DAB_PRBS_WORDS]; };
constexpr DabPrbs dab_prbs_words() {
    DabPrbs t{};
    uint32_t reg = 0x1FFu;                                         // bit j: p[n - 1 - j]
    uint32_t seq[16] = {};                                         // the 511 bits of one period
    for (uint32_t n = 0; n < DAB_PRBS_PERIOD; ++n) {
        const uint32_t o = ((reg >> 4) ^ (reg >> 8)) & 1u;
        reg = ((reg << 1) | o) & 0x1FFu;
        seq[n / 32] |= o << (n % 32);
    }
    for (uint32_t i = 0; i < 32 * DAB_PRBS_WORDS; ++i) {
        const uint32_t n = i % DAB_PRBS_PERIOD;
        t.w[i / 32] |= ((seq[n / 32] >> (n % 32)) & 1u) << (31u - i % 32);
    }
    return t;
}
__device__ constexpr DabPrbs DAB_PRBS = dab_prbs_words();

struct DabDescrArgs {
    const uint8_t* in;               // frame (r, f) at in + (r * max_frames + f) * stride
    const uint32_t* n_frames;        // [rows] or null
    uint8_t* out;
    uint64_t stride, out_stride;
    uint32_t max_frames, frames;     // frames = rows * max_frames
    uint32_t n_bits, nb;             // nb = ceil(n_bits / 8) >= 1
    uint32_t U;                      // units of a frame: aligned destination dwords it can touch, nb / 4 + 2 at most
    uint64_t units;                  // frames * U < 2^32
};

// the 32 sequence bits from bit o on (o < 511), the first in the highest
__device__ inline uint32_t dab_prbs32(const uint32_t* tab, uint32_t o) {
    const uint32_t hi = tab[o >> 5], lo = tab[(o >> 5) + 1u], sh = o & 31u;
    return sh ? (hi << sh) | (lo >> (32u - sh)) : hi;
}

// the pad of the four frame bytes from byte `at` on, as the little-endian dword they make; bits at or behind n_bits are 0
__device__ inline uint32_t dab_pad4(const DabDescrArgs& a, const uint32_t* tab, uint32_t at) {
    uint32_t p = dab_prbs32(tab, (uint32_t)((8ull * at) % DAB_PRBS_PERIOD));
    const uint64_t end = 8ull * at + 32u;
    if (end > a.n_bits) p &= end - a.n_bits >= 32u ? 0u : 0xFFFFFFFFu << (uint32_t)(end - a.n_bits);
    return __builtin_bswap32(p);
}

// unit t of the call
__device__ inline void dab_descramble_unit(const DabDescrArgs& a, const uint32_t* tab, uint32_t t) {
    const uint32_t fi = t / a.U, u = t - fi * a.U;
    const uint32_t r = fi / a.max_frames, f = fi - r * a.max_frames;
    uint32_t nf = a.n_frames ? a.n_frames[r] : a.max_frames;
    nf = nf < a.max_frames ? nf : a.max_frames;
    if (f >= nf) return;
    const uint8_t* src = a.in + (uint64_t)fi * a.stride;
    uint8_t* dst = a.out + (uint64_t)fi * a.out_stride;
    const uint32_t mis = (uint32_t)((uintptr_t)dst & 3u);
    const int64_t lo = 4 * (int64_t)u - (int64_t)mis;
    if (lo >= (int64_t)a.nb) return;
    if (lo >= 0 && (uint64_t)lo + 4u <= a.nb) {
        const uint8_t* s = src + lo;
        uint32_t x;
        if (((uintptr_t)s & 3u) == 0) x = *(const uint32_t*)s;
        else x = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
        *(uint32_t*)(dst + lo) = x ^ dab_pad4(a, tab, (uint32_t)lo);
    } else {
        for (int64_t i = lo < 0 ? 0 : lo; i < lo + 4 && i < (int64_t)a.nb; ++i) dst[i] = src[i] ^ (uint8_t)dab_pad4(a, tab, (uint32_t)i);
    }
}

__device__ inline void dab_descramble_thread(const DabDescrArgs& a, const uint32_t* tab, uint32_t block, uint32_t tid) {
    const uint64_t t0 = (uint64_t)block * (DAB_UNITS_PER_THREAD * DAB_BLOCK) + tid;
    for (uint32_t j = 0; j < DAB_UNITS_PER_THREAD; ++j)
        if (t0 + j * DAB_BLOCK < a.units) dab_descramble_unit(a, tab, (uint32_t)(t0 + j * DAB_BLOCK));
}

__global__ void __launch_bounds__(DAB_BLOCK) dab_descramble_kernel(DabDescrArgs a) {
    __shared__ uint32_t tab[DAB_PRBS_WORDS];
    if (threadIdx.x < DAB_PRBS_WORDS) tab[threadIdx.x] = DAB_PRBS.w[threadIdx.x];
    __syncthreads();
    dab_descramble_thread(a, tab, blockIdx.x, threadIdx.x);
}

inline uint64_t dab_descramble_blocks(const DabDescrArgs& a) {
    return (a.units + DAB_UNITS_PER_THREAD * DAB_BLOCK - 1) / (DAB_UNITS_PER_THREAD * DAB_BLOCK);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------

// argument rules (include/vit_hip.h): everything the host can know without reading device memory.  sb is the handle's soft_bytes
inline const char* dab_deinterleave_invalid(bool handle, size_t sb, const void* d_in, size_t row_stride, size_t frame_stride, size_t rows,
                                            size_t max_frames, const uint32_t* d_n_frames, size_t n, const int32_t* d_map, size_t spf,
                                            const void* d_hist_in, const uint32_t* d_fill_in, size_t hist_stride, const void* d_out,
                                            const uint32_t* d_n_out, const void* d_hist_out, const uint32_t* d_fill_out) {
    if (!handle || !d_in || !d_out || !d_n_out || !d_hist_out || !d_fill_out) return "NULL handle or buffer";
    if (d_hist_in && !d_fill_in) return "d_hist_in without d_fill_in";
    if (n == 0 || spf == 0) return "n_received and symbols_per_frame must be at least 1";
    if (n > 0xFFFFFFFFull / (DAB_H + 1) || spf > 0xFFFFFFFFull) return "16 * n_received and symbols_per_frame must lie below 2^32";
    if (!d_map && spf != n) return "d_source_index == NULL (the identity) needs symbols_per_frame == n_received";
    const size_t fs = frame_stride ? frame_stride : n;
    if (fs < n) return "in_frame_stride is below n_received";
    if (max_frames > 0xFFFFFFFFFFFFull / fs) return "max_frames * in_frame_stride is too large";
    if (row_stride != 0 && row_stride < max_frames * fs) return "in_row_stride is below max_frames * in_frame_stride";
    if (hist_stride != 0 && hist_stride < DAB_H * n) return "hist_row_stride is below 15 * n_received";
    if (misaligned(d_in, sb) || misaligned(d_out, sb) || misaligned(d_hist_in, sb) || misaligned(d_hist_out, sb))
        return "d_in, d_out and the histories must be aligned to the symbol type";
    if (misaligned(d_map, 4) || misaligned(d_n_frames, 4) || misaligned(d_fill_in, 4) || misaligned(d_n_out, 4) || misaligned(d_fill_out, 4))
        return "d_source_index and the count arrays must be aligned to 4 bytes";
    if (rows == 0 || max_frames == 0) return nullptr;
    if (rows > 0x7FFFFFFFu || max_frames > 0x7FFFFFFFu) return "more than 2^31 - 1 rows or frames";
    if (rows * max_frames > 0xFFFFFFFFull / spf) return "rows * max_frames * symbols_per_frame must lie below 2^32";
    const size_t rs = row_stride ? row_stride : max_frames * fs;
    const size_t in_b = extent(rows, rs, extent(max_frames, fs, n)) * sb, out_b = rows * max_frames * spf * sb;
    const size_t hist_b = extent(rows, hist_stride ? hist_stride : DAB_H * n, DAB_H * n) * sb, cnt_b = rows * sizeof(uint32_t);
    const size_t map_b = spf * sizeof(int32_t);
    if (overlap(d_out, out_b, d_in, in_b) || overlap(d_out, out_b, d_hist_in, hist_b) || overlap(d_out, out_b, d_hist_out, hist_b) ||
        overlap(d_out, out_b, d_map, map_b))
        return "d_out overlaps the input, a history or d_source_index";
    if (overlap(d_hist_out, hist_b, d_in, in_b) || overlap(d_hist_out, hist_b, d_hist_in, hist_b) || overlap(d_hist_out, hist_b, d_map, map_b))
        return "d_hist_out overlaps the input, d_hist_in or d_source_index";
    if (overlap(d_n_out, cnt_b, d_n_frames, cnt_b) || overlap(d_n_out, cnt_b, d_fill_in, cnt_b) || overlap(d_fill_out, cnt_b, d_n_frames, cnt_b) ||
        overlap(d_fill_out, cnt_b, d_fill_in, cnt_b) || overlap(d_n_out, cnt_b, d_fill_out, cnt_b))
        return "the count arrays overlap";
    return nullptr;
}

inline const char* dab_descramble_invalid(bool handle, const uint8_t* d_in, size_t stride, size_t rows, size_t max_frames,
                                          const uint32_t* d_n_frames, size_t n_bits, const uint8_t* d_out, size_t out_stride) {
    if (!handle || !d_in || !d_out) return "NULL handle, d_in or d_out";
    if (n_bits >= 0xFFFFFFFFull - 32) return "n_bits + 32 must lie below 2^32 - 1";
    const size_t nb = (n_bits + 7) / 8;
    if (stride != 0 && stride < nb) return "frame_stride_bytes does not cover n_bits";
    if (out_stride != 0 && out_stride < nb) return "out_stride_bytes does not cover n_bits";
    if (rows == 0 || max_frames == 0 || n_bits == 0) return nullptr;
    if (rows > 0x7FFFFFFFu || max_frames > 0x7FFFFFFFu) return "more than 2^31 - 1 rows or frames";
    const size_t frames = rows * max_frames, s_in = stride ? stride : nb, s_out = out_stride ? out_stride : nb;
    if (frames > 0xFFFFFFFFull / (nb / 4 + 2)) return "rows * max_frames * (ceil(n_bits / 32) + 2) must lie below 2^32";
    if (d_in == d_out ? s_in != s_out : overlap(d_out, extent(frames, s_out, nb), d_in, extent(frames, s_in, nb)))
        return "d_out overlaps d_in without being equal to it at equal strides";
    if (overlap(d_out, extent(frames, s_out, nb), d_n_frames, rows * sizeof(uint32_t))) return "d_out overlaps d_n_frames";
    return nullptr;
}

// ---- launchers (hipGetLastError() after them: 0 / -1) ---------------------------------------------------------------------------

inline int dab_launch_deinterleave(const DabDeintArgs& a, size_t soft_bytes, hipStream_t st) {
    const dim3 grid((unsigned)dab_deinterleave_blocks(a));
    if (soft_bytes == 2) hipLaunchKernelGGL(dab_deinterleave_kernel<int16_t>, grid, dim3(DAB_BLOCK), 0, st, a);
    else hipLaunchKernelGGL(dab_deinterleave_kernel<int8_t>, grid, dim3(DAB_BLOCK), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

inline int dab_launch_descramble(const DabDescrArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(dab_descramble_kernel, dim3((unsigned)dab_descramble_blocks(a)), dim3(DAB_BLOCK), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace vit
