// kernels_wifi.hpp -- the data path of the IEEE 802.11a/g OFDM PHY (clause 17; 802.11p / j at half and quarter clock) around the K = 7,
// R = 1/2 decode: vit_hip_wifi_deinterleave_batch, vit_hip_wifi_signal_batch, vit_hip_wifi_data_batch.
//   wifi_deinterleave_kernel<soft_t>   A gather: every OUTPUT (frame f, trellis step n, polynomial o) finds its soft bit in closed form.
//                       q = 2 n + o is its index in the mother code stream; the puncturing pattern of the frame's rate turns q into the
//                       index c of the punctured stream (1/2: c = q; 2/3: of four the fourth is missing, c = 3 (q / 4) + q % 4; 3/4: of
//                       six the fourth and fifth, c = 4 (q / 6) + (0, 1, 2, -, -, 3)[q % 6]) or into the erasure 0; c = y N_CBPS + k
//                       names OFDM symbol y and de-interleaved place k, which the transmitter sent as bit j of the symbol: with
//                       i = (N_CBPS / 16) (k mod 16) + k / 16 -- so 16 i / N_CBPS = k mod 16 -- j = s (i / s) + (i + N_CBPS - k mod 16)
//                       mod s.  N_CBPS and s are template constants of a four-way switch on the rate pair: no division by a variable
//                       but the two that find (f, n).  Rate and counts are per frame and read from the device; a frame's limits are
//                       worked out when the thread enters it.  Nothing is zeroed first and no table is built.
//                       Stores: the output [F][S][2] is one dense array of F 2S elements at a 4-byte aligned address.  A thread owns the
//                       4 / sizeof(soft_t) consecutive elements of one dword (at soft8 they may belong to two frames) and stores them
//                       as one dword; the at most 4 / sizeof(soft_t) - 1 elements behind the last whole dword are stored one by one by
//                       threads of block 0.  Loads: one element each.
//   wifi_signal_kernel  A thread per frame: the 18 decoded bits of the SIGNAL field as three bytes, the rate pattern through a 16-entry
//                       table held in a 64-bit constant, LENGTH by a 12-bit reversal, the parity by a popcount.
//   wifi_data_kernel    Descrambling, PSDU octets and the FCS of every frame at its own LENGTH in one pass.  A frame is owned by a
//                       group of G lanes (a power of two, 1 .. 64, from the longest PSDU the call allows: crc_geometry of
//                       kernels_crc.hpp), a wave carries 64 / G frames.  Every lane reads the frame's first two bytes: the first seven
//                       decoded bits are the scrambler's sequence itself.  From them it unrolls the 127-bit sequence, a byte a step
//                       with the squared recurrence p[t] = p[t-8] ^ p[t-14], into four dwords plus the dword that wraps (bits 128 ..
//                       159 are bits 1 .. 32), so the 32 bits at any t mod 127 are one funnel shift of two of them, picked by
//                       masks.  The message of the FCS -- PSDU octets 0 .. len - 4 in transmit order -- is right-aligned in G
//                       chunks of C bytes: lane j loads its words by the guarded loads of kernels_crc.hpp, XORs the sequence off,
//                       stores the word bit-reversed (PSDU octets are LSB-first, decoded bytes MSB-first: one v_bfrev_b32 a dword) and
//                       reduces it from a zero register with the slice-by-4 tables in LDS; lanes wholly in front of the message do
//                       nothing.  init = 0xFFFFFFFF enters by linearity as an XOR into the message's first 32 bits, so no power of x
//                       depends on the frame's length; log2 G combine steps with the host constants x^(8 C 2^s).  The group's lane 0
//                       descrambles and stores the four FCS octets (or all of a PSDU shorter than four) and writes the status.
// The FCS runs as the NON-reflected CRC-32 over transmit-order bits; zlib's value is its 32-bit reversal, and so is the syndrome.
// Everything but the exchange itself is plain C++ in device functions that take (block, thread), and the table build strides by
// blockDim.x between barriers: the source also runs on the host (tests/cpp/wifi_host_check.cpp).  Included only from vit_wifi.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vit_hip.h"
#define VIT_CRC_DEVICE_FUNCTIONS_ONLY
#include "kernels_crc.hpp"

namespace vit {

constexpr uint32_t WIFI_BLOCK = 256;
constexpr uint32_t WIFI_MAX_CBPS = 288;
constexpr uint32_t WIFI_FCS_POLY = 0x04C11DB7u;

// ---- rates ----------------------------------------------------------------------------------------------------------------------------

struct WifiRate { uint32_t ncbps, ndbps, kind; };                  // kind 0: rate 1/2, 1: 2/3, 2: 3/4
__host__ __device__ inline WifiRate wifi_rate(uint32_t m) {       // m <= 7
    const uint32_t p = m >> 1, nbpsc = p == 3u ? 6u : 1u << p;
    WifiRate r;
    r.ncbps = 48u * nbpsc;
    r.kind = (m & 1u) ? 2u : (m == 6u ? 1u : 0u);
    r.ndbps = r.kind == 0u ? r.ncbps / 2u : r.kind == 1u ? r.ncbps / 3u * 2u : r.ncbps / 4u * 3u;
    return r;
}

// ---- de-interleaver -------------------------------------------------------------------------------------------------------------------

struct WifiDeintArgs {
    const void* in;                  // soft_t, frame f at f * stride
    void* out;                       // soft_t [frames][S][2], 4-byte aligned
    const uint32_t* rate;            // entry f at f * count_stride, or null: the scalar
    const uint32_t* n_sym;           // or null: max_sym
    const uint32_t* n_steps;         // or null: n_sym * N_DBPS
    uint64_t stride, count_stride;
    uint32_t rate_all, max_sym, S, n2;         // n2 = 2 S
    uint64_t total;                  // frames * n2 < 2^32 * VEC
    uint32_t groups, tail;           // whole dwords; elements behind them
};

// place c of the punctured stream -> element of the frame
template <uint32_t NCBPS, uint32_t S_>
__host__ __device__ inline uint32_t wifi_source_of(uint32_t c) {
    const uint32_t y = c / NCBPS, k = c - y * NCBPS, col = k & 15u;
    const uint32_t i = (NCBPS / 16u) * col + (k >> 4);
    const uint32_t j = S_ * (i / S_) + (i + NCBPS - col) % S_;
    return y * NCBPS + j;
}
__host__ __device__ inline uint32_t wifi_source(uint32_t m, uint32_t c) {
    switch (m >> 1) {
        case 0: return wifi_source_of<48, 1>(c);
        case 1: return wifi_source_of<96, 1>(c);
        case 2: return wifi_source_of<192, 2>(c);
        default: return wifi_source_of<288, 3>(c);
    }
}

// index q of the mother code stream -> place in the punctured stream, or 0xFFFFFFFF where nothing was sent
__host__ __device__ inline uint32_t wifi_punctured(uint32_t kind, uint32_t q) {
    if (kind == 0u) return q;
    if (kind == 1u) {
        const uint32_t r = q & 3u;
        return r == 3u ? 0xFFFFFFFFu : 3u * (q >> 2) + r;
    }
    const uint32_t g = q / 6u, r = q - 6u * g;
    return r == 3u || r == 4u ? 0xFFFFFFFFu : 4u * g + (r == 5u ? 3u : r);
}

// what frame f is: its rate (8: erased whole) and the steps in front of the erasures
struct WifiFrame { uint32_t m, kind, n_steps; };
__device__ inline WifiFrame wifi_frame(const WifiDeintArgs& a, uint64_t f) {
    WifiFrame fr;
    fr.m = a.rate ? a.rate[f * a.count_stride] : a.rate_all;
    fr.kind = 0; fr.n_steps = 0;
    if (fr.m > 7u) { fr.m = 8u; return fr; }
    const WifiRate r = wifi_rate(fr.m);
    fr.kind = r.kind;
    uint32_t ns = a.n_sym ? a.n_sym[f * a.count_stride] : a.max_sym;
    ns = ns < a.max_sym ? ns : a.max_sym;
    const uint32_t lim = ns * r.ndbps;                             // max_sym * 288 < 2^32
    uint32_t st = a.n_steps ? a.n_steps[f * a.count_stride] : lim;
    st = st < lim ? st : lim;
    fr.n_steps = st < a.S ? st : a.S;
    return fr;
}

// out[f][e / 2][e % 2]
template <class soft_t>
__device__ inline soft_t wifi_output(const WifiDeintArgs& a, const WifiFrame& fr, uint64_t f, uint32_t e) {
    if ((e >> 1) >= fr.n_steps) return (soft_t)0;
    const uint32_t c = wifi_punctured(fr.kind, e);
    if (c == 0xFFFFFFFFu) return (soft_t)0;
    return ((const soft_t*)a.in)[f * a.stride + wifi_source(fr.m, c)];
}

// what thread `tid` of block `block` does
template <class soft_t>
__device__ inline void wifi_deint_thread(const WifiDeintArgs& a, uint32_t block, uint32_t tid) {
    constexpr uint32_t VEC = 4u / sizeof(soft_t);
    soft_t* out = (soft_t*)a.out;
    const uint32_t G = block * WIFI_BLOCK + tid;
    if (G < a.groups) {
        const uint64_t g = (uint64_t)G * VEC;
        uint64_t f = g / a.n2;
        uint32_t e = (uint32_t)(g - f * a.n2), word = 0;
        WifiFrame fr = wifi_frame(a, f);
#pragma unroll
        for (uint32_t v = 0; v < VEC; ++v) {
            const soft_t s = wifi_output<soft_t>(a, fr, f, e);
            word |= ((uint32_t)s & (0xFFFFFFFFu >> (32u - 8u * sizeof(soft_t)))) << (8u * sizeof(soft_t) * v);
            if (++e == a.n2 && v + 1 < VEC) { e = 0; ++f; fr = wifi_frame(a, f); }     // soft8 with S odd: f + 1 exists, the dword is whole
        }
        __builtin_memcpy(__builtin_assume_aligned(out + g, 4), &word, 4);
    }
    if (block == 0 && tid < a.tail) {
        const uint64_t g = a.total - a.tail + tid, f = g / a.n2;
        out[g] = wifi_output<soft_t>(a, wifi_frame(a, f), f, (uint32_t)(g - f * a.n2));
    }
}

template <class soft_t>
__global__ void __launch_bounds__(WIFI_BLOCK) wifi_deinterleave_kernel(WifiDeintArgs a) {
    wifi_deint_thread<soft_t>(a, blockIdx.x, threadIdx.x);
}

// the kernel arguments of a call the argument rule has accepted: frames, max_sym, S >= 1, frames * 2 S elements in fewer than 2^32 dwords
inline WifiDeintArgs wifi_deint_args(const void* d_in, size_t in_frame_stride, size_t frames, size_t max_sym, unsigned rate,
                                     const uint32_t* d_rate, const uint32_t* d_n_sym, const uint32_t* d_n_steps, size_t count_stride, size_t S,
                                     void* d_out, size_t soft_bytes) {
    WifiDeintArgs a{};
    a.in = d_in; a.out = d_out; a.rate = d_rate; a.n_sym = d_n_sym; a.n_steps = d_n_steps;
    a.stride = in_frame_stride ? in_frame_stride : max_sym * WIFI_MAX_CBPS;
    a.count_stride = count_stride ? count_stride : 1;
    a.rate_all = rate; a.max_sym = (uint32_t)max_sym; a.S = (uint32_t)S; a.n2 = 2u * a.S;
    a.total = (uint64_t)frames * a.n2;
    const uint32_t vec = 4u / (uint32_t)soft_bytes;
    a.groups = (uint32_t)(a.total / vec);
    a.tail = (uint32_t)(a.total - (uint64_t)a.groups * vec);
    return a;
}

// in 64 bits: groups may reach 2^32 - 1
inline uint32_t wifi_deint_blocks(const WifiDeintArgs& a) { return a.groups ? (uint32_t)(((uint64_t)a.groups + WIFI_BLOCK - 1) / WIFI_BLOCK) : 1u; }

// ---- SIGNAL ---------------------------------------------------------------------------------------------------------------------------

struct WifiSignalArgs {
    const uint8_t* in;               // frame f at f * stride: 3 bytes
    vit_hip_wifi_signal* out;        // [frames]
    uint64_t stride, frames;
};

// R1 R2 R3 R4 as a number, R1 highest -> rate index; 8: no such rate.  One nibble per pattern
__host__ __device__ inline uint32_t wifi_rate_of_pattern(uint32_t pattern) {
    // 1101 -> 0, 1111 -> 1, 0101 -> 2, 0111 -> 3, 1001 -> 4, 1011 -> 5, 0001 -> 6, 0011 -> 7
    constexpr uint64_t table = (8ull << 0) | (6ull << 4) | (8ull << 8) | (7ull << 12) | (8ull << 16) | (2ull << 20) | (8ull << 24) | (3ull << 28) |
                               (8ull << 32) | (4ull << 36) | (8ull << 40) | (5ull << 44) | (8ull << 48) | (0ull << 52) | (8ull << 56) | (1ull << 60);
    return (uint32_t)(table >> (4u * (pattern & 15u))) & 15u;
}

__device__ inline vit_hip_wifi_signal wifi_signal_parse(const uint8_t* p) {
    const uint32_t w = (uint32_t)p[0] << 16 | (uint32_t)p[1] << 8 | p[2];             // decoded bit t is bit 23 - t
    vit_hip_wifi_signal s;
    s.rate_index = wifi_rate_of_pattern(w >> 20);
    uint32_t len = 0;
#pragma unroll
    for (uint32_t i = 0; i < 12; ++i) len |= ((w >> (18u - i)) & 1u) << i;            // bits 5 .. 16, LSB first
    s.length = len;
    const uint32_t reserved = (w >> 19) & 1u, parity = (uint32_t)__builtin_popcount(w >> 6) & 1u;     // bits 0 .. 17
    s.valid = s.rate_index < 8u && parity == 0u && reserved == 0u && len >= 1u ? 1u : 0u;
    s.n_steps = s.valid ? 16u + 8u * len + 6u : 0u;
    const uint32_t ndbps = s.valid ? wifi_rate(s.rate_index).ndbps : 1u;
    s.n_sym = (s.n_steps + ndbps - 1u) / ndbps;
    return s;
}

__global__ void __launch_bounds__(WIFI_BLOCK) wifi_signal_kernel(WifiSignalArgs a) {
    const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f < a.frames) a.out[f] = wifi_signal_parse(a.in + f * a.stride);
}

// ---- DATA: descramble, PSDU octets, FCS ---------------------------------------------------------------------------------------------------

struct WifiDataArgs {
    const uint8_t* in;               // frame f at f * stride: ceil(n_bits / 8) decoded bytes
    const uint32_t* length;          // entry f at f * length_stride
    uint8_t* psdu;                   // frame f at f * psdu_stride
    vit_hip_wifi_status* status;     // [frames]
    uint64_t stride, length_stride, psdu_stride, frames;
    uint32_t n_bits, nb, max_len;    // nb = ceil(n_bits / 8); max_len = min(max_length, (n_bits - 16) / 8)
    uint32_t logG, C;                // lanes of a frame = 1 << logG; bytes of a chunk, a multiple of 4
    uint32_t m[6];                   // m[s] = x^(8 C 2^s) mod P, s < logG
};

__host__ __device__ inline uint32_t wifi_bitrev32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bitreverse32(x);
#else
    x = (x >> 16) | (x << 16);
    x = ((x & 0xFF00FF00u) >> 8) | ((x & 0x00FF00FFu) << 8);
    x = ((x & 0xF0F0F0F0u) >> 4) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x & 0xCCCCCCCCu) >> 2) | ((x & 0x33333333u) << 2);
    return ((x & 0xAAAAAAAAu) >> 1) | ((x & 0x55555555u) << 1);
#endif
}

// bits 0 .. 159 of the sequence that starts with the seven bits of `seed` (p[0] highest), bit t being bit 31 - t%32 of w[t/32]
struct WifiSeq { uint32_t w0, w1, w2, w3, w4; };                   // named members: never an indexed array, so never scratch
// eight more bits by the squared recurrence p[t] = p[t-8] ^ p[t-14]; the latest bit lowest
__host__ __device__ inline uint64_t wifi_seq_byte(uint64_t acc) { return (acc << 8) | ((acc ^ (acc >> 6)) & 255u); }
__host__ __device__ inline uint64_t wifi_seq_dword(uint64_t acc) { return wifi_seq_byte(wifi_seq_byte(wifi_seq_byte(wifi_seq_byte(acc)))); }
__host__ __device__ inline WifiSeq wifi_sequence(uint32_t seed) {
    uint64_t acc = seed & 127u;
#pragma unroll
    for (uint32_t i = 0; i < 9; ++i) acc = (acc << 1) | (((acc >> 3) ^ (acc >> 6)) & 1u);     // p[t] = p[t-4] ^ p[t-7]: 16 bits
    WifiSeq q;
    acc = wifi_seq_byte(wifi_seq_byte(acc)); q.w0 = (uint32_t)acc;
    acc = wifi_seq_dword(acc); q.w1 = (uint32_t)acc;
    acc = wifi_seq_dword(acc); q.w2 = (uint32_t)acc;
    acc = wifi_seq_dword(acc); q.w3 = (uint32_t)acc;
    acc = wifi_seq_dword(acc); q.w4 = (uint32_t)acc;
    return q;
}

// the 32 bits of the sequence from position pos < 127 on, the first highest
__device__ inline uint32_t wifi_seq_window(const WifiSeq& q, uint32_t pos) {
    const uint32_t i = pos >> 5;
    const uint32_t m0 = 0u - (uint32_t)(i == 0u), m1 = 0u - (uint32_t)(i == 1u), m2 = 0u - (uint32_t)(i == 2u), m3 = 0u - (uint32_t)(i == 3u);
    const uint32_t hi = (q.w0 & m0) | (q.w1 & m1) | (q.w2 & m2) | (q.w3 & m3);      // by masks: a chain of selects becomes an indexed
    const uint32_t lo = (q.w1 & m0) | (q.w2 & m1) | (q.w3 & m2) | (q.w4 & m3);      // table in scratch
    return crc_funnel(hi, lo, pos & 31u);
}

// bytes first .. first + count - 1 of the four descrambled bytes of `word` (byte 0 highest) to PSDU octets at + first ..: PSDU octets
// are LSB-first.  No pointer is formed in front of the PSDU
__device__ inline void wifi_store_octets(uint8_t* psdu, int64_t at, uint32_t word, uint32_t first, uint32_t count) {
    const uint32_t r = wifi_bitrev32(word);                        // octet i in byte i
    if (first == 0u && count == 4u && (((uintptr_t)psdu + (uintptr_t)at) & 3u) == 0u) {
        __builtin_memcpy(__builtin_assume_aligned(psdu + at, 4), &r, 4);
        return;
    }
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i)
        if (i >= first && i < first + count) psdu[at + i] = (uint8_t)(r >> (8u * i));
}

// what global lane t works on
struct WifiDataLane {
    const uint8_t* base;             // the frame's byte 0
    uint8_t* psdu;                   // its PSDU octet 0
    uint64_t f;
    uint32_t j;                      // the lane's place in its group
    uint32_t len;                    // PSDU octets used
    uint32_t msg;                    // octets under the FCS: len - 4, 0 below 4
    uint32_t seed;
    bool active;
    WifiSeq seq;
};
__device__ inline WifiDataLane wifi_data_lane(const WifiDataArgs& a, uint64_t t) {
    WifiDataLane L;
    L.f = t >> a.logG;
    L.j = (uint32_t)t & ((1u << a.logG) - 1u);
    L.active = L.f < a.frames;
    L.base = a.in; L.psdu = a.psdu; L.len = L.msg = L.seed = 0;
    if (L.active) {
        L.base = a.in + L.f * a.stride;
        L.psdu = a.psdu + L.f * a.psdu_stride;
        const uint32_t len = a.length[L.f * a.length_stride];
        L.len = len < a.max_len ? len : a.max_len;
        L.msg = L.len >= 4u ? L.len - 4u : 0u;
        L.seed = L.base[0] >> 1;                                   // decoded bits 0 .. 6
    }
    L.seq = wifi_sequence(L.seed);
    return L;
}

// descrambled frame bits [16 + p, 16 + p + 32), p a multiple of 8 from -24 on, of which only bytes [lo, hi) of the frame are touched
__device__ inline uint32_t wifi_data_word(const WifiDataLane& L, int64_t p, int64_t lo, int64_t hi) {
    const int64_t B = 2 + (p >> 3);                                // the word's first byte in the frame: -1 at the least
    const uint32_t mis = (uint32_t)(((uintptr_t)L.base + (uintptr_t)B) & 3u);
    const int64_t off = B - (int64_t)mis;
    const uint32_t d0 = crc_load_be32(L.base, off, lo, hi), d1 = crc_load_be32(L.base, off + 4, lo, hi);
    const uint32_t pos = (uint32_t)((16 + p + 127) % 127);
    return crc_funnel(d0, d1, 8u * mis) ^ wifi_seq_window(L.seq, pos);
}

// lane j's chunk of the message: descrambled, stored as PSDU octets and reduced from a zero register, init XORed into the first 32 bits
__device__ inline uint32_t wifi_data_chunk(const WifiDataArgs& a, const uint32_t* tab, const WifiDataLane& L) {
    const uint32_t G = 1u << a.logG, words = a.C / 4u;
    const int64_t n = 8 * (int64_t)L.msg;
    const int64_t p0 = n - (int64_t)(G - L.j) * 8 * (int64_t)a.C;                      // the chunk's first bit in the message
    const uint32_t k0 = p0 < 0 ? (uint32_t)((uint64_t)(-p0) >> 5) : 0u;                // words wholly in front of the message
    if (k0 >= words || L.msg == 0u) return 0u;
    const int64_t lo = 2, hi = 2 + (int64_t)L.msg;
    int64_t p = p0 + 32 * (int64_t)k0;                                                 // -24 .. : the first word that holds message bits
    const uint32_t mis = (uint32_t)(((uintptr_t)L.base + (uintptr_t)(2 + (p >> 3))) & 3u), sh = 8u * mis;
    int64_t off = 2 + (p >> 3) - (int64_t)mis;
    uint32_t pos = (uint32_t)((16 + p + 127) % 127);
    uint32_t d0 = crc_load_be32(L.base, off, lo, hi), reg = 0;
    for (uint32_t k = k0; k < words; ++k, p += 32) {
        off += 4;
        const uint32_t d1 = crc_load_be32(L.base, off, lo, hi);
        uint32_t w = crc_funnel(d0, d1, sh) ^ wifi_seq_window(L.seq, pos);
        d0 = d1;
        pos += 32u;
        pos = pos >= 127u ? pos - 127u : pos;
        const uint32_t front = p < 0 ? (uint32_t)(-p) >> 3 : 0u;                       // bytes of the word in front of octet 0
        if (p < 0) w &= 0xFFFFFFFFu >> (uint32_t)(-p);
        wifi_store_octets(L.psdu, p >> 3, w, front, 4u - front);
        if (p < 32) w ^= p < 0 ? 0xFFFFFFFFu >> (uint32_t)(-p) : 0xFFFFFFFFu << (uint32_t)p;    // init over message bits 0 .. 31
        reg ^= w;
        reg = tab[768u + (reg >> 24)] ^ tab[512u + ((reg >> 16) & 255u)] ^ tab[256u + ((reg >> 8) & 255u)] ^ tab[reg & 255u];
    }
    return reg;
}

__device__ inline uint32_t wifi_data_combine(const WifiDataArgs& a, uint32_t mine, uint32_t theirs, uint32_t s) {
    return crc_mul(mine, a.m[s], WIFI_FCS_POLY) ^ theirs;
}

// the group's lane 0: the octets behind the message and the frame's status, from the register over the whole message
__device__ inline void wifi_data_finish(const WifiDataArgs& a, const WifiDataLane& L, uint32_t reg) {
    vit_hip_wifi_status st;
    st.length_used = L.len;
    st.seed = L.seed;
    const uint32_t b1 = a.nb > 1u ? L.base[1] : 0u;                                    // n_bits >= 16: always there
    st.service = wifi_bitrev32((((uint32_t)L.base[0] << 8 | b1) << 16) ^ (L.seq.w0 & 0xFFFF0000u));
    st.fcs_syndrome = 0xFFFFFFFFu;
    const uint32_t rest = L.len - L.msg;                                               // 4, or len below 4
    if (rest) {
        const int64_t p = 8 * (int64_t)L.msg;
        uint32_t w = wifi_data_word(L, p, 2 + (int64_t)L.msg, 2 + (int64_t)L.len);
        if (rest < 4u) w &= 0xFFFFFFFFu << (32u - 8u * rest);
        wifi_store_octets(L.psdu, (int64_t)L.msg, w, 0u, rest);
        if (L.len >= 4u) {
            if (L.msg < 4u) {                                                          // a message of n < 32 bits took the high n bits of
                uint32_t init = 0xFFFFFFFFu >> (8u * L.msg);                           // init; the low 32 - n ride n bits further
                for (uint32_t i = 0; i < 8u * L.msg; ++i) init = crc_timesx(init, WIFI_FCS_POLY);
                reg ^= init;
            }
            st.fcs_syndrome = wifi_bitrev32((reg ^ 0xFFFFFFFFu) ^ w);
        }
    }
    a.status[L.f] = st;
}

__global__ void __launch_bounds__(WIFI_BLOCK) wifi_data_kernel(WifiDataArgs a) {
    __shared__ uint32_t tab[1024];
    crc_build_tables(tab, WIFI_FCS_POLY, threadIdx.x, blockDim.x);
    const WifiDataLane L = wifi_data_lane(a, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
    uint32_t reg = L.active ? wifi_data_chunk(a, tab, L) : 0u;
    for (uint32_t s = 0; s < a.logG; ++s) reg = wifi_data_combine(a, reg, __shfl_xor(reg, 1 << s), s);
    if (L.active && L.j == 0) wifi_data_finish(a, L, reg);
}

// the kernel arguments of a call the argument rule has accepted: frames >= 1, 16 <= n_bits
inline WifiDataArgs wifi_data_args(const uint8_t* d_bytes, size_t stride, size_t frames, size_t n_bits, const uint32_t* d_length,
                                   size_t length_stride, size_t max_length, uint8_t* d_psdu, size_t psdu_stride, vit_hip_wifi_status* d_status) {
    WifiDataArgs a{};
    a.in = d_bytes; a.length = d_length; a.psdu = d_psdu; a.status = d_status;
    a.n_bits = (uint32_t)n_bits; a.nb = (uint32_t)((n_bits + 7) / 8);
    a.stride = stride ? stride : a.nb;
    a.length_stride = length_stride ? length_stride : 1;
    const size_t room = (n_bits - 16) / 8;
    a.max_len = (uint32_t)(max_length < room ? max_length : room);
    a.psdu_stride = psdu_stride ? psdu_stride : max_length;
    a.frames = frames;
    const CrcGeometry g = crc_geometry(a.max_len > 4u ? 8ull * (a.max_len - 4u) : 0ull);
    a.logG = g.logG; a.C = g.C;
    uint32_t m = crc_xpow(8ull * g.C, WIFI_FCS_POLY);
    for (uint32_t s = 0; s < g.logG; ++s, m = crc_mul(m, m, WIFI_FCS_POLY)) a.m[s] = m;
    return a;
}

inline uint64_t wifi_data_blocks(const WifiDataArgs& a) { return ((a.frames << a.logG) + WIFI_BLOCK - 1) / WIFI_BLOCK; }

// ---- host side -----------------------------------------------------------------------------------------------------------------------------

// argument rules (include/vit_hip.h): everything the host can know without reading device memory.  R and sb are the handle's
inline const char* wifi_deinterleave_invalid(bool handle, int R, size_t sb, const void* d_in, size_t stride, size_t frames, size_t max_sym,
                                             unsigned rate, const uint32_t* d_rate, const uint32_t* d_n_sym, const uint32_t* d_n_steps,
                                             size_t count_stride, size_t S, const void* d_out) {
    if (!handle || !d_in || !d_out) return "NULL handle, d_in or d_symbols_out";
    if (R != 2) return "the handle's code rate must be 1/2";
    if (!d_rate && rate > 7) return "rate must be 0 .. 7";
    if (misaligned(d_in, sb) || misaligned(d_out, 4)) return "d_in must be aligned to the symbol type, d_symbols_out to 4 bytes";
    if (misaligned(d_rate, 4) || misaligned(d_n_sym, 4) || misaligned(d_n_steps, 4)) return "d_rate, d_n_sym and d_n_steps must be aligned to 4 bytes";
    if (frames == 0) return nullptr;
    if (max_sym == 0 || S == 0) return "max_sym and S must be at least 1";
    if (max_sym > 0xFFFFFFFFull / WIFI_MAX_CBPS) return "max_sym * 288 must lie below 2^32";
    if (S >= 0x7FFFFFFFull) return "S must lie below 2^31 - 1";
    const size_t least = max_sym * (d_rate ? WIFI_MAX_CBPS : wifi_rate(rate).ncbps);
    if (stride != 0 && stride < least) return "in_frame_stride below max_sym * N_CBPS (288 with d_rate)";
    if (frames > (0xFFFFFFFFull * (4 / sb)) / (2 * S)) return "frames * 2 S symbols must fill fewer than 2^32 dwords";
    if (count_stride > 0xFFFFFFFFull || frames > 0xFFFFFFFFull) return "frames and count_stride must lie below 2^32";
    const size_t in_stride = stride ? stride : max_sym * WIFI_MAX_CBPS;
    const size_t out_b = frames * 2 * S * sb, in_b = extent(frames, in_stride, stride ? least : in_stride) * sb;
    const size_t cnt_b = extent(frames, count_stride ? count_stride : 1, 1) * sizeof(uint32_t);
    if (overlap(d_out, out_b, d_in, in_b)) return "d_symbols_out overlaps d_in";
    if (overlap(d_out, out_b, d_rate, cnt_b) || overlap(d_out, out_b, d_n_sym, cnt_b) || overlap(d_out, out_b, d_n_steps, cnt_b))
        return "d_symbols_out overlaps d_rate, d_n_sym or d_n_steps";
    return nullptr;
}

inline const char* wifi_signal_invalid(bool handle, const uint8_t* d_bytes, size_t stride, size_t frames, const vit_hip_wifi_signal* d_signal) {
    if (!handle || !d_bytes || !d_signal) return "NULL handle, d_bytes or d_signal";
    if (stride != 0 && stride < 3) return "frame_stride_bytes below 3";
    if (misaligned(d_signal, 4)) return "d_signal must be aligned to 4 bytes";
    if (frames == 0) return nullptr;
    if (frames > (uint64_t)0x7FFFFFFFu * WIFI_BLOCK) return "more than 2^31 - 1 blocks";
    if (overlap(d_signal, frames * sizeof(vit_hip_wifi_signal), d_bytes, extent(frames, stride ? stride : 3, 3))) return "d_signal overlaps d_bytes";
    return nullptr;
}

inline const char* wifi_data_invalid(bool handle, const uint8_t* d_bytes, size_t stride, size_t frames, size_t S, const uint32_t* d_length,
                                     size_t length_stride, size_t max_length, const uint8_t* d_psdu, size_t psdu_stride,
                                     const vit_hip_wifi_status* d_status) {
    if (!handle || !d_bytes || !d_length || !d_psdu || !d_status) return "NULL handle, d_bytes, d_length, d_psdu or d_status";
    if (S < 22 || S >= 0x7FFFFFFFull) return "S must be 22 .. 2^31 - 2: the SERVICE field and the tail";
    if (max_length > 0x0FFFFFFFull) return "max_length must lie below 2^28";
    const size_t n_bits = S - 6, nb = (n_bits + 7) / 8;
    if (stride != 0 && stride < nb) return "frame_stride_bytes below ceil((S - 6) / 8)";
    const size_t room = (n_bits - 16) / 8, longest = max_length < room ? max_length : room;
    if (psdu_stride != 0 && psdu_stride < longest) return "psdu_stride below the longest PSDU the call can write";
    if (misaligned(d_length, 4) || misaligned(d_status, 4)) return "d_length and d_status must be aligned to 4 bytes";
    if (frames == 0) return nullptr;
    if (length_stride > 0xFFFFFFFFull) return "length_stride must lie below 2^32";
    const uint32_t logG = crc_geometry(longest > 4 ? 8ull * (longest - 4) : 0ull).logG;
    if (frames > ((uint64_t)0x7FFFFFFFu * WIFI_BLOCK) >> logG) return "more than 2^31 - 1 blocks";
    const size_t in_b = extent(frames, stride ? stride : nb, nb), len_b = extent(frames, length_stride ? length_stride : 1, 1) * sizeof(uint32_t);
    const size_t psdu_b = longest ? extent(frames, psdu_stride ? psdu_stride : max_length, longest) : 0;
    const size_t st_b = frames * sizeof(vit_hip_wifi_status);
    if (overlap(d_psdu, psdu_b, d_bytes, in_b) || overlap(d_status, st_b, d_bytes, in_b)) return "an output overlaps d_bytes";
    if (overlap(d_psdu, psdu_b, d_length, len_b) || overlap(d_status, st_b, d_length, len_b)) return "an output overlaps d_length";
    if (overlap(d_psdu, psdu_b, d_status, st_b)) return "d_psdu overlaps d_status";
    return nullptr;
}

// ---- launchers (hipGetLastError() after each: 0 / -1) --------------------------------------------------------------------------------

inline int wifi_launch_deinterleave(const WifiDeintArgs& a, size_t soft_bytes, hipStream_t st) {
    if (soft_bytes == 2) hipLaunchKernelGGL(wifi_deinterleave_kernel<int16_t>, dim3(wifi_deint_blocks(a)), dim3(WIFI_BLOCK), 0, st, a);
    else hipLaunchKernelGGL(wifi_deinterleave_kernel<int8_t>, dim3(wifi_deint_blocks(a)), dim3(WIFI_BLOCK), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

inline int wifi_launch_signal(const WifiSignalArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(wifi_signal_kernel, dim3((unsigned)((a.frames + WIFI_BLOCK - 1) / WIFI_BLOCK)), dim3(WIFI_BLOCK), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

inline int wifi_launch_data(const WifiDataArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(wifi_data_kernel, dim3((unsigned)wifi_data_blocks(a)), dim3(WIFI_BLOCK), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace vit
