// kernels_dvbt.hpp -- the inner de-interleaver of DVB-T (ETSI EN 300 744 clause 4.3.4: symbol interleaver, bit interleaver, demultiplexer)
// fused with depuncturing (clause 4.3.3) in front of the K = 7, R = 1/2 decode: vit_hip_dvbt_deinterleave_batch.
//   dvbt_deinterleave_kernel<soft_t>   A gather: every OUTPUT (row, OFDM symbol y, trellis step n, polynomial o) finds its soft bit in
//                       closed form but for one table look-up.  A puncturing period of k steps sends k + 1 bits; a 64-bit constant of
//                       nibbles names, for (n mod k, o), the place in the period or "not sent" (0, the erasure).  Place di of the
//                       symbol's punctured stream is bit e of the demultiplexer's word do = di / v, e = (r / (v/2)) + 2 (r mod (v/2)) with
//                       r = di mod v; the bit interleaver put it into cell 126 (do / 126) + (do mod 126 - s_e) mod 126; the symbol
//                       interleaver sent that cell on carrier H(cell) in a symbol of even parity and H^-1(cell) in an odd one.
//                       Work is cut into UNITS of 504 cells = 4 bit-interleaver blocks: at every v and rate a unit is whole puncturing
//                       periods AND whole output dwords at both symbol widths, so a workgroup owns one unit of one symbol, needs the
//                       504 table entries of its cells and nothing else of H -- 1008 bytes of LDS, two coalesced reads --
//                       and never shares a dword with another.  The full tables H and H^-1 of the three modes (42 KB of uint16) are
//                       constants of the code object, generated at compile time by the standard's own recurrence (dvbt_perm): no
//                       workspace, nothing built at run time, no per-symbol map.  Divisions by k and v are a multiply and a shift
//                       (exact over a unit's range: tests/cpp/dvbt_host_check.cpp walks it); the only divisions by a variable are the
//                       few scalar ones that find (row, symbol, unit).
//                       Stores: one aligned dword per thread and pass -- the (Y, X) pair of a step at soft16, two steps at soft8.
//                       Loads: one element each; the v soft bits of a cell are all read by the one workgroup that owns the cell.
//                       Workgroup ids are remapped so that the units of one symbol carry the same id mod 8: they read the same cache
//                       lines of the symbol.  A speed choice alone, kept for what it measures (a fifth less time at 8k / 64-QAM,
//                       profiles/dvbt_remap_ab.txt): nothing depends on where a workgroup runs.
//                       Parity: the symbol's is (first + y) & 1, first the scalar or the row's counter; the workgroup of a row's
//                       first unit writes first + n_sym to the OTHER counter array.
// X = 171 octal is output index 1 of a step and Y = 133 octal index 0: the order of the stock code (109, 79) = (133, 171) in this
// package's convention.
// Everything is plain C++ in functions that take (workgroup, thread, threads): the source also runs on the host
// (tests/cpp/dvbt_host_check.cpp), the argument rule included.  Included only from vit_dvbt.hip.
// Out of scope: hierarchical modes, the DVB-H in-depth interleaver, OFDM demodulation, pilots, TPS decoding and demapping, DVB-T2, a
// transmitter on the card.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arg_rules.hpp"

namespace vit {

constexpr uint32_t DVBT_BLOCK = 256;
constexpr uint32_t DVBT_UNIT = 504;                                // cells of a unit: 4 bit-interleaver blocks of 126
constexpr uint32_t DVBT_MODES = 3, DVBT_RATES = 5;

// ---- the symbol permutation ---------------------------------------------------------------------------------------------------------------

template <uint32_t N>
struct DvbtPerm { uint16_t h[N], inv[N]; };                        // H(q) and H^-1(carrier)

constexpr uint32_t dvbt_nmax(uint32_t mode) { return 1512u << mode; }
constexpr uint32_t dvbt_nr(uint32_t mode) { return 11u + mode; }

// bit t of the list is for bit Nr - 2 - t of R'
struct DvbtWiring { uint32_t taps; uint8_t to[12]; };
constexpr DvbtWiring DVBT_WIRING[DVBT_MODES] = {
    {0x009u, {0, 7, 5, 1, 8, 2, 6, 9, 3, 4, 0, 0}},
    {0x005u, {7, 10, 5, 8, 1, 2, 4, 9, 0, 3, 6, 0}},
    {0x053u, {5, 11, 3, 0, 10, 8, 6, 9, 2, 4, 1, 7}},
};

template <uint32_t MODE>
constexpr DvbtPerm<dvbt_nmax(MODE)> dvbt_perm() {
    constexpr uint32_t NR = dvbt_nr(MODE), NMAX = dvbt_nmax(MODE), MMAX = 2048u << MODE;
    DvbtPerm<NMAX> p{};
    uint32_t rp = 0, q = 0;
    for (uint32_t i = 0; i < MMAX; ++i) {
        if (i == 2) rp = 1;
        else if (i > 2) {
            uint32_t t = rp & DVBT_WIRING[MODE].taps, bit = 0;
            for (; t; t &= t - 1) bit ^= 1u;
            rp = (rp >> 1) | (bit << (NR - 2));
        }
        uint32_t r = 0;
        for (uint32_t t = 0; t + 1 < NR; ++t) r |= ((rp >> (NR - 2 - t)) & 1u) << DVBT_WIRING[MODE].to[t];
        const uint32_t hq = ((i & 1u) << (NR - 1)) + r;
        if (hq < NMAX) {
            p.h[q] = (uint16_t)hq;
            p.inv[hq] = (uint16_t)q;
            ++q;
        }
    }
    return p;
}

__device__ constexpr DvbtPerm<1512> DVBT_PERM_2K = dvbt_perm<0>();
__device__ constexpr DvbtPerm<3024> DVBT_PERM_4K = dvbt_perm<1>();
__device__ constexpr DvbtPerm<6048> DVBT_PERM_8K = dvbt_perm<2>();

// H (odd = 0) or H^-1 (odd = 1) of a mode
__device__ inline const uint16_t* dvbt_table(uint32_t mode, uint32_t odd) {
    if (mode == 0u) return odd ? DVBT_PERM_2K.inv : DVBT_PERM_2K.h;
    if (mode == 1u) return odd ? DVBT_PERM_4K.inv : DVBT_PERM_4K.h;
    return odd ? DVBT_PERM_8K.inv : DVBT_PERM_8K.h;
}

// ---- puncturing ----------------------------------------------------------------------------------------------------------------------------

// steps of a period (it sends one bit more) and, nibble 2 j + o, the place in the period of output o (0 = Y, 1 = X) of its step j; 15:
// not sent.  1/2: X1 Y1; 2/3: X1 Y1 Y2; 3/4: X1 Y1 Y2 X3; 5/6: X1 Y1 Y2 X3 Y4 X5; 7/8: X1 Y1 Y2 Y3 Y4 X5 Y6 X7
constexpr uint32_t DVBT_PERIOD[DVBT_RATES] = {1, 2, 3, 5, 7};
constexpr uint64_t DVBT_PLACES[DVBT_RATES] = {
    0x01ull, 0xF201ull, 0x3FF201ull, 0x5FF43FF201ull, 0x7FF65FF4F3F201ull,
};
// s_e of the bit interleavers, a byte each
constexpr uint64_t DVBT_SHIFTS = 0ull | 63ull << 8 | 105ull << 16 | 42ull << 24 | 21ull << 32 | 84ull << 40;

inline uint32_t dvbt_steps_per_symbol(uint32_t mode, uint32_t v, uint32_t rate) {
    return dvbt_nmax(mode) * v / (DVBT_PERIOD[rate] + 1u) * DVBT_PERIOD[rate];
}

// ---- the call --------------------------------------------------------------------------------------------------------------------------------

struct DvbtArgs {
    const void* in;                  // soft_t, row r at r * in_stride: [n_sym][Nmax][v]
    void* out;                       // soft_t, row r at r * out_stride: [n_sym * steps][2]; 4-byte aligned rows
    const uint32_t* par_in;          // [rows] or null: `parity`
    uint32_t* par_out;               // [rows] or null
    uint64_t in_stride, out_stride;  // elements
    uint64_t pattern;                // DVBT_PLACES[rate]
    uint32_t rows, n_sym, parity, mode;
    uint32_t units;                  // of a symbol: Nmax / 504
    uint32_t v, half, v_magic;       // x / v == (x * v_magic) >> 16 below 504 * 6
    uint32_t k, kp1, k_magic;        // likewise x / k below a unit's steps
    uint32_t unit_steps, sym_in;     // steps of a unit: 504 v k / (k + 1); elements of a symbol: Nmax v
    uint32_t blocks;                 // rows * n_sym * units
};

// element ue of a unit's output [unit_steps][2] -> cell * 8 + e of the unit, or 0xFFFFFFFF where nothing was sent
__host__ __device__ inline uint32_t dvbt_source(const DvbtArgs& a, uint32_t ue) {
    const uint32_t n = ue >> 1, per = (n * a.k_magic) >> 16, j = n - per * a.k;
    const uint32_t pos = (uint32_t)(a.pattern >> (4u * (2u * j + (ue & 1u)))) & 15u;
    if (pos == 15u) return 0xFFFFFFFFu;
    const uint32_t di = per * a.kp1 + pos;
    const uint32_t word = (di * a.v_magic) >> 16, r = di - word * a.v;
    const uint32_t hi = r >= a.half ? 1u : 0u, e = hi + 2u * (r - (hi ? a.half : 0u));
    const uint32_t blk = word / 126u, w = word - 126u * blk;
    uint32_t c = w + 126u - ((uint32_t)(DVBT_SHIFTS >> (8u * e)) & 255u);
    c = c >= 126u ? c - 126u : c;
    return (126u * blk + c) * 8u + e;
}

struct DvbtPlace { uint32_t row, y, unit, odd, first; };
// workgroup `block` of the grid -> its unit.  Ids that agree mod 8 get consecutive units (bijective for any count)
__device__ inline DvbtPlace dvbt_place(const DvbtArgs& a, uint32_t block) {
    const uint32_t q = a.blocks >> 3, r = a.blocks & 7u, x = block & 7u;
    const uint32_t w = (x < r ? x * (q + 1u) : r * (q + 1u) + (x - r) * q) + (block >> 3);
    DvbtPlace p;
    const uint32_t s = w / a.units;
    p.unit = w - s * a.units;
    p.row = s / a.n_sym;
    p.y = s - p.row * a.n_sym;
    p.first = a.par_in ? a.par_in[p.row] : a.parity;
    p.odd = (p.first + p.y) & 1u;
    return p;
}

// the unit's 504 table entries
__device__ inline void dvbt_load(const DvbtArgs& a, const DvbtPlace& p, uint16_t* cells, uint32_t tid, uint32_t threads) {
    const uint16_t* src = dvbt_table(a.mode, p.odd) + p.unit * DVBT_UNIT;
    for (uint32_t i = tid; i < DVBT_UNIT; i += threads) cells[i] = src[i];
}

template <class soft_t>
__device__ inline void dvbt_store(const DvbtArgs& a, const DvbtPlace& p, const uint16_t* cells, uint32_t tid, uint32_t threads) {
    constexpr uint32_t VEC = 4u / sizeof(soft_t);
    const soft_t* in = (const soft_t*)a.in + (uint64_t)p.row * a.in_stride + (uint64_t)p.y * a.sym_in;
    soft_t* out = (soft_t*)a.out + (uint64_t)p.row * a.out_stride + 2ull * ((uint64_t)p.y * a.units + p.unit) * a.unit_steps;
    const uint32_t dwords = 2u * a.unit_steps / VEC;
    for (uint32_t d = tid; d < dwords; d += threads) {
        uint32_t word = 0;
#pragma unroll
        for (uint32_t i = 0; i < VEC; ++i) {
            const uint32_t src = dvbt_source(a, d * VEC + i);
            const soft_t s = src == 0xFFFFFFFFu ? (soft_t)0 : in[(uint32_t)cells[src >> 3] * a.v + (src & 7u)];
            word |= ((uint32_t)s & (0xFFFFFFFFu >> (32u - 8u * sizeof(soft_t)))) << (8u * sizeof(soft_t) * i);
        }
        __builtin_memcpy(__builtin_assume_aligned(out + (uint64_t)d * VEC, 4), &word, 4);
    }
    if (a.par_out && p.y == 0u && p.unit == 0u && tid == 0u) a.par_out[p.row] = p.first + a.n_sym;
}

template <class soft_t>
__global__ void __launch_bounds__(DVBT_BLOCK) dvbt_deinterleave_kernel(DvbtArgs a) {
    __shared__ uint16_t lds[DVBT_UNIT];
    const DvbtPlace p = dvbt_place(a, blockIdx.x);
    dvbt_load(a, p, lds, threadIdx.x, blockDim.x);
    __syncthreads();
    dvbt_store<soft_t>(a, p, lds, threadIdx.x, blockDim.x);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------

// argument rules (include/vit_hip.h): everything the host can know without reading device memory.  R and soft_bytes are the handle's
inline const char* dvbt_invalid(bool handle, int R, size_t sb, const void* d_in, size_t in_row_stride, size_t rows, size_t n_sym, unsigned mode,
                                unsigned v, unsigned rate, const uint32_t* d_parity_in, const uint32_t* d_parity_out, const void* d_out,
                                size_t out_row_stride) {
    if (!handle || !d_in || !d_out) return "NULL handle, d_in or d_symbols_out";
    if (R != 2) return "the handle's code rate must be 1/2";
    if (mode >= DVBT_MODES) return "mode must be 0 (2k), 1 (4k) or 2 (8k)";
    if (v != 2 && v != 4 && v != 6) return "v must be 2, 4 or 6";
    if (rate >= DVBT_RATES) return "rate must be 0 .. 4";
    if (misaligned(d_in, sb) || misaligned(d_out, 4)) return "d_in must be aligned to the symbol type, d_symbols_out to 4 bytes";
    if (misaligned(d_parity_in, 4) || misaligned(d_parity_out, 4)) return "d_parity_in and d_parity_out must be aligned to 4 bytes";
    if (rows == 0 || n_sym == 0) return nullptr;
    const uint64_t sym_in = (uint64_t)dvbt_nmax(mode) * v, sps = dvbt_steps_per_symbol(mode, v, rate);
    if (n_sym > 0xFFFFFFFFull / sym_in) return "n_sym * Nmax * v must lie below 2^32";
    if (rows > 0xFFFFFFFFull) return "rows must lie below 2^32";
    const uint64_t row_in = n_sym * sym_in, row_steps = n_sym * sps;
    if (in_row_stride != 0 && in_row_stride < row_in) return "in_row_stride below n_sym * Nmax * v";
    if (out_row_stride != 0 && out_row_stride < row_steps) return "out_row_stride below n_sym * steps per symbol";
    const uint64_t is = in_row_stride ? in_row_stride : row_in, os = out_row_stride ? out_row_stride : row_steps;
    if (is > 0xFFFFFFFFull || os > 0xFFFFFFFFull) return "the row strides must lie below 2^32";
    if (sb == 1 && rows > 1 && (os & 1u)) return "out_row_stride must be even at 8-bit symbols: every row starts a dword";
    const uint64_t in_el = extent(rows, is, row_in), out_el = 2 * extent(rows, os, row_steps);
    if (in_el * sb >= 4 * 0x100000000ull || out_el * sb >= 4 * 0x100000000ull) return "input and output must each fill fewer than 2^32 dwords";
    if (rows * n_sym * (dvbt_nmax(mode) / DVBT_UNIT) > 0x7FFFFFF8ull) return "more than 2^31 - 8 blocks";
    const uint64_t in_b = in_el * sb, out_b = out_el * sb, par_b = rows * 4;
    if (overlap(d_out, out_b, d_in, in_b)) return "d_symbols_out overlaps d_in";
    if (overlap(d_out, out_b, d_parity_in, par_b) || overlap(d_out, out_b, d_parity_out, par_b))
        return "d_symbols_out overlaps d_parity_in or d_parity_out";
    if (overlap(d_parity_out, par_b, d_in, in_b) || overlap(d_parity_out, par_b, d_parity_in, par_b))
        return "d_parity_out overlaps d_in or d_parity_in";
    return nullptr;
}

// x / d == (x * magic) >> 16 for x (d - 1) < 65536
constexpr uint32_t dvbt_magic(uint32_t d) { return 65536u / d + 1u; }

// the kernel arguments of a call the argument rule has accepted, rows and n_sym at least 1
inline DvbtArgs dvbt_args(const void* d_in, size_t in_row_stride, size_t rows, size_t n_sym, unsigned mode, unsigned v, unsigned rate,
                          unsigned parity, const uint32_t* d_parity_in, uint32_t* d_parity_out, void* d_out, size_t out_row_stride) {
    DvbtArgs a{};
    a.in = d_in; a.out = d_out; a.par_in = d_parity_in; a.par_out = d_parity_out;
    a.rows = (uint32_t)rows; a.n_sym = (uint32_t)n_sym; a.parity = parity; a.mode = mode;
    a.units = dvbt_nmax(mode) / DVBT_UNIT;
    a.v = v; a.half = v / 2u; a.v_magic = dvbt_magic(v);
    a.k = DVBT_PERIOD[rate]; a.kp1 = a.k + 1u; a.k_magic = dvbt_magic(a.k);
    a.pattern = DVBT_PLACES[rate];
    a.unit_steps = DVBT_UNIT * v / a.kp1 * a.k;
    a.sym_in = dvbt_nmax(mode) * v;
    a.in_stride = in_row_stride ? in_row_stride : (uint64_t)n_sym * a.sym_in;
    a.out_stride = 2ull * (out_row_stride ? out_row_stride : (uint64_t)n_sym * a.units * a.unit_steps);
    a.blocks = (uint32_t)(rows * n_sym * a.units);
    return a;
}

inline int dvbt_launch(const DvbtArgs& a, size_t soft_bytes, hipStream_t st) {
    if (soft_bytes == 2) hipLaunchKernelGGL(dvbt_deinterleave_kernel<int16_t>, dim3(a.blocks), dim3(DVBT_BLOCK), 0, st, a);
    else hipLaunchKernelGGL(dvbt_deinterleave_kernel<int8_t>, dim3(a.blocks), dim3(DVBT_BLOCK), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace vit
