// dvbt_host_check -- the source of the DVB-T inner de-interleaver (viterbidecodercpp_amd/csrc/kernels_dvbt.hpp) compiled for the HOST with
// the HIP built-ins stubbed (hip_stub/hip/hip_runtime.h), as a program of its own for the address and undefined-behaviour sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Itests/cpp/hip_stub -o dvbt_host_check dvbt_host_check.cpp
//   ./dvbt_host_check [shapes = 90] [seed = 1]
// It checks, with no GPU: the compile-time tables against H built from lists of bits, with the check values of include/vit_hip.h; the
// multiply-and-shift divisions over every value a unit can hold; the workgroup remap as a bijection onto (row, symbol, unit) at the units
// of every mode, several rows and symbols and every remainder of the block count mod 8; every INVALID_ARG case of the
// argument rule and the zero-work cases; and random shapes of every mode, v, rate and symbol width whose input ends its heap block and
// whose output rows sit in a pitch with guard elements: every thread of the grid runs through the kernel's own functions, and every
// byte of the output buffer is compared with the transmit side walked literally -- puncture, demultiplex, bit-interleave, symbol-
// interleave a stream of labels, then look every label up.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../viterbidecodercpp_amd/csrc/kernels_dvbt.hpp"

static uint64_t rng_state = 1;
static uint64_t rnd() {                                            // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t below(uint64_t n) { return rnd() % n; }

static const int TAPS[3][4] = {{0, 3, -1, -1}, {0, 2, -1, -1}, {0, 1, 4, 6}};
static const int WIRES[3][12] = {{0, 7, 5, 1, 8, 2, 6, 9, 3, 4}, {7, 10, 5, 8, 1, 2, 4, 9, 0, 3, 6}, {5, 11, 3, 0, 10, 8, 6, 9, 2, 4, 1, 7}};
static const uint32_t CHECK8[3][8] = {{0, 1024, 16, 1025, 128, 1056, 2, 1280}, {0, 2048, 64, 2176, 1024, 2080, 256, 2050}, {0, 4096, 128, 4128, 2048, 4104, 1, 5120}};
static const uint32_t CHECKSUM[3] = {52702, 9494, 57713};
// what a period sends, in order: output (1 = X, 0 = Y) and step
static const int SENT_N[5] = {2, 3, 4, 6, 8}, PERIOD[5] = {1, 2, 3, 5, 7};
static const int SENT[5][8][2] = {{{1, 0}, {0, 0}}, {{1, 0}, {0, 0}, {0, 1}}, {{1, 0}, {0, 0}, {0, 1}, {1, 2}},
                                  {{1, 0}, {0, 0}, {0, 1}, {1, 2}, {0, 3}, {1, 4}}, {{1, 0}, {0, 0}, {0, 1}, {0, 2}, {0, 3}, {1, 4}, {0, 5}, {1, 6}}};
static const int SHIFT[6] = {0, 63, 105, 42, 21, 84};

// H from lists of bits: R' as an array, the new bit in front, the wiring bit by bit
static std::vector<uint32_t> rule_h(int mode) {
    const int nr = 11 + mode, mmax = 2048 << mode, nmax = 1512 << mode;
    std::vector<int> rp(nr - 1, 0);                                // rp[b] = bit b of R'
    std::vector<uint32_t> h;
    for (int i = 0; i < mmax; ++i) {
        if (i == 2) rp[0] = 1;
        else if (i > 2) {
            int bit = 0;
            for (int t = 0; t < 4; ++t) if (TAPS[mode][t] >= 0) bit ^= rp[TAPS[mode][t]];
            rp.erase(rp.begin());
            rp.push_back(bit);
        }
        uint32_t r = 0;
        for (int t = 0; t < nr - 1; ++t) if (rp[nr - 2 - t]) r += 1u << WIRES[mode][t];
        const uint32_t hq = (i % 2) * (1u << (nr - 1)) + r;
        if (hq < (uint32_t)nmax) h.push_back(hq);
    }
    return h;
}

// where[n * 2 + o] of one symbol: the element [carrier][e] it was sent as, or -1
static std::vector<int64_t> rule_symbol(const std::vector<uint32_t>& h, int v, int rate, int odd) {
    const int nmax = (int)h.size(), k = PERIOD[rate], steps = nmax * v / (k + 1) * k;
    std::vector<int64_t> sent;                                     // the label 2 n + o of every punctured bit, in order
    for (int n0 = 0; n0 < steps; n0 += k)
        for (int s = 0; s < SENT_N[rate]; ++s) sent.push_back(2 * (n0 + SENT[rate][s][1]) + SENT[rate][s][0]);
    std::vector<std::vector<int64_t>> b(v, std::vector<int64_t>(nmax)), a(v, std::vector<int64_t>(nmax));
    for (int di = 0; di < nmax * v; ++di) {
        const int r = di % v, e = r / (v / 2) + 2 * (r % (v / 2));
        b[e][di / v] = sent[di];
    }
    for (int e = 0; e < v; ++e)
        for (int q = 0; q < nmax; ++q) a[e][q] = b[e][q / 126 * 126 + (q % 126 + SHIFT[e]) % 126];
    std::vector<int64_t> where(2 * steps, -1);
    for (int q = 0; q < nmax; ++q)
        for (int e = 0; e < v; ++e) {
            const int carrier = odd ? q : (int)h[q], cell = odd ? (int)h[q] : q;      // even: y[H(q)] = y'[q]; odd: y[q] = y'[H(q)]
            where[a[e][cell]] = (int64_t)carrier * v + e;
        }
    return where;
}

static int tables() {
    for (int mode = 0; mode < 3; ++mode) {
        const std::vector<uint32_t> h = rule_h(mode);
        const uint32_t nmax = 1512u << mode;
        if (h.size() != nmax) { printf("MISMATCH mode %d: %zu carriers\n", mode, h.size()); return 1; }
        uint64_t sum = 0;
        for (uint32_t q = 0; q < nmax; ++q) {
            const uint16_t* t = vit::dvbt_table(mode, 0);
            const uint16_t* inv = vit::dvbt_table(mode, 1);
            if (t[q] != h[q] || inv[h[q]] != q) { printf("MISMATCH mode %d: H(%u) = %u, rule %u, inverse %u\n", mode, q, t[q], h[q], inv[h[q]]); return 1; }
            if (q < 8 && h[q] != CHECK8[mode][q]) { printf("MISMATCH mode %d: H(%u) = %u\n", mode, q, h[q]); return 1; }
            sum += (uint64_t)q * h[q];
        }
        if (sum % 65521 != CHECKSUM[mode]) { printf("MISMATCH mode %d: checksum %llu\n", mode, (unsigned long long)(sum % 65521)); return 1; }
    }
    for (uint32_t d = 1; d <= 7; ++d)
        for (uint32_t x = 0; x < 504 * 6 + 8; ++x)
            if (((x * vit::dvbt_magic(d)) >> 16) != x / d) { printf("MISMATCH: %u / %u by the multiply\n", x, d); return 1; }
    for (uint32_t blocks : {1u, 3u, 7u, 8u, 9u, 12u, 100u, 1001u}) {                   // the remap is a bijection onto the units
        vit::DvbtArgs a{};
        a.blocks = blocks; a.units = 1; a.n_sym = blocks; a.rows = 1;
        std::vector<int> seen(blocks, 0);
        for (uint32_t b = 0; b < blocks; ++b) {
            const vit::DvbtPlace p = vit::dvbt_place(a, b);
            if (p.row != 0 || p.unit != 0 || p.y >= blocks || seen[p.y]++) { printf("MISMATCH: remap of %u blocks at %u\n", blocks, b); return 1; }
        }
    }
    // the same with the units of a real mode, several rows and symbols: every (row, y, unit) exactly once.  The shapes of
    // tests/test_gpu_dvbt_edges.py first -- blocks & 7 takes every value 0 .. 7, blocks below 8 and from 64 on -- then more of 4k and 8k
    static const uint32_t SHAPES[][3] = {{3, 1, 1}, {3, 5, 1}, {3, 7, 1}, {3, 3, 5}, {3, 2, 4}, {3, 9, 3}, {3, 11, 5}, {3, 64, 1}, {3, 67, 3},
                                         {6, 1, 1}, {6, 3, 3}, {12, 1, 1}, {3, 2, 3}, {3, 13, 6}, {6, 5, 3}, {6, 7, 2}, {6, 13, 9}, {12, 2, 68}, {12, 5, 3}, {12, 7, 5}};
    uint32_t low = 0;
    for (const auto& s : SHAPES) {
        vit::DvbtArgs a{};
        a.units = s[0]; a.rows = s[1]; a.n_sym = s[2]; a.blocks = s[0] * s[1] * s[2];
        low |= 1u << (a.blocks & 7u);
        std::vector<int> seen(a.blocks, 0);
        for (uint32_t b = 0; b < a.blocks; ++b) {
            const vit::DvbtPlace p = vit::dvbt_place(a, b);
            if (p.row >= a.rows || p.y >= a.n_sym || p.unit >= a.units || seen[(p.row * a.n_sym + p.y) * a.units + p.unit]++) {
                printf("MISMATCH: remap of %u rows x %u symbols x %u units at block %u: row %u y %u unit %u\n", s[1], s[2], s[0], b, p.row, p.y, p.unit);
                return 1;
            }
        }
    }
    if (low != 0xFFu) { printf("MISMATCH: the remap shapes leave a remainder out: %02x\n", low); return 1; }
    return 0;
}

#define WANT(expr, bad)                                                                     \
    do {                                                                                    \
        const char* why_ = (expr);                                                          \
        if ((why_ != nullptr) != (bad)) { printf("MISMATCH line %d: %s\n", __LINE__, why_ ? why_ : "accepted"); return 1; } \
    } while (0)

static int arguments() {
    alignas(8) static uint8_t in[8], out[8];
    uint8_t* far = (uint8_t*)(uintptr_t)0x100000000000ull;                             // addresses only: the rule reads no memory
    uint32_t* pa = (uint32_t*)(far + 0x40000000000ull);
    uint32_t* pb = pa + 1024;
    const uint8_t* big_in = far + 0x10000000000ull;
    using vit::dvbt_invalid;
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 3, 2, 0, 2, 0, pa, pb, far, 0), false);
    WANT(dvbt_invalid(false, 2, 2, big_in, 0, 3, 2, 0, 2, 0, pa, pb, far, 0), true);           // NULL handle
    WANT(dvbt_invalid(true, 2, 2, nullptr, 0, 3, 2, 0, 2, 0, pa, pb, far, 0), true);           // NULL input
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 3, 2, 0, 2, 0, pa, pb, nullptr, 0), true);        // NULL output
    WANT(dvbt_invalid(true, 3, 2, big_in, 0, 3, 2, 0, 2, 0, pa, pb, far, 0), true);            // R != 2
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 3, 2, 3, 2, 0, pa, pb, far, 0), true);            // mode
    for (unsigned v : {0u, 1u, 3u, 5u, 7u, 8u}) WANT(dvbt_invalid(true, 2, 2, big_in, 0, 3, 2, 0, v, 0, pa, pb, far, 0), true);
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 3, 2, 0, 2, 5, pa, pb, far, 0), true);            // rate
    WANT(dvbt_invalid(true, 2, 2, big_in + 1, 0, 3, 2, 0, 2, 0, pa, pb, far, 0), true);        // input not aligned to soft16
    WANT(dvbt_invalid(true, 2, 1, big_in + 1, 0, 3, 2, 0, 2, 0, pa, pb, far, 0), false);       // soft8: any address
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 3, 2, 0, 2, 0, pa, pb, far + 2, 0), true);        // output not aligned to a dword
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 3, 2, 0, 2, 0, (uint32_t*)((uint8_t*)pa + 2), pb, far, 0), true);
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 3, 2, 0, 2, 0, pa, (uint32_t*)((uint8_t*)pb + 1), far, 0), true);
    WANT(dvbt_invalid(true, 2, 1, big_in, 0, 3, 2, 0, 2, 0, pa, pb, far, 3025), true);         // soft8: odd pitch, several rows
    WANT(dvbt_invalid(true, 2, 1, big_in, 0, 1, 2, 0, 2, 0, pa, pb, far, 3025), false);        //        one row: never used
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 3, 2, 0, 2, 0, pa, pb, far, 3025), false);        // soft16: any pitch
    WANT(dvbt_invalid(true, 2, 2, big_in, 6047, 3, 2, 0, 2, 0, pa, pb, far, 0), true);         // input stride below the row
    WANT(dvbt_invalid(true, 2, 2, big_in, 6048, 3, 2, 0, 2, 0, pa, pb, far, 0), false);
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 3, 2, 0, 2, 0, pa, pb, far, 3023), true);         // output stride below the row
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 3, 2, 0, 2, 0, pa, pb, far, 3024), false);
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 1, 0x100000000ull / 3024 + 1, 0, 2, 0, pa, pb, far, 0), true);        // n_sym Nmax v >= 2^32
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 0x100000000ull, 1, 0, 2, 0, pa, pb, far, 0), true);                    // rows >= 2^32
    WANT(dvbt_invalid(true, 2, 2, big_in, 0x100000000ull, 2, 1, 0, 2, 0, pa, pb, far, 0), true);                    // a stride >= 2^32
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 2, 1, 0, 2, 0, pa, pb, far, 0x100000000ull), true);
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 800000, 1, 2, 6, 0, nullptr, nullptr, far, 0), true);                  // 2^32 dwords of input
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 2000000, 1, 0, 2, 4, nullptr, nullptr, far, 0), true);                 // 2^32 dwords of output alone
    WANT(dvbt_invalid(true, 2, 1, big_in, 0, 1000000, 1, 0, 2, 0, nullptr, nullptr, far, 0), false);
    WANT(dvbt_invalid(true, 2, 2, far + 4, 0, 3, 2, 0, 2, 0, pa, pb, far, 0), true);           // output overlaps input
    WANT(dvbt_invalid(true, 2, 2, far + 2 * 2 * 3 * 3024, 0, 3, 2, 0, 2, 0, pa, pb, far, 0), false);   // input right behind it
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 3, 2, 0, 2, 0, (uint32_t*)(far + 8), pb, far, 0), true);  // output overlaps a counter
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 3, 2, 0, 2, 0, pa, (uint32_t*)(far + 8), far, 0), true);
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 3, 2, 0, 2, 0, pa, pa, far, 0), true);            // the two counters are one
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 3, 2, 0, 2, 0, pa, pa + 2, far, 0), true);
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 3, 2, 0, 2, 0, pa, pa + 3, far, 0), false);
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 3, 2, 0, 2, 0, pa, (uint32_t*)(big_in + 8), far, 0), true);   // the written counter overlaps input
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 3, 2, 0, 2, 0, nullptr, nullptr, far, 0), false); // no counters
    WANT(dvbt_invalid(true, 2, 2, big_in, 0, 3, 2, 0, 2, 0, nullptr, pb, far, 0), false);      // the scalar, counted on
    // no work: rows = 0 or n_sym = 0 is accepted whatever the strides, and still refuses what needs no shape
    WANT(dvbt_invalid(true, 2, 2, in, 1, 0, 5, 0, 2, 0, nullptr, nullptr, out, 1), false);
    WANT(dvbt_invalid(true, 2, 2, in, 1, 5, 0, 2, 6, 4, nullptr, nullptr, out, 1), false);
    WANT(dvbt_invalid(true, 2, 2, in, 1, 0, 0, 2, 6, 5, nullptr, nullptr, out, 1), true);
    WANT(dvbt_invalid(false, 2, 2, in, 1, 0, 0, 2, 6, 4, nullptr, nullptr, out, 1), true);
    return 0;
}

template <class soft_t>
static int shape(int it, const std::vector<uint32_t>* h) {
    const unsigned mode = (unsigned)(it % 3), v = 2 + 2 * (unsigned)((it / 3) % 3), rate = (unsigned)((it / 9) % 5);
    const uint64_t rows = 1 + below(3), n_sym = 1 + below(mode == 2 ? 2 : 3);
    const uint64_t cell = (uint64_t)(1512u << mode) * v, sps = vit::dvbt_steps_per_symbol(mode, v, rate);
    const uint64_t is_arg = below(2) ? 0 : n_sym * cell + below(9), is = is_arg ? is_arg : n_sym * cell;
    uint64_t os_arg = below(2) ? 0 : n_sym * sps + below(9);
    if (sizeof(soft_t) == 1 && rows > 1) os_arg += os_arg & 1;
    const uint64_t os = os_arg ? os_arg : n_sym * sps;
    const bool counters = below(2);
    const unsigned parity = (unsigned)below(4);
    std::vector<uint32_t> pin(rows), pout(rows, 0x5A5A5A5Au);
    for (auto& p : pin) p = (uint32_t)rnd();
    const uint64_t n_in = (rows - 1) * is + n_sym * cell, n_out = 2 * rows * os;
    soft_t* in = (soft_t*)malloc(n_in * sizeof(soft_t));           // ends with the last element a thread may read
    for (uint64_t i = 0; i < n_in; ++i) in[i] = (soft_t)rnd();
    soft_t* out = (soft_t*)malloc(n_out * sizeof(soft_t));
    memset(out, 0x5A, n_out * sizeof(soft_t));
    if (const char* why = vit::dvbt_invalid(true, 2, sizeof(soft_t), in, is_arg, rows, n_sym, mode, v, rate, counters ? pin.data() : nullptr,
                                            pout.data(), out, os_arg)) {
        printf("MISMATCH shape %d refused: %s\n", it, why);
        return 1;
    }
    const vit::DvbtArgs a = vit::dvbt_args(in, is_arg, rows, n_sym, mode, v, rate, parity, counters ? pin.data() : nullptr, pout.data(), out, os_arg);
    uint16_t lds[vit::DVBT_UNIT];
    for (uint32_t b = 0; b < a.blocks; ++b) {
        const vit::DvbtPlace p = vit::dvbt_place(a, b);
        for (uint32_t t = 0; t < vit::DVBT_BLOCK; ++t) vit::dvbt_load(a, p, lds, t, vit::DVBT_BLOCK);
        for (uint32_t t = 0; t < vit::DVBT_BLOCK; ++t) vit::dvbt_store<soft_t>(a, p, lds, t, vit::DVBT_BLOCK);
    }
    std::vector<int64_t> where[2] = {rule_symbol(h[mode], v, rate, 0), rule_symbol(h[mode], v, rate, 1)};
    std::vector<soft_t> want(n_out);
    memset(want.data(), 0x5A, n_out * sizeof(soft_t));
    for (uint64_t r = 0; r < rows; ++r) {
        const uint32_t first = counters ? pin[r] : parity;
        if (pout[r] != first + (uint32_t)n_sym) { printf("MISMATCH shape %d: counter of row %llu\n", it, (unsigned long long)r); return 1; }
        for (uint64_t y = 0; y < n_sym; ++y)
            for (uint64_t g = 0; g < 2 * sps; ++g) {
                const int64_t w = where[(first + y) & 1][g];
                want[2 * r * os + 2 * y * sps + g] = w < 0 ? (soft_t)0 : in[r * is + y * cell + w];
            }
    }
    for (uint64_t i = 0; i < n_out; ++i)
        if (out[i] != want[i]) {
            printf("MISMATCH shape %d: soft_bytes %zu mode %u v %u rate %u rows %llu n_sym %llu strides %llu %llu: element %llu got %d want %d\n", it,
                   sizeof(soft_t), mode, v, rate, (unsigned long long)rows, (unsigned long long)n_sym, (unsigned long long)is_arg,
                   (unsigned long long)os_arg, (unsigned long long)i, (int)out[i], (int)want[i]);
            return 1;
        }
    free(in); free(out);
    return 0;
}

int main(int argc, char** argv) {
    const int shapes = argc > 1 ? atoi(argv[1]) : 90;
    rng_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 1;
    if (tables() || arguments()) return 1;
    const std::vector<uint32_t> h[3] = {rule_h(0), rule_h(1), rule_h(2)};
    {                                                              // the spot rule: 2k, QPSK, 1/2, even symbol
        const std::vector<int64_t> w = rule_symbol(h[0], 2, 0, 0);
        if (w[1] != 0 || w[0] != (int64_t)h[0][63] * 2 + 1) { printf("MISMATCH: the spot rule\n"); return 1; }
    }
    for (int it = 0; it < shapes; ++it)
        if ((it / 45) % 2 ? shape<int8_t>(it, h) : shape<int16_t>(it, h)) return 1;
    printf("ok: %d shapes, the tables, the argument rule\n", shapes);
    return 0;
}
