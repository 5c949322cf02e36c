// crc_host_check -- the source of crc_batch_kernel (viterbidecodercpp_amd/csrc/kernels_crc.hpp) compiled for the HOST with the HIP
// built-ins stubbed (hip_stub/hip/hip_runtime.h), one thread per block, as a program of its own for the address and
// undefined-behaviour sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Itests/cpp/hip_stub -o crc_host_check crc_host_check.cpp
//   ./crc_host_check [shapes = 600] [seed = 1]
// Every random shape puts the frames and both outputs into heap blocks that END with their last byte (the bytes in front of an odd
// base address are poisoned under the address sanitizer), runs every lane of the grid through the kernel's own device functions --
// crc_build_tables, crc_lane, crc_chunk, crc_combine, crc_finish, with the arguments crc_batch_args makes -- and compares both outputs
// whole with a bit-by-bit restatement of the rule over a 0xA5 fill.  The one part of the kernel body that stays off the host is the
// __shfl_xor exchange: here the lanes of a group are run one after the other and the partner's register is read from an array.
// In front of the shapes: the argument rule (crc_invalid) at an accepted call, at every INVALID_ARG case tests/test_gpu_crc.py sends
// through the library, and at the zero-work cases; every random shape must pass it too.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../viterbidecodercpp_amd/csrc/kernels_crc.hpp"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) __asan_poison_memory_region((p), (n))
#define UNPOISON(p, n) __asan_unpoison_memory_region((p), (n))
#else
#define POISON(p, n) ((void)0)
#define UNPOISON(p, n) ((void)0)
#endif

static uint64_t rng_state = 1;
static uint64_t rnd() {                                            // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t below(uint64_t n) { return rnd() % n; }

static uint32_t frame_bit(const uint8_t* f, uint64_t t) { return (f[t >> 3] >> (7 - (t & 7))) & 1u; }

// the rule of include/vit_hip.h, bit by bit
static uint32_t rule_crc(const vit_hip_crc_params& c, const uint8_t* f, uint64_t first, uint64_t n) {
    const uint64_t mask = (1ull << c.width) - 1;
    uint64_t reg = c.init;
    for (uint64_t k = 0; k < n; ++k) {
        const uint64_t top = (reg >> (c.width - 1)) & 1;
        reg = (reg << 1) & mask;
        if (top ^ frame_bit(f, first + k)) reg ^= c.poly;
    }
    return (uint32_t)(reg ^ c.xorout);
}

// the grid, one thread per block: what crc_batch_kernel does, with the exchange done through `regs`
static void run_kernel(const vit::CrcArgs& a) {
    static uint32_t tab[1024];
    vit::crc_build_tables(tab, a.poly, 0, 1);
    const uint32_t G = 1u << a.logG;
    std::vector<uint32_t> regs(G), next(G);
    std::vector<vit::CrcLane> lanes(G);
    const uint64_t threads = vit::crc_blocks(a) * vit::CRC_BLOCK;
    for (uint64_t t0 = 0; t0 < threads; t0 += G) {
        for (uint32_t j = 0; j < G; ++j) {
            lanes[j] = vit::crc_lane(a, t0 + j);
            regs[j] = lanes[j].active ? vit::crc_chunk(a, tab, lanes[j].base, lanes[j].j) : 0u;
        }
        for (uint32_t s = 0; s < a.logG; ++s) {
            for (uint32_t j = 0; j < G; ++j) next[j] = vit::crc_combine(a, regs[j], regs[j ^ (1u << s)], s);
            regs.swap(next);
        }
        for (uint32_t j = 0; j < G; ++j)
            if (lanes[j].active && lanes[j].j == 0) vit::crc_finish(a, lanes[j], regs[j]);
    }
}

// one call of the argument rule: the accepted base call, which a case changes in a field or two
struct RuleCall {
    bool handle = true;
    const vit_hip_crc_params* code;
    const uint8_t* frames;
    size_t stride = 8, rows = 2, mf = 3, first = 0, n = 40;
    const uint32_t *crc, *syn;
    const char* operator()() const { return vit::crc_invalid(handle, code, frames, stride, rows, mf, first, n, crc, syn); }
};

#define WANT(set, bad)                                                                      \
    do {                                                                                    \
        RuleCall k = base;                                                                  \
        set;                                                                                \
        const char* why_ = k();                                                             \
        if ((why_ != nullptr) != (bad)) { printf("MISMATCH line %d: %s\n", __LINE__, why_ ? why_ : "accepted"); return 1; } \
    } while (0)

static int arguments() {
    const size_t rows = 2, mf = 3, stride = 8;
    std::vector<uint8_t> buf(rows * mf * stride);                                      // heap blocks the rule never reads
    std::vector<uint32_t> outs(2 * rows * mf + 1);
    const uint8_t* a = buf.data();
    const uint32_t *c = outs.data(), *s = c + rows * mf;
    const vit_hip_crc_params good = {16, 0x1021, 0xFFFF, 0};
    RuleCall base;
    base.code = &good; base.frames = a; base.crc = c; base.syn = s;
    WANT((void)0, false);
    WANT(k.handle = false, true);
    WANT(k.code = nullptr, true);
    WANT(k.frames = nullptr, true);
    WANT((k.crc = nullptr, k.syn = nullptr), true);
    static const vit_hip_crc_params codes[] = {{0, 0, 0, 0}, {33, 1, 0, 0}, {8, 0x100, 0, 0}, {8, 1, 0x100, 0}, {8, 1, 0, 0x100}, {31, 0x80000000u, 0, 0}};
    for (const vit_hip_crc_params& p : codes) WANT(k.code = &p, true);
    WANT(k.stride = 6, true);                                                           // 40 + 16 bits need 7 bytes, 40 alone 5
    WANT(k.n = 49, true);
    WANT(k.first = 9, true);
    WANT((k.stride = 4, k.syn = nullptr), true);
    WANT(k.syn = c, true);                                                              // the outputs on each other, on the frames
    WANT(k.syn = c + rows * mf - 1, true);
    WANT(k.crc = (const uint32_t*)a, true);
    WANT(k.syn = (const uint32_t*)(a + rows * mf * stride - 4), true);
    WANT(k.crc = (const uint32_t*)((uintptr_t)a - 4 * rows * mf + 1), true);
    WANT(k.crc = (const uint32_t*)((uintptr_t)a - 4 * rows * mf), false);               // right in front of them
    WANT(k.rows = (size_t)1 << 31, true);
    WANT(k.mf = (size_t)1 << 31, true);
    WANT((k.rows = ((size_t)1 << 31) - 1, k.mf = ((size_t)1 << 31) - 1, k.crc = nullptr), true);
    WANT(k.n = (size_t)1 << 32, true);
    WANT(k.first = (size_t)1 << 32, true);
    WANT(k.stride = 7, false);                                                          // the edges that pass
    WANT((k.stride = 5, k.syn = nullptr), false);
    WANT((k.stride = 0, k.n = 48), false);
    WANT(k.rows = 0, false);                                                            // no work
    WANT(k.mf = 0, false);
    WANT((k.rows = 0, k.stride = 6), true);                                             // ... still refuses what needs no shape
    WANT((k.mf = 0, k.handle = false), true);
    return 0;
}

int main(int argc, char** argv) {
    const int shapes = argc > 1 ? atoi(argv[1]) : 600;
    rng_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 1;
    if (arguments()) return 1;
    static const uint64_t edges[] = {0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 136, 240, 256, 257, 264, 512, 520, 1024, 1032,
                                     2048, 2056, 4096, 4104, 8904, 32771};
    uint32_t seen_logG = 0;
    uint64_t frames_checked = 0;
    for (int it = 0; it < shapes; ++it) {
        vit_hip_crc_params c;
        c.width = 1 + (uint32_t)below(32);
        if (below(4) == 0) c.width = (uint32_t[]){1, 8, 16, 24, 31, 32}[below(6)];
        const uint64_t top = 1ull << c.width;
        c.poly = (uint32_t)below(top); c.init = (uint32_t)below(top); c.xorout = (uint32_t)below(top);
        uint64_t n_bits;
        switch (below(4)) {
            case 0: n_bits = below(80); break;
            case 1: n_bits = edges[below(sizeof(edges) / sizeof(edges[0]))]; break;
            case 2: n_bits = below(3000); break;
            default: n_bits = below(40000); break;
        }
        if (below(8) == 0) n_bits = c.width - below(2);
        const uint64_t first_bit = below(3) ? below(16) : below(300);
        const bool want_syn = below(4) != 0, want_crc = !want_syn || below(3) != 0;
        const uint64_t rows = 1 + below(3), max_frames = n_bits > 4000 ? 1 + below(3) : 1 + below(20);
        const uint64_t need = (first_bit + n_bits + (want_syn ? c.width : 0) + 7) / 8;
        const uint64_t stride_arg = below(3) == 0 ? 0 : need + below(6);
        const uint64_t stride = stride_arg ? stride_arg : need;
        const uint64_t N = rows * max_frames;
        const uint64_t in_bytes = need ? (N - 1) * stride + need : 0;
        const uint64_t lead = below(2) ? 0 : below(8);

        uint8_t* block = (uint8_t*)malloc(lead + in_bytes + (lead + in_bytes == 0));
        uint8_t* frames = block + lead;
        for (uint64_t i = 0; i < lead + in_bytes; ++i) block[i] = (uint8_t)rnd();
        POISON(block, lead);
        uint32_t* n_frames = nullptr;
        if (below(3)) {
            n_frames = (uint32_t*)malloc(rows * sizeof(uint32_t));
            for (uint64_t r = 0; r < rows; ++r)
                n_frames[r] = below(4) == 0 ? (uint32_t)rnd() : below(4) == 0 ? 0u : (uint32_t)below(max_frames + 2);
        }
        uint32_t* d_crc = want_crc ? (uint32_t*)malloc(N * sizeof(uint32_t)) : nullptr;
        uint32_t* d_syn = want_syn ? (uint32_t*)malloc(N * sizeof(uint32_t)) : nullptr;
        if (d_crc) memset(d_crc, 0xA5, N * sizeof(uint32_t));
        if (d_syn) memset(d_syn, 0xA5, N * sizeof(uint32_t));

        if (const char* why = vit::crc_invalid(true, &c, frames, stride_arg, rows, max_frames, first_bit, n_bits, d_crc, d_syn)) {
            printf("MISMATCH shape %d refused: %s\n", it, why);
            return 1;
        }
        const vit::CrcArgs a = vit::crc_batch_args(c, frames, stride_arg, rows, max_frames, n_frames, first_bit, n_bits, d_crc, d_syn);
        seen_logG |= 1u << a.logG;
        run_kernel(a);

        for (uint64_t r = 0; r < rows; ++r) {
            uint64_t nf = n_frames ? n_frames[r] : max_frames;
            nf = nf < max_frames ? nf : max_frames;
            for (uint64_t f = 0; f < max_frames; ++f) {
                const uint64_t fi = r * max_frames + f;
                uint32_t want_c = 0xA5A5A5A5u, want_s = 0xA5A5A5A5u;
                if (f < nf) {
                    const uint8_t* fr = frames + fi * stride;
                    want_c = rule_crc(c, fr, first_bit, n_bits);
                    if (want_syn) {
                        uint32_t field = 0;
                        for (uint32_t k = 0; k < c.width; ++k) field = (field << 1) | frame_bit(fr, first_bit + n_bits + k);
                        want_s = want_c ^ field;
                    }
                    ++frames_checked;
                }
                if ((d_crc && d_crc[fi] != want_c) || (d_syn && d_syn[fi] != want_s)) {
                    printf("MISMATCH shape %d: width %u poly %#x init %#x xorout %#x n_bits %llu first_bit %llu stride %llu rows %llu max_frames %llu "
                           "frame (%llu, %llu) nf %llu logG %u C %u: crc %#x want %#x, syndrome %#x want %#x\n",
                           it, c.width, c.poly, c.init, c.xorout, (unsigned long long)n_bits, (unsigned long long)first_bit,
                           (unsigned long long)stride_arg, (unsigned long long)rows, (unsigned long long)max_frames, (unsigned long long)r,
                           (unsigned long long)f, (unsigned long long)nf, a.logG, a.C, d_crc ? d_crc[fi] : 0, want_c, d_syn ? d_syn[fi] : 0,
                           want_s);
                    return 1;
                }
            }
        }
        UNPOISON(block, lead);
        free(block); free(n_frames); free(d_crc); free(d_syn);
    }
    printf("ok: %d shapes, %llu frames, group sizes seen (mask of log2 G) %#x\n", shapes, (unsigned long long)frames_checked, seen_logG);
    return 0;
}
