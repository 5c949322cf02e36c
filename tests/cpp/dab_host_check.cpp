// dab_host_check -- the source of dab_deinterleave_kernel and dab_descramble_kernel (viterbidecodercpp_amd/csrc/kernels_dab.hpp) compiled
// for the HOST with the HIP built-ins stubbed (hip_stub/hip/hip_runtime.h), as a program of its own for the address and
// undefined-behaviour sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Itests/cpp/hip_stub -o dab_host_check dab_host_check.cpp
//   ./dab_host_check [shapes = 300] [seed = 1]
// Every random shape puts the input, the map, the counts, the histories and the outputs into heap blocks that END with their last byte
// (the elements in front of an output that starts off a dword boundary are poisoned under the address sanitizer), fills the count, fill
// and map memory with values of every size, runs every thread of the grid through the kernels' own thread functions, and compares every
// element of every output with a literal restatement of the rule over a 0x5A fill.
// In front of them: both argument rules (dab_deinterleave_invalid, dab_descramble_invalid) at an accepted call, at every INVALID_ARG
// case tests/test_gpu_dab.py sends through the library, and at the zero-work cases.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../viterbidecodercpp_amd/csrc/kernels_dab.hpp"

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

static const uint32_t DELAY[16] = {0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15};

static uint32_t odd_count(uint32_t most) {
    return below(6) == 0 ? (uint32_t)rnd() : below(5) == 0 ? 0u : (uint32_t)below(most + 3);
}

template <class soft_t>
static int deinterleave_shape(int it) {
    const uint32_t H = vit::DAB_H;
    static const uint32_t ns[] = {1, 15, 16, 17, 100, 256, 5000};
    const uint32_t n = below(2) ? ns[below(7)] : 1 + (uint32_t)below(300);
    const uint32_t rows = 1 + (uint32_t)below(4), mf = 1 + (uint32_t)below(below(3) ? 20 : 45);
    const bool with_map = below(2), with_count = below(2), with_hist = below(3) != 0;
    const uint32_t spf = with_map ? 1 + (uint32_t)below(2 * n + 9) : n;
    const uint64_t fs = n + (below(2) ? 0 : below(9)), rs = mf * fs + (below(2) ? 0 : below(9)), hs = (uint64_t)H * n + (below(2) ? 0 : below(5));
    const uint64_t in_n = (rows - 1) * rs + (mf - 1) * fs + n, hist_n = (rows - 1) * hs + (uint64_t)H * n;

    soft_t* in = (soft_t*)malloc(in_n * sizeof(soft_t));
    for (uint64_t k = 0; k < in_n; ++k) in[k] = (soft_t)rnd();
    soft_t* hist = (soft_t*)malloc(hist_n * sizeof(soft_t));
    for (uint64_t k = 0; k < hist_n; ++k) hist[k] = (soft_t)rnd();
    int32_t* map = (int32_t*)malloc(spf * sizeof(int32_t));
    for (uint32_t q = 0; q < spf; ++q) map[q] = below(8) == 0 ? (int32_t)rnd() : (int32_t)below(n + 2) - 1;
    uint32_t* count = (uint32_t*)malloc(rows * sizeof(uint32_t));
    uint32_t* fill = (uint32_t*)malloc(rows * sizeof(uint32_t));
    for (uint32_t r = 0; r < rows; ++r) { count[r] = odd_count(mf); fill[r] = odd_count(H); }
    const uint64_t total = (uint64_t)rows * mf * spf, lead = below(4 / sizeof(soft_t));
    soft_t* block = (soft_t*)malloc((lead + total) * sizeof(soft_t));
    soft_t* out = block + lead;
    memset(block, 0x5A, (lead + total) * sizeof(soft_t));
    POISON(block, lead * sizeof(soft_t));
    soft_t* hist_out = (soft_t*)malloc(hist_n * sizeof(soft_t));
    memset(hist_out, 0x5A, hist_n * sizeof(soft_t));
    uint32_t* n_out = (uint32_t*)malloc(rows * sizeof(uint32_t));
    uint32_t* fill_out = (uint32_t*)malloc(rows * sizeof(uint32_t));

    vit::DabDeintArgs a{};
    a.in = in; a.n_frames = with_count ? count : nullptr; a.map = with_map ? map : nullptr; a.hist_in = with_hist ? hist : nullptr;
    a.fill_in = with_hist ? fill : nullptr; a.out = out; a.n_out = n_out; a.hist_out = hist_out; a.fill_out = fill_out;
    a.row_stride = rs; a.frame_stride = fs; a.hist_stride = hs;
    a.rows = rows; a.max_frames = mf; a.n = n; a.spf = spf; a.total = (uint32_t)total;
    vit::dab_deinterleave_split(a, sizeof(soft_t));
    const uint64_t blocks = vit::dab_deinterleave_blocks(a);
    for (uint64_t b = 0; b < blocks; ++b)
        for (uint32_t t = 0; t < vit::DAB_BLOCK; ++t) {
            if (b < a.ob) vit::dab_output_thread<soft_t>(a, (uint32_t)b, t);
            else vit::dab_history_thread<soft_t>(a, (uint32_t)(b - a.ob), t, vit::DAB_BLOCK);
        }

    soft_t poison;
    memset(&poison, 0x5A, sizeof(poison));
    int bad = 0;
    for (uint32_t r = 0; r < rows && !bad; ++r) {
        const uint32_t nf = with_count ? (count[r] < mf ? count[r] : mf) : mf;
        const uint32_t fl = with_hist ? (fill[r] < H ? fill[r] : H) : 0;
        const uint32_t T = fl + nf, nout = T > H ? T - H : 0, keep = T < H ? T : H;
        auto S = [&](uint32_t s, uint32_t i) { return s < fl ? hist[r * hs + (uint64_t)(H - fl + s) * n + i] : in[r * rs + (uint64_t)(s - fl) * fs + i]; };
        if (n_out[r] != nout || fill_out[r] != keep) bad = 1;
        for (uint32_t k = 0; k < mf && !bad; ++k)
            for (uint32_t q = 0; q < spf; ++q) {
                soft_t want = poison;
                if (k < nout) {
                    const int64_t p = with_map ? map[q] : (int64_t)q;
                    want = p >= 0 && p < (int64_t)n ? S(k + DELAY[p & 15], (uint32_t)p) : (soft_t)0;
                }
                if (out[((uint64_t)r * mf + k) * spf + q] != want) { bad = 2; break; }
            }
        for (uint32_t h = 0; h < H && !bad; ++h)
            for (uint32_t i = 0; i < n; ++i) {
                const soft_t want = h < H - keep ? poison : S(T - (H - h), i);
                if (hist_out[r * hs + (uint64_t)h * n + i] != want) { bad = 3; break; }
            }
        for (uint64_t i = (uint64_t)H * n; r + 1 < rows && i < hs && !bad; ++i)
            if (hist_out[r * hs + i] != poison) bad = 4;
    }
    if (bad)
        printf("MISMATCH (%d) deinterleave shape %d: soft_bytes %zu n %u rows %u mf %u spf %u map %d count %d hist %d fs %llu rs %llu hs %llu lead %llu\n",
               bad, it, sizeof(soft_t), n, rows, mf, spf, with_map, with_count, with_hist, (unsigned long long)fs, (unsigned long long)rs,
               (unsigned long long)hs, (unsigned long long)lead);
    UNPOISON(block, lead * sizeof(soft_t));
    free(block); free(in); free(hist); free(map); free(count); free(fill); free(hist_out); free(n_out); free(fill_out);
    return bad;
}

static int descramble_shape(int it) {
    static const uint32_t lens[] = {1, 7, 8, 9, 511, 512, 768, 1025, 6144};
    const uint32_t n_bits = below(2) ? lens[below(9)] : 1 + (uint32_t)below(3000), nb = (n_bits + 7) / 8;
    const uint32_t rows = 1 + (uint32_t)below(3), mf = 1 + (uint32_t)below(12);
    const bool in_place = below(2), with_count = below(2);
    const uint64_t stride = nb + (below(2) ? 0 : below(7)), out_stride = in_place ? stride : nb + (below(2) ? 0 : below(7));
    const uint64_t frames = (uint64_t)rows * mf, in_b = (frames - 1) * stride + nb, out_b = (frames - 1) * out_stride + nb;
    const uint64_t lead_in = below(4), lead_out = in_place ? lead_in : below(4);
    uint8_t* in_block = (uint8_t*)malloc(lead_in + in_b);
    uint8_t* in = in_block + lead_in;
    for (uint64_t k = 0; k < in_b; ++k) in[k] = (uint8_t)rnd();
    std::vector<uint8_t> before(in, in + in_b);
    uint8_t* out_block = in_place ? in_block : (uint8_t*)malloc(lead_out + out_b);
    uint8_t* out = out_block + lead_out;
    if (!in_place) memset(out_block, 0x5A, lead_out + out_b);
    POISON(in_block, lead_in);
    if (!in_place) POISON(out_block, lead_out);
    uint32_t* count = (uint32_t*)malloc(rows * sizeof(uint32_t));
    for (uint32_t r = 0; r < rows; ++r) count[r] = odd_count(mf);

    vit::DabDescrArgs a{};
    a.in = in; a.n_frames = with_count ? count : nullptr; a.out = out;
    a.stride = stride; a.out_stride = out_stride; a.max_frames = mf; a.frames = (uint32_t)frames;
    a.n_bits = n_bits; a.nb = nb; a.U = nb / 4u + 2u; a.units = (uint64_t)a.frames * a.U;
    const uint64_t blocks = vit::dab_descramble_blocks(a);
    for (uint64_t b = 0; b < blocks; ++b)
        for (uint32_t t = 0; t < vit::DAB_BLOCK; ++t) vit::dab_descramble_thread(a, vit::DAB_PRBS.w, (uint32_t)b, t);

    std::vector<uint8_t> seq(n_bits);
    uint32_t reg = 0x1FF;
    for (uint32_t t = 0; t < n_bits; ++t) {
        const uint32_t o = ((reg >> 4) ^ (reg >> 8)) & 1u;
        seq[t] = (uint8_t)o;
        reg = ((reg << 1) | o) & 0x1FFu;
    }
    std::vector<uint8_t> want(out_b, 0x5A);
    if (in_place) want = before;
    for (uint32_t r = 0; r < rows; ++r) {
        const uint32_t nf = with_count ? (count[r] < mf ? count[r] : mf) : mf;
        for (uint32_t f = 0; f < nf; ++f)
            for (uint32_t j = 0; j < nb; ++j) {
                uint8_t pad = 0;
                for (uint32_t b = 0; b < 8; ++b)
                    if (8 * j + b < n_bits) pad |= (uint8_t)(seq[8 * j + b] << (7 - b));
                want[((uint64_t)r * mf + f) * out_stride + j] = before[((uint64_t)r * mf + f) * stride + j] ^ pad;
            }
    }
    int bad = memcmp(want.data(), out, out_b) != 0 || (!in_place && memcmp(before.data(), in, in_b) != 0);
    if (bad)
        printf("MISMATCH descramble shape %d: n_bits %u rows %u mf %u in_place %d count %d stride %llu out_stride %llu leads %llu %llu\n", it, n_bits,
               rows, mf, in_place, with_count, (unsigned long long)stride, (unsigned long long)out_stride, (unsigned long long)lead_in,
               (unsigned long long)lead_out);
    UNPOISON(in_block, lead_in);
    if (!in_place) { UNPOISON(out_block, lead_out); free(out_block); }
    free(in_block); free(count);
    return bad;
}

// one call of either argument rule: the accepted base call, which a case changes in a field or two
struct DeintCall {
    bool handle = true;
    size_t sb = 2;
    const void* d_in;
    size_t rs = 0, fs = 0, rows = 2, mf = 4;
    const uint32_t* nfr;
    size_t n = 32;
    const int32_t* idx;
    size_t spf = 40;
    const void* hist;
    const uint32_t* fill;
    size_t hs = 0;
    const void* out;
    const uint32_t* n_out;
    const void* hist_out;
    const uint32_t* fill_out;
    const char* operator()() const {
        return vit::dab_deinterleave_invalid(handle, sb, d_in, rs, fs, rows, mf, nfr, n, idx, spf, hist, fill, hs, out, n_out, hist_out, fill_out);
    }
};
struct DescrCall {
    bool handle = true;
    const uint8_t* d_in;
    size_t s = 0, rows = 2, mf = 4;
    const uint32_t* nfr;
    size_t bits = 90;
    const uint8_t* out;
    size_t os = 0;
    const char* operator()() const { return vit::dab_descramble_invalid(handle, d_in, s, rows, mf, nfr, bits, out, os); }
};

#define WANT(base, set, bad)                                                                \
    do {                                                                                    \
        auto k = base;                                                                      \
        set;                                                                                \
        const char* why_ = k();                                                             \
        if ((why_ != nullptr) != (bad)) { printf("MISMATCH line %d: %s\n", __LINE__, why_ ? why_ : "accepted"); return 1; } \
    } while (0)

static int arguments() {
    const size_t n = 32, mf = 4, rows = 2, spf = 40, H = vit::DAB_H;
    std::vector<int16_t> big(4096), out(rows * mf * spf), hist_out(rows * H * n);       // heap blocks the rules never read
    std::vector<uint32_t> cnts(8);
    std::vector<int32_t> idx(spf);
    const int16_t *d_in = big.data(), *d_hist = big.data() + 512;
    const uint32_t *n_out = cnts.data(), *fill_out = n_out + 2, *fill_in = n_out + 4, *n_frames = n_out + 6;
    auto plus = [](const void* p, size_t bytes) { return (const void*)((const uint8_t*)p + bytes); };
    DeintCall g;
    g.d_in = d_in; g.nfr = n_frames; g.idx = idx.data(); g.hist = d_hist; g.fill = fill_in;
    g.out = out.data(); g.n_out = n_out; g.hist_out = hist_out.data(); g.fill_out = fill_out;
    WANT(g, (void)0, false);
    WANT(g, k.handle = false, true);
    WANT(g, k.d_in = nullptr, true);
    WANT(g, k.out = nullptr, true);
    WANT(g, k.n_out = nullptr, true);
    WANT(g, k.hist_out = nullptr, true);
    WANT(g, k.fill_out = nullptr, true);
    WANT(g, k.fill = nullptr, true);                                                     // a history without its fill
    WANT(g, (k.hist = nullptr, k.fill = nullptr, k.nfr = nullptr), false);               // the optional ones absent
    WANT(g, k.n = 0, true);
    WANT(g, k.spf = 0, true);
    WANT(g, k.fs = n - 1, true);                                                         // strides
    WANT(g, k.rs = mf * n - 1, true);
    WANT(g, (k.fs = n + 1, k.rs = mf * (n + 1) - 1), true);
    WANT(g, k.hs = H * n - 1, true);
    WANT(g, k.idx = nullptr, true);                                                      // the identity needs spf == n
    WANT(g, (k.idx = nullptr, k.spf = n + 1), true);
    WANT(g, (k.idx = nullptr, k.spf = n), false);
    WANT(g, k.n = (size_t)1 << 28, true);
    WANT(g, k.spf = (size_t)1 << 32, true);
    WANT(g, k.d_in = plus(d_in, 1), true);                                               // alignment
    WANT(g, k.out = plus(out.data(), 1), true);
    WANT(g, k.hist = plus(d_hist, 1), true);
    WANT(g, k.hist_out = plus(hist_out.data(), 1), true);
    WANT(g, k.idx = (const int32_t*)plus(idx.data(), 2), true);
    WANT(g, k.n_out = (const uint32_t*)plus(n_out, 2), true);
    WANT(g, k.nfr = (const uint32_t*)plus(n_frames, 1), true);
    WANT(g, (k.sb = 1, k.d_in = plus(d_in, 1), k.hist = plus(d_hist, 1)), false);        // soft8: any address
    WANT(g, k.out = d_in, true);                                                         // overlaps
    WANT(g, k.out = d_hist, true);
    WANT(g, k.out = hist_out.data(), true);
    WANT(g, k.out = idx.data(), true);
    WANT(g, k.hist_out = d_in, true);
    WANT(g, k.hist_out = d_hist, true);
    WANT(g, k.hist_out = idx.data(), true);
    WANT(g, k.n_out = n_frames, true);
    WANT(g, k.n_out = fill_in, true);
    WANT(g, k.fill_out = n_frames, true);
    WANT(g, k.fill_out = fill_in, true);
    WANT(g, k.fill_out = n_out, true);
    WANT(g, k.out = d_hist + rows * H * n, false);                                       // right behind the history
    WANT(g, k.out = d_hist + rows * H * n - 1, true);
    WANT(g, k.rows = (size_t)1 << 31, true);                                             // counts
    WANT(g, (k.mf = (size_t)1 << 31, k.fs = n), true);
    WANT(g, (k.rows = (size_t)1 << 20, k.mf = (size_t)1 << 20), true);
    WANT(g, (k.rows = (size_t)1 << 13, k.mf = (size_t)1 << 14, k.spf = (size_t)1 << 5), true);
    WANT(g, k.rows = 0, false);                                                          // no work
    WANT(g, k.mf = 0, false);
    WANT(g, (k.rows = 0, k.n = 0), true);                                                // ... still refuses what needs no shape

    std::vector<uint8_t> frames(rows * mf * 12), dout(rows * mf * 12);
    DescrCall d;
    d.d_in = frames.data(); d.nfr = n_frames; d.out = dout.data();
    WANT(d, (void)0, false);
    WANT(d, k.handle = false, true);
    WANT(d, k.d_in = nullptr, true);
    WANT(d, k.out = nullptr, true);
    WANT(d, k.bits = ((size_t)1 << 32) - 33, true);
    WANT(d, k.s = 11, true);
    WANT(d, k.os = 11, true);
    WANT(d, k.rows = (size_t)1 << 31, true);
    WANT(d, k.mf = (size_t)1 << 31, true);
    WANT(d, (k.rows = (size_t)1 << 16, k.mf = (size_t)1 << 15), true);
    WANT(d, (k.out = frames.data(), k.os = 13), true);                                   // in place needs equal strides
    WANT(d, k.out = frames.data(), false);
    WANT(d, (k.out = frames.data(), k.s = 13, k.os = 13), false);
    WANT(d, k.out = frames.data() + 1, true);
    WANT(d, k.out = frames.data() + 12, true);
    WANT(d, k.out = frames.data() + rows * mf * 12, false);                              // right behind the input
    WANT(d, k.out = (const uint8_t*)n_frames, true);
    WANT(d, k.rows = 0, false);                                                          // no work
    WANT(d, k.mf = 0, false);
    WANT(d, k.bits = 0, false);
    WANT(d, (k.rows = 0, k.s = 11), true);                                               // ... still refuses what needs no shape
    return 0;
}

int main(int argc, char** argv) {
    const int shapes = argc > 1 ? atoi(argv[1]) : 300;
    rng_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 1;
    static const uint8_t first[8] = {0x07, 0xBE, 0x2E, 0x64, 0x12, 0x9D, 0xA3, 0xCF};
    for (uint32_t i = 0; i < 8; ++i)
        if (((vit::DAB_PRBS.w[i / 4] >> (24 - 8 * (i % 4))) & 0xFFu) != first[i]) { printf("MISMATCH: sequence byte %u\n", i); return 1; }
    for (uint32_t j = 0; j < 16; ++j)
        if (vit::dab_delay(j) != DELAY[j] || vit::dab_delay(j + 16) != DELAY[j]) { printf("MISMATCH: delay %u\n", j); return 1; }
    if (arguments()) return 1;
    for (int it = 0; it < shapes; ++it) {
        if (it % 2 ? deinterleave_shape<int8_t>(it) : deinterleave_shape<int16_t>(it)) return 1;
        if (descramble_shape(it)) return 1;
    }
    printf("ok: %d shapes of either kernel\n", shapes);
    return 0;
}
