// wifi_host_check -- the source of the three 802.11a/g kernels (viterbidecodercpp_amd/csrc/kernels_wifi.hpp) compiled for the HOST with the
// HIP built-ins stubbed (hip_stub/hip/hip_runtime.h), as a program of its own for the address and undefined-behaviour sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Itests/cpp/hip_stub -o wifi_host_check wifi_host_check.cpp
//   ./wifi_host_check [shapes = 300] [seed = 1]
// Every random shape puts its inputs, its per-frame arrays and its outputs into heap blocks that END with their last byte (the bytes in
// front of an odd base address are poisoned under the address sanitizer), runs every thread of the grid through the kernels' own device
// functions with the arguments the *_args functions make, and compares every byte of every output with a literal restatement of the rule
// over a fill pattern: the interleaver as the two permutations of the standard applied on the transmit side and inverted by table,
// puncturing as a mask walked bit by bit, the scrambler as a shift register stepped bit by bit, the FCS as the reflected CRC-32 bit by
// bit.  Rates, symbol counts, step counts and lengths include hostile values (above 7, 0xFFFFFFFF).  The one part of the DATA kernel that
// stays off the host is the __shfl_xor exchange: the lanes of a group run one after the other and the partner's register comes from an
// array.  The SIGNAL parser is run over all 2^18 fields.  Behind the random shapes come the one-byte de-interleaver shapes with frames in
// {1, 3, 5, 31, 257} and S in {1, 3, 37, 433}, three times each: two elements behind the last whole dword, and at (1, 1) no whole dword.
// In front of them: the three argument rules (wifi_deinterleave_invalid, wifi_signal_invalid, wifi_data_invalid) at an accepted call, at
// every INVALID_ARG case tests/test_gpu_wifi.py sends through the library, and at the zero-work cases.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../viterbidecodercpp_amd/csrc/kernels_wifi.hpp"

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

static const uint32_t N_BPSC[8] = {1, 1, 2, 2, 4, 4, 6, 6}, N_DBPS[8] = {24, 36, 48, 72, 96, 144, 192, 216};
static const int MASK_LEN[8] = {2, 6, 2, 6, 2, 6, 4, 6};
static const int MASK[3][6] = {{1, 1, 0, 0, 0, 0}, {1, 1, 1, 0, 0, 0}, {1, 1, 1, 0, 0, 1}};     // by length 2, 4, 6
static const int PATTERN[8] = {0xD, 0xF, 0x5, 0x7, 0x9, 0xB, 0x1, 0x3};

// table[k] = the transmitted place of coded bit k: the numbers 0 .. N - 1 sent through both permutations
static std::vector<uint32_t> rule_table(uint32_t m) {
    const uint32_t n = 48 * N_BPSC[m], s = N_BPSC[m] / 2 > 1 ? N_BPSC[m] / 2 : 1;
    std::vector<uint32_t> first(n), sent(n), table(n);
    for (uint32_t k = 0; k < n; ++k) first[(n / 16) * (k % 16) + k / 16] = k;
    for (uint32_t i = 0; i < n; ++i) sent[s * (i / s) + (i + n - 16 * i / n) % s] = first[i];
    for (uint32_t j = 0; j < n; ++j) table[sent[j]] = j;
    return table;
}

// a per-frame array of `frames` entries at `stride` elements that ends with its last entry; hostile values among them
static uint32_t* per_frame(uint64_t frames, uint64_t stride, uint64_t ordinary) {
    const uint64_t n = (frames - 1) * stride + 1;
    uint32_t* p = (uint32_t*)malloc(n * sizeof(uint32_t));
    for (uint64_t i = 0; i < n; ++i) p[i] = (uint32_t)rnd();
    for (uint64_t f = 0; f < frames; ++f)
        p[f * stride] = below(8) == 0 ? 0xFFFFFFFFu : below(8) == 0 ? (uint32_t)rnd() : below(8) == 0 ? 0u : (uint32_t)below(ordinary + 1);
    return p;
}

// what the de-interleaver shapes reached: calls with elements behind the last whole dword, calls with no whole dword
static uint32_t seen_tails = 0, seen_no_dword = 0;

// a random shape; with force_frames and force_S those two are given and the rest is random
template <class soft_t>
static int deint_shape(int it, uint64_t force_frames = 0, uint64_t force_S = 0) {
    const uint64_t frames = force_frames ? force_frames : 1 + below(below(3) ? 5 : 40), max_sym = 1 + below(4);
    const bool with_rate = below(3) != 0, with_sym = below(2), with_steps = below(2);
    const uint32_t rate = (uint32_t)below(8);
    const uint64_t S = force_S ? force_S : 1 + below(below(4) ? max_sym * 216 + 10 : 30), cs = 1 + (below(2) ? 0 : below(6));
    const uint64_t least = max_sym * (with_rate ? 288 : 48 * N_BPSC[rate]);
    const uint64_t stride_arg = below(2) ? 0 : least + below(7), stride = stride_arg ? stride_arg : max_sym * 288;
    uint32_t* rates = with_rate ? per_frame(frames, cs, 9) : nullptr;
    uint32_t* syms = with_sym ? per_frame(frames, cs, max_sym + 1) : nullptr;
    uint32_t* steps = with_steps ? per_frame(frames, cs, max_sym * 216 + 3) : nullptr;
    // the input ends with the last element the LAST frame may read: max_sym * N_CBPS of its own rate
    const uint32_t m_last = with_rate ? rates[(frames - 1) * cs] : rate;
    const uint64_t n_in = (frames - 1) * stride + max_sym * (m_last <= 7 ? 48 * N_BPSC[m_last] : 0);
    soft_t* in = (soft_t*)malloc(n_in * sizeof(soft_t) + (n_in == 0));
    for (uint64_t i = 0; i < n_in; ++i) in[i] = (soft_t)rnd();
    const uint64_t total = frames * 2 * S;
    soft_t* out = (soft_t*)malloc(total * sizeof(soft_t));         // malloc: aligned to more than 4 bytes
    memset(out, 0x5A, total * sizeof(soft_t));

    const vit::WifiDeintArgs a = vit::wifi_deint_args(in, stride_arg, frames, max_sym, rate, rates, syms, steps, with_rate || with_sym || with_steps ? cs : 0,
                                                      S, out, sizeof(soft_t));
    seen_tails += a.tail != 0;
    seen_no_dword += a.groups == 0;
    for (uint32_t b = 0; b < vit::wifi_deint_blocks(a); ++b)
        for (uint32_t t = 0; t < vit::WIFI_BLOCK; ++t) vit::wifi_deint_thread<soft_t>(a, b, t);

    for (uint64_t f = 0; f < frames; ++f) {
        const uint32_t m = with_rate ? rates[f * cs] : rate;
        std::vector<soft_t> want(2 * S, (soft_t)0);
        if (m <= 7) {
            uint64_t ns = with_sym ? syms[f * cs] : max_sym;
            ns = ns < max_sym ? ns : max_sym;
            const uint64_t lim = ns * N_DBPS[m];
            uint64_t st = with_steps ? steps[f * cs] : lim;
            st = st < lim ? st : lim;
            st = st < S ? st : S;
            const std::vector<uint32_t> table = rule_table(m);
            const uint32_t n = 48 * N_BPSC[m];
            const int* mask = MASK[MASK_LEN[m] / 2 - 1];
            uint64_t c = 0;
            for (uint64_t q = 0; q < 2 * st; ++q)
                if (mask[q % MASK_LEN[m]]) {
                    want[q] = in[f * stride + (c / n) * n + table[c % n]];
                    ++c;
                }
        }
        for (uint64_t q = 0; q < 2 * S; ++q)
            if (out[f * 2 * S + q] != want[q]) {
                printf("MISMATCH de-interleave shape %d: soft_bytes %zu frames %llu max_sym %llu S %llu rate %u (%d %d %d) stride %llu cs %llu: frame %llu "
                       "m %u q %llu got %d want %d\n", it, sizeof(soft_t), (unsigned long long)frames, (unsigned long long)max_sym, (unsigned long long)S,
                       rate, with_rate, with_sym, with_steps, (unsigned long long)stride_arg, (unsigned long long)cs, (unsigned long long)f, m,
                       (unsigned long long)q, (int)out[f * 2 * S + q], (int)want[q]);
                return 1;
            }
    }
    free(in); free(out); free(rates); free(syms); free(steps);
    return 0;
}

static int signal_all() {
    uint8_t* p = (uint8_t*)malloc(3);
    for (uint32_t v = 0; v < (1u << 18); ++v) {
        const uint32_t w = v << 6 | (uint32_t)below(64);
        p[0] = (uint8_t)(w >> 16); p[1] = (uint8_t)(w >> 8); p[2] = (uint8_t)w;
        const vit_hip_wifi_signal got = vit::wifi_signal_parse(p);
        int bit[18], ones = 0;
        for (int t = 0; t < 18; ++t) { bit[t] = (p[t / 8] >> (7 - t % 8)) & 1; ones += bit[t]; }
        uint32_t m = 8, len = 0;
        for (uint32_t r = 0; r < 8; ++r)
            if (PATTERN[r] == (bit[0] << 3 | bit[1] << 2 | bit[2] << 1 | bit[3])) m = r;
        for (int i = 0; i < 12; ++i) len |= (uint32_t)bit[5 + i] << i;
        const uint32_t valid = m < 8 && ones % 2 == 0 && !bit[4] && len >= 1;
        const uint32_t st = valid ? 16 + 8 * len + 6 : 0, ns = valid ? (st + N_DBPS[m] - 1) / N_DBPS[m] : 0;
        if (got.rate_index != m || got.length != len || got.valid != valid || got.n_steps != st || got.n_sym != ns) {
            printf("MISMATCH SIGNAL %#x: got %u %u %u %u %u want %u %u %u %u %u\n", w, got.rate_index, got.length, got.n_sym, got.n_steps, got.valid, m, len,
                   ns, st, valid);
            return 1;
        }
    }
    free(p);
    return 0;
}

// the grid of wifi_data_kernel, one thread per block, with the exchange done through `regs`
static void run_data(const vit::WifiDataArgs& a) {
    static uint32_t tab[1024];
    vit::crc_build_tables(tab, vit::WIFI_FCS_POLY, 0, 1);
    const uint32_t G = 1u << a.logG;
    std::vector<uint32_t> regs(G), next(G);
    std::vector<vit::WifiDataLane> lanes(G);
    const uint64_t threads = vit::wifi_data_blocks(a) * vit::WIFI_BLOCK;
    for (uint64_t t0 = 0; t0 < threads; t0 += G) {
        for (uint32_t j = 0; j < G; ++j) {
            lanes[j] = vit::wifi_data_lane(a, t0 + j);
            regs[j] = lanes[j].active ? vit::wifi_data_chunk(a, tab, lanes[j]) : 0u;
        }
        for (uint32_t s = 0; s < a.logG; ++s) {
            for (uint32_t j = 0; j < G; ++j) next[j] = vit::wifi_data_combine(a, regs[j], regs[j ^ (1u << s)], s);
            regs.swap(next);
        }
        for (uint32_t j = 0; j < G; ++j)
            if (lanes[j].active && lanes[j].j == 0) vit::wifi_data_finish(a, lanes[j], regs[j]);
    }
}

static uint32_t seen_logG = 0;

static int data_shape(int it) {
    static const uint64_t edge[] = {0, 1, 3, 4, 5, 7, 8, 9, 20, 63, 64, 65, 68, 69, 100, 1028, 1500, 4095};
    const uint64_t cap = below(3) ? edge[below(sizeof(edge) / sizeof(edge[0]))] : below(300);          // the PSDU octets the frame has room for
    const uint64_t S = 22 + 8 * cap + below(8), n_bits = S - 6, nb = (n_bits + 7) / 8;
    const uint64_t max_length = below(3) ? 4095 : below(cap + 3);
    const uint64_t frames = cap > 1000 ? 1 + below(3) : 1 + below(70);
    const uint64_t stride_arg = below(2) ? 0 : nb + below(6), stride = stride_arg ? stride_arg : nb;
    const uint64_t ls = 1 + (below(2) ? 0 : below(6));
    const uint64_t longest = max_length < cap ? max_length : cap;
    const uint64_t ps_arg = below(2) ? 0 : longest + below(5), ps = ps_arg ? ps_arg : max_length;
    const uint64_t lead = below(2) ? 0 : below(8);
    const uint64_t in_bytes = (frames - 1) * stride + nb;
    uint8_t* block = (uint8_t*)malloc(lead + in_bytes);
    uint8_t* in = block + lead;
    for (uint64_t i = 0; i < lead + in_bytes; ++i) block[i] = (uint8_t)rnd();
    for (uint64_t f = 0; f < frames; ++f)
        if (below(6) == 0) in[f * stride] &= 1;                    // seven zero bits in front: no scrambler gives them
    POISON(block, lead);
    uint32_t* lengths = per_frame(frames, ls, cap + 2);
    const uint64_t psdu_bytes = longest ? (frames - 1) * ps + longest : 0, plead = below(4);
    uint8_t* pblock = (uint8_t*)malloc(plead + psdu_bytes + (plead + psdu_bytes == 0));
    uint8_t* psdu = pblock + plead;
    memset(pblock, 0x5A, plead + psdu_bytes);
    POISON(pblock, plead);
    vit_hip_wifi_status* status = (vit_hip_wifi_status*)malloc(frames * sizeof(vit_hip_wifi_status));
    memset(status, 0x5A, frames * sizeof(vit_hip_wifi_status));

    const vit::WifiDataArgs a = vit::wifi_data_args(in, stride_arg, frames, n_bits, lengths, ls, max_length, psdu, ps_arg, status);
    seen_logG |= 1u << a.logG;
    run_data(a);

    std::vector<uint8_t> want(psdu_bytes, 0x5A);
    for (uint64_t f = 0; f < frames; ++f) {
        const uint8_t* fr = in + f * stride;
        std::vector<uint8_t> d(n_bits), u(n_bits);
        for (uint64_t t = 0; t < n_bits; ++t) d[t] = (fr[t >> 3] >> (7 - (t & 7))) & 1;
        uint8_t x[7];                                              // the register: the last seven bits of the sequence, x[0] the latest
        uint32_t seed = 0;
        for (int t = 0; t < 7; ++t) { x[6 - t] = d[t]; u[t] = 0; seed = seed << 1 | d[t]; }
        for (uint64_t t = 7; t < n_bits; ++t) {
            const uint8_t bit = x[3] ^ x[6];
            memmove(x + 1, x, 6);
            x[0] = bit;
            u[t] = d[t] ^ bit;
        }
        uint64_t len = lengths[f * ls];
        len = len < max_length ? len : max_length;
        len = len < cap ? len : cap;
        uint32_t service = 0, crc = 0xFFFFFFFFu, syndrome = 0xFFFFFFFFu;
        for (int t = 0; t < 16; ++t) service |= (uint32_t)u[t] << t;
        for (uint64_t g = 0; g < len; ++g) {
            uint8_t o = 0;
            for (int b = 0; b < 8; ++b) o |= u[16 + 8 * g + b] << b;
            want[f * ps + g] = o;
        }
        if (len >= 4) {
            for (uint64_t g = 0; g + 4 < len; ++g) {                // the reflected CRC-32, bit by bit
                crc ^= want[f * ps + g];
                for (int b = 0; b < 8; ++b) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
            }
            const uint8_t* e = &want[f * ps + len - 4];
            syndrome = ~crc ^ ((uint32_t)e[0] | (uint32_t)e[1] << 8 | (uint32_t)e[2] << 16 | (uint32_t)e[3] << 24);
        }
        const vit_hip_wifi_status& s = status[f];
        if (s.length_used != len || s.seed != seed || s.service != service || s.fcs_syndrome != syndrome) {
            printf("MISMATCH DATA shape %d: S %llu frames %llu max_length %llu stride %llu ls %llu logG %u C %u frame %llu: status %u %#x %#x %#x want %llu "
                   "%#x %#x %#x\n", it, (unsigned long long)S, (unsigned long long)frames, (unsigned long long)max_length, (unsigned long long)stride_arg,
                   (unsigned long long)ls, a.logG, a.C, (unsigned long long)f, s.length_used, s.seed, s.service, s.fcs_syndrome, (unsigned long long)len,
                   seed, service, syndrome);
            return 1;
        }
    }
    if (psdu_bytes && memcmp(psdu, want.data(), psdu_bytes) != 0) {
        uint64_t i = 0;
        while (psdu[i] == want[i]) ++i;
        printf("MISMATCH DATA shape %d: S %llu frames %llu max_length %llu ps %llu logG %u C %u: PSDU byte %llu (frame %llu octet %llu) got %#x want %#x\n",
               it, (unsigned long long)S, (unsigned long long)frames, (unsigned long long)max_length, (unsigned long long)ps, a.logG, a.C,
               (unsigned long long)i, (unsigned long long)(i / ps), (unsigned long long)(i % ps), psdu[i], want[i]);
        return 1;
    }
    UNPOISON(block, lead); UNPOISON(pblock, plead);
    free(block); free(pblock); free(lengths); free(status);
    return 0;
}

// one call of an argument rule: the accepted base call, which a case changes in a field or two
struct DeintCall {
    bool handle = true;
    int R = 2;
    size_t sb = 2;
    const void* src;
    size_t stride = 0, frames = 4, max_sym = 1;
    unsigned rate = 0;
    const uint32_t *d_rate = nullptr, *d_n_sym = nullptr, *d_n_steps = nullptr;
    size_t cs = 0, S = 216;
    const void* dst;
    const char* operator()() const {
        return vit::wifi_deinterleave_invalid(handle, R, sb, src, stride, frames, max_sym, rate, d_rate, d_n_sym, d_n_steps, cs, S, dst);
    }
};
struct SignalCall {
    bool handle = true;
    const uint8_t* src;
    size_t stride = 0, frames = 4;
    const vit_hip_wifi_signal* sig;
    const char* operator()() const { return vit::wifi_signal_invalid(handle, src, stride, frames, sig); }
};
struct DataCall {
    bool handle = true;
    const uint8_t* src;
    size_t stride = 0, frames = 4, S = 22 + 8 * 16;
    const uint32_t* lengths;
    size_t ls = 0, max_length = 16;
    const uint8_t* dst;
    size_t ps = 0;
    const vit_hip_wifi_status* st;
    const char* operator()() const { return vit::wifi_data_invalid(handle, src, stride, frames, S, lengths, ls, max_length, dst, ps, st); }
};

#define WANT(base, set, bad)                                                                \
    do {                                                                                    \
        auto k = base;                                                                      \
        set;                                                                                \
        const char* why_ = k();                                                             \
        if ((why_ != nullptr) != (bad)) { printf("MISMATCH line %d: %s\n", __LINE__, why_ ? why_ : "accepted"); return 1; } \
    } while (0)

static int arguments() {
    std::vector<int16_t> d_in(4 * 288), out(4 * 216 * 2 + 8);                           // heap blocks the rules never read
    std::vector<uint32_t> counts(32);                                                    // room for the outputs the cases place inside it
    auto plus = [](const void* p, size_t bytes) { return (const void*)((const uint8_t*)p + bytes); };
    DeintCall g;
    g.src = d_in.data(); g.dst = out.data();
    WANT(g, (void)0, false);
    WANT(g, k.handle = false, true);
    WANT(g, k.src = nullptr, true);
    WANT(g, k.dst = nullptr, true);
    WANT(g, k.R = 3, true);
    WANT(g, k.rate = 8, true);
    WANT(g, (k.rate = 8, k.d_rate = counts.data()), false);                             // with d_rate the scalar is not looked at
    WANT(g, k.max_sym = 0, true);
    WANT(g, k.S = 0, true);
    WANT(g, k.stride = 47, true);                                                        // strides
    WANT(g, k.stride = 48, false);
    WANT(g, (k.d_rate = counts.data(), k.stride = 287), true);
    WANT(g, (k.d_rate = counts.data(), k.stride = 288), false);
    WANT(g, k.dst = plus(out.data(), 2), true);                                          // alignment
    WANT(g, k.src = plus(d_in.data(), 1), true);
    WANT(g, (k.sb = 1, k.src = plus(d_in.data(), 1)), false);
    WANT(g, k.d_n_sym = (const uint32_t*)plus(counts.data(), 2), true);
    WANT(g, k.dst = d_in.data(), true);                                                  // overlaps
    WANT(g, k.dst = d_in.data() + 4 * 288 - 2, true);
    WANT(g, k.dst = d_in.data() + 4 * 288, false);
    WANT(g, k.d_rate = (const uint32_t*)out.data(), true);
    WANT(g, k.d_n_steps = (const uint32_t*)out.data() + 4 * 216 - 1, true);
    WANT(g, k.d_n_steps = (const uint32_t*)out.data() + 4 * 216, false);
    WANT(g, (k.d_n_steps = (const uint32_t*)out.data() - 4, k.cs = 2), true);            // entries two apart reach further
    WANT(g, k.d_n_steps = (const uint32_t*)out.data() - 4, false);
    WANT(g, k.max_sym = ((size_t)1 << 32) / 288 + 1, true);                              // counts
    WANT(g, k.S = ((size_t)1 << 31) - 1, true);
    WANT(g, (k.frames = (size_t)1 << 33, k.S = 1), true);
    WANT(g, k.cs = (size_t)1 << 32, true);
    WANT(g, (k.frames = 0, k.max_sym = 0, k.S = 0), false);                              // no work
    WANT(g, (k.frames = 0, k.R = 3), true);                                              // ... still refuses what needs no shape

    std::vector<uint8_t> b(4 * 40), psdu(4 * 16);
    std::vector<vit_hip_wifi_signal> sig(5);
    SignalCall q;
    q.src = b.data(); q.sig = sig.data();
    WANT(q, (void)0, false);
    WANT(q, k.handle = false, true);
    WANT(q, k.src = nullptr, true);
    WANT(q, k.sig = nullptr, true);
    WANT(q, k.stride = 2, true);
    WANT(q, k.stride = 3, false);
    WANT(q, k.sig = (const vit_hip_wifi_signal*)plus(sig.data(), 2), true);
    WANT(q, k.src = (const uint8_t*)sig.data(), true);
    WANT(q, k.src = (const uint8_t*)sig.data() + 4 * sizeof(vit_hip_wifi_signal) - 1, true);
    WANT(q, k.src = (const uint8_t*)sig.data() + 4 * sizeof(vit_hip_wifi_signal), false);
    WANT(q, k.frames = (size_t)0x7FFFFFFFu * 256 + 1, true);
    WANT(q, k.frames = 0, false);                                                        // no work
    WANT(q, (k.frames = 0, k.stride = 2), true);

    std::vector<vit_hip_wifi_status> status(4);
    DataCall d;
    d.src = b.data(); d.lengths = counts.data(); d.dst = psdu.data(); d.st = status.data();
    WANT(d, (void)0, false);
    WANT(d, k.handle = false, true);
    WANT(d, k.src = nullptr, true);
    WANT(d, k.lengths = nullptr, true);
    WANT(d, k.dst = nullptr, true);
    WANT(d, k.st = nullptr, true);
    WANT(d, k.S = 21, true);
    WANT(d, k.S = ((size_t)1 << 31) - 1, true);
    WANT(d, k.stride = 17, true);                                                        // strides
    WANT(d, k.stride = 18, false);
    WANT(d, k.ps = 15, true);
    WANT(d, k.ps = 16, false);
    WANT(d, k.st = (const vit_hip_wifi_status*)plus(status.data(), 2), true);            // alignment
    WANT(d, k.lengths = (const uint32_t*)plus(counts.data(), 1), true);
    WANT(d, k.dst = b.data(), true);                                                     // overlaps
    WANT(d, k.dst = b.data() + 3 * 18 + 17, true);
    WANT(d, k.dst = b.data() + 3 * 18 + 18, false);
    WANT(d, k.st = (const vit_hip_wifi_status*)counts.data(), true);
    WANT(d, k.dst = (const uint8_t*)(counts.data() + 3), true);
    WANT(d, k.dst = (const uint8_t*)(counts.data() + 4), false);
    WANT(d, (k.dst = (const uint8_t*)(counts.data() + 4), k.ls = 2), true);              // lengths two apart reach further
    WANT(d, k.dst = (const uint8_t*)status.data() + 4 * sizeof(vit_hip_wifi_status) - 1, true);
    WANT(d, k.max_length = (size_t)1 << 28, true);
    WANT(d, k.ls = (size_t)1 << 32, true);
    WANT(d, k.frames = 0, false);                                                        // no work
    WANT(d, (k.frames = 0, k.S = 21), true);                                             // ... still refuses what needs no shape
    return 0;
}

int main(int argc, char** argv) {
    const int shapes = argc > 1 ? atoi(argv[1]) : 300;
    rng_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 1;
    if (arguments()) return 1;
    // the closed form of the place against the table, and the checks of the permutation
    for (uint32_t m = 0; m < 8; ++m) {
        const std::vector<uint32_t> table = rule_table(m);
        const uint32_t n = 48 * N_BPSC[m];
        for (uint32_t c = 0; c < 3 * n; ++c)
            if (vit::wifi_source(m, c) != (c / n) * n + table[c % n]) { printf("MISMATCH rate %u place %u\n", m, c); return 1; }
        const vit::WifiRate r = vit::wifi_rate(m);
        if (r.ncbps != n || r.ndbps != N_DBPS[m]) { printf("MISMATCH rate %u: N_CBPS %u N_DBPS %u\n", m, r.ncbps, r.ndbps); return 1; }
    }
    if (vit::wifi_source(0, 1) != 3 || vit::wifi_source(4, 1) != 13) { printf("MISMATCH: k = 1 must give j = 3 at 48, 13 at 192\n"); return 1; }
    const vit::WifiSeq q = vit::wifi_sequence(7);
    if (q.w0 >> 16 != 0x0EF2) { printf("MISMATCH: the sequence from 0000111 starts %#x\n", q.w0 >> 16); return 1; }
    {                                                              // the block count of the largest output the argument rule accepts
        vit::WifiDeintArgs big{};
        big.groups = 0xFFFFFFFFu;
        if (vit::wifi_deint_blocks(big) != 0x1000000u) { printf("MISMATCH: %u blocks for 2^32 - 1 dwords\n", vit::wifi_deint_blocks(big)); return 1; }
    }
    if (signal_all()) return 1;
    for (int it = 0; it < shapes; ++it) {
        if (it % 2 ? deint_shape<int8_t>(it) : deint_shape<int16_t>(it)) return 1;
        if (data_shape(it)) return 1;
    }
    // the one-byte shapes whose output does not end with a dword: frames and S both odd leave two elements behind the last whole dword,
    // which threads of block 0 store one by one; one frame of one step has no whole dword at all.  The output ends its heap block: an
    // element too many is a heap overflow
    const uint32_t random_tails = seen_tails;
    static const uint64_t odd_frames[] = {1, 3, 5, 31, 257}, odd_S[] = {1, 3, 37, 433};
    for (uint64_t frames : odd_frames)
        for (uint64_t S : odd_S)
            for (int again = 0; again < 3; ++again) {
                const uint32_t tails = seen_tails, none = seen_no_dword;
                if (deint_shape<int8_t>(-1, frames, S)) return 1;
                if (seen_tails != tails + 1 || (seen_no_dword != none) != (frames == 1 && S == 1)) {
                    printf("MISMATCH: frames %llu S %llu at one byte: a tail of two and a dword unless both are 1\n", (unsigned long long)frames,
                           (unsigned long long)S);
                    return 1;
                }
            }
    if (deint_shape<int16_t>(-1, 1, 1) || deint_shape<int16_t>(-1, 257, 433) || seen_tails != random_tails + 60) {
        printf("MISMATCH: a tail at two bytes\n");
        return 1;
    }
    printf("ok: %d shapes, all SIGNAL fields, group sizes seen (mask of log2 G) %#x, %u + 60 de-interleaver calls with a tail, %u without a dword\n", shapes,
           seen_logG, random_tails, seen_no_dword);
    return 0;
}
