// dabplus_host_check -- the source of the DAB+ kernels (viterbidecodercpp_amd/csrc/kernels_dabplus.hpp) compiled for the HOST with the HIP
// built-ins stubbed (hip_stub/hip/hip_runtime.h), one thread per block, as a program of its own for the address and undefined-behaviour
// sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Itests/cpp/hip_stub -o dabplus_host_check dabplus_host_check.cpp
//   ./dabplus_host_check [shapes = 300] [seed = 1]
// Every random shape puts the frames into a heap block that ENDS with the last byte the rule reads (byte 10 of the last frame, byte
// 110 s - 1 of the last superframe; the bytes in front of an odd base address are poisoned under the address sanitizer) and the outputs
// into blocks of their exact size over a 0xA5 fill.  The sync, zero and pick kernels run as they stand, block by block; of the AU
// kernel the 64 lanes of a wave run one after the other through its own device functions and the partner's register is read from an
// array.  Headers are hostile on purpose: random start fields, 0xFFF, decreasing, beyond 110 s, with a Fire code made right afterwards
// so that the length logic is what keeps the reads inside.  Everything is compared whole with a bit-by-bit restatement.
// In front of them: both argument rules (dabplus_sync_invalid, dabplus_au_invalid) at an accepted call, at every INVALID_ARG case
// tests/test_gpu_dabplus.py sends through the library, and at the zero-work cases.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include <hip/hip_runtime.h>
inline uint32_t atomicAdd(uint32_t* p, uint32_t v) { const uint32_t old = *p; *p += v; return old; }   // one thread: the stub has none

#include "../../viterbidecodercpp_amd/csrc/kernels_dabplus.hpp"

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

static uint32_t get_bit(const uint8_t* f, uint64_t t) { return (f[t >> 3] >> (7 - (t & 7))) & 1u; }

// the rule, bit by bit
static uint32_t rule_reg(const uint8_t* f, uint64_t first_byte, uint64_t n_bytes, uint32_t poly, uint32_t init) {
    uint32_t reg = init;
    for (uint64_t t = 8 * first_byte; t < 8 * (first_byte + n_bytes); ++t) {
        const uint32_t top = (reg >> 15) & 1u;
        reg = (reg << 1) & 0xFFFFu;
        if (top ^ get_bit(f, t)) reg ^= poly;
    }
    return reg;
}
static bool rule_hit(const uint8_t* f) {
    bool any = false;
    for (int i = 0; i < 11; ++i) any |= f[i] != 0;
    return any && rule_reg(f, 2, 9, 0x782F, 0) == (uint32_t)f[0] * 256u + f[1];
}
static void make_fire(uint8_t* f) {
    const uint32_t c = rule_reg(f, 2, 9, 0x782F, 0);
    f[0] = (uint8_t)(c >> 8); f[1] = (uint8_t)c;
}

template <class K, class A>
static void run_grid(K kernel, unsigned blocks, const A& a) {
    gridDim = dim3(blocks);
    for (unsigned b = 0; b < blocks; ++b) { blockIdx = dim3(b); kernel(a); }
}

static int check_sync(int it) {
    const uint64_t rows = 1 + below(3), mf = below(5) == 0 ? 250 + below(30) : below(12);
    const uint64_t fb = 11 + below(30), fs = below(2) ? fb : fb + below(7), rs = mf * fs + (below(2) ? 0 : below(9));
    const uint32_t frame0 = (uint32_t)below(5);
    const uint64_t lead = below(4);
    const uint64_t in_bytes = mf ? (rows - 1) * rs + (mf - 1) * fs + 11 : 0;
    uint8_t* block = (uint8_t*)malloc(lead + in_bytes + 1);
    uint8_t* frames = block + lead;
    for (uint64_t i = 0; i < lead + in_bytes; ++i) block[i] = (uint8_t)rnd();
    for (uint64_t r = 0; r < rows; ++r)
        for (uint64_t f = 0; f < mf; ++f) {
            uint8_t* p = frames + r * rs + f * fs;
            const uint64_t kind = below(4);
            if (kind == 0) make_fire(p);
            if (kind == 1) memset(p, 0, 11);
            if (kind == 2) { make_fire(p); p[below(11)] ^= (uint8_t)(1u << below(8)); }
        }
    POISON(block, lead);
    POISON(block + lead + in_bytes, 1);
    uint32_t* n_frames = nullptr;
    if (below(3)) {
        n_frames = (uint32_t*)malloc(rows * sizeof(uint32_t));
        for (uint64_t r = 0; r < rows; ++r) n_frames[r] = below(4) == 0 ? (uint32_t)rnd() : (uint32_t)below(mf + 2);
    }
    const bool accumulate = below(2);
    uint32_t* hits = (uint32_t*)malloc(rows * 5 * sizeof(uint32_t));
    uint32_t* count = (uint32_t*)malloc(rows * 5 * sizeof(uint32_t));
    vit_hip_marker_lock* lock = (vit_hip_marker_lock*)malloc(rows * sizeof(vit_hip_marker_lock));
    std::vector<uint32_t> want_h(rows * 5), want_c(rows * 5);
    for (uint64_t i = 0; i < rows * 5; ++i) {
        hits[i] = accumulate ? (uint32_t)below(50) : 0xA5A5A5A5u;
        count[i] = accumulate ? hits[i] + (uint32_t)below(50) : 0xA5A5A5A5u;
        want_h[i] = accumulate ? hits[i] : 0;
        want_c[i] = accumulate ? count[i] : 0;
    }
    memset(lock, 0xA5, rows * sizeof(vit_hip_marker_lock));

    if (!accumulate) {
        gridDim = dim3(1); blockIdx = dim3(0);
        vit::dabplus_zero_kernel(hits, count, rows * 5);
    }
    if (mf) {
        const vit::DabplusSyncArgs a = vit::dabplus_sync_args(frames, rs, fs, rows, mf, n_frames, frame0, hits, count);
        run_grid(vit::dabplus_sync_kernel, (unsigned)(a.items < 3 ? a.items : 1 + below(a.items)), a);
    }
    gridDim = dim3(1); blockIdx = dim3(0);
    vit::dabplus_pick_kernel(hits, count, lock, rows, (uint32_t)fb);

    int bad = 0;
    for (uint64_t r = 0; r < rows; ++r) {
        uint64_t nf = n_frames ? n_frames[r] : mf;
        nf = nf < mf ? nf : mf;
        for (uint64_t f = 0; f < nf; ++f) {
            const uint32_t p = (uint32_t)((frame0 + f) % 5);
            want_c[r * 5 + p] += 1;
            want_h[r * 5 + p] += rule_hit(frames + r * rs + f * fs) ? 1u : 0u;
        }
        uint32_t best = 0;
        for (uint32_t p = 1; p < 5; ++p) {
            const uint64_t ea = want_c[r * 5 + p] - want_h[r * 5 + p], ca = want_c[r * 5 + p];
            const uint64_t eb = want_c[r * 5 + best] - want_h[r * 5 + best], cb = want_c[r * 5 + best];
            if (ca > 0 && (cb == 0 || ea * cb < eb * ca)) best = p;
        }
        for (uint32_t p = 0; p < 5; ++p) bad += hits[r * 5 + p] != want_h[r * 5 + p] || count[r * 5 + p] != want_c[r * 5 + p];
        bad += lock[r].phase != best * 8 * fb || lock[r].inverted != 0 || lock[r].compared != want_c[r * 5 + best] ||
               lock[r].errors != want_c[r * 5 + best] - want_h[r * 5 + best];
    }
    if (bad) printf("MISMATCH sync shape %d: rows %llu max_frames %llu frame_bytes %llu stride %llu frame0 %u accumulate %d\n", it,
                    (unsigned long long)rows, (unsigned long long)mf, (unsigned long long)fb, (unsigned long long)fs, frame0, (int)accumulate);
    UNPOISON(block, lead + in_bytes + 1);
    free(block); free(n_frames); free(hits); free(count); free(lock);
    return bad;
}

static uint32_t field12(const uint8_t* f, uint32_t t) {
    uint32_t v = 0;
    for (uint32_t j = 0; j < 12; ++j) v = 2 * v + get_bit(f, t + j);
    return v;
}
static void put12(uint8_t* f, uint32_t t, uint32_t v) {
    for (uint32_t j = 0; j < 12; ++j) {
        const uint32_t at = t + j, m = 1u << (7 - (at & 7));
        f[at >> 3] = (uint8_t)((f[at >> 3] & ~m) | (((v >> (11 - j)) & 1u) ? m : 0u));
    }
}

static uint64_t aus_checked = 0;

static int check_au(int it) {
    const uint32_t s = below(3) == 0 ? (uint32_t[]){1, 2, 24}[below(3)] : 1 + (uint32_t)below(24);
    const uint64_t rows = 1 + below(2), mf = 1 + below(5), N = rows * mf, data = 110ull * s;
    const uint64_t stride_arg = below(3) == 0 ? 0 : data + below(2) * (10 * s + below(9));
    const uint64_t stride = stride_arg ? stride_arg : 120ull * s;
    const uint64_t lead = below(4), in_bytes = (N - 1) * stride + data;
    uint8_t* block = (uint8_t*)malloc(lead + in_bytes + 1);
    uint8_t* in = block + lead;
    for (uint64_t i = 0; i < lead + in_bytes; ++i) block[i] = (uint8_t)rnd();
    static const uint32_t n_of[4] = {4, 2, 6, 3}, first_of[4] = {8, 5, 11, 6};      // index = dac * 2 + sbr
    for (uint64_t i = 0; i < N; ++i) {
        uint8_t* sf = in + i * stride;
        const uint32_t fmt = (sf[2] >> 5) & 3u, n = n_of[fmt];
        const uint64_t kind = below(8);
        if (kind < 5) {                                            // a consistent header: ascending starts, gaps of at least 3
            uint32_t at = first_of[fmt];
            for (uint32_t k = 1; k < n; ++k) {
                const uint32_t room = (uint32_t)data - at - 3 * (n - k) - 3;
                at += 3 + (uint32_t)below((below(3) == 0 && room > 3 ? 3 : room) + 1);  // short access units often
                put12(sf, 24 + 12 * (k - 1), at);
            }
            if (kind == 0)                                         // and every AU's CRC made right
                for (uint32_t k = 0; k < n; ++k) {
                    const uint32_t a0 = k ? field12(sf, 24 + 12 * (k - 1)) : first_of[fmt], a1 = k + 1 < n ? field12(sf, 24 + 12 * k) : (uint32_t)data;
                    const uint32_t c = rule_reg(sf, a0, a1 - a0 - 2, 0x1021, 0xFFFF) ^ 0xFFFFu;
                    sf[a1 - 2] = (uint8_t)(c >> 8); sf[a1 - 1] = (uint8_t)c;
                }
        } else if (kind == 5) {
            for (uint32_t k = 1; k < n; ++k) put12(sf, 24 + 12 * (k - 1), 0xFFF);
        } else if (kind == 6) {
            for (uint32_t k = 1; k < n; ++k) put12(sf, 24 + 12 * (k - 1), (uint32_t)data - 1 - (uint32_t)below(4) * k);
        }                                                          // kind 7: random fields
        if (below(6)) make_fire(sf);
    }
    POISON(block, lead);
    POISON(block + lead + in_bytes, 1);
    uint32_t* n_frames = nullptr;
    if (below(3)) {
        n_frames = (uint32_t*)malloc(rows * sizeof(uint32_t));
        for (uint64_t r = 0; r < rows; ++r) n_frames[r] = below(4) == 0 ? (uint32_t)rnd() : (uint32_t)below(mf + 2);
    }
    int32_t* status = nullptr;
    if (below(2)) {
        status = (int32_t*)malloc(N * s * sizeof(int32_t));
        for (uint64_t i = 0; i < N * s; ++i) status[i] = below(12) == 0 ? -1 : (int32_t)below(6);
    }
    uint32_t* info = (uint32_t*)malloc(N * sizeof(uint32_t));
    vit_hip_dabplus_au* au = (vit_hip_dabplus_au*)malloc(N * 6 * sizeof(vit_hip_dabplus_au));
    memset(info, 0xA5, N * sizeof(uint32_t));
    memset(au, 0xA5, N * 6 * sizeof(vit_hip_dabplus_au));

    const vit::DabplusAuArgs a = vit::dabplus_au_args(in, stride_arg, rows, mf, n_frames, s, status, info, au);
    static uint32_t tab[1024];
    vit::crc_build_tables(tab, vit::DABPLUS_AU_POLY, 0, 1);
    const uint64_t threads = vit::dabplus_au_blocks(a) * vit::DABPLUS_BLOCK;
    std::vector<uint32_t> regs(64), next(64);
    std::vector<vit::DabplusAuLane> lanes(64);
    for (uint64_t t0 = 0; t0 < threads; t0 += 64) {
        for (uint32_t j = 0; j < 64; ++j) {
            lanes[j] = vit::dabplus_au_lane(a, t0 + j);
            regs[j] = lanes[j].has ? vit::dabplus_au_chunk(tab, lanes[j].base, lanes[j].start, lanes[j].next - lanes[j].start - 2u, a.C, j) : 0u;
        }
        for (uint32_t t = 0; t < 6; ++t) {
            for (uint32_t j = 0; j < 64; ++j) next[j] = vit::dabplus_au_combine(a, regs[j], regs[j ^ (1u << t)], t);
            regs.swap(next);
        }
        if (lanes[0].active) vit::dabplus_au_finish(a, lanes[0], regs[0]);
    }

    int bad = 0;
    for (uint64_t r = 0; r < rows; ++r) {
        uint64_t nf = n_frames ? n_frames[r] : mf;
        nf = nf < mf ? nf : mf;
        for (uint64_t f = 0; f < mf; ++f) {
            const uint64_t i = r * mf + f;
            uint32_t want_info = 0xA5A5A5A5u;
            vit_hip_dabplus_au want[6];
            memset(want, 0xA5, sizeof(want));
            if (f < nf) {
                const uint8_t* sf = in + i * stride;
                const uint32_t fmt = (sf[2] >> 5) & 3u, n = n_of[fmt];
                uint32_t st[7];
                st[0] = first_of[fmt];
                for (uint32_t k = 1; k < n; ++k) st[k] = field12(sf, 24 + 12 * (k - 1));
                st[n] = (uint32_t)data;
                bool consistent = true;
                for (uint32_t k = 0; k < n; ++k) consistent &= st[k + 1] >= st[k] + 3;
                const bool fire = rule_hit(sf), valid = fire && consistent;
                uint32_t failed = 0;
                if (status) for (uint32_t c = 0; c < s; ++c) failed |= status[i * s + c] < 0;
                want_info = (fire ? 1u : 0u) | (consistent ? 2u : 0u) | failed << 2 | (valid ? n : 0u) << 4 | (uint32_t)sf[2] << 8;
                for (uint32_t k = 0; k < 6; ++k) {
                    want[k].start = 0; want[k].bytes = 0; want[k].syndrome = 0xFFFFFFFFu;
                    if (valid && k < n) {
                        const uint32_t nb = st[k + 1] - st[k] - 2;
                        want[k].start = st[k]; want[k].bytes = nb;
                        want[k].syndrome = (rule_reg(sf, st[k], nb, 0x1021, 0xFFFF) ^ 0xFFFFu) ^ ((uint32_t)sf[st[k] + nb] << 8 | sf[st[k] + nb + 1]);
                        ++aus_checked;
                    }
                }
            }
            bad += info[i] != want_info || memcmp(au + i * 6, want, sizeof(want)) != 0;
        }
    }
    if (bad) printf("MISMATCH au shape %d: s %u rows %llu max_frames %llu stride %llu C %u\n", it, s, (unsigned long long)rows,
                    (unsigned long long)mf, (unsigned long long)stride_arg, a.C);
    UNPOISON(block, lead + in_bytes + 1);
    free(block); free(n_frames); free(status); free(info); free(au);
    return bad;
}

// one call of either argument rule: the accepted base call, which a case changes in a field or two
struct SyncCall {
    bool handle = true;
    const uint8_t* d;
    size_t rs = 0, fs = 0, fb = 24, rows = 2, mf = 4;
    const uint32_t* n;
    unsigned f0 = 0, flags = 0;
    const uint32_t *hi, *co;
    const vit_hip_marker_lock* lo;
    const char* operator()() const { return vit::dabplus_sync_invalid(handle, d, rs, fs, fb, rows, mf, n, f0, flags, hi, co, lo); }
};
struct AuCall {
    bool handle = true;
    const uint8_t* d;
    size_t stride = 0, rows = 2, mf = 2;
    const uint32_t* n;
    unsigned s = 2;
    const int32_t* rs = nullptr;
    const uint32_t* i;
    const vit_hip_dabplus_au* a;
    const char* operator()() const { return vit::dabplus_au_invalid(handle, d, stride, rows, mf, n, s, rs, i, a); }
};

#define WANT(base, set, bad)                                                                \
    do {                                                                                    \
        auto k = base;                                                                      \
        set;                                                                                \
        const char* why_ = k();                                                             \
        if ((why_ != nullptr) != (bad)) { printf("MISMATCH line %d: %s\n", __LINE__, why_ ? why_ : "accepted"); return 1; } \
    } while (0)

static int arguments() {
    std::vector<uint8_t> buf(4096);                                                      // heap blocks the rules never read
    std::vector<uint32_t> hits(64), count(64), info(64), nf(2);
    std::vector<vit_hip_marker_lock> lock(16);
    std::vector<vit_hip_dabplus_au> au(4 * vit::DABPLUS_SLOTS);
    std::vector<int32_t> status(4 * 2);
    auto plus = [](const void* p, size_t bytes) { return (const void*)((const uint8_t*)p + bytes); };
    SyncCall g;
    g.d = buf.data(); g.n = nf.data(); g.hi = hits.data(); g.co = count.data(); g.lo = lock.data();
    WANT(g, (void)0, false);
    WANT(g, k.handle = false, true);
    WANT(g, k.d = nullptr, true);
    WANT(g, k.hi = nullptr, true);
    WANT(g, k.co = nullptr, true);
    WANT(g, (k.lo = nullptr, k.n = nullptr), false);                                     // the optional ones absent
    WANT(g, k.flags = 2, true);
    WANT(g, k.flags = VIT_HIP_MARKER_ACCUMULATE, false);
    WANT(g, k.fb = 10, true);
    WANT(g, k.fb = ((size_t)1 << 31) / 40 + 1, true);
    WANT(g, k.f0 = 5, true);
    WANT(g, k.fs = 23, true);                                                            // strides
    WANT(g, k.rs = 95, true);
    WANT(g, (k.fs = 24, k.rs = 96), false);
    WANT(g, k.rows = (size_t)1 << 31, true);
    WANT(g, k.mf = (size_t)1 << 31, true);
    WANT(g, k.n = (const uint32_t*)plus(nf.data(), 2), true);                            // alignment
    WANT(g, k.lo = (const vit_hip_marker_lock*)plus(lock.data(), 2), true);
    WANT(g, k.co = hits.data(), true);                                                   // overlaps
    WANT(g, k.co = hits.data() + 2 * vit::DABPLUS_PHASES - 1, true);
    WANT(g, k.co = hits.data() + 2 * vit::DABPLUS_PHASES, false);
    WANT(g, k.lo = (const vit_hip_marker_lock*)hits.data(), true);
    WANT(g, k.hi = (const uint32_t*)buf.data(), true);
    WANT(g, k.hi = (const uint32_t*)(buf.data() + 2 * 4 * 24 - 4), true);
    WANT(g, k.hi = (const uint32_t*)(buf.data() + 2 * 4 * 24), false);                   // right behind the frames
    WANT(g, k.lo = (const vit_hip_marker_lock*)nf.data(), true);
    WANT(g, k.rows = 0, false);                                                          // no work
    WANT(g, (k.mf = 0, k.lo = nullptr), false);
    WANT(g, (k.mf = 0, k.hi = (const uint32_t*)buf.data()), false);                      // no frames: nothing of them to overlap
    WANT(g, (k.rows = 0, k.f0 = 5), true);                                               // ... still refuses what needs no shape

    AuCall t;
    t.d = buf.data(); t.n = nf.data(); t.i = info.data(); t.a = au.data();
    WANT(t, (void)0, false);
    WANT(t, k.rs = status.data(), false);
    WANT(t, k.handle = false, true);
    WANT(t, k.d = nullptr, true);
    WANT(t, k.i = nullptr, true);
    WANT(t, k.a = nullptr, true);
    WANT(t, k.s = 0, true);
    WANT(t, k.s = 25, true);
    WANT(t, k.stride = 219, true);
    WANT(t, k.stride = 220, false);
    WANT(t, k.rows = (size_t)1 << 31, true);
    WANT(t, k.mf = (size_t)1 << 31, true);
    WANT(t, (k.rows = ((size_t)1 << 31) - 1, k.mf = ((size_t)1 << 31) - 1), true);
    WANT(t, k.i = (const uint32_t*)plus(info.data(), 2), true);                          // alignment
    WANT(t, k.rs = (const int32_t*)plus(status.data(), 1), true);
    WANT(t, k.a = (const vit_hip_dabplus_au*)info.data(), true);                         // overlaps
    WANT(t, k.i = (const uint32_t*)buf.data(), true);
    WANT(t, k.i = (const uint32_t*)(buf.data() + 3 * 240 + 216), true);
    WANT(t, k.i = (const uint32_t*)(buf.data() + 3 * 240 + 220), false);                 // right behind the last superframe's data
    WANT(t, (k.rs = status.data(), k.i = (const uint32_t*)status.data() + 7), true);
    WANT(t, k.a = (const vit_hip_dabplus_au*)nf.data(), true);
    WANT(t, k.rows = 0, false);                                                          // no work
    WANT(t, k.mf = 0, false);
    WANT(t, (k.mf = 0, k.s = 25), true);                                                 // ... still refuses what needs no shape
    return 0;
}

int main(int argc, char** argv) {
    const int shapes = argc > 1 ? atoi(argv[1]) : 300;
    rng_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 1;
    if (arguments()) return 1;
    for (int it = 0; it < shapes; ++it)
        if (check_sync(it) || check_au(it)) return 1;
    printf("ok: %d shapes of each kernel, %llu access units checked\n", shapes, (unsigned long long)aus_checked);
    return 0;
}
