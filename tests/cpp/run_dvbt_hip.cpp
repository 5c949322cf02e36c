// run_dvbt_hip.cpp -- the front of the DVB-T route from C++: ViterbiDecoder_HIP_Batch::dvbt_deinterleave
// (include/viterbi_hip/viterbi_decoder_hip_batch.h) against a host loop of the rule as include/vit_hip.h states it, one mode per
// constellation: 2k / QPSK / 2/3, 4k / 16-QAM / 5/6, 8k / 64-QAM / 7/8.  Two rows of three OFDM symbols at an input stride and an output
// pitch larger than a row, the parity of each row's first symbol from a counter on the device; the output buffer is pre-filled with 0x5A
// and compared whole, the counters too.  Needs no case file.  Prints PASS only if everything matches.
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "viterbi_hip/viterbi_decoder_hip_batch.h"
#include "test_support.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

static std::vector<uint32_t> permutation(unsigned mode) {
    static const unsigned taps[3] = {0x9, 0x5, 0x53};
    static const unsigned wires[3][12] = {{0, 7, 5, 1, 8, 2, 6, 9, 3, 4}, {7, 10, 5, 8, 1, 2, 4, 9, 0, 3, 6}, {5, 11, 3, 0, 10, 8, 6, 9, 2, 4, 1, 7}};
    const unsigned nr = 11 + mode, mmax = 2048u << mode, nmax = 1512u << mode;
    std::vector<uint32_t> h;
    unsigned rp = 0;
    for (unsigned i = 0; i < mmax; ++i) {
        if (i == 2) rp = 1;
        else if (i > 2) rp = (rp >> 1) | ((unsigned)(__builtin_popcount(rp & taps[mode]) & 1) << (nr - 2));
        unsigned r = 0;
        for (unsigned t = 0; t + 1 < nr; ++t) r |= ((rp >> (nr - 2 - t)) & 1u) << wires[mode][t];
        const unsigned hq = (i & 1u) * (1u << (nr - 1)) + r;
        if (hq < nmax) h.push_back(hq);
    }
    return h;
}

// place in the period of (step j, output o: 0 = Y, 1 = X), or -1
static int place_of(unsigned rate, unsigned j, unsigned o) {
    static const char* sent[5] = {"X1Y1", "X1Y1Y2", "X1Y1Y2X3", "X1Y1Y2X3Y4X5", "X1Y1Y2Y3Y4X5Y6X7"};
    for (int at = 0; sent[rate][2 * at]; ++at)
        if ((sent[rate][2 * at] == 'X') == (o == 1) && (unsigned)(sent[rate][2 * at + 1] - '1') == j) return at;
    return -1;
}

static int run_case(unsigned mode, unsigned v, unsigned rate) {
    constexpr size_t K = 7, R = 2;
    const uint8_t G[R] = {109, 79};
    const auto setup = soft16_setup(R);
    auto table = ViterbiBranchTable<K, R, int16_t>(G, setup.high, setup.low);
    ViterbiDecoder_HIP_Batch<K, R, uint16_t, int16_t> batch(table, setup.config);

    static const unsigned period[5] = {1, 2, 3, 5, 7}, shift[6] = {0, 63, 105, 42, 21, 84};
    const size_t rows = 2, n_sym = 3, nmax = 1512u << mode, cell = nmax * v, k = period[rate], steps = cell / (k + 1) * k;
    const size_t in_stride = n_sym * cell + 5, pitch = n_sym * steps + 3;
    const std::vector<uint32_t> h = permutation(mode);
    std::vector<uint32_t> inv(nmax);
    for (size_t q = 0; q < nmax; ++q) inv[h[q]] = (uint32_t)q;
    std::vector<int16_t> in(rows * in_stride), want(rows * pitch * 2, 0x5A5A);
    uint32_t x = 12345u + mode;
    for (auto& s : in) { x = x * 1664525u + 1013904223u; s = (int16_t)(x >> 16); }
    const uint32_t first[2] = {6, 0xFFFFFFFFu};                     // an even count and an odd one that wraps
    for (size_t r = 0; r < rows; ++r)
        for (size_t y = 0; y < n_sym; ++y)
            for (size_t n = 0; n < steps; ++n)
                for (unsigned o = 0; o < 2; ++o) {
                    int16_t& out = want[(r * pitch + y * steps + n) * 2 + o];
                    const int place = place_of(rate, (unsigned)(n % k), o);
                    if (place < 0) { out = 0; continue; }
                    const size_t di = (k + 1) * (n / k) + place, word = di / v, rr = di % v, e = rr / (v / 2) + 2 * (rr % (v / 2));
                    const size_t q = 126 * (word / 126) + (word % 126 + 126 - shift[e]) % 126;
                    const bool odd = ((first[r] + y) & 1u) != 0;
                    out = in[r * in_stride + y * cell + (odd ? inv[q] : h[q]) * v + e];
                }
    int16_t *d_in, *d_out;
    uint32_t *d_par;
    HIP_OK(hipMalloc((void**)&d_in, in.size() * 2));
    HIP_OK(hipMalloc((void**)&d_out, want.size() * 2));
    HIP_OK(hipMalloc((void**)&d_par, 4 * sizeof(uint32_t)));
    HIP_OK(hipMemcpy(d_in, in.data(), in.size() * 2, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_out, 0x5A, want.size() * 2));
    HIP_OK(hipMemset(d_par, 0x5A, 4 * sizeof(uint32_t)));
    HIP_OK(hipMemcpy(d_par, first, sizeof(first), hipMemcpyHostToDevice));
    batch.dvbt_deinterleave(d_in, rows, n_sym, mode, v, rate, d_out, 0, d_par, d_par + 2, in_stride, pitch);
    HIP_OK(hipDeviceSynchronize());
    std::vector<int16_t> got(want.size());
    uint32_t par[4];
    HIP_OK(hipMemcpy(got.data(), d_out, got.size() * 2, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(par, d_par, sizeof(par), hipMemcpyDeviceToHost));
    long long bad = 0;
    for (size_t i = 0; i < want.size(); ++i) bad += got[i] != want[i];
    const bool counters = par[0] == first[0] && par[1] == first[1] && par[2] == first[0] + 3 && par[3] == first[1] + 3;
    printf("mode %u v %u rate %u: %zu steps a symbol, mismatches %lld, counters %s\n", mode, v, rate, steps, bad, counters ? "ok" : "WRONG");
    (void)hipFree(d_in); (void)hipFree(d_out); (void)hipFree(d_par);
    return bad == 0 && counters ? 0 : 1;
}

int main() {
    int rc = run_case(0, 2, 1);
    rc |= run_case(1, 4, 3);
    rc |= run_case(2, 6, 4);
    printf(rc == 0 ? "PASS\n" : "FAIL\n");
    return rc;
}
