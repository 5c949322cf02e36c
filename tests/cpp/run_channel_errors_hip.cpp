// run_channel_errors_hip.cpp -- the re-encoded channel symbol error count from C++: ViterbiDecoder_HIP_Batch::synth -> decode ->
// channel_errors (include/viterbi_hip/viterbi_decoder_hip_batch.h), checked per frame against the counting rule applied on the
// host to the oracle's encoder (vo_encode, oracle/viterbi_oracle.h) run over the decoded bytes; and ::encode of the decoded bytes
// against vo_encode symbol for symbol.  Voyager <7, 2, uint16_t, int16_t> soft16, 130 frames of 1024 bits at 2 dB, and LTE
// <7, 3, uint8_t, int8_t> hard8, 64 frames of 41 bits.  The device generator makes whole info bytes only, so the 41-bit frames take
// their bits from synth's bytes, are encoded by ::encode (L = 41, zero tail) and disturbed on the host: 4 % of the symbols inverted,
// 3 % erased (the midpoint 0, which the count skips).  Prints PASS only if every frame matches.
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "viterbi_hip/viterbi_decoder_hip_batch.h"
#include "test_support.h"
#include "../../oracle/viterbi_oracle.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

template <size_t K, size_t R, typename error_t, typename soft_t>
static int run(const char* name, const uint8_t (&G)[R], const DecodeSetup<soft_t, error_t>& setup, size_t F, size_t L, float ebn0_db,
               uint64_t seed) {
    auto table = ViterbiBranchTable<K, R, soft_t>(G, setup.high, setup.low);
    ViterbiDecoder_HIP_Batch<K, R, error_t, soft_t> batch(table, setup.config);
    const size_t S = L + K - 1, nb = (L + 7) / 8, L8 = 8 * nb, n_sym = S * R;
    uint8_t *d_tx, *d_out;
    soft_t *d_sym, *d_enc;
    uint32_t *d_err, *d_cmp;
    void* d_ws;
    const size_t ws_bytes = batch.workspace_bytes(F, L);
    HIP_OK(hipMalloc((void**)&d_tx, F * nb));
    HIP_OK(hipMalloc((void**)&d_out, F * nb));
    HIP_OK(hipMalloc((void**)&d_sym, F * (L8 + K - 1) * R * sizeof(soft_t)));
    HIP_OK(hipMalloc((void**)&d_enc, F * n_sym * sizeof(soft_t)));
    HIP_OK(hipMalloc((void**)&d_err, F * sizeof(uint32_t)));
    HIP_OK(hipMalloc((void**)&d_cmp, F * sizeof(uint32_t)));
    HIP_OK(hipMalloc(&d_ws, ws_bytes));
    HIP_OK(hipMemset(d_err, 0xFF, F * sizeof(uint32_t)));
    HIP_OK(hipMemset(d_cmp, 0xFF, F * sizeof(uint32_t)));

    std::vector<soft_t> symbols(F * n_sym);
    if (L % 8 == 0) {
        batch.synth(F, L, seed, 0, ebn0_db, false, d_tx, d_sym);
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(symbols.data(), d_sym, symbols.size() * sizeof(soft_t), hipMemcpyDeviceToHost));
    } else {
        batch.synth(F, L8, seed, 0, 0.0f, true, d_tx, d_sym);       // the bytes; these symbols are overwritten
        batch.encode(d_tx, F, L, d_sym);
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(symbols.data(), d_sym, symbols.size() * sizeof(soft_t), hipMemcpyDeviceToHost));
        XorShift rng(seed);
        for (soft_t& v : symbols) {
            const uint32_t r = rng.next() % 100;
            if (r < 4) v = soft_t(-v); else if (r < 7) v = 0;
        }
        HIP_OK(hipMemcpy(d_sym, symbols.data(), symbols.size() * sizeof(soft_t), hipMemcpyHostToDevice));
    }

    batch.decode(d_sym, F, L, d_ws, ws_bytes, d_out);
    batch.channel_errors(d_sym, d_out, F, L, d_err, d_cmp);
    batch.encode(d_out, F, L, d_enc);
    HIP_OK(hipDeviceSynchronize());
    std::vector<uint8_t> out(F * nb);
    std::vector<uint32_t> err(F), cmp(F);
    std::vector<soft_t> enc(F * n_sym);
    HIP_OK(hipMemcpy(out.data(), d_out, out.size(), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(err.data(), d_err, F * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(cmp.data(), d_cmp, F * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(enc.data(), d_enc, enc.size() * sizeof(soft_t), hipMemcpyDeviceToHost));
    (void)hipFree(d_tx); (void)hipFree(d_out); (void)hipFree(d_sym); (void)hipFree(d_enc); (void)hipFree(d_err); (void)hipFree(d_cmp);
    (void)hipFree(d_ws);

    uint32_t G32[R];
    for (size_t i = 0; i < R; i++) G32[i] = G[i];
    const int mid = int(setup.high) + int(setup.low);
    size_t bad_counts = 0, bad_encode = 0, total_err = 0, total_cmp = 0;
    std::vector<uint8_t> coded((L8 + K - 1) * R), bytes(nb);
    for (size_t f = 0; f < F; f++) {
        // pad bits are not data: with them cleared the first L + K-1 steps of the whole-byte encoder are the frame's
        memcpy(bytes.data(), &out[f * nb], nb);
        if (L % 8) bytes[nb - 1] &= uint8_t(0xFFu << (8 - L % 8));
        vo_encode(int(K), int(R), G32, bytes.data(), nb, coded.data());
        uint32_t e = 0, c = 0;
        for (size_t k = 0; k < n_sym; k++) {
            const int twice = 2 * int(symbols[f * n_sym + k]);
            if (twice != mid) { c++; e += (twice > mid) != (coded[k] != 0); }
            bad_encode += enc[f * n_sym + k] != (coded[k] ? setup.high : setup.low);
        }
        bad_counts += e != err[f] || c != cmp[f];
        total_err += e; total_cmp += c;
    }
    printf("%s: %zu frames x %zu bits, %zu of %zu compared symbols differ, mismatching frames=%zu, mismatching encoded symbols=%zu\n",
           name, F, L, total_err, total_cmp, bad_counts, bad_encode);
    // a count that is trivially zero, or a batch without a single compared symbol, would prove nothing
    return bad_counts == 0 && bad_encode == 0 && total_err > 0 && total_cmp > total_err ? 0 : 1;
}

int main() {
    const uint8_t voyager[2] = {109, 79};
    const uint8_t lte[3] = {91, 117, 121};
    int rc = run<7, 2, uint16_t, int16_t>("Voyager K7 R2 soft16", voyager, soft16_setup(2), 130, 1024, 2.0f, 31);
    if (rc == 0) rc = run<7, 3, uint8_t, int8_t>("LTE K7 R3 hard8", lte, hard8_setup(3), 64, 41, 0.0f, 32);
    printf(rc == 0 ? "PASS\n" : "FAIL\n");
    return rc;
}
