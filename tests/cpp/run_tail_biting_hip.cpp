// run_tail_biting_hip.cpp -- tail-biting frames from C++: ViterbiDecoder_HIP_Batch::decode_tail_biting
// (include/viterbi_hip/viterbi_decoder_hip_batch.h) on noisy tail-biting codewords, checked bit for bit (bytes, end states,
// tail-biting flags) against the rule restated on the oracle's update / chainback (oracle/viterbi_oracle.h): extension
// ext[e] = symbols[(e - head) mod L], every metric at initial_start_error, argmin of the final metrics (lowest state on a tie),
// chainback over the extension, bits [head, head + L).  LTE <7, 3, uint16_t, int16_t> with the default extension (head = tail =
// 0: 8*(K-1) each) and <2, 2, uint8_t, int8_t> with an explicit one.  Prints PASS only if everything matches.
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "viterbi_hip/viterbi_decoder_hip_batch.h"
#include "test_support.h"
#include "../../oracle/viterbi_oracle.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

// the oracle's restatement of one tail-biting frame
template <typename soft_t>
static void reference_frame(const vo_params& p, const int16_t* table, const soft_t* sym, size_t L, size_t head, size_t tail,
                            uint8_t* out, uint32_t* end_state, uint8_t* ok) {
    const size_t K = size_t(p.K), R = size_t(p.R), N = vo_num_states(p.K), W = vo_decision_words(p.K);
    const size_t S_ext = head + L + tail, L_ext = S_ext - (K - 1);
    std::vector<soft_t> ext(S_ext * R);
    for (size_t e = 0; e < S_ext; e++) memcpy(&ext[e * R], &sym[((e + L - head % L) % L) * R], R * sizeof(soft_t));
    std::vector<uint32_t> metrics(N, p.initial_start_error);
    std::vector<uint64_t> dec(S_ext * W);
    vo_update(&p, table, metrics.data(), ext.data(), S_ext, dec.data());
    size_t best = 0;
    for (size_t s = 1; s < N; s++)
        if (metrics[s] < metrics[best]) best = s;
    std::vector<uint8_t> bytes((L_ext + 7) / 8);
    vo_chainback(int(K), dec.data(), L_ext, best, bytes.data());
    auto bit = [&](size_t i) { return (bytes[i / 8] >> (7 - i % 8)) & 1u; };
    memset(out, 0, (L + 7) / 8);
    for (size_t i = 0; i < L; i++) out[i / 8] |= uint8_t(bit(head + i) << (7 - i % 8));
    *end_state = uint32_t(best);
    *ok = 1;
    for (size_t i = 0; i + 1 < K; i++)
        if (bit(head - (K - 1) + i) != bit(head + L - (K - 1) + i)) *ok = 0;
}

template <size_t K, size_t R, typename error_t, typename soft_t>
static int run(const char* name, const uint8_t (&G)[R], const DecodeSetup<soft_t, error_t>& setup, size_t frames, size_t L,
               size_t head, size_t tail, uint64_t seed) {
    // tail-biting codewords: the register starts with the frame's last K-1 bits; ~12 % of the symbols weakened or flipped
    XorShift rng(seed);
    std::vector<soft_t> symbols(frames * L * R);
    for (size_t f = 0; f < frames; f++) {
        std::vector<uint8_t> x(L);
        for (auto& b : x) b = uint8_t(rng.next() & 1u);
        uint32_t reg = 0;
        for (size_t i = 0; i + 1 < K; i++) reg = (reg << 1) | x[L - (K - 1) + i];
        for (size_t t = 0; t < L; t++) {
            reg = (reg << 1) | x[t];
            for (size_t i = 0; i < R; i++) {
                soft_t v = (__builtin_popcount(reg & uint32_t(G[i]) & ((1u << K) - 1u)) & 1) ? setup.high : setup.low;
                const uint32_t r = rng.next() % 100;
                if (r < 4) v = soft_t(-v); else if (r < 12) v = soft_t(v / 2);
                symbols[(f * L + t) * R + i] = v;
            }
        }
    }

    auto table = ViterbiBranchTable<K, R, soft_t>(G, setup.high, setup.low);
    ViterbiDecoder_HIP_Batch<K, R, error_t, soft_t> batch(table, setup.config);
    const size_t nb = (L + 7) / 8;
    const size_t ws_bytes = batch.tail_biting_workspace_bytes(frames, L, head, tail);
    soft_t* d_sym; void* d_ws; uint8_t* d_out; uint32_t* d_ends; uint8_t* d_ok;
    HIP_OK(hipMalloc((void**)&d_sym, symbols.size() * sizeof(soft_t)));
    HIP_OK(hipMalloc(&d_ws, ws_bytes));
    HIP_OK(hipMalloc((void**)&d_out, frames * nb));
    HIP_OK(hipMalloc((void**)&d_ends, frames * sizeof(uint32_t)));
    HIP_OK(hipMalloc((void**)&d_ok, frames));
    HIP_OK(hipMemcpy(d_sym, symbols.data(), symbols.size() * sizeof(soft_t), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_ws, 0xA5, ws_bytes));
    HIP_OK(hipMemset(d_out, 0xA5, frames * nb));
    HIP_OK(hipMemset(d_ends, 0xA5, frames * sizeof(uint32_t)));
    HIP_OK(hipMemset(d_ok, 0xA5, frames));
    batch.decode_tail_biting(d_sym, frames, L, d_ws, ws_bytes, d_out, d_ends, d_ok, head, tail);
    HIP_OK(hipDeviceSynchronize());
    std::vector<uint8_t> out(frames * nb), ok(frames);
    std::vector<uint32_t> ends(frames);
    HIP_OK(hipMemcpy(out.data(), d_out, out.size(), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(ends.data(), d_ends, ends.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(ok.data(), d_ok, ok.size(), hipMemcpyDeviceToHost));
    (void)hipFree(d_sym); (void)hipFree(d_ws); (void)hipFree(d_out); (void)hipFree(d_ends); (void)hipFree(d_ok);

    const size_t ext = 8 * (K - 1);
    const size_t h = head ? head : ext, t = tail ? tail : ext;
    vo_params p = {int32_t(K), int32_t(R), int32_t(sizeof(soft_t)), int32_t(sizeof(error_t)), setup.config.soft_decision_max_error,
                   setup.config.initial_start_error, setup.config.initial_non_start_error, setup.config.renormalisation_threshold};
    uint32_t G32[R];
    for (size_t i = 0; i < R; i++) G32[i] = G[i];
    std::vector<int16_t> otable(R * (vo_num_states(int(K)) / 2 ? vo_num_states(int(K)) / 2 : 1));
    vo_branch_table(int(K), int(R), G32, setup.high, setup.low, otable.data());
    size_t bad = 0, tb_ok = 0;
    std::vector<uint8_t> want(nb);
    for (size_t f = 0; f < frames; f++) {
        uint32_t want_end; uint8_t want_ok;
        reference_frame(p, otable.data(), &symbols[f * L * R], L, h, t, want.data(), &want_end, &want_ok);
        bad += memcmp(&out[f * nb], want.data(), nb) != 0 || ends[f] != want_end || ok[f] != want_ok;
        tb_ok += want_ok;
    }
    printf("%s: %zu frames of %zu bits, head %zu tail %zu, %zu valid tail-biting paths, mismatching frames=%zu\n", name, frames, L,
           h, t, tb_ok, bad);
    return bad == 0 ? 0 : 1;
}

int main() {
    const uint8_t lte[3] = {91, 117, 121};
    const uint8_t k2[2] = {3, 1};
    int rc = run<7, 3, uint16_t, int16_t>("LTE K7 R3 soft16", lte, soft16_setup(3), 1031, 40, 0, 0, 11);
    rc |= run<2, 2, uint8_t, int8_t>("K2 R2 soft8", k2, soft8_setup(2), 517, 21, 5, 9, 12);
    printf(rc == 0 ? "PASS\n" : "FAIL\n");
    return rc;
}
