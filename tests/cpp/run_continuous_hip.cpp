// run_continuous_hip.cpp -- one long unterminated stream from C++: ViterbiDecoder_HIP_Batch::decode_stream
// (include/viterbi_hip/viterbi_decoder_hip_batch.h) on a noisy stream cut into segments, checked bit for bit against the rule
// restated on the oracle's update / chainback (oracle/viterbi_oracle.h): windows of W steps with `head` steps of lead-in and `tail`
// of look-ahead, window 0 under BEGIN from reset(0) and every other one from all-equal metrics, the last window under END ending
// in state 0 and every other one in the argmin of its final metrics, each window's share [head, head + W) stitched into one bit
// stream.  Voyager <7, 2, uint16_t, int16_t> at the defaults (W = 1024, head = tail = 48) and <5, 2, uint8_t, int8_t> with an
// explicit odd window and extension.  The segments chain as a receiver would: the next one starts head + tail steps before the end
// of the last.  Prints PASS only if every segment matches and the lightly disturbed stream comes back with under 1 % bit errors.
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "viterbi_hip/viterbi_decoder_hip_batch.h"
#include "test_support.h"
#include "../../oracle/viterbi_oracle.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

// the oracle's restatement of one segment: bits [a, b) as one byte per bit
template <typename soft_t>
static std::vector<uint8_t> reference_segment(const vo_params& p, const int16_t* table, const soft_t* sym, size_t T, size_t W,
                                              size_t head, size_t tail, bool begin, bool end) {
    const size_t K = size_t(p.K), R = size_t(p.R), N = vo_num_states(p.K), DW = vo_decision_words(p.K);
    const size_t a = begin ? 0 : head, b = end ? T - (K - 1) : T - tail;
    size_t n = (b - head) / W;
    if (n < 1) n = 1;
    std::vector<uint8_t> bits(b - a);
    for (size_t i = 0; i < n; i++) {
        const bool last = i == n - 1;
        const size_t first = i * W, steps = last ? T - first : head + W + tail;
        std::vector<uint32_t> metrics(N, p.initial_start_error);
        if (i == 0 && begin)
            for (size_t s = 1; s < N; s++) metrics[s] = p.initial_non_start_error;
        std::vector<uint64_t> dec(steps * DW);
        vo_update(&p, table, metrics.data(), sym + first * R, steps, dec.data());
        size_t best = 0;
        if (!(last && end))
            for (size_t s = 1; s < N; s++)
                if (metrics[s] < metrics[best]) best = s;
        const size_t Lw = steps - (K - 1);
        std::vector<uint8_t> bytes((Lw + 7) / 8);
        vo_chainback(int(K), dec.data(), Lw, best, bytes.data());
        const size_t lo = i == 0 ? a : head + i * W, hi = last ? b : head + (i + 1) * W;
        for (size_t j = lo; j < hi; j++) bits[j - a] = (bytes[(j - first) / 8] >> (7 - (j - first) % 8)) & 1u;
    }
    return bits;
}

template <size_t K, size_t R, typename error_t, typename soft_t>
static int run(const char* name, const uint8_t (&G)[R], const DecodeSetup<soft_t, error_t>& setup, size_t L, size_t W, size_t head,
               size_t tail, const std::vector<size_t>& windows_per_segment, uint64_t seed) {
    // one terminated stream of L bits; ~6 % of the symbols weakened or flipped
    XorShift rng(seed);
    const size_t T = L + K - 1;
    std::vector<uint8_t> x(T, 0);
    for (size_t t = 0; t < L; t++) x[t] = uint8_t(rng.next() & 1u);
    std::vector<soft_t> symbols(T * R);
    uint32_t reg = 0;
    for (size_t t = 0; t < T; t++) {
        reg = (reg << 1) | x[t];
        for (size_t i = 0; i < R; i++) {
            soft_t v = (__builtin_popcount(reg & uint32_t(G[i]) & ((1u << K) - 1u)) & 1) ? setup.high : setup.low;
            const uint32_t r = rng.next() % 100;
            if (r < 2) v = soft_t(-v); else if (r < 6) v = soft_t(v / 2);
            symbols[t * R + i] = v;
        }
    }
    auto table = ViterbiBranchTable<K, R, soft_t>(G, setup.high, setup.low);
    ViterbiDecoder_HIP_Batch<K, R, error_t, soft_t> batch(table, setup.config);
    const size_t w = W ? W : 1024, h = head ? head : 8 * (K - 1), tl = tail ? tail : 8 * (K - 1);
    vo_params p = {int32_t(K), int32_t(R), int32_t(sizeof(soft_t)), int32_t(sizeof(error_t)), setup.config.soft_decision_max_error,
                   setup.config.initial_start_error, setup.config.initial_non_start_error, setup.config.renormalisation_threshold};
    uint32_t G32[R];
    for (size_t i = 0; i < R; i++) G32[i] = G[i];
    std::vector<int16_t> otable(R * (vo_num_states(int(K)) / 2));
    vo_branch_table(int(K), int(R), G32, setup.high, setup.low, otable.data());

    soft_t* d_sym;
    HIP_OK(hipMalloc((void**)&d_sym, symbols.size() * sizeof(soft_t)));
    HIP_OK(hipMemcpy(d_sym, symbols.data(), symbols.size() * sizeof(soft_t), hipMemcpyHostToDevice));
    size_t pos = 0, bad_segments = 0, total_bits = 0, bit_errors = 0;
    for (size_t s = 0; s <= windows_per_segment.size(); s++) {
        const bool begin = s == 0, end = s == windows_per_segment.size();
        const size_t steps = end ? T - pos : h + windows_per_segment[s] * w + tl;
        if (pos + steps > T) { printf("%s: the stream is too short for the segments\n", name); return 1; }
        const size_t ws_bytes = batch.stream_workspace_bytes(steps, begin, end, W, head, tail);
        if (ws_bytes == 0) { printf("%s: segment %zu rejected\n", name, s); return 1; }
        const size_t a = begin ? 0 : h, b = end ? steps - (K - 1) : steps - tl, nb = (b - a + 7) / 8;
        void* d_ws; uint8_t* d_out;
        HIP_OK(hipMalloc(&d_ws, ws_bytes));
        HIP_OK(hipMalloc((void**)&d_out, nb + 16));
        HIP_OK(hipMemset(d_ws, 0xA5, ws_bytes));
        HIP_OK(hipMemset(d_out, 0xA5, nb + 16));
        const size_t n_bits = batch.decode_stream(d_sym + pos * R, steps, begin, end, d_ws, ws_bytes, d_out, W, head, tail);
        HIP_OK(hipDeviceSynchronize());
        std::vector<uint8_t> out(nb + 16);
        HIP_OK(hipMemcpy(out.data(), d_out, nb + 16, hipMemcpyDeviceToHost));
        (void)hipFree(d_ws); (void)hipFree(d_out);
        const std::vector<uint8_t> want = reference_segment(p, otable.data(), &symbols[pos * R], steps, w, h, tl, begin, end);
        bool bad = n_bits != want.size();
        for (size_t j = 0; j < 8 * nb && !bad; j++) {
            const uint8_t got = (out[j / 8] >> (7 - j % 8)) & 1u;
            bad = got != (j < want.size() ? want[j] : 0);             // pad bits 0
        }
        for (size_t j = nb; j < nb + 16; j++) bad = bad || out[j] != 0xA5;
        bad_segments += bad;
        for (size_t j = 0; j < want.size(); j++) bit_errors += want[j] != x[pos + a + j];
        total_bits += want.size();
        pos += steps - h - tl;
    }
    (void)hipFree(d_sym);
    printf("%s: %zu bits in %zu segments, W %zu head %zu tail %zu, %zu bit errors, mismatching segments=%zu\n", name, total_bits,
           windows_per_segment.size() + 1, w, h, tl, bit_errors, bad_segments);
    return bad_segments == 0 && total_bits == L && bit_errors * 100 < L ? 0 : 1;
}

int main() {
    const uint8_t voyager[2] = {109, 79};
    const uint8_t k5[2] = {0b10111, 0b11001};
    int rc = run<7, 2, uint16_t, int16_t>("Voyager K7 R2 soft16", voyager, soft16_setup(2), 200003, 0, 0, 0, {40, 1, 77}, 21);
    rc |= run<5, 2, uint8_t, int8_t>("K5 R2 soft8", k5, soft8_setup(2), 30011, 67, 9, 13, {3, 200, 1, 50}, 22);
    printf(rc == 0 ? "PASS\n" : "FAIL\n");
    return rc;
}
