// run_marker_search_hip.cpp -- frame synchronisation from C++: ViterbiDecoder_HIP_Batch::marker_search
// (include/viterbi_hip/viterbi_decoder_hip_batch.h) on rows of bytes read from a case file, checked against the per-phase totals and the
// locks the file carries -- tests/test_gpu_cpp_marker_search.py writes it from the numpy rule (tests/marker_reference.py).  The call is
// made once in one piece and once as two accumulating calls over the halves of the rows, the second with the history of the first.
// Case file, whitespace-separated integers:
//   rows n_bits stride marker_hi32 marker_lo32 marker_bits period phase0 history_bits
//   {history_hi32 history_lo32}[rows]   bytes[rows * stride]   distance[rows * period]   count[rows * period]   lock[rows * 4]
// Prints PASS only if everything matches.
#include <hip/hip_runtime_api.h>
#include <stdio.h>

#include <vector>

#include "viterbi_hip/viterbi_decoder_hip_batch.h"
#include "test_support.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

static bool read_ints(FILE* f, std::vector<long long>& v, size_t n) {
    v.resize(n);
    for (size_t i = 0; i < n; i++)
        if (fscanf(f, "%lld", &v[i]) != 1) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) { printf("usage: run_marker_search_hip <case file>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    std::vector<long long> hd, hist_raw, bytes_raw, want_d, want_c, want_lock;
    if (!read_ints(f, hd, 9)) { printf("bad case file\n"); return 2; }
    const size_t rows = hd[0], n_bits = hd[1], stride = hd[2], P = hd[6], phase0 = hd[7];
    const uint64_t marker = (uint64_t(hd[3]) << 32) | uint64_t(hd[4]);
    const unsigned m = unsigned(hd[5]), hb = unsigned(hd[8]);
    if (!read_ints(f, hist_raw, 2 * rows) || !read_ints(f, bytes_raw, rows * stride) || !read_ints(f, want_d, rows * P) ||
        !read_ints(f, want_c, rows * P) || !read_ints(f, want_lock, rows * 4)) { printf("bad case file\n"); return 2; }
    fclose(f);

    constexpr size_t K = 7, R = 2;
    const uint8_t G[R] = {109, 79};
    const auto setup = soft16_setup(R);
    auto table = ViterbiBranchTable<K, R, int16_t>(G, setup.high, setup.low);
    ViterbiDecoder_HIP_Batch<K, R, uint16_t, int16_t> batch(table, setup.config);

    std::vector<uint8_t> bytes(bytes_raw.begin(), bytes_raw.end());
    std::vector<uint64_t> hist(rows);
    for (size_t r = 0; r < rows; r++) hist[r] = (uint64_t(hist_raw[2 * r]) << 32) | uint64_t(hist_raw[2 * r + 1]);

    uint8_t* d_bytes;
    uint64_t* d_hist;
    uint32_t *d_dist, *d_count;
    vit_hip_marker_lock* d_lock;
    HIP_OK(hipMalloc((void**)&d_bytes, bytes.size()));
    HIP_OK(hipMalloc((void**)&d_hist, rows * sizeof(uint64_t)));
    HIP_OK(hipMalloc((void**)&d_dist, rows * P * sizeof(uint32_t)));
    HIP_OK(hipMalloc((void**)&d_count, rows * P * sizeof(uint32_t)));
    HIP_OK(hipMalloc((void**)&d_lock, rows * sizeof(vit_hip_marker_lock)));
    HIP_OK(hipMemcpy(d_bytes, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_hist, hist.data(), rows * sizeof(uint64_t), hipMemcpyHostToDevice));

    std::vector<uint32_t> dist(rows * P), count(rows * P);
    std::vector<vit_hip_marker_lock> lock(rows);
    auto mismatches = [&](const char* what) -> long long {
        if (hipDeviceSynchronize() != hipSuccess) return -1;
        if (hipMemcpy(dist.data(), d_dist, dist.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
        if (hipMemcpy(count.data(), d_count, count.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
        if (hipMemcpy(lock.data(), d_lock, lock.size() * sizeof(vit_hip_marker_lock), hipMemcpyDeviceToHost) != hipSuccess) return -1;
        long long bad = 0;
        for (size_t i = 0; i < rows * P; i++) bad += dist[i] != uint32_t(want_d[i]) || count[i] != uint32_t(want_c[i]);
        for (size_t r = 0; r < rows; r++) {
            const bool ok = lock[r].phase == uint32_t(want_lock[4 * r]) && lock[r].inverted == uint32_t(want_lock[4 * r + 1]) &&
                            lock[r].errors == uint32_t(want_lock[4 * r + 2]) && lock[r].compared == uint32_t(want_lock[4 * r + 3]);
            bad += !ok;
            printf("%s, row %zu: phase %u, inverted %u, %u of %u marker bits differ%s\n", what, r, lock[r].phase, lock[r].inverted,
                   lock[r].errors, lock[r].compared, ok ? "" : "   <-- MISMATCH");
        }
        return bad;
    };

    // one call: the outputs are overwritten, whatever they held
    HIP_OK(hipMemset(d_dist, 0xFF, rows * P * sizeof(uint32_t)));
    HIP_OK(hipMemset(d_count, 0xFF, rows * P * sizeof(uint32_t)));
    HIP_OK(hipMemset(d_lock, 0xFF, rows * sizeof(vit_hip_marker_lock)));
    batch.marker_search(d_bytes, rows, n_bits, marker, m, P, d_dist, d_count, d_lock, phase0, hb ? d_hist : nullptr, hb, 0, stride);
    const long long bad_one = mismatches("one call");

    // two accumulating calls: the first n1 bits (whole bytes), then the rest with the bits in front of it as history
    long long bad_two = 0;
    const size_t n1 = n_bits / 16 * 8;
    const unsigned hb2 = unsigned(n1 + hb < m - 1 ? n1 + hb : m - 1);
    if (n1 + hb >= m && n_bits - n1 + hb2 >= m) {
        std::vector<uint64_t> hist2(rows);
        for (size_t r = 0; r < rows; r++) {
            // the 64 stream bits in front of bit n1: the history, then the row's own bits
            uint64_t w = hb ? hist[r] : 0;
            for (size_t t = n1 > 64 ? n1 - 64 : 0; t < n1; t++) w = (w << 1) | ((bytes[r * stride + t / 8] >> (7 - t % 8)) & 1u);
            hist2[r] = w;
        }
        uint64_t* d_hist2;
        HIP_OK(hipMalloc((void**)&d_hist2, rows * sizeof(uint64_t)));
        HIP_OK(hipMemcpy(d_hist2, hist2.data(), rows * sizeof(uint64_t), hipMemcpyHostToDevice));
        HIP_OK(hipMemset(d_dist, 0, rows * P * sizeof(uint32_t)));
        HIP_OK(hipMemset(d_count, 0, rows * P * sizeof(uint32_t)));
        batch.marker_search(d_bytes, rows, n1, marker, m, P, d_dist, d_count, nullptr, phase0, hb ? d_hist : nullptr, hb,
                            VIT_HIP_MARKER_ACCUMULATE, stride);
        batch.marker_search(d_bytes + n1 / 8, rows, n_bits - n1, marker, m, P, d_dist, d_count, d_lock, (phase0 + n1) % P,
                            hb2 ? d_hist2 : nullptr, hb2, VIT_HIP_MARKER_ACCUMULATE, stride);
        bad_two = mismatches("two accumulating calls");
        (void)hipFree(d_hist2);
    } else {
        printf("two accumulating calls: the case is too short to cut\n");
    }
    printf("mismatches of one call=%lld, of two accumulating calls=%lld\n", bad_one, bad_two);
    (void)hipFree(d_bytes); (void)hipFree(d_hist); (void)hipFree(d_dist); (void)hipFree(d_count); (void)hipFree(d_lock);
    const int rc = bad_one == 0 && bad_two == 0 ? 0 : 1;
    printf(rc == 0 ? "PASS\n" : "FAIL\n");
    return rc;
}
