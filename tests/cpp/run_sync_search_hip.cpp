// run_sync_search_hip.cpp -- node synchronisation from C++: ViterbiDecoder_HIP_Batch::sync_search
// (include/viterbi_hip/viterbi_decoder_hip_batch.h) on a received buffer and a set of hypotheses read from a case file, checked
// against the counts and the winner the file carries -- tests/test_gpu_cpp_sync_search.py writes it from the oracle-side composition
// (tests/sync_reference.py).  Then ::sync_build of the winner alone against the stream rule restated here.  Voyager
// <7, 2, uint16_t, int16_t> soft16.  Case file, whitespace-separated integers:
//   T W head tail n_received n_hyp period_symbols kept_per_period      (period_symbols = 0: unpunctured)
//   source_index[period_symbols]   {offset flags}[n_hyp]   received[n_received]   errors[n_hyp]   compared[n_hyp]   best
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
    if (argc != 2) { printf("usage: run_sync_search_hip <case file>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    std::vector<long long> head_line, map, hyp_raw, rec_raw, want_err, want_cmp, want_best;
    if (!read_ints(f, head_line, 8)) { printf("bad case file\n"); return 2; }
    const size_t T = head_line[0], W = head_line[1], head = head_line[2], tail = head_line[3], n_received = head_line[4],
                 n_hyp = head_line[5], period = head_line[6], kept = head_line[7];
    if (!read_ints(f, map, period) || !read_ints(f, hyp_raw, 2 * n_hyp) || !read_ints(f, rec_raw, n_received) ||
        !read_ints(f, want_err, n_hyp) || !read_ints(f, want_cmp, n_hyp) || !read_ints(f, want_best, 1)) { printf("bad case file\n"); return 2; }
    fclose(f);

    constexpr size_t K = 7, R = 2;
    const uint8_t G[R] = {109, 79};
    const auto setup = soft16_setup(R);
    auto table = ViterbiBranchTable<K, R, int16_t>(G, setup.high, setup.low);
    ViterbiDecoder_HIP_Batch<K, R, uint16_t, int16_t> batch(table, setup.config);

    std::vector<int16_t> received(rec_raw.begin(), rec_raw.end());
    std::vector<int32_t> source(map.begin(), map.end());
    std::vector<vit_hip_sync_hypothesis> hyps(n_hyp);
    for (size_t i = 0; i < n_hyp; i++) hyps[i] = {uint32_t(hyp_raw[2 * i]), uint32_t(hyp_raw[2 * i + 1])};

    const size_t ws_bytes = batch.sync_search_workspace_bytes(n_hyp, T, W, head, tail);
    if (ws_bytes == 0) { printf("the library rejects the case's shape\n"); return 1; }
    int16_t *d_rec, *d_stream;
    int32_t* d_map = nullptr;
    uint32_t *d_err, *d_cmp, *d_best;
    void* d_ws;
    HIP_OK(hipMalloc((void**)&d_rec, received.size() * sizeof(int16_t)));
    HIP_OK(hipMalloc((void**)&d_stream, T * R * sizeof(int16_t)));
    HIP_OK(hipMalloc((void**)&d_err, n_hyp * sizeof(uint32_t)));
    HIP_OK(hipMalloc((void**)&d_cmp, n_hyp * sizeof(uint32_t)));
    HIP_OK(hipMalloc((void**)&d_best, sizeof(uint32_t)));
    HIP_OK(hipMalloc(&d_ws, ws_bytes));
    if (period) {
        HIP_OK(hipMalloc((void**)&d_map, period * sizeof(int32_t)));
        HIP_OK(hipMemcpy(d_map, source.data(), period * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    HIP_OK(hipMemcpy(d_rec, received.data(), received.size() * sizeof(int16_t), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_err, 0xFF, n_hyp * sizeof(uint32_t)));
    HIP_OK(hipMemset(d_cmp, 0xFF, n_hyp * sizeof(uint32_t)));
    HIP_OK(hipMemset(d_best, 0xFF, sizeof(uint32_t)));

    batch.sync_search(d_rec, n_received, d_map, period, kept, hyps.data(), n_hyp, T, d_ws, ws_bytes, d_err, d_cmp, d_best, W, head, tail);
    HIP_OK(hipDeviceSynchronize());
    std::vector<uint32_t> err(n_hyp), cmp(n_hyp);
    uint32_t best = 0;
    HIP_OK(hipMemcpy(err.data(), d_err, n_hyp * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(cmp.data(), d_cmp, n_hyp * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(&best, d_best, sizeof(uint32_t), hipMemcpyDeviceToHost));

    size_t bad = 0;
    for (size_t i = 0; i < n_hyp; i++) {
        const bool ok = err[i] == uint32_t(want_err[i]) && cmp[i] == uint32_t(want_cmp[i]);
        bad += !ok;
        printf("hypothesis %2zu (offset %u, flags %u): %u of %u compared symbols differ%s\n", i, hyps[i].offset, hyps[i].flags, err[i], cmp[i],
               ok ? "" : "   <-- MISMATCH");
    }
    printf("mismatching hypotheses=%zu, best=%u (want %lld)\n", bad, best, want_best[0]);

    // the winner alone, as a receiver feeds it to decode_stream: every symbol against the stream rule
    size_t bad_symbols = T * R;
    if (best < n_hyp) {
        batch.sync_build(d_rec, n_received, d_map, period, kept, &hyps[best], 1, T, d_stream);
        HIP_OK(hipDeviceSynchronize());
        std::vector<int16_t> stream(T * R);
        HIP_OK(hipMemcpy(stream.data(), d_stream, stream.size() * sizeof(int16_t), hipMemcpyDeviceToHost));
        const size_t per = period ? period : R, kp = period ? kept : R;
        bad_symbols = 0;
        for (size_t k = 0; k < T * R; k++) {
            const long long s = period ? source[k % per] : (long long)(k % per);
            int v = 0;
            if (s >= 0) {
                const size_t j = hyps[best].offset + (k / per) * kp + size_t(s);
                v = received[(hyps[best].flags & VIT_HIP_SYNC_SWAP_PAIRS) ? j ^ 1 : j];
                if (hyps[best].flags & ((j & 1) ? VIT_HIP_SYNC_NEGATE_ODD : VIT_HIP_SYNC_NEGATE_EVEN)) {
                    v = int(setup.high) + int(setup.low) - v;
                    v = v < -32768 ? -32768 : v > 32767 ? 32767 : v;
                }
            }
            bad_symbols += stream[k] != int16_t(v);
        }
    }
    printf("mismatching symbols of the winner's stream=%zu\n", bad_symbols);
    (void)hipFree(d_rec); (void)hipFree(d_stream); (void)hipFree(d_err); (void)hipFree(d_cmp); (void)hipFree(d_best); (void)hipFree(d_ws);
    if (d_map) (void)hipFree(d_map);
    const int rc = bad == 0 && bad_symbols == 0 && best == uint32_t(want_best[0]) ? 0 : 1;
    printf(rc == 0 ? "PASS\n" : "FAIL\n");
    return rc;
}
