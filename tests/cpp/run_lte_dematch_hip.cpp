// run_lte_dematch_hip.cpp -- LTE rate de-matching from C++: ViterbiDecoder_HIP_Batch::lte_rate_dematch
// (include/viterbi_hip/viterbi_decoder_hip_batch.h) on soft bits read from a case file, checked against the image of the output buffer
// the file carries -- tests/test_gpu_cpp_lte_dematch.py writes it from the scalar loop of tests/lte_reference.py.  The output buffer is
// pre-filled with 0x5A and compared whole with its image (`lead` elements in front of the output and a guard behind it keep the fill),
// and the input is compared with what was uploaded.
// Case file, whitespace-separated integers:
//   frames D E_max n_received stride has_offsets has_counts mask_bytes period shift clamp_lo clamp_hi lead out_elements
//   offsets[frames]   counts[frames]   mask[mask_bytes]   received[n_received]   out[out_elements]
// Prints PASS only if everything matches.
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <string.h>

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

template <class T>
static int upload(T** d, const std::vector<long long>& raw, size_t count, int fill = -1) {
    std::vector<T> host(count ? count : 1);
    if (hipMalloc((void**)d, host.size() * sizeof(T)) != hipSuccess) return 1;
    if (fill >= 0) return hipMemset(*d, fill, host.size() * sizeof(T)) != hipSuccess;         // an output: `raw` is its image, for later
    for (size_t i = 0; i < count; i++) host[i] = T(raw[i]);
    return hipMemcpy(*d, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess;
}

template <class T>
static long long differ(const T* d, const std::vector<long long>& image, size_t count) {
    std::vector<T> host(count ? count : 1);
    if (hipMemcpy(host.data(), d, count * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    long long bad = 0;
    for (size_t i = 0; i < count; i++) bad += host[i] != T(image[i]);
    return bad;
}

int main(int argc, char** argv) {
    if (argc != 2) { printf("usage: run_lte_dematch_hip <case file>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    std::vector<long long> hd, offsets, counts, mask, in, out;
    if (!read_ints(f, hd, 14)) { printf("bad case file\n"); return 2; }
    const size_t frames = hd[0], D = hd[1], E_max = hd[2], n = hd[3], stride = hd[4], mask_bytes = hd[7], period = hd[8], lead = hd[12],
                 out_elements = hd[13];
    const bool has_offsets = hd[5] != 0, has_counts = hd[6] != 0;
    const unsigned shift = unsigned(hd[9]);
    const int lo = int(hd[10]), hi = int(hd[11]);
    if (!read_ints(f, offsets, frames) || !read_ints(f, counts, frames) || !read_ints(f, mask, mask_bytes) || !read_ints(f, in, n) ||
        !read_ints(f, out, out_elements) || lead + frames * D * 3 > out_elements) {
        printf("bad case file\n");
        return 2;
    }
    fclose(f);

    constexpr size_t K = 7, R = 3;
    const uint8_t G[R] = {91, 121, 117};
    const auto setup = soft16_setup(R);
    auto table = ViterbiBranchTable<K, R, int16_t>(G, setup.high, setup.low);
    ViterbiDecoder_HIP_Batch<K, R, uint16_t, int16_t> batch(table, setup.config);

    int16_t *d_in, *d_out;
    uint32_t *d_offsets, *d_counts;
    uint8_t* d_mask;
    if (upload(&d_in, in, n) || upload(&d_offsets, offsets, frames) || upload(&d_counts, counts, frames) || upload(&d_mask, mask, mask_bytes) ||
        upload(&d_out, out, out_elements, 0x5A)) { printf("HIP allocation failed\n"); return 1; }

    batch.lte_rate_dematch(d_in, n, stride, has_offsets ? d_offsets : nullptr, has_counts ? d_counts : nullptr, frames, D, E_max,
                           mask_bytes ? d_mask : nullptr, period, shift, lo, hi, d_out + lead);
    HIP_OK(hipDeviceSynchronize());
    const long long bad_in = differ(d_in, in, n), bad_out = differ(d_out, out, out_elements);
    printf("mismatches input=%lld, output=%lld\n", bad_in, bad_out);
    (void)hipFree(d_in); (void)hipFree(d_offsets); (void)hipFree(d_counts); (void)hipFree(d_mask); (void)hipFree(d_out);
    const int rc = bad_in == 0 && bad_out == 0 ? 0 : 1;
    printf(rc == 0 ? "PASS\n" : "FAIL\n");
    return rc;
}
