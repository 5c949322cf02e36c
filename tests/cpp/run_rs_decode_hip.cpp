// run_rs_decode_hip.cpp -- Reed-Solomon decoding from C++: ViterbiDecoder_HIP_Batch::rs_create / rs_decode
// (include/viterbi_hip/viterbi_decoder_hip_batch.h) on frames read from a case file, checked against the images of the output buffers
// the file carries -- tests/test_gpu_cpp_rs_decode.py writes it from the rule of tests/rs_reference.py.
// The call is made once in place (every byte of the buffer must equal the image, written or not) and once out of place into a buffer
// filled with 0xA5: the n * interleave bytes of every frame below its row's count must equal the image, every other byte must still be
// 0xA5, and the input must be untouched.  The status buffer is pre-filled with 0xA5A5A5A5 both times and compared whole.
// Case file, whitespace-separated integers:
//   gfpoly fcr prim nroots pad dual_basis interleave rows max_frames stride has_counts
//   counts[rows] if has_counts   in[rows * max_frames * stride]   image[rows * max_frames * stride]
//   status[rows * max_frames * interleave]
// Prints PASS only if everything matches.
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
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
    if (argc != 2) { printf("usage: run_rs_decode_hip <case file>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    std::vector<long long> hd, counts_raw, in_raw, image_raw, status_raw;
    if (!read_ints(f, hd, 11)) { printf("bad case file\n"); return 2; }
    const vit_hip_rs_params params = {uint32_t(hd[0]), uint32_t(hd[1]), uint32_t(hd[2]), uint32_t(hd[3]), uint32_t(hd[4]), uint32_t(hd[5])};
    const size_t I = hd[6], rows = hd[7], max_frames = hd[8], stride = hd[9];
    const bool has_counts = hd[10] != 0;
    const size_t n = 255 - params.pad, bytes = rows * max_frames * stride, entries = rows * max_frames * I;
    if (!read_ints(f, counts_raw, has_counts ? rows : 0) || !read_ints(f, in_raw, bytes) || !read_ints(f, image_raw, bytes) ||
        !read_ints(f, status_raw, entries)) { printf("bad case file\n"); return 2; }
    fclose(f);

    constexpr size_t K = 7, R = 2;
    const uint8_t G[R] = {109, 79};
    const auto setup = soft16_setup(R);
    auto table = ViterbiBranchTable<K, R, int16_t>(G, setup.high, setup.low);
    ViterbiDecoder_HIP_Batch<K, R, uint16_t, int16_t> batch(table, setup.config);
    vit_hip_rs_code code = batch.rs_create(params);

    std::vector<uint8_t> in(bytes), got(bytes);
    std::vector<uint32_t> counts(rows);
    std::vector<int32_t> status(entries);
    for (size_t i = 0; i < bytes; i++) in[i] = uint8_t(in_raw[i]);
    for (size_t r = 0; r < rows; r++) counts[r] = has_counts ? uint32_t(counts_raw[r]) : uint32_t(max_frames);

    uint8_t *d_a, *d_b;
    uint32_t* d_counts;
    int32_t* d_status;
    HIP_OK(hipMalloc((void**)&d_a, bytes));
    HIP_OK(hipMalloc((void**)&d_b, bytes));
    HIP_OK(hipMalloc((void**)&d_counts, rows * sizeof(uint32_t)));
    HIP_OK(hipMalloc((void**)&d_status, entries * sizeof(int32_t)));
    HIP_OK(hipMemcpy(d_counts, counts.data(), rows * sizeof(uint32_t), hipMemcpyHostToDevice));

    // in place
    HIP_OK(hipMemcpy(d_a, in.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_status, 0xA5, entries * sizeof(int32_t)));
    batch.rs_decode(code, d_a, d_a, rows, max_frames, has_counts ? d_counts : nullptr, I, d_status, stride);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(got.data(), d_a, bytes, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(status.data(), d_status, entries * sizeof(int32_t), hipMemcpyDeviceToHost));
    long long bad_in_place = 0, corrected = 0, failed = 0;
    for (size_t i = 0; i < bytes; i++) bad_in_place += got[i] != uint8_t(image_raw[i]);
    for (size_t i = 0; i < entries; i++) {
        bad_in_place += status[i] != int32_t(status_raw[i]);
        corrected += status[i] > 0 && status[i] <= 32;
        failed += status[i] == -1;
    }
    printf("in place: %lld codewords corrected, %lld left as received\n", corrected, failed);

    // out of place
    HIP_OK(hipMemcpy(d_a, in.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_b, 0xA5, bytes));
    HIP_OK(hipMemset(d_status, 0xA5, entries * sizeof(int32_t)));
    batch.rs_decode(code, d_a, d_b, rows, max_frames, has_counts ? d_counts : nullptr, I, d_status, stride);
    HIP_OK(hipDeviceSynchronize());
    long long bad_out = 0;
    HIP_OK(hipMemcpy(got.data(), d_a, bytes, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < bytes; i++) bad_out += got[i] != in[i];
    HIP_OK(hipMemcpy(got.data(), d_b, bytes, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(status.data(), d_status, entries * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t r = 0; r < rows; r++)
        for (size_t fr = 0; fr < max_frames; fr++)
            for (size_t i = 0; i < stride; i++) {
                const size_t at = (r * max_frames + fr) * stride + i;
                const bool written = fr < std::min<size_t>(counts[r], max_frames) && i < n * I;
                bad_out += got[at] != (written ? uint8_t(image_raw[at]) : 0xA5);
            }
    for (size_t i = 0; i < entries; i++) bad_out += status[i] != int32_t(status_raw[i]);

    printf("mismatches in place=%lld, out of place=%lld\n", bad_in_place, bad_out);
    batch.rs_destroy(code);
    (void)hipFree(d_a); (void)hipFree(d_b); (void)hipFree(d_counts); (void)hipFree(d_status);
    const int rc = bad_in_place == 0 && bad_out == 0 ? 0 : 1;
    printf(rc == 0 ? "PASS\n" : "FAIL\n");
    return rc;
}
