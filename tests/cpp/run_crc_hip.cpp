// run_crc_hip.cpp -- the frame check from C++: ViterbiDecoder_HIP_Batch::crc_check (include/viterbi_hip/viterbi_decoder_hip_batch.h) on
// frames read from a case file, checked against the images of both output buffers the file carries -- tests/test_gpu_cpp_crc.py writes
// it from the reference of tests/crc_reference.py.  Both outputs are pre-filled with 0xA5 and compared whole with their images, written
// or not (0xA5A5A5A5 words where nothing is written), and the input is compared with what was uploaded.
// Case file, whitespace-separated integers:
//   width poly init xorout rows max_frames stride lead first_bit n_bits has_counts want_crc want_syndrome
//   counts[rows]   in[lead + rows * max_frames * stride]   crc[rows * max_frames]   syndrome[rows * max_frames]
// `lead` bytes in front of frame (0, 0) give the frames an odd base address.  Prints PASS only if everything matches.
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
    if (argc != 2) { printf("usage: run_crc_hip <case file>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    std::vector<long long> hd, counts, in, crc, syndrome;
    if (!read_ints(f, hd, 13)) { printf("bad case file\n"); return 2; }
    const vit_hip_crc_params code = {uint32_t(hd[0]), uint32_t(hd[1]), uint32_t(hd[2]), uint32_t(hd[3])};
    const size_t rows = hd[4], mf = hd[5], stride = hd[6], lead = hd[7], first_bit = hd[8], n_bits = hd[9];
    const bool has_counts = hd[10] != 0, want_crc = hd[11] != 0, want_syndrome = hd[12] != 0;
    const size_t bytes = lead + rows * mf * stride, frames = rows * mf;
    if (!read_ints(f, counts, rows) || !read_ints(f, in, bytes) || !read_ints(f, crc, frames) || !read_ints(f, syndrome, frames)) {
        printf("bad case file\n");
        return 2;
    }
    fclose(f);

    constexpr size_t K = 7, R = 2;
    const uint8_t G[R] = {109, 79};
    const auto setup = soft16_setup(R);
    auto table = ViterbiBranchTable<K, R, int16_t>(G, setup.high, setup.low);
    ViterbiDecoder_HIP_Batch<K, R, uint16_t, int16_t> batch(table, setup.config);

    uint8_t* d_in;
    uint32_t *d_counts, *d_crc, *d_syndrome;
    if (upload(&d_in, in, bytes) || upload(&d_counts, counts, rows) || upload(&d_crc, crc, frames, 0xA5) ||
        upload(&d_syndrome, syndrome, frames, 0xA5)) { printf("HIP allocation failed\n"); return 1; }

    batch.crc_check(code, d_in + lead, rows, mf, has_counts ? d_counts : nullptr, first_bit, n_bits, want_crc ? d_crc : nullptr,
                    want_syndrome ? d_syndrome : nullptr, stride);
    HIP_OK(hipDeviceSynchronize());
    const long long bad_in = differ(d_in, in, bytes), bad_crc = differ(d_crc, crc, frames), bad_syndrome = differ(d_syndrome, syndrome, frames);
    printf("mismatches input=%lld, crc=%lld, syndrome=%lld\n", bad_in, bad_crc, bad_syndrome);
    (void)hipFree(d_in); (void)hipFree(d_counts); (void)hipFree(d_crc); (void)hipFree(d_syndrome);
    const int rc = bad_in == 0 && bad_crc == 0 && bad_syndrome == 0 ? 0 : 1;
    printf(rc == 0 ? "PASS\n" : "FAIL\n");
    return rc;
}
