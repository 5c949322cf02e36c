// run_dab_hip.cpp -- the DAB receive chain from C++: ViterbiDecoder_HIP_Batch::dab_deinterleave and ::dab_descramble
// (include/viterbi_hip/viterbi_decoder_hip_batch.h) on buffers read from a case file, checked against the images of the output buffers
// the file carries -- tests/test_gpu_cpp_dab.py writes them from the restatement of tests/dab_reference.py.  Every output buffer is
// pre-filled with 0x5A and compared whole with its image, and the input is compared with what was uploaded.
// Case file, whitespace-separated integers:
//   0 rows max_frames n spf has_counts has_map has_hist lead out_elements
//     counts[rows] map[spf] fills[rows] hist[rows * 15 n] in[rows * max_frames * n]
//     out[out_elements] n_out[rows] hist_out[rows * 15 n] fill_out[rows]
//   1 rows max_frames n_bits stride has_counts in_place
//     counts[rows] in[rows * max_frames * stride] out[rows * max_frames * stride]
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

typedef ViterbiDecoder_HIP_Batch<7, 4, uint16_t, int16_t> Batch;

static int run_deinterleave(FILE* f, Batch& batch) {
    std::vector<long long> hd, counts, map, fills, hist, in, out, n_out, hist_out, fill_out;
    if (!read_ints(f, hd, 9)) return 2;
    const size_t rows = hd[0], mf = hd[1], n = hd[2], spf = hd[3], lead = hd[7], out_elements = hd[8];
    const bool has_counts = hd[4] != 0, has_map = hd[5] != 0, has_hist = hd[6] != 0;
    if (!read_ints(f, counts, rows) || !read_ints(f, map, spf) || !read_ints(f, fills, rows) || !read_ints(f, hist, rows * 15 * n) ||
        !read_ints(f, in, rows * mf * n) || !read_ints(f, out, out_elements) || !read_ints(f, n_out, rows) ||
        !read_ints(f, hist_out, rows * 15 * n) || !read_ints(f, fill_out, rows) || lead + rows * mf * spf > out_elements)
        return 2;
    int16_t *d_in, *d_hist, *d_out, *d_hist_out;
    uint32_t *d_counts, *d_fills, *d_n_out, *d_fill_out;
    int32_t* d_map;
    if (upload(&d_in, in, in.size()) || upload(&d_hist, hist, hist.size()) || upload(&d_counts, counts, rows) || upload(&d_fills, fills, rows) ||
        upload(&d_map, map, spf) || upload(&d_out, out, out_elements, 0x5A) || upload(&d_hist_out, hist_out, hist_out.size(), 0x5A) ||
        upload(&d_n_out, n_out, rows, 0x5A) || upload(&d_fill_out, fill_out, rows, 0x5A)) { printf("HIP allocation failed\n"); return 1; }
    batch.dab_deinterleave(d_in, rows, mf, has_counts ? d_counts : nullptr, n, has_map ? d_map : nullptr, spf, has_hist ? d_hist : nullptr,
                           has_hist ? d_fills : nullptr, d_out + lead, d_n_out, d_hist_out, d_fill_out);
    HIP_OK(hipDeviceSynchronize());
    const long long bad_in = differ(d_in, in, in.size()), bad_out = differ(d_out, out, out_elements);
    const long long bad_hist = differ(d_hist_out, hist_out, hist_out.size());
    const long long bad_counts = differ(d_n_out, n_out, rows) + differ(d_fill_out, fill_out, rows);
    printf("mismatches input=%lld, output=%lld, history=%lld, counts=%lld\n", bad_in, bad_out, bad_hist, bad_counts);
    (void)hipFree(d_in); (void)hipFree(d_hist); (void)hipFree(d_counts); (void)hipFree(d_fills); (void)hipFree(d_map); (void)hipFree(d_out);
    (void)hipFree(d_hist_out); (void)hipFree(d_n_out); (void)hipFree(d_fill_out);
    return bad_in == 0 && bad_out == 0 && bad_hist == 0 && bad_counts == 0 ? 0 : 1;
}

static int run_descramble(FILE* f, Batch& batch) {
    std::vector<long long> hd, counts, in, out;
    if (!read_ints(f, hd, 6)) return 2;
    const size_t rows = hd[0], mf = hd[1], n_bits = hd[2], stride = hd[3];
    const bool has_counts = hd[4] != 0, in_place = hd[5] != 0;
    if (!read_ints(f, counts, rows) || !read_ints(f, in, rows * mf * stride) || !read_ints(f, out, rows * mf * stride)) return 2;
    uint8_t *d_in, *d_out;
    uint32_t* d_counts;
    if (upload(&d_in, in, in.size()) || upload(&d_counts, counts, rows) || upload(&d_out, out, out.size(), 0x5A)) {
        printf("HIP allocation failed\n");
        return 1;
    }
    batch.dab_descramble(d_in, rows, mf, has_counts ? d_counts : nullptr, n_bits, in_place ? d_in : d_out, stride, stride);
    HIP_OK(hipDeviceSynchronize());
    const long long bad_in = in_place ? 0 : differ(d_in, in, in.size());
    const long long bad_out = differ(in_place ? d_in : d_out, out, out.size());
    printf("mismatches input=%lld, output=%lld, history=0, counts=0\n", bad_in, bad_out);
    (void)hipFree(d_in); (void)hipFree(d_counts); (void)hipFree(d_out);
    return bad_in == 0 && bad_out == 0 ? 0 : 1;
}

int main(int argc, char** argv) {
    if (argc != 2) { printf("usage: run_dab_hip <case file>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    long long which = -1;
    if (fscanf(f, "%lld", &which) != 1 || (which != 0 && which != 1)) { printf("bad case file\n"); return 2; }

    constexpr size_t K = 7, R = 4;
    const uint8_t G[R] = {109, 79, 83, 109};
    const auto setup = soft16_setup(R);
    auto table = ViterbiBranchTable<K, R, int16_t>(G, setup.high, setup.low);
    Batch batch(table, setup.config);

    const int rc = which == 0 ? run_deinterleave(f, batch) : run_descramble(f, batch);
    fclose(f);
    if (rc == 2) printf("bad case file\n");
    printf(rc == 0 ? "PASS\n" : "FAIL\n");
    return rc;
}
