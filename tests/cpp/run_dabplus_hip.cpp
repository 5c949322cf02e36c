// run_dabplus_hip.cpp -- DAB+ superframes from C++: ViterbiDecoder_HIP_Batch::dabplus_sync and ::dabplus_au_table
// (include/viterbi_hip/viterbi_decoder_hip_batch.h) on buffers read from a case file, checked against the images of the output buffers
// the file carries -- tests/test_gpu_cpp_dabplus.py writes them from the restatement of tests/dabplus_reference.py.  Every output buffer
// is pre-filled (0x5A, or the totals the case accumulates onto) and compared whole with its image, and the input is compared with what
// was uploaded.
// Case file, whitespace-separated integers:
//   0 rows max_frames frame_bytes frame_stride frame0 has_counts accumulate
//     counts[rows] in[rows * max_frames * frame_stride] hits_in[rows * 5] count_in[rows * 5]
//     hits[rows * 5] count[rows * 5] lock[rows * 4]
//   1 rows max_frames s stride has_counts has_status
//     counts[rows] in[rows * max_frames * stride] status[rows * max_frames * s] info[rows * max_frames] au[rows * max_frames * 18]
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

static int run_sync(FILE* f, Batch& batch) {
    std::vector<long long> hd, counts, in, hits_in, count_in, hits, count, lock;
    if (!read_ints(f, hd, 7)) return 2;
    const size_t rows = hd[0], mf = hd[1], fb = hd[2], fs = hd[3];
    const unsigned frame0 = (unsigned)hd[4];
    const bool has_counts = hd[5] != 0, accumulate = hd[6] != 0;
    if (!read_ints(f, counts, rows) || !read_ints(f, in, rows * mf * fs) || !read_ints(f, hits_in, rows * 5) || !read_ints(f, count_in, rows * 5) ||
        !read_ints(f, hits, rows * 5) || !read_ints(f, count, rows * 5) || !read_ints(f, lock, rows * 4))
        return 2;
    uint8_t* d_in;
    uint32_t *d_counts, *d_hits, *d_count, *d_lock;
    if (upload(&d_in, in, in.size()) || upload(&d_counts, counts, rows) || upload(&d_hits, hits_in, rows * 5, accumulate ? -1 : 0x5A) ||
        upload(&d_count, count_in, rows * 5, accumulate ? -1 : 0x5A) || upload(&d_lock, lock, rows * 4, 0x5A)) {
        printf("HIP allocation failed\n");
        return 1;
    }
    batch.dabplus_sync(d_in, rows, mf, has_counts ? d_counts : nullptr, fb, frame0, d_hits, d_count, (vit_hip_marker_lock*)d_lock,
                       accumulate ? VIT_HIP_MARKER_ACCUMULATE : 0u, 0, fs);
    HIP_OK(hipDeviceSynchronize());
    const long long bad_in = differ(d_in, in, in.size());
    const long long bad_out = differ(d_hits, hits, rows * 5) + differ(d_count, count, rows * 5) + differ(d_lock, lock, rows * 4);
    printf("mismatches input=%lld, output=%lld\n", bad_in, bad_out);
    (void)hipFree(d_in); (void)hipFree(d_counts); (void)hipFree(d_hits); (void)hipFree(d_count); (void)hipFree(d_lock);
    return bad_in == 0 && bad_out == 0 ? 0 : 1;
}

static int run_au(FILE* f, Batch& batch) {
    std::vector<long long> hd, counts, in, status, info, au;
    if (!read_ints(f, hd, 6)) return 2;
    const size_t rows = hd[0], mf = hd[1], s = hd[2], stride = hd[3];
    const bool has_counts = hd[4] != 0, has_status = hd[5] != 0;
    if (!read_ints(f, counts, rows) || !read_ints(f, in, rows * mf * stride) || !read_ints(f, status, rows * mf * s) ||
        !read_ints(f, info, rows * mf) || !read_ints(f, au, rows * mf * 18))
        return 2;
    uint8_t* d_in;
    uint32_t *d_counts, *d_info, *d_au;
    int32_t* d_status;
    if (upload(&d_in, in, in.size()) || upload(&d_counts, counts, rows) || upload(&d_status, status, status.size()) ||
        upload(&d_info, info, info.size(), 0x5A) || upload(&d_au, au, au.size(), 0x5A)) {
        printf("HIP allocation failed\n");
        return 1;
    }
    batch.dabplus_au_table(d_in, rows, mf, has_counts ? d_counts : nullptr, (unsigned)s, has_status ? d_status : nullptr, d_info,
                           (vit_hip_dabplus_au*)d_au, stride);
    HIP_OK(hipDeviceSynchronize());
    const long long bad_in = differ(d_in, in, in.size());
    const long long bad_out = differ(d_info, info, info.size()) + differ(d_au, au, au.size());
    printf("mismatches input=%lld, output=%lld\n", bad_in, bad_out);
    (void)hipFree(d_in); (void)hipFree(d_counts); (void)hipFree(d_status); (void)hipFree(d_info); (void)hipFree(d_au);
    return bad_in == 0 && bad_out == 0 ? 0 : 1;
}

int main(int argc, char** argv) {
    if (argc != 2) { printf("usage: run_dabplus_hip <case file>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    long long which = -1;
    if (fscanf(f, "%lld", &which) != 1 || (which != 0 && which != 1)) { printf("bad case file\n"); return 2; }

    constexpr size_t K = 7, R = 4;
    const uint8_t G[R] = {109, 79, 83, 109};
    const auto setup = soft16_setup(R);
    auto table = ViterbiBranchTable<K, R, int16_t>(G, setup.high, setup.low);
    Batch batch(table, setup.config);

    const int rc = which == 0 ? run_sync(f, batch) : run_au(f, batch);
    fclose(f);
    if (rc == 2) printf("bad case file\n");
    printf(rc == 0 ? "PASS\n" : "FAIL\n");
    return rc;
}
