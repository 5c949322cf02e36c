// run_dvb_hip.cpp -- the DVB-S outer stages from C++: ViterbiDecoder_HIP_Batch::deinterleave / dvb_derandomize
// (include/viterbi_hip/viterbi_decoder_hip_batch.h) on packets read from a case file, checked against the images of the output buffers
// the file carries -- tests/test_gpu_cpp_dvb.py writes it from the numpy rules of viterbidecodercpp_amd.dvb.
// Every output buffer is pre-filled with 0xA5 and compared whole with its image, written or not: the de-interleaved packets, their
// counts, the new history and fill; then, on the de-interleaved packets as they stand, the derandomised packets, the next phases
// and the sync errors (packet_bytes >= 188 only; 0xA5A5A5A5 words where nothing is written).
// Case file, whitespace-separated integers:
//   branches cell packet_bytes rows max_frames stride has_history derandomize
//   counts[rows]   fills[rows]   phases[rows]   in[rows * max_frames * stride]   hist[rows * H * n] if has_history
//   out[rows * max_frames * stride]   n_out[rows]   hist_out[rows * H * n]   fill_out[rows]
//   if derandomize: packets[rows * max_frames * 188]   phase_out[rows]   sync_errors[rows * max_frames]
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
    if (argc != 2) { printf("usage: run_dvb_hip <case file>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    std::vector<long long> hd, counts, fills, phases, in, hist, out, n_out, hist_out, fill_out, packets, phase_out, sync_errors;
    if (!read_ints(f, hd, 8)) { printf("bad case file\n"); return 2; }
    const size_t B = hd[0], M = hd[1], n = hd[2], rows = hd[3], mf = hd[4], stride = hd[5];
    const bool has_history = hd[6] != 0, derandomize = hd[7] != 0;
    const size_t H = ((B - 1) * M * B + n - 1) / n, bytes = rows * mf * stride, hbytes = rows * H * n;
    if (!read_ints(f, counts, rows) || !read_ints(f, fills, rows) || !read_ints(f, phases, rows) || !read_ints(f, in, bytes) ||
        !read_ints(f, hist, has_history ? hbytes : 0) || !read_ints(f, out, bytes) || !read_ints(f, n_out, rows) ||
        !read_ints(f, hist_out, hbytes) || !read_ints(f, fill_out, rows)) { printf("bad case file\n"); return 2; }
    if (derandomize && (!read_ints(f, packets, rows * mf * 188) || !read_ints(f, phase_out, rows) || !read_ints(f, sync_errors, rows * mf))) {
        printf("bad case file\n");
        return 2;
    }
    fclose(f);

    constexpr size_t K = 7, R = 2;
    const uint8_t G[R] = {109, 79};
    const auto setup = soft16_setup(R);
    auto table = ViterbiBranchTable<K, R, int16_t>(G, setup.high, setup.low);
    ViterbiDecoder_HIP_Batch<K, R, uint16_t, int16_t> batch(table, setup.config);

    uint8_t *d_in, *d_hist = nullptr, *d_out, *d_hist_out, *d_packets;
    uint32_t *d_counts, *d_fills, *d_phases, *d_n_out, *d_fill_out, *d_phase_out, *d_sync;
    if (upload(&d_in, in, bytes) || upload(&d_counts, counts, rows) || upload(&d_fills, fills, rows) || upload(&d_phases, phases, rows) ||
        (has_history && upload(&d_hist, hist, hbytes)) || upload(&d_out, out, bytes, 0xA5) || upload(&d_hist_out, hist_out, hbytes, 0xA5) ||
        upload(&d_n_out, n_out, rows, 0xA5) || upload(&d_fill_out, fill_out, rows, 0xA5) || upload(&d_packets, packets, rows * mf * 188, 0xA5) ||
        upload(&d_phase_out, phase_out, rows, 0xA5) || upload(&d_sync, sync_errors, rows * mf, 0xA5)) { printf("HIP allocation failed\n"); return 1; }

    batch.deinterleave(d_in, rows, mf, d_counts, B, M, n, d_hist, has_history ? d_fills : nullptr, d_out, d_n_out, d_hist_out, d_fill_out, stride, stride);
    HIP_OK(hipDeviceSynchronize());
    const long long bad_in = differ(d_in, in, bytes);
    const long long bad_deint = differ(d_out, out, bytes) + differ(d_n_out, n_out, rows) + differ(d_hist_out, hist_out, hbytes) + differ(d_fill_out, fill_out, rows);
    long long written = 0;
    for (size_t r = 0; r < rows; r++) written += n_out[r];
    printf("deinterleave: %lld packets out\n", written);

    long long bad_derand = 0;
    if (derandomize) {
        batch.dvb_derandomize(d_out, n, rows, mf, d_n_out, d_phases, d_packets, d_phase_out, nullptr, d_sync, stride);
        HIP_OK(hipDeviceSynchronize());
        bad_derand = differ(d_packets, packets, rows * mf * 188) + differ(d_phase_out, phase_out, rows) + differ(d_sync, sync_errors, rows * mf) +
                     differ(d_out, out, bytes);
    }
    printf("mismatches input=%lld, deinterleave=%lld, derandomize=%lld\n", bad_in, bad_deint, bad_derand);
    (void)hipFree(d_in); (void)hipFree(d_hist); (void)hipFree(d_out); (void)hipFree(d_hist_out); (void)hipFree(d_packets); (void)hipFree(d_counts);
    (void)hipFree(d_fills); (void)hipFree(d_phases); (void)hipFree(d_n_out); (void)hipFree(d_fill_out); (void)hipFree(d_phase_out); (void)hipFree(d_sync);
    const int rc = bad_in == 0 && bad_deint == 0 && bad_derand == 0 ? 0 : 1;
    printf(rc == 0 ? "PASS\n" : "FAIL\n");
    return rc;
}
