// run_wifi_hip.cpp -- the 802.11a/g receive chain from C++: ViterbiDecoder_HIP_Batch::wifi_deinterleave, ::decode, ::wifi_signal_parse,
// ::wifi_descramble (include/viterbi_hip/viterbi_decoder_hip_batch.h) on the soft bits of a case file, the six calls of the chain with the
// per-frame arguments of the DATA stages pointing into the SIGNAL structs on the device, checked against the arrays the file carries --
// tests/test_gpu_cpp_wifi.py writes them from the CPU composition (the numpy rules around the oracle decoder).  The PSDU buffer is
// pre-filled with 0x5A and compared whole with its image.
// Case file, whitespace-separated integers:
//   frames max_sym max_length
//   signal_soft[frames][48]   data_soft[frames][max_sym * 288]   signal[frames][5]   status[frames][4]   psdu[frames][max_length]
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
static long long differ(const T* d, const std::vector<long long>& image, size_t count) {
    std::vector<T> host(count ? count : 1);
    if (hipMemcpy(host.data(), d, count * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    long long bad = 0;
    for (size_t i = 0; i < count; i++) bad += host[i] != T(image[i]);
    return bad;
}

int main(int argc, char** argv) {
    if (argc != 2) { printf("usage: run_wifi_hip <case file>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    std::vector<long long> hd, sig_soft, data_soft, signal, status, psdu;
    if (!read_ints(f, hd, 3)) { printf("bad case file\n"); return 2; }
    const size_t frames = hd[0], max_sym = hd[1], max_length = hd[2];
    const size_t S = max_sym * 216, L = S - 6, nb = (L + 7) / 8;
    if (!frames || !max_sym || !read_ints(f, sig_soft, frames * 48) || !read_ints(f, data_soft, frames * max_sym * 288) ||
        !read_ints(f, signal, frames * 5) || !read_ints(f, status, frames * 4) || !read_ints(f, psdu, frames * max_length)) {
        printf("bad case file\n");
        return 2;
    }
    fclose(f);

    constexpr size_t K = 7, R = 2;
    const uint8_t G[R] = {109, 79};
    const auto setup = soft16_setup(R);
    auto table = ViterbiBranchTable<K, R, int16_t>(G, setup.high, setup.low);
    ViterbiDecoder_HIP_Batch<K, R, uint16_t, int16_t> batch(table, setup.config);

    std::vector<int16_t> h_sig(sig_soft.begin(), sig_soft.end()), h_data(data_soft.begin(), data_soft.end());
    int16_t *d_sig, *d_data, *d_sig_sym, *d_sym;
    uint8_t *d_sig_bytes, *d_bytes, *d_psdu;
    vit_hip_wifi_signal* d_signal;
    vit_hip_wifi_status* d_status;
    void* d_ws;
    const size_t ws_sig = batch.workspace_bytes(frames, 18), ws_data = batch.workspace_bytes(frames, L), ws = ws_sig > ws_data ? ws_sig : ws_data;
    HIP_OK(hipMalloc((void**)&d_sig, h_sig.size() * 2));
    HIP_OK(hipMalloc((void**)&d_data, h_data.size() * 2));
    HIP_OK(hipMalloc((void**)&d_sig_sym, frames * 24 * 2 * 2));
    HIP_OK(hipMalloc((void**)&d_sym, frames * S * 2 * 2));
    HIP_OK(hipMalloc((void**)&d_sig_bytes, frames * 3));
    HIP_OK(hipMalloc((void**)&d_bytes, frames * nb));
    HIP_OK(hipMalloc((void**)&d_psdu, frames * max_length + 1));
    HIP_OK(hipMalloc((void**)&d_signal, frames * sizeof(vit_hip_wifi_signal)));
    HIP_OK(hipMalloc((void**)&d_status, frames * sizeof(vit_hip_wifi_status)));
    HIP_OK(hipMalloc(&d_ws, ws));
    HIP_OK(hipMemcpy(d_sig, h_sig.data(), h_sig.size() * 2, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_data, h_data.data(), h_data.size() * 2, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_psdu, 0x5A, frames * max_length + 1));

    batch.wifi_deinterleave(d_sig, frames, 1, 24, d_sig_sym, 0, nullptr, nullptr, nullptr, 0, 48);
    batch.decode(d_sig_sym, frames, 18, d_ws, ws, d_sig_bytes);
    batch.wifi_signal_parse(d_sig_bytes, frames, d_signal);
    const uint32_t* col = (const uint32_t*)d_signal;               // rate_index, length, n_sym, n_steps, valid
    batch.wifi_deinterleave(d_data, frames, max_sym, S, d_sym, 0, col, col + 2, col + 3, 5);
    batch.decode(d_sym, frames, L, d_ws, ws, d_bytes);
    batch.wifi_descramble(d_bytes, frames, S, col + 1, 5, max_length, d_psdu, d_status);
    HIP_OK(hipDeviceSynchronize());

    const long long bad_signal = differ((const uint32_t*)d_signal, signal, frames * 5), bad_status = differ((const uint32_t*)d_status, status, frames * 4),
                    bad_psdu = differ(d_psdu, psdu, frames * max_length);
    printf("mismatches signal=%lld, status=%lld, psdu=%lld\n", bad_signal, bad_status, bad_psdu);
    (void)hipFree(d_sig); (void)hipFree(d_data); (void)hipFree(d_sig_sym); (void)hipFree(d_sym); (void)hipFree(d_sig_bytes); (void)hipFree(d_bytes);
    (void)hipFree(d_psdu); (void)hipFree(d_signal); (void)hipFree(d_status); (void)hipFree(d_ws);
    const int rc = bad_signal == 0 && bad_status == 0 && bad_psdu == 0 ? 0 : 1;
    printf(rc == 0 ? "PASS\n" : "FAIL\n");
    return rc;
}
