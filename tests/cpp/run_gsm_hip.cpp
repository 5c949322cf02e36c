// run_gsm_hip.cpp -- GSM channel decoding from C++: ViterbiDecoder_HIP_Batch::gsm_deinterleave, ::gsm_fire and ::gsm_tchfs
// (include/viterbi_hip/viterbi_decoder_hip_batch.h) on one small batch, checked against the arrays its case file carries --
// tests/test_gpu_cpp_gsm.py writes them from the numpy rules of viterbidecodercpp_amd/gsm.py.  The bursts lie at strides of their own; every
// output buffer is pre-filled with 0x5A and compared whole, guard bytes included.
// Case file, whitespace-separated integers:
//   rows  m  frames
//   bursts[rows][4 m][116]   then for the block mode and for the diagonal mode (no history):
//     full[rows][m][456]  class1[rows][m][378]  class2[rows][m][78]  steal[rows][m]  n_out[rows]
//   fire_in[frames][28]  fire_status[frames][4]  fire_data[frames][23]        (max_burst 12, octets LSB-first)
//   tch_in[frames][24]  tch_class2[frames][78]  speech[frames][33]  tch_status[frames][2]
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

// a device buffer of `count` T behind a 0x5A fill, `guard` more behind them
template <class T>
static T* filled(size_t count, size_t guard) {
    T* d = nullptr;
    if (hipMalloc((void**)&d, (count + guard) * sizeof(T)) != hipSuccess || hipMemset(d, 0x5A, (count + guard) * sizeof(T)) != hipSuccess) return nullptr;
    return d;
}

template <class T>
static T* upload(const std::vector<T>& h) {
    T* d = nullptr;
    if (hipMalloc((void**)&d, h.size() * sizeof(T)) != hipSuccess || hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return d;
}

// elements that differ from image[i] (row r of `width` at `stride`), and guard or gap bytes that lost their fill
template <class T>
static long long differ(const T* d, const std::vector<long long>& image, size_t rows, size_t width, size_t stride, size_t guard) {
    const size_t count = rows * stride + guard;
    std::vector<T> host(count);
    if (hipMemcpy(host.data(), d, count * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    T fill;
    memset(&fill, 0x5A, sizeof(T));
    long long bad = 0;
    for (size_t i = 0; i < count; i++) {
        const size_t r = i / stride, c = i % stride;
        bad += host[i] != (r < rows && c < width ? T(image[r * width + c]) : fill);
    }
    return bad;
}

int main(int argc, char** argv) {
    if (argc != 2) { printf("usage: run_gsm_hip <case file>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    std::vector<long long> hd, bursts, full[2], class1[2], class2[2], steal[2], n_out[2], fire_in, fire_status, fire_data, tch_in, tch_c2, speech, tch_status;
    bool ok = read_ints(f, hd, 3) && hd[0] > 0 && hd[1] > 0 && hd[2] > 0;
    const size_t rows = ok ? (size_t)hd[0] : 0, m = ok ? (size_t)hd[1] : 0, frames = ok ? (size_t)hd[2] : 0, blocks = rows * m;
    ok = ok && read_ints(f, bursts, rows * 4 * m * 116);
    for (int mode = 0; mode < 2; ++mode)
        ok = ok && read_ints(f, full[mode], blocks * 456) && read_ints(f, class1[mode], blocks * 378) && read_ints(f, class2[mode], blocks * 78) &&
             read_ints(f, steal[mode], blocks) && read_ints(f, n_out[mode], rows);
    ok = ok && read_ints(f, fire_in, frames * 28) && read_ints(f, fire_status, frames * 4) && read_ints(f, fire_data, frames * 23) &&
         read_ints(f, tch_in, frames * 24) && read_ints(f, tch_c2, frames * 78) && read_ints(f, speech, frames * 33) && read_ints(f, tch_status, frames * 2);
    fclose(f);
    if (!ok) { printf("bad case file\n"); return 2; }

    constexpr size_t K = 5, R = 2;
    const uint16_t G[R] = {25, 27};
    const auto setup = soft16_setup(R);
    auto table = ViterbiBranchTable<K, R, int16_t>(G, setup.high, setup.low);
    ViterbiDecoder_HIP_Batch<K, R, uint16_t, int16_t> batch(table, setup.config);

    // bursts 119 elements apart, rows 5 elements further apart than their bursts
    const size_t bs = 119, rs = 4 * m * bs + 5;
    std::vector<int16_t> h_in(rows * rs, -77);
    for (size_t r = 0; r < rows; ++r)
        for (size_t b = 0; b < 4 * m; ++b)
            for (size_t e = 0; e < 116; ++e) h_in[r * rs + b * bs + e] = (int16_t)bursts[(r * 4 * m + b) * 116 + e];
    int16_t* d_in = upload(h_in);
    if (!d_in) { printf("no memory\n"); return 1; }
    long long bad_out = 0;
    for (int mode = 0; mode < 2; ++mode) {
        int16_t *d_full = filled<int16_t>(blocks * 456, 8), *d_c1 = filled<int16_t>(blocks * 378, 8), *d_c2 = filled<int16_t>(blocks * 78, 8);
        int32_t* d_steal = filled<int32_t>(blocks, 2);
        uint32_t* d_n = filled<uint32_t>(rows, 2);
        int16_t* d_hist = filled<int16_t>(rows * 464, 8);
        uint32_t* d_fill = filled<uint32_t>(rows, 2);
        if (!d_full || !d_c1 || !d_c2 || !d_steal || !d_n || !d_hist || !d_fill) { printf("no memory\n"); return 1; }
        batch.gsm_deinterleave(d_in, rows, 4 * m, mode ? VIT_HIP_GSM_DIAGONAL : VIT_HIP_GSM_BLOCK, d_full, d_c1, d_c2, d_steal, d_n, 0, nullptr, nullptr,
                               mode ? d_hist : nullptr, mode ? d_fill : nullptr, rs, bs);
        HIP_OK(hipDeviceSynchronize());
        bad_out += differ(d_full, full[mode], 1, blocks * 456, blocks * 456, 8) + differ(d_c1, class1[mode], 1, blocks * 378, blocks * 378, 8) +
                   differ(d_c2, class2[mode], 1, blocks * 78, blocks * 78, 8) + differ(d_steal, steal[mode], 1, blocks, blocks, 2) +
                   differ((int32_t*)d_n, n_out[mode], 1, rows, rows, 2);
        if (mode) {                                                    // the carried state: the last four bursts of every row, 4
            std::vector<long long> last(rows * 464), four(rows, 4);
            for (size_t r = 0; r < rows; ++r)
                for (size_t e = 0; e < 464; ++e) last[r * 464 + e] = bursts[(r * 4 * m + 4 * m - 4) * 116 + e];
            bad_out += differ(d_hist, last, 1, rows * 464, rows * 464, 8) + differ((int32_t*)d_fill, four, 1, rows, rows, 2);
        } else {
            bad_out += differ(d_hist, {}, 0, 0, 1, rows * 464 + 8);    // untouched
        }
        (void)hipFree(d_full); (void)hipFree(d_c1); (void)hipFree(d_c2); (void)hipFree(d_steal); (void)hipFree(d_n); (void)hipFree(d_hist); (void)hipFree(d_fill);
    }

    // the Fire code: frames 30 bytes apart, data rows 25
    const size_t fs = 30, ds = 25;
    std::vector<uint8_t> h_fire(frames * fs, 0xEE);
    for (size_t r = 0; r < frames; ++r)
        for (size_t i = 0; i < 28; ++i) h_fire[r * fs + i] = (uint8_t)fire_in[r * 28 + i];
    uint8_t* d_fire = upload(h_fire);
    int32_t* d_fstatus = filled<int32_t>(frames * 4, 4);
    uint8_t* d_data = filled<uint8_t>(frames * ds, 8);
    if (!d_fire || !d_fstatus || !d_data) { printf("no memory\n"); return 1; }
    batch.gsm_fire(d_fire, frames, (vit_hip_gsm_fire*)d_fstatus, d_data, 12, VIT_HIP_GSM_LSB_FIRST, fs, ds);
    HIP_OK(hipDeviceSynchronize());
    const long long bad_fire = differ(d_fstatus, fire_status, frames, 4, 4, 4) + differ(d_data, fire_data, frames, 23, ds, 8);

    // the TCH/FS frame: decoded bytes 26 apart, speech rows 36
    const size_t ts = 26, ss = 36;
    std::vector<uint8_t> h_tch(frames * ts, 0xEE);
    std::vector<int16_t> h_c2(frames * 78);
    for (size_t r = 0; r < frames; ++r)
        for (size_t i = 0; i < 24; ++i) h_tch[r * ts + i] = (uint8_t)tch_in[r * 24 + i];
    for (size_t i = 0; i < frames * 78; ++i) h_c2[i] = (int16_t)tch_c2[i];
    uint8_t* d_tch = upload(h_tch);
    int16_t* d_tc2 = upload(h_c2);
    uint8_t* d_speech = filled<uint8_t>(frames * ss, 8);
    int32_t* d_tstatus = filled<int32_t>(frames * 2, 4);
    if (!d_tch || !d_tc2 || !d_speech || !d_tstatus) { printf("no memory\n"); return 1; }
    batch.gsm_tchfs(d_tch, d_tc2, frames, d_speech, (vit_hip_gsm_tchfs*)d_tstatus, ts, ss);
    HIP_OK(hipDeviceSynchronize());
    const long long bad_tch = differ(d_speech, speech, frames, 33, ss, 8) + differ(d_tstatus, tch_status, frames, 2, 2, 4);
    printf("mismatches deinterleave=%lld, fire=%lld, tchfs=%lld\n", bad_out, bad_fire, bad_tch);
    (void)hipFree(d_in); (void)hipFree(d_fire); (void)hipFree(d_fstatus); (void)hipFree(d_data); (void)hipFree(d_tch); (void)hipFree(d_tc2);
    (void)hipFree(d_speech); (void)hipFree(d_tstatus);
    const int rc = bad_out == 0 && bad_fire == 0 && bad_tch == 0 ? 0 : 1;
    printf(rc == 0 ? "PASS\n" : "FAIL\n");
    return rc;
}
