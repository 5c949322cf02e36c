// run_is95_hip.cpp -- the IS-95A forward traffic channel from C++: ViterbiDecoder_HIP_Batch::is95_deinterleave, ::is95_channel_errors and ::is95_rate_decide
// (include/viterbi_hip/viterbi_decoder_hip_batch.h) on one small batch of mixed rates, checked against the arrays its case file carries --
// tests/test_gpu_cpp_is95.py writes them from the numpy rules of viterbidecodercpp_amd/is95.py around the oracle decoder.  Input frames
// and masks lie at strides of their own; every output buffer is pre-filled with 0x5A and compared whole, guard bytes included.
// Case file, whitespace-separated integers:
//   frames
//   symbols[frames][384]   scramble[frames][48]   out_0[frames][384]  out_1[frames][192]  out_2[frames][96]  out_3[frames][48]
//   bytes_0[frames][23]  bytes_1[frames][11]  bytes_2[frames][5]  bytes_3[frames][2]   errors[4][frames]   compared[4][frames]
//   syndrome[2][frames]   max_ser_num[4]   ser_den   decision[frames][4]   info[frames][22]
//   counted_errors[4][frames]   counted_compared[4][frames]      (what channel_errors makes of out_h and bytes_h: ::is95_channel_errors)
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
    if (argc != 2) { printf("usage: run_is95_hip <case file>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    static const size_t NB[4] = {23, 11, 5, 2};
    std::vector<long long> hd, symbols, scramble, out[4], bytes[4], errors, compared, syndrome, num, den, decision, info, counted_e, counted_c;
    bool ok = read_ints(f, hd, 1) && hd[0] > 0;
    const size_t frames = ok ? (size_t)hd[0] : 0;
    ok = ok && read_ints(f, symbols, frames * 384) && read_ints(f, scramble, frames * 48);
    for (int h = 0; h < 4; ++h) ok = ok && read_ints(f, out[h], frames * (384 >> h));
    for (int h = 0; h < 4; ++h) ok = ok && read_ints(f, bytes[h], frames * NB[h]);
    ok = ok && read_ints(f, errors, 4 * frames) && read_ints(f, compared, 4 * frames) && read_ints(f, syndrome, 2 * frames) && read_ints(f, num, 4) &&
         read_ints(f, den, 1) && read_ints(f, decision, frames * 4) && read_ints(f, info, frames * 22) && read_ints(f, counted_e, 4 * frames) &&
         read_ints(f, counted_c, 4 * frames);
    fclose(f);
    if (!ok) { printf("bad case file\n"); return 2; }

    constexpr size_t K = 9, R = 2;
    const uint16_t G[R] = {491, 369};
    const auto setup = soft16_setup(R);
    auto table = ViterbiBranchTable<K, R, int16_t>(G, setup.high, setup.low);
    ViterbiDecoder_HIP_Batch<K, R, uint16_t, int16_t> batch(table, setup.config);

    // frames 389 elements apart, masks 50 bytes apart
    const size_t in_stride = 389, mask_stride = 50;
    std::vector<int16_t> h_in(frames * in_stride, -77);
    std::vector<uint8_t> h_mask(frames * mask_stride, 0xEE);
    for (size_t r = 0; r < frames; ++r) {
        for (size_t i = 0; i < 384; ++i) h_in[r * in_stride + i] = (int16_t)symbols[r * 384 + i];
        for (size_t i = 0; i < 48; ++i) h_mask[r * mask_stride + i] = (uint8_t)scramble[r * 48 + i];
    }
    int16_t* d_in;
    uint8_t* d_mask;
    HIP_OK(hipMalloc((void**)&d_in, h_in.size() * 2));
    HIP_OK(hipMalloc((void**)&d_mask, h_mask.size()));
    HIP_OK(hipMemcpy(d_in, h_in.data(), h_in.size() * 2, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_mask, h_mask.data(), h_mask.size(), hipMemcpyHostToDevice));
    int16_t* d_out[4];
    for (int h = 0; h < 4; ++h)
        if (!(d_out[h] = filled<int16_t>(frames * (384 >> h), 8))) { printf("no memory\n"); return 1; }
    batch.is95_deinterleave(d_in, frames, d_out, d_mask, mask_stride, 0, -127, 127, in_stride);
    HIP_OK(hipDeviceSynchronize());
    long long bad_out = 0;
    for (int h = 0; h < 4; ++h) bad_out += differ(d_out[h], out[h], frames, 384 >> h, 384 >> h, 8);

    // the decision on the file's decodes and counts; the bytes of hypothesis 1 at a stride of 13, the info rows at 25
    const size_t st[4] = {0, 13, 0, 0}, info_stride = 25;
    uint8_t* d_bytes[4];
    uint32_t *d_err[4], *d_cmp[4], *d_syn[2];
    for (int h = 0; h < 4; ++h) {
        const size_t stride = st[h] ? st[h] : NB[h];
        std::vector<uint8_t> hb(frames * stride, 0xEE);
        for (size_t r = 0; r < frames; ++r)
            for (size_t i = 0; i < NB[h]; ++i) hb[r * stride + i] = (uint8_t)bytes[h][r * NB[h] + i];
        std::vector<uint32_t> he(frames), hc(frames), hs(frames);
        for (size_t r = 0; r < frames; ++r) { he[r] = (uint32_t)errors[h * frames + r]; hc[r] = (uint32_t)compared[h * frames + r]; if (h < 2) hs[r] = (uint32_t)syndrome[h * frames + r]; }
        HIP_OK(hipMalloc((void**)&d_bytes[h], hb.size()));
        HIP_OK(hipMalloc((void**)&d_err[h], frames * 4));
        HIP_OK(hipMalloc((void**)&d_cmp[h], frames * 4));
        HIP_OK(hipMemcpy(d_bytes[h], hb.data(), hb.size(), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_err[h], he.data(), frames * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_cmp[h], hc.data(), frames * 4, hipMemcpyHostToDevice));
        if (h < 2) {
            HIP_OK(hipMalloc((void**)&d_syn[h], frames * 4));
            HIP_OK(hipMemcpy(d_syn[h], hs.data(), frames * 4, hipMemcpyHostToDevice));
        }
    }
    // the error counts of the file's decodes against the symbols the de-interleave just wrote, in one call
    uint32_t *d_ce[4], *d_cc[4];
    for (int h = 0; h < 4; ++h)
        if (!(d_ce[h] = filled<uint32_t>(frames, 2)) || !(d_cc[h] = filled<uint32_t>(frames, 2))) { printf("no memory\n"); return 1; }
    batch.is95_channel_errors(d_out, d_bytes, frames, d_ce, d_cc, st);
    HIP_OK(hipDeviceSynchronize());
    long long bad_counts = 0;
    for (int h = 0; h < 4; ++h) {
        const std::vector<long long> we(counted_e.begin() + h * frames, counted_e.begin() + (h + 1) * frames), wc(counted_c.begin() + h * frames, counted_c.begin() + (h + 1) * frames);
        bad_counts += differ(d_ce[h], we, 1, frames, frames, 2) + differ(d_cc[h], wc, 1, frames, frames, 2);
        (void)hipFree(d_ce[h]); (void)hipFree(d_cc[h]);
    }
    uint32_t* d_decision = filled<uint32_t>(frames * 4, 4);
    uint8_t* d_info = filled<uint8_t>(frames * info_stride, 8);
    if (!d_decision || !d_info) { printf("no memory\n"); return 1; }
    const uint32_t max_num[4] = {(uint32_t)num[0], (uint32_t)num[1], (uint32_t)num[2], (uint32_t)num[3]};
    batch.is95_rate_decide(d_bytes, d_err, d_cmp, d_syn, frames, max_num, (uint32_t)den[0], (vit_hip_is95_decision*)d_decision, d_info, info_stride, st);
    HIP_OK(hipDeviceSynchronize());
    const long long bad_decision = differ(d_decision, decision, frames, 4, 4, 4), bad_info = differ(d_info, info, frames, 22, info_stride, 8);
    printf("mismatches out=%lld, counts=%lld, decision=%lld, info=%lld\n", bad_out, bad_counts, bad_decision, bad_info);
    (void)hipFree(d_in); (void)hipFree(d_mask); (void)hipFree(d_decision); (void)hipFree(d_info);
    for (int h = 0; h < 4; ++h) { (void)hipFree(d_out[h]); (void)hipFree(d_bytes[h]); (void)hipFree(d_err[h]); (void)hipFree(d_cmp[h]); }
    (void)hipFree(d_syn[0]); (void)hipFree(d_syn[1]);
    const int rc = bad_out == 0 && bad_counts == 0 && bad_decision == 0 && bad_info == 0 ? 0 : 1;
    printf(rc == 0 ? "PASS\n" : "FAIL\n");
    return rc;
}
