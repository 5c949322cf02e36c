// run_frames_extract_hip.cpp -- frame extraction from C++: ViterbiDecoder_HIP_Batch::frames_extract
// (include/viterbi_hip/viterbi_decoder_hip_batch.h) on rows of bytes, carries and locks read from a case file, checked against the images
// of the output buffers the file carries -- tests/test_gpu_cpp_frames_extract.py writes it from the rule of tests/frames_reference.py.
// The call is made once in one piece over buffers filled with 0xA5 (every byte must equal the image, written or not) and once as two
// calls over the halves of the rows, the second with the carry the first wrote: their frames in order, and the last carry, must be those
// of the one call.
// Case file, whitespace-separated integers:
//   rows n_bits stride period phase0 marker_hi32 marker_lo32 marker_bits drop_bits has_pad max_frames carry_stride
//   lock[rows * 4]   carry_bits[rows]   carry[rows * carry_stride]   bytes[rows * stride]   pad[ceil(Q/8)] if has_pad
//   n_frames[rows]   carry_bits_out[rows]   frames[rows * max_frames * ceil(Q/8)]   marker_errors[rows * max_frames]
//   carry_out[rows * carry_stride]
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
static std::vector<T> narrowed(const std::vector<long long>& v) {
    std::vector<T> out(v.size());
    for (size_t i = 0; i < v.size(); i++) out[i] = T(v[i]);
    return out;
}

int main(int argc, char** argv) {
    if (argc != 2) { printf("usage: run_frames_extract_hip <case file>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    std::vector<long long> hd, lock_raw, cbits_raw, carry_raw, bytes_raw, pad_raw, want_n, want_cb, want_frames, want_err, want_carry;
    if (!read_ints(f, hd, 12)) { printf("bad case file\n"); return 2; }
    const size_t rows = hd[0], n_bits = hd[1], stride = hd[2], P = hd[3], phase0 = hd[4], drop = hd[8], max_frames = hd[10], cstride = hd[11];
    const uint64_t marker = (uint64_t(hd[5]) << 32) | uint64_t(hd[6]);
    const unsigned m = unsigned(hd[7]);
    const bool has_pad = hd[9] != 0;
    const size_t qb = (P - drop + 7) / 8;
    if (!read_ints(f, lock_raw, rows * 4) || !read_ints(f, cbits_raw, rows) || !read_ints(f, carry_raw, rows * cstride) ||
        !read_ints(f, bytes_raw, rows * stride) || !read_ints(f, pad_raw, has_pad ? qb : 0) || !read_ints(f, want_n, rows) ||
        !read_ints(f, want_cb, rows) || !read_ints(f, want_frames, rows * max_frames * qb) || !read_ints(f, want_err, rows * max_frames) ||
        !read_ints(f, want_carry, rows * cstride)) { printf("bad case file\n"); return 2; }
    fclose(f);

    constexpr size_t K = 7, R = 2;
    const uint8_t G[R] = {109, 79};
    const auto setup = soft16_setup(R);
    auto table = ViterbiBranchTable<K, R, int16_t>(G, setup.high, setup.low);
    ViterbiDecoder_HIP_Batch<K, R, uint16_t, int16_t> batch(table, setup.config);

    const std::vector<uint8_t> bytes = narrowed<uint8_t>(bytes_raw), carry = narrowed<uint8_t>(carry_raw), pad = narrowed<uint8_t>(pad_raw);
    const std::vector<uint32_t> cbits = narrowed<uint32_t>(cbits_raw), lock = narrowed<uint32_t>(lock_raw);
    const size_t frames_bytes = rows * max_frames * qb, carry_bytes = rows * cstride;

    uint8_t *d_bytes, *d_carry[3], *d_pad = nullptr, *d_frames;
    uint32_t *d_cbits[3], *d_n, *d_err;
    vit_hip_marker_lock* d_lock;
    HIP_OK(hipMalloc((void**)&d_bytes, bytes.size()));
    for (int i = 0; i < 3; i++) {
        HIP_OK(hipMalloc((void**)&d_carry[i], carry_bytes));
        HIP_OK(hipMalloc((void**)&d_cbits[i], rows * sizeof(uint32_t)));
    }
    if (has_pad) HIP_OK(hipMalloc((void**)&d_pad, qb));
    HIP_OK(hipMalloc((void**)&d_frames, frames_bytes));
    HIP_OK(hipMalloc((void**)&d_n, rows * sizeof(uint32_t)));
    HIP_OK(hipMalloc((void**)&d_err, rows * max_frames * sizeof(uint32_t)));
    HIP_OK(hipMalloc((void**)&d_lock, rows * sizeof(vit_hip_marker_lock)));
    HIP_OK(hipMemcpy(d_bytes, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_carry[0], carry.data(), carry_bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_cbits[0], cbits.data(), rows * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_lock, lock.data(), rows * sizeof(vit_hip_marker_lock), hipMemcpyHostToDevice));
    if (has_pad) HIP_OK(hipMemcpy(d_pad, pad.data(), qb, hipMemcpyHostToDevice));

    std::vector<uint8_t> frames(frames_bytes), carry_out(carry_bytes);
    std::vector<uint32_t> n(rows), cb_out(rows), err(rows * max_frames);
    auto poison = [&](int c) -> bool {
        return hipMemset(d_frames, 0xA5, frames_bytes) == hipSuccess && hipMemset(d_carry[c], 0xA5, carry_bytes) == hipSuccess &&
               hipMemset(d_err, 0xA5, rows * max_frames * sizeof(uint32_t)) == hipSuccess &&
               hipMemset(d_n, 0xA5, rows * sizeof(uint32_t)) == hipSuccess && hipMemset(d_cbits[c], 0xA5, rows * sizeof(uint32_t)) == hipSuccess;
    };
    auto fetch = [&](int c) -> bool {
        return hipDeviceSynchronize() == hipSuccess && hipMemcpy(frames.data(), d_frames, frames_bytes, hipMemcpyDeviceToHost) == hipSuccess &&
               hipMemcpy(carry_out.data(), d_carry[c], carry_bytes, hipMemcpyDeviceToHost) == hipSuccess &&
               hipMemcpy(n.data(), d_n, rows * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess &&
               hipMemcpy(cb_out.data(), d_cbits[c], rows * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess &&
               hipMemcpy(err.data(), d_err, err.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess;
    };

    // one call: every byte of every output equals its image
    if (!poison(1)) { printf("hipMemset failed\n"); return 1; }
    batch.frames_extract(d_bytes, rows, n_bits, P, phase0, d_lock, d_carry[0], d_cbits[0], d_frames, max_frames, d_n, d_carry[1], d_cbits[1], d_err,
                         marker, m, drop, d_pad, stride, cstride, 0);
    if (!fetch(1)) { printf("read-back failed\n"); return 1; }
    long long bad_one = 0;
    for (size_t i = 0; i < frames_bytes; i++) bad_one += frames[i] != uint8_t(want_frames[i]);
    for (size_t i = 0; i < carry_bytes; i++) bad_one += carry_out[i] != uint8_t(want_carry[i]);
    for (size_t i = 0; i < rows * max_frames; i++) bad_one += err[i] != uint32_t(want_err[i]);
    for (size_t r = 0; r < rows; r++) {
        bad_one += n[r] != uint32_t(want_n[r]) || cb_out[r] != uint32_t(want_cb[r]);
        printf("one call, row %zu: %u frames, %u bits carried\n", r, n[r], cb_out[r]);
    }

    // two calls over the halves (whole bytes), the carry ping-ponged: the same frames in order, the same last carry
    long long bad_two = 0;
    const size_t n1 = n_bits / 16 * 8;
    if (n1 > 0 && n1 < n_bits) {
        std::vector<std::vector<uint8_t>> got(rows);
        std::vector<std::vector<uint32_t>> got_err(rows);
        const size_t part[2] = {n1, n_bits - n1};
        for (int call = 0; call < 2; call++) {
            if (!poison(call + 1)) { printf("hipMemset failed\n"); return 1; }
            batch.frames_extract(d_bytes + (call ? n1 / 8 : 0), rows, part[call], P, (phase0 + (call ? n1 : 0)) % P, d_lock, d_carry[call],
                                 d_cbits[call], d_frames, max_frames, d_n, d_carry[call + 1], d_cbits[call + 1], d_err, marker, m, drop, d_pad,
                                 stride, cstride, 0);
            if (!fetch(call + 1)) { printf("read-back failed\n"); return 1; }
            for (size_t r = 0; r < rows; r++) {
                if (n[r] > max_frames) { bad_two++; continue; }
                got[r].insert(got[r].end(), frames.begin() + r * max_frames * qb, frames.begin() + (r * max_frames + n[r]) * qb);
                got_err[r].insert(got_err[r].end(), err.begin() + r * max_frames, err.begin() + r * max_frames + n[r]);
            }
        }
        for (size_t r = 0; r < rows; r++) {
            const size_t nf = size_t(want_n[r]);
            bad_two += got[r].size() != nf * qb || cb_out[r] != uint32_t(want_cb[r]);
            for (size_t i = 0; i < got[r].size() && i < nf * qb; i++) bad_two += got[r][i] != uint8_t(want_frames[r * max_frames * qb + i]);
            for (size_t i = 0; i < got_err[r].size() && i < nf; i++) bad_two += got_err[r][i] != uint32_t(want_err[r * max_frames + i]);
            for (size_t i = 0; i < (size_t(want_cb[r]) + 7) / 8; i++) bad_two += carry_out[r * cstride + i] != uint8_t(want_carry[r * cstride + i]);
            printf("two calls, row %zu: %zu frames, %u bits carried\n", r, got[r].size() / qb, cb_out[r]);
        }
    } else {
        printf("two calls: the case is too short to cut\n");
    }
    printf("mismatches of one call=%lld, of two calls=%lld\n", bad_one, bad_two);
    (void)hipFree(d_bytes); (void)hipFree(d_pad); (void)hipFree(d_frames); (void)hipFree(d_n); (void)hipFree(d_err); (void)hipFree(d_lock);
    for (int i = 0; i < 3; i++) { (void)hipFree(d_carry[i]); (void)hipFree(d_cbits[i]); }
    const int rc = bad_one == 0 && bad_two == 0 ? 0 : 1;
    printf(rc == 0 ? "PASS\n" : "FAIL\n");
    return rc;
}
