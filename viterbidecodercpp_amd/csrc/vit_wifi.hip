// vit_wifi.hip -- the IEEE 802.11a/g OFDM data path of the C ABI: vit_hip_wifi_deinterleave_batch (the per-symbol de-interleaver fused
// with depuncturing, rate and length per frame, writing the [F][S][2] symbols vit_hip_decode_batch reads), vit_hip_wifi_signal_batch (the
// SIGNAL field's decoded bits to rate, LENGTH and the counts of the DATA field) and vit_hip_wifi_data_batch (scrambler seed recovery,
// descrambling, PSDU octets and the FCS at every frame's own LENGTH).  They work on the caller's buffers alone and read the handle for its
// device, its symbol width and its rate.  The kernels of kernels_wifi.hpp are launched only here.  Host-side logic only: argument
// checking, a handful of constants and the launch.
// Out of scope: synchronisation, channel estimation and demapping; 802.11n/ac (other interleavers, LDPC, several encoders) and 802.11b;
// bucketing frames by length; a transmitter on the card; A-MPDU delimiters.
#include "vit_internal.hpp"
#include "kernels_wifi.hpp"

using namespace vit;

namespace {

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}

// bytes a per-frame uint32 array of `frames` entries at `stride` elements spans
size_t span4(size_t frames, size_t stride) { return ((frames - 1) * (stride ? stride : 1) + 1) * sizeof(uint32_t); }

// argument rules (include/vit_hip.h): everything the host can know without reading device memory
const char* deint_invalid(vit_hip_handle h, const void* d_in, size_t stride, size_t frames, size_t max_sym, unsigned rate, const uint32_t* d_rate,
                          const uint32_t* d_n_sym, const uint32_t* d_n_steps, size_t count_stride, size_t S, const void* d_out) {
    if (!h || !d_in || !d_out) return "NULL handle, d_in or d_symbols_out";
    if (h->R != 2) return "the handle's code rate must be 1/2";
    if (!d_rate && rate > 7) return "rate must be 0 .. 7";
    const size_t sb = (size_t)h->soft_bytes;
    if ((uintptr_t)d_in % sb || (uintptr_t)d_out % 4) return "d_in must be aligned to the symbol type, d_symbols_out to 4 bytes";
    if ((uintptr_t)d_rate % 4 || (uintptr_t)d_n_sym % 4 || (uintptr_t)d_n_steps % 4) return "d_rate, d_n_sym and d_n_steps must be aligned to 4 bytes";
    if (frames == 0) return nullptr;
    if (max_sym == 0 || S == 0) return "max_sym and S must be at least 1";
    if (max_sym > 0xFFFFFFFFull / WIFI_MAX_CBPS) return "max_sym * 288 must lie below 2^32";
    if (S >= 0x7FFFFFFFull) return "S must lie below 2^31 - 1";
    const size_t least = max_sym * (d_rate ? WIFI_MAX_CBPS : wifi_rate(rate).ncbps);
    if (stride != 0 && stride < least) return "in_frame_stride below max_sym * N_CBPS (288 with d_rate)";
    if (frames > (0xFFFFFFFFull * (4 / sb)) / (2 * S)) return "frames * 2 S symbols must fill fewer than 2^32 dwords";
    if (count_stride > 0xFFFFFFFFull || frames > 0xFFFFFFFFull) return "frames and count_stride must lie below 2^32";
    const size_t in_stride = stride ? stride : max_sym * WIFI_MAX_CBPS;
    const size_t out_b = frames * 2 * S * sb, in_b = ((frames - 1) * in_stride + (stride ? least : in_stride)) * sb, cnt_b = span4(frames, count_stride);
    if (overlap(d_out, out_b, d_in, in_b)) return "d_symbols_out overlaps d_in";
    if (overlap(d_out, out_b, d_rate, cnt_b) || overlap(d_out, out_b, d_n_sym, cnt_b) || overlap(d_out, out_b, d_n_steps, cnt_b))
        return "d_symbols_out overlaps d_rate, d_n_sym or d_n_steps";
    return nullptr;
}

const char* signal_invalid(vit_hip_handle h, const uint8_t* d_bytes, size_t stride, size_t frames, const vit_hip_wifi_signal* d_signal) {
    if (!h || !d_bytes || !d_signal) return "NULL handle, d_bytes or d_signal";
    if (stride != 0 && stride < 3) return "frame_stride_bytes below 3";
    if ((uintptr_t)d_signal % 4) return "d_signal must be aligned to 4 bytes";
    if (frames == 0) return nullptr;
    if (frames > (uint64_t)0x7FFFFFFFu * WIFI_BLOCK) return "more than 2^31 - 1 blocks";
    if (overlap(d_signal, frames * sizeof(vit_hip_wifi_signal), d_bytes, (frames - 1) * (stride ? stride : 3) + 3)) return "d_signal overlaps d_bytes";
    return nullptr;
}

const char* data_invalid(vit_hip_handle h, const uint8_t* d_bytes, size_t stride, size_t frames, size_t S, const uint32_t* d_length,
                         size_t length_stride, size_t max_length, const uint8_t* d_psdu, size_t psdu_stride, const vit_hip_wifi_status* d_status) {
    if (!h || !d_bytes || !d_length || !d_psdu || !d_status) return "NULL handle, d_bytes, d_length, d_psdu or d_status";
    if (S < 22 || S >= 0x7FFFFFFFull) return "S must be 22 .. 2^31 - 2: the SERVICE field and the tail";
    if (max_length > 0x0FFFFFFFull) return "max_length must lie below 2^28";
    const size_t n_bits = S - 6, nb = (n_bits + 7) / 8;
    if (stride != 0 && stride < nb) return "frame_stride_bytes below ceil((S - 6) / 8)";
    const size_t room = (n_bits - 16) / 8, longest = max_length < room ? max_length : room;
    if (psdu_stride != 0 && psdu_stride < longest) return "psdu_stride below the longest PSDU the call can write";
    if ((uintptr_t)d_length % 4 || (uintptr_t)d_status % 4) return "d_length and d_status must be aligned to 4 bytes";
    if (frames == 0) return nullptr;
    if (length_stride > 0xFFFFFFFFull) return "length_stride must lie below 2^32";
    const uint32_t logG = crc_geometry(longest > 4 ? 8ull * (longest - 4) : 0ull).logG;
    if (frames > ((uint64_t)0x7FFFFFFFu * WIFI_BLOCK) >> logG) return "more than 2^31 - 1 blocks";
    const size_t in_b = (frames - 1) * (stride ? stride : nb) + nb, len_b = span4(frames, length_stride);
    const size_t ps = psdu_stride ? psdu_stride : max_length, psdu_b = longest ? (frames - 1) * ps + longest : 0;
    const size_t st_b = frames * sizeof(vit_hip_wifi_status);
    if (overlap(d_psdu, psdu_b, d_bytes, in_b) || overlap(d_status, st_b, d_bytes, in_b)) return "an output overlaps d_bytes";
    if (overlap(d_psdu, psdu_b, d_length, len_b) || overlap(d_status, st_b, d_length, len_b)) return "an output overlaps d_length";
    if (overlap(d_psdu, psdu_b, d_status, st_b)) return "d_psdu overlaps d_status";
    return nullptr;
}

}  // namespace

extern "C" {

int vit_hip_wifi_deinterleave_batch(vit_hip_handle h, const void* d_in, size_t in_frame_stride, size_t frames, size_t max_sym, unsigned rate,
                                    const uint32_t* d_rate, const uint32_t* d_n_sym, const uint32_t* d_n_steps, size_t count_stride, size_t S,
                                    void* d_symbols_out, vit_hip_stream_t stream) {
    if (const char* why = deint_invalid(h, d_in, in_frame_stride, frames, max_sym, rate, d_rate, d_n_sym, d_n_steps, count_stride, S, d_symbols_out))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (frames == 0) return VIT_HIP_OK;
    const WifiDeintArgs a = wifi_deint_args(d_in, in_frame_stride, frames, max_sym, rate, d_rate, d_n_sym, d_n_steps, count_stride, S,
                                            d_symbols_out, (size_t)h->soft_bytes);
    VIT_HIP_ON_DEVICE(h->device);
    if (wifi_launch_deinterleave(a, (size_t)h->soft_bytes, (hipStream_t)stream) != 0)
        return fail(VIT_HIP_ERR_RUNTIME, "wifi de-interleave launch failed");
    return VIT_HIP_OK;
}

int vit_hip_wifi_signal_batch(vit_hip_handle h, const uint8_t* d_bytes, size_t frame_stride_bytes, size_t frames, vit_hip_wifi_signal* d_signal,
                              vit_hip_stream_t stream) {
    if (const char* why = signal_invalid(h, d_bytes, frame_stride_bytes, frames, d_signal)) return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (frames == 0) return VIT_HIP_OK;
    WifiSignalArgs a{};
    a.in = d_bytes; a.out = d_signal; a.stride = frame_stride_bytes ? frame_stride_bytes : 3; a.frames = frames;
    VIT_HIP_ON_DEVICE(h->device);
    if (wifi_launch_signal(a, (hipStream_t)stream) != 0) return fail(VIT_HIP_ERR_RUNTIME, "wifi SIGNAL launch failed");
    return VIT_HIP_OK;
}

int vit_hip_wifi_data_batch(vit_hip_handle h, const uint8_t* d_bytes, size_t frame_stride_bytes, size_t frames, size_t S,
                            const uint32_t* d_length, size_t length_stride, size_t max_length, uint8_t* d_psdu, size_t psdu_stride,
                            vit_hip_wifi_status* d_status, vit_hip_stream_t stream) {
    if (const char* why = data_invalid(h, d_bytes, frame_stride_bytes, frames, S, d_length, length_stride, max_length, d_psdu, psdu_stride, d_status))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (frames == 0) return VIT_HIP_OK;
    const WifiDataArgs a = wifi_data_args(d_bytes, frame_stride_bytes, frames, S - 6, d_length, length_stride, max_length, d_psdu, psdu_stride,
                                          d_status);
    VIT_HIP_ON_DEVICE(h->device);
    if (wifi_launch_data(a, (hipStream_t)stream) != 0) return fail(VIT_HIP_ERR_RUNTIME, "wifi DATA launch failed");
    return VIT_HIP_OK;
}

}  // extern "C"
