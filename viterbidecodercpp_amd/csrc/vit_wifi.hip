// vit_wifi.hip -- the IEEE 802.11a/g OFDM data path of the C ABI: vit_hip_wifi_deinterleave_batch (the per-symbol de-interleaver fused
// with depuncturing, rate and length per frame, writing the [F][S][2] symbols vit_hip_decode_batch reads), vit_hip_wifi_signal_batch (the
// SIGNAL field's decoded bits to rate, LENGTH and the counts of the DATA field) and vit_hip_wifi_data_batch (scrambler seed recovery,
// descrambling, PSDU octets and the FCS at every frame's own LENGTH).  They work on the caller's buffers alone and read the handle for its
// device, its symbol width and its rate.  The kernels of kernels_wifi.hpp are launched only here.  Host-side logic only: the argument
// rules (kernels_wifi.hpp, so that they run without a device), a handful of constants and the launch.
// Out of scope: synchronisation, channel estimation and demapping; 802.11n/ac (other interleavers, LDPC, several encoders) and 802.11b;
// bucketing frames by length; a transmitter on the card; A-MPDU delimiters.
#include "vit_internal.hpp"
#include "kernels_wifi.hpp"

using namespace vit;

extern "C" {

int vit_hip_wifi_deinterleave_batch(vit_hip_handle h, const void* d_in, size_t in_frame_stride, size_t frames, size_t max_sym, unsigned rate,
                                    const uint32_t* d_rate, const uint32_t* d_n_sym, const uint32_t* d_n_steps, size_t count_stride, size_t S,
                                    void* d_symbols_out, vit_hip_stream_t stream) {
    if (const char* why = wifi_deinterleave_invalid(h != nullptr, h ? h->R : 0, h ? (size_t)h->soft_bytes : 1, d_in, in_frame_stride, frames, max_sym,
                                                    rate, d_rate, d_n_sym, d_n_steps, count_stride, S, d_symbols_out))
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
    if (const char* why = wifi_signal_invalid(h != nullptr, d_bytes, frame_stride_bytes, frames, d_signal)) return fail(VIT_HIP_ERR_INVALID_ARG, why);
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
    if (const char* why = wifi_data_invalid(h != nullptr, d_bytes, frame_stride_bytes, frames, S, d_length, length_stride, max_length, d_psdu,
                                            psdu_stride, d_status))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (frames == 0) return VIT_HIP_OK;
    const WifiDataArgs a = wifi_data_args(d_bytes, frame_stride_bytes, frames, S - 6, d_length, length_stride, max_length, d_psdu, psdu_stride,
                                          d_status);
    VIT_HIP_ON_DEVICE(h->device);
    if (wifi_launch_data(a, (hipStream_t)stream) != 0) return fail(VIT_HIP_ERR_RUNTIME, "wifi DATA launch failed");
    return VIT_HIP_OK;
}

}  // extern "C"
