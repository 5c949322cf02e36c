// vit_gsm.hip -- the GSM channel decoding route of the C ABI (3GPP TS 45.003), around vit_hip_decode_batch on a K = 5, R = 1/2 handle:
// vit_hip_gsm_deinterleave_batch (the block and the diagonal burst de-interleaver, writing the [228][2] and [189][2] buffers the decode reads,
// the class II soft bits and the stealing-flag sums), vit_hip_gsm_fire_batch (the 40-bit Fire code of the control channels: check and
// correction of one error burst) and vit_hip_gsm_tchfs_batch (class I reorder, parity and class II hard decisions of a TCH/FS frame).  They
// work on the caller's buffers alone and read the handle for its device, its symbol width, its rate and its decision levels.  The
// kernels of kernels_gsm.hpp are launched only here.  Host-side logic only: the argument rules (kernels_gsm.hpp, so that they run without a
// device) and the launch.
// Out of scope: GPRS CS-2..4 and EGPRS (puncturing tables, USF precoding); TCH/HS, EFR's preliminary CRC-8, AMR; SACCH/TCH multiframe
// scheduling and deciphering (the caller negates with the A5 keystream); burst demodulation; per-row burst counts in one call; a
// transmitter on the card.
#include "vit_internal.hpp"
#include "kernels_gsm.hpp"

using namespace vit;

extern "C" {

int vit_hip_gsm_deinterleave_batch(vit_hip_handle h, const void* d_in, size_t in_row_stride, size_t in_burst_stride, size_t rows, size_t bursts,
                                   unsigned mode, unsigned flags, const void* d_hist_in, const uint32_t* d_fill_in, void* d_hist_out,
                                   uint32_t* d_fill_out, uint32_t* d_n_out, void* d_full, void* d_class1, void* d_class2, int32_t* d_steal,
                                   vit_hip_stream_t stream) {
    const size_t sb = h ? (size_t)h->soft_bytes : 1;
    if (const char* why = gsm_deinterleave_invalid(h != nullptr, h ? h->R : 0, sb, d_in, in_row_stride, in_burst_stride, rows, bursts, mode, flags,
                                                   d_hist_in, d_fill_in, d_hist_out, d_fill_out, d_n_out, d_full, d_class1, d_class2, d_steal))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (rows == 0 || bursts == 0) return VIT_HIP_OK;
    const GsmArgs a = gsm_args(sb, d_in, in_row_stride, in_burst_stride, rows, bursts, mode, flags, d_hist_in, d_fill_in, d_hist_out, d_fill_out,
                               d_n_out, d_full, d_class1, d_class2, d_steal);
    VIT_HIP_ON_DEVICE(h->device);
    if (gsm_launch_deinterleave(a, sb, (hipStream_t)stream) != 0) return fail(VIT_HIP_ERR_RUNTIME, "GSM de-interleave launch failed");
    return VIT_HIP_OK;
}

int vit_hip_gsm_fire_batch(vit_hip_handle h, const uint8_t* d_bytes, size_t bytes_frame_stride, size_t frames, unsigned max_burst, unsigned flags,
                           vit_hip_gsm_fire* d_status, uint8_t* d_data, size_t data_stride, vit_hip_stream_t stream) {
    if (const char* why = gsm_fire_invalid(h != nullptr, d_bytes, bytes_frame_stride, frames, max_burst, flags, d_status, d_data, data_stride))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (frames == 0) return VIT_HIP_OK;
    const GsmFireArgs a = gsm_fire_args(d_bytes, bytes_frame_stride, frames, max_burst, flags, d_status, d_data, data_stride);
    VIT_HIP_ON_DEVICE(h->device);
    if (gsm_launch_fire(a, (hipStream_t)stream) != 0) return fail(VIT_HIP_ERR_RUNTIME, "GSM Fire code launch failed");
    return VIT_HIP_OK;
}

int vit_hip_gsm_tchfs_batch(vit_hip_handle h, const uint8_t* d_bytes, size_t bytes_frame_stride, const void* d_class2, size_t frames,
                            uint8_t* d_speech, size_t speech_stride, vit_hip_gsm_tchfs* d_status, vit_hip_stream_t stream) {
    const size_t sb = h ? (size_t)h->soft_bytes : 1;
    if (const char* why = gsm_tchfs_invalid(h != nullptr, sb, d_bytes, bytes_frame_stride, d_class2, frames, d_speech, speech_stride, d_status))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (frames == 0) return VIT_HIP_OK;
    const GsmTchfsArgs a = gsm_tchfs_args(h->high, h->low, d_bytes, bytes_frame_stride, d_class2, frames, d_speech, speech_stride, d_status);
    VIT_HIP_ON_DEVICE(h->device);
    if (gsm_launch_tchfs(a, sb, (hipStream_t)stream) != 0) return fail(VIT_HIP_ERR_RUNTIME, "GSM TCH/FS launch failed");
    return VIT_HIP_OK;
}

}  // extern "C"
