// vit_is95.hip -- the IS-95A forward traffic channel route of the C ABI, rate set 1, around vit_hip_decode_batch on a K = 9, R = 1/2 handle:
// vit_hip_is95_deinterleave_batch (long-code descrambling, the 384-symbol block de-interleaver and the combining of the repetitions under the
// four rate hypotheses, writing the four [frames][S_h][2] buffers the decode reads), vit_hip_is95_channel_errors_batch (the re-encoded symbol
// error counts of the four decodes behind one zeroing kernel, around the body of vit_hip_channel_errors_batch) and
// vit_hip_is95_rate_decide_batch (the blind rate decision from the frame quality indicator and the re-encoded symbol error rate of the four decodes, and the winner's info bits).  They
// work on the caller's buffers alone and read the handle for its device, its symbol width and its rate.  The kernels of kernels_is95.hpp
// are launched only here.  Host-side logic only: the argument rules (kernels_is95.hpp, so that they run without a device) and the launch.
// Out of scope: rate set 2 (14400 and its puncturing), the long-code generator (the caller supplies the decimated bits), power-control
// bit extraction, sync and paging channels (continuous encoding: vit_hip_decode_stream), the reverse link, cdma2000 radio configurations 3
// and up, any rate-decision policy beyond the stated rule.
#include "vit_internal.hpp"
#include "kernels_is95.hpp"

using namespace vit;

extern "C" {

int vit_hip_is95_deinterleave_batch(vit_hip_handle h, const void* d_in, size_t in_frame_stride, size_t frames, const uint8_t* d_scramble,
                                    size_t scramble_frame_stride, unsigned shift, int clamp_lo, int clamp_hi, void* const d_out[4],
                                    vit_hip_stream_t stream) {
    if (const char* why = is95_deinterleave_invalid(h != nullptr, h ? h->R : 0, h ? (size_t)h->soft_bytes : 1, d_in, in_frame_stride, frames,
                                                    d_scramble, scramble_frame_stride, shift, clamp_lo, clamp_hi, d_out))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (frames == 0) return VIT_HIP_OK;
    const Is95Args a = is95_args(d_in, in_frame_stride, frames, d_scramble, scramble_frame_stride, shift, clamp_lo, clamp_hi, d_out);
    VIT_HIP_ON_DEVICE(h->device);
    if (is95_launch_deinterleave(a, (size_t)h->soft_bytes, (hipStream_t)stream) != 0)
        return fail(VIT_HIP_ERR_RUNTIME, "IS-95 de-interleave launch failed");
    return VIT_HIP_OK;
}

int vit_hip_is95_channel_errors_batch(vit_hip_handle h, const void* const d_symbols[4], const uint8_t* const d_bytes[4],
                                      const size_t bytes_frame_stride[4], size_t frames, uint32_t* const d_errors[4],
                                      uint32_t* const d_compared[4], vit_hip_stream_t stream) {
    if (const char* why = is95_errors_invalid(h != nullptr, h ? h->K : 0, h ? h->R : 0, h ? (size_t)h->soft_bytes : 1, d_symbols, d_bytes,
                                              bytes_frame_stride, frames, d_errors, d_compared))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (!h->linear) return fail(VIT_HIP_ERR_UNSUPPORTED, "the branch table is not that of a linear code: nothing to encode with");
    if (frames == 0) return VIT_HIP_OK;
    Is95ZeroArgs z{};
    for (int k = 0; k < 4; ++k) {
        z.counters[2 * k] = d_bytes[k] ? d_errors[k] : nullptr;
        z.counters[2 * k + 1] = d_bytes[k] ? d_compared[k] : nullptr;
    }
    z.frames = (uint32_t)frames;
    {
        VIT_HIP_ON_DEVICE(h->device);
        if (is95_launch_zero(z, (hipStream_t)stream) != 0) return fail(VIT_HIP_ERR_RUNTIME, "IS-95 counter zeroing launch failed");
    }
    // the rule above has refused everything the body refuses at these fixed L, K = 9 and R = 2 (NULL buffers, strides, alignment, a
    // table that is not linear, counts), so behind the zeroing only a runtime error can end the loop early
    for (uint32_t k = 0; k < 4; ++k) {
        if (!d_bytes[k]) continue;
        const int rc = channel_errors_impl(h, d_symbols[k], 0, d_bytes[k], bytes_frame_stride ? bytes_frame_stride[k] : 0, frames, is95_steps(k) - 8,
                                           VIT_HIP_ENCODE_TAIL, nullptr, d_errors[k], d_compared[k], false, stream);
        if (rc != VIT_HIP_OK) return rc;
    }
    return VIT_HIP_OK;
}

int vit_hip_is95_rate_decide_batch(vit_hip_handle h, const uint8_t* const d_bytes[4], const size_t bytes_frame_stride[4],
                                   const uint32_t* const d_errors[4], const uint32_t* const d_compared[4], const uint32_t* const d_syndrome[2],
                                   size_t frames, const uint32_t max_ser_num[4], uint32_t ser_den, vit_hip_is95_decision* d_decision,
                                   uint8_t* d_info, size_t info_stride, vit_hip_stream_t stream) {
    if (const char* why = is95_decide_invalid(h != nullptr, d_bytes, bytes_frame_stride, d_errors, d_compared, d_syndrome, frames, max_ser_num,
                                              ser_den, d_decision, d_info, info_stride))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (frames == 0) return VIT_HIP_OK;
    const Is95DecideArgs a = is95_decide_args(d_bytes, bytes_frame_stride, d_errors, d_compared, d_syndrome, frames, max_ser_num, ser_den,
                                              d_decision, d_info, info_stride);
    VIT_HIP_ON_DEVICE(h->device);
    if (is95_launch_decide(a, (hipStream_t)stream) != 0) return fail(VIT_HIP_ERR_RUNTIME, "IS-95 rate decision launch failed");
    return VIT_HIP_OK;
}

}  // extern "C"
