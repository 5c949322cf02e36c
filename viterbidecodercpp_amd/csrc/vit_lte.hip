// vit_lte.hip -- the front of the LTE control-channel route of the C ABI: vit_hip_lte_rate_dematch_batch (the descrambling and the
// inverse of the rate matching of 3GPP TS 36.212 5.1.4.2, writing the [F][D][3] symbols vit_hip_decode_tail_biting_batch reads).
// It works on the caller's elements alone and reads the handle for its device, its symbol width and its rate.  The kernel of
// kernels_lte.hpp is launched only here.  Host-side logic only: the argument rule (kernels_lte.hpp, so that it runs without a device),
// the handful of constants of D and the launch.
// Out of scope: turbo-code rate matching; PDCCH REG de-interleaving and the cyclic shift; per-frame D in one call; the transmit side.
#include "vit_internal.hpp"
#include "kernels_lte.hpp"

using namespace vit;

extern "C" {

int vit_hip_lte_rate_dematch_batch(vit_hip_handle h, const void* d_received, size_t n_received, size_t received_frame_stride,
                                   const uint32_t* d_offset, const uint32_t* d_count, size_t frames, size_t D, size_t E_max,
                                   const uint8_t* d_scramble, size_t scramble_period, unsigned shift, int clamp_lo, int clamp_hi,
                                   void* d_symbols_out, vit_hip_stream_t stream) {
    if (const char* why = lte_invalid(h != nullptr, h ? h->R : 0, h ? (size_t)h->soft_bytes : 1, d_received, n_received, received_frame_stride,
                                      d_offset, d_count, frames, D, E_max, shift, clamp_lo, clamp_hi, d_symbols_out))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (frames == 0) return VIT_HIP_OK;
    const LteArgs a = lte_dematch_args(d_received, n_received, received_frame_stride, d_offset, d_count, frames, D, E_max, d_scramble,
                                       scramble_period, shift, clamp_lo, clamp_hi, d_symbols_out, (size_t)h->soft_bytes);
    VIT_HIP_ON_DEVICE(h->device);
    if (lte_launch_dematch(a, (size_t)h->soft_bytes, (hipStream_t)stream) != 0) return fail(VIT_HIP_ERR_RUNTIME, "lte de-match launch failed");
    return VIT_HIP_OK;
}

}  // extern "C"
