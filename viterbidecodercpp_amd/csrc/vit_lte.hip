// vit_lte.hip -- the front of the LTE control-channel route of the C ABI: vit_hip_lte_rate_dematch_batch (the descrambling and the
// inverse of the rate matching of 3GPP TS 36.212 5.1.4.2, writing the [F][D][3] symbols vit_hip_decode_tail_biting_batch reads).
// It works on the caller's elements alone and reads the handle for its device, its symbol width and its rate.  The kernel of
// kernels_lte.hpp is launched only here.  Host-side logic only: argument checking, the handful of constants of D and the launch.
// Out of scope: turbo-code rate matching; PDCCH REG de-interleaving and the cyclic shift; per-frame D in one call; the transmit side.
#include "vit_internal.hpp"
#include "kernels_lte.hpp"

using namespace vit;

namespace {

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}

// argument rule (include/vit_hip.h): everything the host can know without reading device memory
const char* lte_invalid(vit_hip_handle h, const void* d_received, size_t n_received, size_t stride, const uint32_t* d_offset,
                        const uint32_t* d_count, size_t frames, size_t D, size_t E_max, const uint8_t* d_scramble, unsigned shift, int lo, int hi,
                        const void* d_out) {
    if (!h || !d_received || !d_out) return "NULL handle, d_received or d_symbols_out";
    if (h->R != 3) return "the handle's code rate must be 1/3";
    if (D == 0 || D > LTE_MAX_D) return "D must be 1 .. 8192";
    if (E_max == 0 || E_max >= (1u << 24)) return "E_max must be 1 .. 2^24 - 1";
    if (n_received >= 0x100000000ull) return "n_received must lie below 2^32";
    if (shift > 15) return "shift must be 0 .. 15";
    const int top = h->soft_bytes == 2 ? 32767 : 127;
    if (lo > hi || lo < -top - 1 || hi > top) return "clamp_lo .. clamp_hi must be a range of the symbol type";
    const size_t sb = (size_t)h->soft_bytes;
    if ((uintptr_t)d_received % sb || (uintptr_t)d_out % sb) return "d_received and d_symbols_out must be aligned to the symbol type";
    if (frames == 0) return nullptr;
    if (!d_offset && (stride < E_max || n_received < E_max || (frames - 1) > (n_received - E_max) / stride))
        return "received_frame_stride below E_max, or (frames - 1) * stride + E_max above n_received";
    if (frames > 0xFFFFFFFFull / (3 * D)) return "frames * 3 D must lie below 2^32";
    const size_t out_b = frames * 3 * D * sb;
    if (overlap(d_out, out_b, d_received, n_received * sb)) return "d_symbols_out overlaps d_received";
    if (overlap(d_out, out_b, d_offset, frames * sizeof(uint32_t)) || overlap(d_out, out_b, d_count, frames * sizeof(uint32_t)))
        return "d_symbols_out overlaps d_offset or d_count";
    (void)d_scramble;
    return nullptr;
}

}  // namespace

extern "C" {

int vit_hip_lte_rate_dematch_batch(vit_hip_handle h, const void* d_received, size_t n_received, size_t received_frame_stride,
                                   const uint32_t* d_offset, const uint32_t* d_count, size_t frames, size_t D, size_t E_max,
                                   const uint8_t* d_scramble, size_t scramble_period, unsigned shift, int clamp_lo, int clamp_hi,
                                   void* d_symbols_out, vit_hip_stream_t stream) {
    if (const char* why = lte_invalid(h, d_received, n_received, received_frame_stride, d_offset, d_count, frames, D, E_max, d_scramble, shift,
                                      clamp_lo, clamp_hi, d_symbols_out))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (frames == 0) return VIT_HIP_OK;
    const LteArgs a = lte_dematch_args(d_received, n_received, received_frame_stride, d_offset, d_count, frames, D, E_max, d_scramble,
                                       scramble_period, shift, clamp_lo, clamp_hi, d_symbols_out, (size_t)h->soft_bytes);
    VIT_HIP_ON_DEVICE(h->device);
    if (lte_launch_dematch(a, (size_t)h->soft_bytes, (hipStream_t)stream) != 0) return fail(VIT_HIP_ERR_RUNTIME, "lte de-match launch failed");
    return VIT_HIP_OK;
}

}  // extern "C"
