// vit_crc.hip -- the frame check of the C ABI: vit_hip_crc_batch (the CRC of a bit range of every frame in the layout
// vit_hip_frames_extract writes, any width up to 32, and its syndrome against the transmitted field: CCSDS FECF, LTE, DAB, MPEG-2 PSI).
// It works on the caller's bytes alone and reads the handle only for its device.  The kernel of kernels_crc.hpp is launched only here.
// Host-side logic only: the argument rule (kernels_crc.hpp, so that it runs without a device), the handful of constants of the code and
// the launch.
// Out of scope: reflected CRCs; widths above 32; per-frame lengths or codes in one call; a GPU-side CRC append.
#include "vit_internal.hpp"
#include "kernels_crc.hpp"

using namespace vit;

extern "C" {

int vit_hip_crc_batch(vit_hip_handle h, const vit_hip_crc_params* crc, const uint8_t* d_frames, size_t frame_stride_bytes, size_t rows,
                      size_t max_frames, const uint32_t* d_n_frames, size_t first_bit, size_t n_bits, uint32_t* d_crc, uint32_t* d_syndrome,
                      vit_hip_stream_t stream) {
    if (const char* why = crc_invalid(h != nullptr, crc, d_frames, frame_stride_bytes, rows, max_frames, first_bit, n_bits, d_crc, d_syndrome))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (rows == 0 || max_frames == 0) return VIT_HIP_OK;
    const CrcArgs a = crc_batch_args(*crc, d_frames, frame_stride_bytes, rows, max_frames, d_n_frames, first_bit, n_bits, d_crc, d_syndrome);
    VIT_HIP_ON_DEVICE(h->device);
    if (crc_launch_batch(a, (hipStream_t)stream) != 0) return fail(VIT_HIP_ERR_RUNTIME, "crc launch failed");
    return VIT_HIP_OK;
}

}  // extern "C"
