// vit_frames.hip -- frame extraction of the C ABI: vit_hip_frames_extract (the frames of decoded, bit-packed rows cut at the lock that
// vit_hip_marker_search wrote, byte-aligned, complemented, derandomised, with the unfinished frame carried to the next call) and
// vit_hip_frames_capacity.  It works on the caller's bytes alone and reads the handle only for its device.  The kernel of
// kernels_frames.hpp is launched only here.  Host-side logic only: argument checking and the launch.
#include "vit_internal.hpp"
#include "kernels_frames.hpp"

using namespace vit;

namespace {

// argument rule (include/vit_hip.h): everything the host can know without reading device memory
const char* frames_invalid(const uint8_t* d_bytes, size_t stride, size_t rows, size_t n_bits, size_t P, size_t phase0,
                           const vit_hip_marker_lock* d_lock, const uint8_t* d_carry_in, const uint32_t* d_carry_bits_in,
                           size_t carry_stride, uint64_t marker, unsigned m, size_t drop, const uint8_t* d_frames, size_t frame_stride,
                           size_t max_frames, const uint32_t* d_n_frames, const uint8_t* d_carry_out, const uint32_t* d_carry_bits_out) {
    if (!d_bytes || !d_lock || !d_frames || !d_n_frames || !d_carry_out || !d_carry_bits_out) return "NULL buffer";
    if (d_carry_in && !d_carry_bits_in) return "d_carry_in without d_carry_bits_in";
    if (P < 8 || P >= 0x80000000ull) return "period_bits must be 8 .. 2^31 - 1";
    if (phase0 >= P) return "phase0 must be below period_bits";
    if (drop >= P) return "drop_bits must be below period_bits";
    if (m > 64 || m > P) return "marker_bits must be 0 .. 64 and at most period_bits";
    if (m < 64 && (marker >> m) != 0) return "marker has bits above marker_bits";
    if (n_bits == 0 || n_bits >= 0x100000000ull - 64) return "n_bits must be 1 .. 2^32 - 65";
    if (stride != 0 && stride < (n_bits + 7) / 8) return "bytes_row_stride is below ceil(n_bits / 8)";
    if (carry_stride != 0 && carry_stride < (P - 1 + 7) / 8) return "carry_row_stride is below ceil((period_bits - 1) / 8)";
    if (frame_stride != 0 && frame_stride < (P - drop + 7) / 8) return "frame_stride_bytes is below ceil((period_bits - drop_bits) / 8)";
    if (max_frames < vit_hip_frames_capacity(n_bits, P)) return "max_frames is below vit_hip_frames_capacity";
    if (rows > 0x7FFFFFFFu) return "more than 2^31 - 1 rows";
    return nullptr;
}

}  // namespace

extern "C" {

size_t vit_hip_frames_capacity(size_t n_bits, size_t period_bits) {
    return period_bits ? n_bits / period_bits + (n_bits % period_bits ? 1 : 0) : 0;
}

int vit_hip_frames_extract(vit_hip_handle h, const uint8_t* d_bytes, size_t bytes_row_stride, size_t rows, size_t n_bits,
                           size_t period_bits, size_t phase0, const vit_hip_marker_lock* d_lock, const uint8_t* d_carry_in,
                           const uint32_t* d_carry_bits_in, size_t carry_row_stride, uint64_t marker, unsigned marker_bits,
                           size_t drop_bits, const uint8_t* d_pad, uint8_t* d_frames, size_t frame_stride_bytes, size_t max_frames,
                           uint32_t* d_n_frames, uint32_t* d_marker_errors, uint8_t* d_carry_out, uint32_t* d_carry_bits_out,
                           vit_hip_stream_t stream) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    if (const char* why = frames_invalid(d_bytes, bytes_row_stride, rows, n_bits, period_bits, phase0, d_lock, d_carry_in, d_carry_bits_in,
                                         carry_row_stride, marker, marker_bits, drop_bits, d_frames, frame_stride_bytes, max_frames,
                                         d_n_frames, d_carry_out, d_carry_bits_out))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (rows == 0) return VIT_HIP_OK;
    const FramesArgs a = frames_extract_args(d_bytes, bytes_row_stride, rows, n_bits, (uint32_t)period_bits, phase0, d_lock, d_carry_in,
                                             d_carry_bits_in, carry_row_stride, marker, marker_bits, (uint32_t)drop_bits, d_pad, d_frames,
                                             frame_stride_bytes, max_frames, d_n_frames, d_marker_errors, d_carry_out, d_carry_bits_out);
    VIT_HIP_ON_DEVICE(h->device);
    if (frames_launch_extract(a, (hipStream_t)stream) != 0) return fail(VIT_HIP_ERR_RUNTIME, "frames extract launch failed");
    return VIT_HIP_OK;
}

}  // extern "C"
