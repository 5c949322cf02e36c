// vit_crc.hip -- the frame check of the C ABI: vit_hip_crc_batch (the CRC of a bit range of every frame in the layout
// vit_hip_frames_extract writes, any width up to 32, and its syndrome against the transmitted field: CCSDS FECF, LTE, DAB, MPEG-2 PSI).
// It works on the caller's bytes alone and reads the handle only for its device.  The kernel of kernels_crc.hpp is launched only here.
// Host-side logic only: argument checking, the handful of constants of the code and the launch.
// Out of scope: reflected CRCs; widths above 32; per-frame lengths or codes in one call; a GPU-side CRC append.
#include "vit_internal.hpp"
#include "kernels_crc.hpp"

using namespace vit;

namespace {

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}

// argument rule (include/vit_hip.h): everything the host can know without reading device memory
const char* crc_invalid(vit_hip_handle h, const vit_hip_crc_params* c, const uint8_t* d_frames, size_t stride, size_t rows, size_t max_frames,
                        size_t first_bit, size_t n_bits, const uint32_t* d_crc, const uint32_t* d_syndrome) {
    if (!h || !c || !d_frames) return "NULL handle, crc or d_frames";
    if (!d_crc && !d_syndrome) return "d_crc and d_syndrome are both NULL";
    if (c->width < 1 || c->width > 32) return "width must be 1 .. 32";
    const uint64_t top = 1ull << c->width;
    if (c->poly >= top || c->init >= top || c->xorout >= top) return "poly, init and xorout must lie below 2^width";
    if (first_bit >= 0xFFFFFFFFull || n_bits >= 0xFFFFFFFFull || first_bit + n_bits + 32 >= 0xFFFFFFFFull)
        return "first_bit + n_bits + 32 must lie below 2^32 - 1";
    const size_t need = (first_bit + n_bits + (d_syndrome ? c->width : 0u) + 7) / 8;
    if (stride != 0 && stride < need) return "frame_stride_bytes does not cover first_bit + n_bits (+ width)";
    if (rows == 0 || max_frames == 0) return nullptr;
    if (rows > 0x7FFFFFFFu || max_frames > 0x7FFFFFFFu) return "more than 2^31 - 1 blocks";
    const size_t frames = rows * max_frames;
    if (frames > ((uint64_t)0x7FFFFFFFu * CRC_BLOCK) >> crc_geometry(n_bits).logG) return "more than 2^31 - 1 blocks";
    const size_t in_b = (frames - 1) * (stride ? stride : need) + need, out_b = frames * sizeof(uint32_t);
    if (overlap(d_crc, out_b, d_syndrome, out_b)) return "d_crc overlaps d_syndrome";
    if (overlap(d_crc, out_b, d_frames, in_b) || overlap(d_syndrome, out_b, d_frames, in_b)) return "an output overlaps d_frames";
    return nullptr;
}

}  // namespace

extern "C" {

int vit_hip_crc_batch(vit_hip_handle h, const vit_hip_crc_params* crc, const uint8_t* d_frames, size_t frame_stride_bytes, size_t rows,
                      size_t max_frames, const uint32_t* d_n_frames, size_t first_bit, size_t n_bits, uint32_t* d_crc, uint32_t* d_syndrome,
                      vit_hip_stream_t stream) {
    if (const char* why = crc_invalid(h, crc, d_frames, frame_stride_bytes, rows, max_frames, first_bit, n_bits, d_crc, d_syndrome))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (rows == 0 || max_frames == 0) return VIT_HIP_OK;
    const CrcArgs a = crc_batch_args(*crc, d_frames, frame_stride_bytes, rows, max_frames, d_n_frames, first_bit, n_bits, d_crc, d_syndrome);
    VIT_HIP_ON_DEVICE(h->device);
    if (crc_launch_batch(a, (hipStream_t)stream) != 0) return fail(VIT_HIP_ERR_RUNTIME, "crc launch failed");
    return VIT_HIP_OK;
}

}  // extern "C"
