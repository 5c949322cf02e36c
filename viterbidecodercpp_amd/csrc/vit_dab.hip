// vit_dab.hip -- the DAB receive chain of the C ABI around vit_hip_decode_batch (ETSI EN 300 401): vit_hip_dab_deinterleave_batch (the
// time de-interleaver of clause 12 with its 15 frames of history carried between calls, fused with the depuncturing of clause 11: it
// writes the [frames][S][4] symbols the decode reads) and vit_hip_dab_descramble_batch (the energy-dispersal sequence of clause 10 XORed
// off the decoded bytes).  Both work on the caller's elements alone and read the handle for its device and its symbol width.  The
// kernels of kernels_dab.hpp are launched only here.  Host-side logic only: the argument rules (kernels_dab.hpp, so that they run without
// a device) and the launches.
// Out of scope: the UEP profile table; a fast path for one short push; OFDM demodulation and frequency de-interleaving.  DAB+
// superframes are vit_dabplus.hip.
#include "vit_internal.hpp"
#include "kernels_dab.hpp"

using namespace vit;

extern "C" {

int vit_hip_dab_deinterleave_batch(vit_hip_handle h, const void* d_in, size_t in_row_stride, size_t in_frame_stride, size_t rows,
                                   size_t max_frames, const uint32_t* d_n_frames, size_t n_received, const int32_t* d_source_index,
                                   size_t symbols_per_frame, const void* d_hist_in, const uint32_t* d_fill_in, size_t hist_row_stride,
                                   void* d_out, uint32_t* d_n_out, void* d_hist_out, uint32_t* d_fill_out, vit_hip_stream_t stream) {
    if (const char* why = dab_deinterleave_invalid(h != nullptr, h ? (size_t)h->soft_bytes : 1, d_in, in_row_stride, in_frame_stride, rows, max_frames,
                                                   d_n_frames, n_received, d_source_index, symbols_per_frame, d_hist_in, d_fill_in, hist_row_stride,
                                                   d_out, d_n_out, d_hist_out, d_fill_out))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (rows == 0 || max_frames == 0) return VIT_HIP_OK;
    DabDeintArgs a{};
    a.in = d_in; a.n_frames = d_n_frames; a.map = d_source_index; a.hist_in = d_hist_in; a.fill_in = d_hist_in ? d_fill_in : nullptr;
    a.out = d_out; a.n_out = d_n_out; a.hist_out = d_hist_out; a.fill_out = d_fill_out;
    a.frame_stride = in_frame_stride ? in_frame_stride : n_received;
    a.row_stride = in_row_stride ? in_row_stride : max_frames * a.frame_stride;
    a.hist_stride = hist_row_stride ? hist_row_stride : DAB_H * n_received;
    a.rows = (uint32_t)rows; a.max_frames = (uint32_t)max_frames; a.n = (uint32_t)n_received; a.spf = (uint32_t)symbols_per_frame;
    a.total = (uint32_t)(rows * max_frames * symbols_per_frame);
    dab_deinterleave_split(a, (size_t)h->soft_bytes);
    if (dab_deinterleave_blocks(a) > 0x7FFFFFFFu) return fail(VIT_HIP_ERR_INVALID_ARG, "more than 2^31 - 1 blocks");
    VIT_HIP_ON_DEVICE(h->device);
    if (dab_launch_deinterleave(a, (size_t)h->soft_bytes, (hipStream_t)stream) != 0)
        return fail(VIT_HIP_ERR_RUNTIME, "dab deinterleave launch failed");
    return VIT_HIP_OK;
}

int vit_hip_dab_descramble_batch(vit_hip_handle h, const uint8_t* d_in, size_t frame_stride_bytes, size_t rows, size_t max_frames,
                                 const uint32_t* d_n_frames, size_t n_bits, uint8_t* d_out, size_t out_stride_bytes, vit_hip_stream_t stream) {
    if (const char* why = dab_descramble_invalid(h != nullptr, d_in, frame_stride_bytes, rows, max_frames, d_n_frames, n_bits, d_out, out_stride_bytes))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (rows == 0 || max_frames == 0 || n_bits == 0) return VIT_HIP_OK;
    DabDescrArgs a{};
    a.in = d_in; a.n_frames = d_n_frames; a.out = d_out;
    a.n_bits = (uint32_t)n_bits; a.nb = (uint32_t)((n_bits + 7) / 8);
    a.stride = frame_stride_bytes ? frame_stride_bytes : a.nb;
    a.out_stride = out_stride_bytes ? out_stride_bytes : a.nb;
    a.max_frames = (uint32_t)max_frames; a.frames = (uint32_t)(rows * max_frames);
    a.U = a.nb / 4u + 2u;                                          // ceil((nb + 3) / 4) dwords at the worst alignment, and one to spare
    a.units = (uint64_t)a.frames * a.U;
    if (dab_descramble_blocks(a) > 0x7FFFFFFFu) return fail(VIT_HIP_ERR_INVALID_ARG, "more than 2^31 - 1 blocks");
    VIT_HIP_ON_DEVICE(h->device);
    if (dab_launch_descramble(a, (hipStream_t)stream) != 0) return fail(VIT_HIP_ERR_RUNTIME, "dab descramble launch failed");
    return VIT_HIP_OK;
}

}  // extern "C"
