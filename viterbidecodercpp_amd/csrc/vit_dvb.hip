// vit_dvb.hip -- the DVB-S outer chain of the C ABI around vit_hip_rs_decode_batch: vit_hip_deinterleave_batch (the convolutional
// de-interleaver, any (branches, cell, packet) with its history carried between calls) and vit_hip_dvb_derandomize_batch (the
// energy-dispersal sequence XORed off, the inverted every-eighth sync byte put upright, the group phase carried or voted).  Both work
// on the caller's bytes alone and read the handle only for its device.  The kernels of kernels_dvb.hpp are launched only here.
// Host-side logic only: argument checking and the launches.
#include "vit_internal.hpp"
#include "kernels_dvb.hpp"

using namespace vit;

namespace {

// argument rule (include/vit_hip.h): everything the host can know without reading device memory.  *H_out: packets of history
const char* deinterleave_invalid(vit_hip_handle h, const uint8_t* d_in, size_t stride, size_t rows, size_t max_frames, const uint32_t* d_n_frames,
                                 size_t B, size_t M, size_t n, const uint8_t* d_hist_in, const uint32_t* d_fill_in, size_t hist_stride,
                                 const uint8_t* d_out, size_t out_stride, const uint32_t* d_n_out, const uint8_t* d_hist_out,
                                 const uint32_t* d_fill_out, size_t* H_out) {
    if (!h || !d_in || !d_out || !d_n_out || !d_hist_out || !d_fill_out) return "NULL handle or buffer";
    if (d_hist_in && !d_fill_in) return "d_hist_in without d_fill_in";
    if (B < 2 || M < 1 || n == 0 || n % B != 0) return "branches must be at least 2, cell at least 1, packet_bytes a multiple of branches";
    if (n > DVB_LDS_BYTES || M > DVB_LDS_BYTES) return "(H + 1) * packet_bytes is above 32768";
    const size_t D = (B - 1) * M * B, H = (D + n - 1) / n;
    if ((H + 1) * n > DVB_LDS_BYTES) return "(H + 1) * packet_bytes is above 32768";
    if (stride != 0 && stride < n) return "frame_stride_bytes is below packet_bytes";
    if (out_stride != 0 && out_stride < n) return "out_stride_bytes is below packet_bytes";
    if (hist_stride != 0 && hist_stride < H * n) return "hist_row_stride is below H * packet_bytes";
    *H_out = H;
    if (rows == 0 || max_frames == 0) return nullptr;
    if (rows > 0x7FFFFFFFu || max_frames > 0x7FFFFFFFu) return "more than 2^31 - 1 rows or packets";
    const size_t packets = rows * max_frames;
    const size_t in_b = extent(packets, stride ? stride : n, n), out_b = extent(packets, out_stride ? out_stride : n, n);
    const size_t hist_b = extent(rows, hist_stride ? hist_stride : H * n, H * n), cnt_b = rows * sizeof(uint32_t);
    if (overlap(d_out, out_b, d_in, in_b) || overlap(d_out, out_b, d_hist_in, hist_b) || overlap(d_out, out_b, d_hist_out, hist_b))
        return "d_out overlaps the input or a history";
    if (overlap(d_hist_out, hist_b, d_in, in_b) || overlap(d_hist_out, hist_b, d_hist_in, hist_b)) return "d_hist_out overlaps the input or d_hist_in";
    if (overlap(d_n_out, cnt_b, d_n_frames, cnt_b) || overlap(d_n_out, cnt_b, d_fill_in, cnt_b) || overlap(d_fill_out, cnt_b, d_n_frames, cnt_b) ||
        overlap(d_fill_out, cnt_b, d_fill_in, cnt_b) || overlap(d_n_out, cnt_b, d_fill_out, cnt_b))
        return "the count arrays overlap";
    return nullptr;
}

const char* derandomize_invalid(vit_hip_handle h, const uint8_t* d_in, size_t stride, size_t n, size_t rows, size_t max_frames,
                                const uint32_t* d_phase_in, const uint8_t* d_out, size_t out_stride, const uint32_t* d_phase_out) {
    if (!h || !d_in || !d_out || !d_phase_out) return "NULL handle or buffer";
    if (n < DVB_PACKET) return "packet_bytes is below 188";
    if (stride != 0 && stride < n) return "frame_stride_bytes is below packet_bytes";
    if (out_stride != 0 && out_stride < DVB_PACKET) return "out_stride_bytes is below 188";
    if (rows == 0 || max_frames == 0) return nullptr;
    if (rows > 0x7FFFFFFFu || max_frames > 0x7FFFFFFFu) return "more than 2^31 - 1 rows or packets";
    const size_t packets = rows * max_frames, s_in = stride ? stride : n, s_out = out_stride ? out_stride : DVB_PACKET;
    if (d_in == d_out ? s_in != s_out : overlap(d_out, extent(packets, s_out, DVB_PACKET), d_in, extent(packets, s_in, DVB_PACKET)))
        return "d_out overlaps d_in without being equal to it at equal strides";
    if (overlap(d_phase_out, rows * sizeof(uint32_t), d_phase_in, rows * sizeof(uint32_t))) return "d_phase_out overlaps d_phase_in";
    return nullptr;
}

}  // namespace

extern "C" {

int vit_hip_deinterleave_batch(vit_hip_handle h, const uint8_t* d_in, size_t frame_stride_bytes, size_t rows, size_t max_frames,
                               const uint32_t* d_n_frames, size_t branches, size_t cell, size_t packet_bytes, const uint8_t* d_hist_in,
                               const uint32_t* d_fill_in, size_t hist_row_stride, uint8_t* d_out, size_t out_stride_bytes, uint32_t* d_n_out,
                               uint8_t* d_hist_out, uint32_t* d_fill_out, vit_hip_stream_t stream) {
    size_t H = 0;
    if (const char* why = deinterleave_invalid(h, d_in, frame_stride_bytes, rows, max_frames, d_n_frames, branches, cell, packet_bytes, d_hist_in,
                                               d_fill_in, hist_row_stride, d_out, out_stride_bytes, d_n_out, d_hist_out, d_fill_out, &H))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (rows == 0 || max_frames == 0) return VIT_HIP_OK;
    const size_t n = packet_bytes;
    DeintArgs a{};
    a.in = d_in; a.n_frames = d_n_frames; a.hist_in = d_hist_in; a.fill_in = d_hist_in ? d_fill_in : nullptr;
    a.out = d_out; a.n_out = d_n_out; a.hist_out = d_hist_out; a.fill_out = d_fill_out;
    a.stride = frame_stride_bytes ? frame_stride_bytes : n;
    a.out_stride = out_stride_bytes ? out_stride_bytes : n;
    a.hist_stride = hist_row_stride ? hist_row_stride : H * n;
    a.max_frames = max_frames;
    a.B = (uint32_t)branches; a.MB = (uint32_t)(cell * branches); a.n = (uint32_t)n; a.H = (uint32_t)H;
    a.magic = (uint32_t)((0x100000000ull + branches - 1) / branches);
    size_t G = DVB_LDS_BYTES / n - H;                              // >= 1: the argument rule
    G = G < DVB_G_MAX ? G : DVB_G_MAX;
    G = G < max_frames ? G : max_frames;
    const size_t GH = DVB_HIST_BLOCK_BYTES / n ? DVB_HIST_BLOCK_BYTES / n : 1;
    const size_t ob = (max_frames + G - 1) / G, hb = (H + GH - 1) / GH;
    if (rows * (ob + hb) > 0x7FFFFFFFu) return fail(VIT_HIP_ERR_INVALID_ARG, "more than 2^31 - 1 blocks");
    a.G = (uint32_t)G; a.GH = (uint32_t)GH; a.ob = (uint32_t)ob; a.hb = (uint32_t)hb;
    VIT_HIP_ON_DEVICE(h->device);
    if (dvb_launch_deinterleave(a, rows, (hipStream_t)stream) != 0) return fail(VIT_HIP_ERR_RUNTIME, "deinterleave launch failed");
    return VIT_HIP_OK;
}

int vit_hip_dvb_derandomize_batch(vit_hip_handle h, const uint8_t* d_in, size_t frame_stride_bytes, size_t packet_bytes, size_t rows,
                                  size_t max_frames, const uint32_t* d_n_frames, const uint32_t* d_phase_in, const int32_t* d_rs_status,
                                  uint8_t* d_out, size_t out_stride_bytes, uint32_t* d_phase_out, uint32_t* d_sync_errors,
                                  vit_hip_stream_t stream) {
    if (const char* why = derandomize_invalid(h, d_in, frame_stride_bytes, packet_bytes, rows, max_frames, d_phase_in, d_out, out_stride_bytes,
                                              d_phase_out))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (rows == 0 || max_frames == 0) return VIT_HIP_OK;
    DerandArgs a{};
    a.in = d_in; a.n_frames = d_n_frames; a.phase_in = d_phase_in; a.rs_status = d_rs_status;
    a.out = d_out; a.phase_out = d_phase_out; a.sync_errors = d_sync_errors;
    a.stride = frame_stride_bytes ? frame_stride_bytes : packet_bytes;
    a.out_stride = out_stride_bytes ? out_stride_bytes : DVB_PACKET;
    a.max_frames = max_frames;
    const bool in_place = d_in == d_out;
    // out of place at most 128 blocks a row: with an unknown phase EVERY block of a row reads all of the row's sync bytes
    const size_t PB = in_place ? max_frames : (max_frames + 127) / 128 > 32 ? (max_frames + 127) / 128 : 32;
    const size_t bpr = (max_frames + PB - 1) / PB;
    if (rows * bpr > 0x7FFFFFFFu) return fail(VIT_HIP_ERR_INVALID_ARG, "more than 2^31 - 1 blocks");
    a.PB = (uint32_t)PB; a.bpr = (uint32_t)bpr;
    VIT_HIP_ON_DEVICE(h->device);
    if (dvb_launch_derandomize(a, rows, in_place, (hipStream_t)stream) != 0) return fail(VIT_HIP_ERR_RUNTIME, "dvb derandomize launch failed");
    return VIT_HIP_OK;
}

}  // extern "C"
