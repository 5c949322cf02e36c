// vit_dab.hip -- the DAB receive chain of the C ABI around vit_hip_decode_batch (ETSI EN 300 401): vit_hip_dab_deinterleave_batch (the
// time de-interleaver of clause 12 with its 15 frames of history carried between calls, fused with the depuncturing of clause 11: it
// writes the [frames][S][4] symbols the decode reads) and vit_hip_dab_descramble_batch (the energy-dispersal sequence of clause 10 XORed
// off the decoded bytes).  Both work on the caller's elements alone and read the handle for its device and its symbol width.  The
// kernels of kernels_dab.hpp are launched only here.  Host-side logic only: argument checking and the launches.
// Out of scope: the UEP profile table; a fast path for one short push; OFDM demodulation and frequency de-interleaving.  DAB+
// superframes are vit_dabplus.hip.
#include "vit_internal.hpp"
#include "kernels_dab.hpp"

using namespace vit;

namespace {

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}

// units from the first item's first to the last item's last
size_t extent(size_t items, size_t stride, size_t each) { return items ? (items - 1) * stride + each : 0; }

// argument rule (include/vit_hip.h): everything the host can know without reading device memory
const char* deinterleave_invalid(vit_hip_handle h, const void* d_in, size_t row_stride, size_t frame_stride, size_t rows, size_t max_frames,
                                 const uint32_t* d_n_frames, size_t n, const int32_t* d_map, size_t spf, const void* d_hist_in,
                                 const uint32_t* d_fill_in, size_t hist_stride, const void* d_out, const uint32_t* d_n_out,
                                 const void* d_hist_out, const uint32_t* d_fill_out) {
    if (!h || !d_in || !d_out || !d_n_out || !d_hist_out || !d_fill_out) return "NULL handle or buffer";
    if (d_hist_in && !d_fill_in) return "d_hist_in without d_fill_in";
    if (n == 0 || spf == 0) return "n_received and symbols_per_frame must be at least 1";
    if (n > 0xFFFFFFFFull / (DAB_H + 1) || spf > 0xFFFFFFFFull) return "16 * n_received and symbols_per_frame must lie below 2^32";
    if (!d_map && spf != n) return "d_source_index == NULL (the identity) needs symbols_per_frame == n_received";
    const size_t fs = frame_stride ? frame_stride : n;
    if (fs < n) return "in_frame_stride is below n_received";
    if (max_frames > 0xFFFFFFFFFFFFull / fs) return "max_frames * in_frame_stride is too large";
    if (row_stride != 0 && row_stride < max_frames * fs) return "in_row_stride is below max_frames * in_frame_stride";
    if (hist_stride != 0 && hist_stride < DAB_H * n) return "hist_row_stride is below 15 * n_received";
    const size_t sb = (size_t)h->soft_bytes;
    if ((uintptr_t)d_in % sb || (uintptr_t)d_out % sb || (uintptr_t)d_hist_in % sb || (uintptr_t)d_hist_out % sb)
        return "d_in, d_out and the histories must be aligned to the symbol type";
    if ((uintptr_t)d_map % 4 || (uintptr_t)d_n_frames % 4 || (uintptr_t)d_fill_in % 4 || (uintptr_t)d_n_out % 4 || (uintptr_t)d_fill_out % 4)
        return "d_source_index and the count arrays must be aligned to 4 bytes";
    if (rows == 0 || max_frames == 0) return nullptr;
    if (rows > 0x7FFFFFFFu || max_frames > 0x7FFFFFFFu) return "more than 2^31 - 1 rows or frames";
    if (rows * max_frames > 0xFFFFFFFFull / spf) return "rows * max_frames * symbols_per_frame must lie below 2^32";
    const size_t rs = row_stride ? row_stride : max_frames * fs;
    const size_t in_b = ((rows - 1) * rs + extent(max_frames, fs, n)) * sb, out_b = rows * max_frames * spf * sb;
    const size_t hist_b = extent(rows, hist_stride ? hist_stride : DAB_H * n, DAB_H * n) * sb, cnt_b = rows * sizeof(uint32_t);
    const size_t map_b = spf * sizeof(int32_t);
    if (overlap(d_out, out_b, d_in, in_b) || overlap(d_out, out_b, d_hist_in, hist_b) || overlap(d_out, out_b, d_hist_out, hist_b) ||
        overlap(d_out, out_b, d_map, map_b))
        return "d_out overlaps the input, a history or d_source_index";
    if (overlap(d_hist_out, hist_b, d_in, in_b) || overlap(d_hist_out, hist_b, d_hist_in, hist_b) || overlap(d_hist_out, hist_b, d_map, map_b))
        return "d_hist_out overlaps the input, d_hist_in or d_source_index";
    if (overlap(d_n_out, cnt_b, d_n_frames, cnt_b) || overlap(d_n_out, cnt_b, d_fill_in, cnt_b) || overlap(d_fill_out, cnt_b, d_n_frames, cnt_b) ||
        overlap(d_fill_out, cnt_b, d_fill_in, cnt_b) || overlap(d_n_out, cnt_b, d_fill_out, cnt_b))
        return "the count arrays overlap";
    return nullptr;
}

const char* descramble_invalid(vit_hip_handle h, const uint8_t* d_in, size_t stride, size_t rows, size_t max_frames, const uint32_t* d_n_frames,
                               size_t n_bits, const uint8_t* d_out, size_t out_stride) {
    if (!h || !d_in || !d_out) return "NULL handle, d_in or d_out";
    if (n_bits >= 0xFFFFFFFFull - 32) return "n_bits + 32 must lie below 2^32 - 1";
    const size_t nb = (n_bits + 7) / 8;
    if (stride != 0 && stride < nb) return "frame_stride_bytes does not cover n_bits";
    if (out_stride != 0 && out_stride < nb) return "out_stride_bytes does not cover n_bits";
    if (rows == 0 || max_frames == 0 || n_bits == 0) return nullptr;
    if (rows > 0x7FFFFFFFu || max_frames > 0x7FFFFFFFu) return "more than 2^31 - 1 rows or frames";
    const size_t frames = rows * max_frames, s_in = stride ? stride : nb, s_out = out_stride ? out_stride : nb;
    if (frames > 0xFFFFFFFFull / (nb / 4 + 2)) return "rows * max_frames * (ceil(n_bits / 32) + 2) must lie below 2^32";
    if (d_in == d_out ? s_in != s_out : overlap(d_out, extent(frames, s_out, nb), d_in, extent(frames, s_in, nb)))
        return "d_out overlaps d_in without being equal to it at equal strides";
    if (overlap(d_out, extent(frames, s_out, nb), d_n_frames, rows * sizeof(uint32_t))) return "d_out overlaps d_n_frames";
    return nullptr;
}

}  // namespace

extern "C" {

int vit_hip_dab_deinterleave_batch(vit_hip_handle h, const void* d_in, size_t in_row_stride, size_t in_frame_stride, size_t rows,
                                   size_t max_frames, const uint32_t* d_n_frames, size_t n_received, const int32_t* d_source_index,
                                   size_t symbols_per_frame, const void* d_hist_in, const uint32_t* d_fill_in, size_t hist_row_stride,
                                   void* d_out, uint32_t* d_n_out, void* d_hist_out, uint32_t* d_fill_out, vit_hip_stream_t stream) {
    if (const char* why = deinterleave_invalid(h, d_in, in_row_stride, in_frame_stride, rows, max_frames, d_n_frames, n_received, d_source_index,
                                               symbols_per_frame, d_hist_in, d_fill_in, hist_row_stride, d_out, d_n_out, d_hist_out, d_fill_out))
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
    if (const char* why = descramble_invalid(h, d_in, frame_stride_bytes, rows, max_frames, d_n_frames, n_bits, d_out, out_stride_bytes))
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
