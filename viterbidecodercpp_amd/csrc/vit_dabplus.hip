// vit_dabplus.hip -- DAB+ audio superframes of the C ABI (ETSI TS 102 563) behind the DAB receive chain: vit_hip_dabplus_sync (which of
// five logical frames starts a superframe: the Fire code over the header, summed per phase, and the lock vit_hip_frames_extract reads) and
// vit_hip_dabplus_au_batch (behind vit_hip_rs_decode_batch: the header's access-unit table and the CRC-16 of every access unit, over
// ranges the device reads from the superframe itself).  Both work on the caller's bytes alone and read the handle only for its device.
// The kernels of kernels_dabplus.hpp are launched only here.  Host-side logic only: argument checking and the launches.
// Out of scope: AAC decoding, PAD extraction, compacting the access units, DMB and enhanced packet mode, a lock policy, s > 24, UEP.
#include "vit_internal.hpp"
#include "kernels_dabplus.hpp"

using namespace vit;

namespace {

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}

// argument rules (include/vit_hip.h): everything the host can know without reading device memory
const char* sync_invalid(vit_hip_handle h, const uint8_t* d_frames, size_t row_stride, size_t frame_stride, size_t frame_bytes, size_t rows,
                         size_t max_frames, const uint32_t* d_n_frames, unsigned frame0, unsigned flags, const uint32_t* d_hits,
                         const uint32_t* d_count, const vit_hip_marker_lock* d_lock) {
    if (!h || !d_frames || !d_hits || !d_count) return "NULL handle, d_frames, d_hits or d_count";
    if (flags & ~VIT_HIP_MARKER_ACCUMULATE) return "unknown flag bits";
    if (frame_bytes < 11) return "frame_bytes must be at least 11";
    if (frame_bytes > 0x7FFFFFFFull / 40) return "40 * frame_bytes must lie below 2^31";
    if (frame0 >= DABPLUS_PHASES) return "frame0 must be below 5";
    const size_t fs = frame_stride ? frame_stride : frame_bytes;
    if (fs < frame_bytes) return "frame_stride is below frame_bytes";
    if (rows > 0x7FFFFFFFu || max_frames > 0x7FFFFFFFu) return "more than 2^31 - 1 rows or frames";
    if (fs > 0xFFFFFFFFFFFFull / (max_frames ? max_frames : 1)) return "max_frames * frame_stride is too large";
    if (row_stride != 0 && row_stride < max_frames * fs) return "row_stride is below max_frames * frame_stride";
    if ((uintptr_t)d_n_frames % 4 || (uintptr_t)d_hits % 4 || (uintptr_t)d_count % 4 || (uintptr_t)d_lock % 4)
        return "the count arrays, the totals and d_lock must be aligned to 4 bytes";
    if (rows == 0) return nullptr;
    const size_t rs = row_stride ? row_stride : max_frames * fs;
    const size_t in_b = max_frames ? (rows - 1) * rs + (max_frames - 1) * fs + frame_bytes : 0, tot_b = rows * DABPLUS_PHASES * sizeof(uint32_t);
    const size_t lock_b = rows * sizeof(vit_hip_marker_lock), cnt_b = rows * sizeof(uint32_t);
    if (overlap(d_hits, tot_b, d_count, tot_b) || overlap(d_hits, tot_b, d_lock, lock_b) || overlap(d_count, tot_b, d_lock, lock_b))
        return "d_hits, d_count and d_lock overlap";
    if (overlap(d_hits, tot_b, d_frames, in_b) || overlap(d_count, tot_b, d_frames, in_b) || overlap(d_lock, lock_b, d_frames, in_b) ||
        overlap(d_hits, tot_b, d_n_frames, cnt_b) || overlap(d_count, tot_b, d_n_frames, cnt_b) || overlap(d_lock, lock_b, d_n_frames, cnt_b))
        return "an output overlaps the frames or d_n_frames";
    return nullptr;
}

const char* au_invalid(vit_hip_handle h, const uint8_t* d_in, size_t stride, size_t rows, size_t max_frames, const uint32_t* d_n_frames,
                       unsigned s, const int32_t* d_rs_status, const uint32_t* d_info, const vit_hip_dabplus_au* d_au) {
    if (!h || !d_in || !d_info || !d_au) return "NULL handle, d_in, d_info or d_au";
    if (s < 1 || s > 24) return "s must be 1 .. 24";
    if (stride != 0 && stride < 110u * s) return "frame_stride_bytes is below 110 s";
    if ((uintptr_t)d_n_frames % 4 || (uintptr_t)d_rs_status % 4 || (uintptr_t)d_info % 4 || (uintptr_t)d_au % 4)
        return "the count array, d_rs_status, d_info and d_au must be aligned to 4 bytes";
    if (rows == 0 || max_frames == 0) return nullptr;
    if (rows > 0x7FFFFFFFu || max_frames > 0x7FFFFFFFu) return "more than 2^31 - 1 rows or frames";
    const size_t frames = rows * max_frames, st = stride ? stride : 120u * s;
    if (frames > 0x7FFFFFFFull * DABPLUS_BLOCK / (DABPLUS_SLOTS * 64u)) return "more than 2^31 - 1 blocks";
    const size_t in_b = (frames - 1) * st + 110u * s, info_b = frames * sizeof(uint32_t), au_b = frames * DABPLUS_SLOTS * sizeof(vit_hip_dabplus_au);
    const size_t rs_b = frames * s * sizeof(int32_t), cnt_b = rows * sizeof(uint32_t);
    if (overlap(d_info, info_b, d_au, au_b)) return "d_info overlaps d_au";
    if (overlap(d_info, info_b, d_in, in_b) || overlap(d_au, au_b, d_in, in_b) || overlap(d_info, info_b, d_rs_status, rs_b) ||
        overlap(d_au, au_b, d_rs_status, rs_b) || overlap(d_info, info_b, d_n_frames, cnt_b) || overlap(d_au, au_b, d_n_frames, cnt_b))
        return "an output overlaps the superframes, d_rs_status or d_n_frames";
    return nullptr;
}

}  // namespace

extern "C" {

int vit_hip_dabplus_sync(vit_hip_handle h, const uint8_t* d_frames, size_t row_stride, size_t frame_stride, size_t frame_bytes, size_t rows,
                         size_t max_frames, const uint32_t* d_n_frames, unsigned frame0, unsigned flags, uint32_t* d_hits, uint32_t* d_count,
                         vit_hip_marker_lock* d_lock, vit_hip_stream_t stream) {
    if (const char* why = sync_invalid(h, d_frames, row_stride, frame_stride, frame_bytes, rows, max_frames, d_n_frames, frame0, flags, d_hits,
                                       d_count, d_lock))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (rows == 0) return VIT_HIP_OK;
    VIT_HIP_ON_DEVICE(h->device);
    hipStream_t st = (hipStream_t)stream;
    // the call overwrites its outputs: the search adds into zeroed totals
    if (!(flags & VIT_HIP_MARKER_ACCUMULATE) && dabplus_launch_zero(d_hits, d_count, (uint64_t)rows * DABPLUS_PHASES, st) != 0)
        return fail(VIT_HIP_ERR_RUNTIME, "dabplus zero launch failed");
    if (max_frames) {
        const size_t fs = frame_stride ? frame_stride : frame_bytes;
        const DabplusSyncArgs a = dabplus_sync_args(d_frames, row_stride ? row_stride : max_frames * fs, fs, rows, max_frames, d_n_frames, frame0,
                                                    d_hits, d_count);
        if (dabplus_launch_sync(a, st) != 0) return fail(VIT_HIP_ERR_RUNTIME, "dabplus sync launch failed");
    }
    if (d_lock && dabplus_launch_pick(d_hits, d_count, d_lock, rows, (uint32_t)frame_bytes, st) != 0)
        return fail(VIT_HIP_ERR_RUNTIME, "dabplus pick launch failed");
    return VIT_HIP_OK;
}

int vit_hip_dabplus_au_batch(vit_hip_handle h, const uint8_t* d_in, size_t frame_stride_bytes, size_t rows, size_t max_frames,
                             const uint32_t* d_n_frames, unsigned s, const int32_t* d_rs_status, uint32_t* d_info, vit_hip_dabplus_au* d_au,
                             vit_hip_stream_t stream) {
    if (const char* why = au_invalid(h, d_in, frame_stride_bytes, rows, max_frames, d_n_frames, s, d_rs_status, d_info, d_au))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (rows == 0 || max_frames == 0) return VIT_HIP_OK;
    const DabplusAuArgs a = dabplus_au_args(d_in, frame_stride_bytes, rows, max_frames, d_n_frames, s, d_rs_status, d_info, d_au);
    VIT_HIP_ON_DEVICE(h->device);
    if (dabplus_launch_au(a, (hipStream_t)stream) != 0) return fail(VIT_HIP_ERR_RUNTIME, "dabplus au launch failed");
    return VIT_HIP_OK;
}

}  // extern "C"
