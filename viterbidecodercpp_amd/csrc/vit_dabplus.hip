// vit_dabplus.hip -- DAB+ audio superframes of the C ABI (ETSI TS 102 563) behind the DAB receive chain: vit_hip_dabplus_sync (which of
// five logical frames starts a superframe: the Fire code over the header, summed per phase, and the lock vit_hip_frames_extract reads) and
// vit_hip_dabplus_au_batch (behind vit_hip_rs_decode_batch: the header's access-unit table and the CRC-16 of every access unit, over
// ranges the device reads from the superframe itself).  Both work on the caller's bytes alone and read the handle only for its device.
// The kernels of kernels_dabplus.hpp are launched only here.  Host-side logic only: the argument rules (kernels_dabplus.hpp, so that they
// run without a device) and the launches.
// Out of scope: AAC decoding, PAD extraction, compacting the access units, DMB and enhanced packet mode, a lock policy, s > 24, UEP.
#include "vit_internal.hpp"
#include "kernels_dabplus.hpp"

using namespace vit;

extern "C" {

int vit_hip_dabplus_sync(vit_hip_handle h, const uint8_t* d_frames, size_t row_stride, size_t frame_stride, size_t frame_bytes, size_t rows,
                         size_t max_frames, const uint32_t* d_n_frames, unsigned frame0, unsigned flags, uint32_t* d_hits, uint32_t* d_count,
                         vit_hip_marker_lock* d_lock, vit_hip_stream_t stream) {
    if (const char* why = dabplus_sync_invalid(h != nullptr, d_frames, row_stride, frame_stride, frame_bytes, rows, max_frames, d_n_frames, frame0,
                                               flags, d_hits, d_count, d_lock))
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
    if (const char* why = dabplus_au_invalid(h != nullptr, d_in, frame_stride_bytes, rows, max_frames, d_n_frames, s, d_rs_status, d_info, d_au))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (rows == 0 || max_frames == 0) return VIT_HIP_OK;
    const DabplusAuArgs a = dabplus_au_args(d_in, frame_stride_bytes, rows, max_frames, d_n_frames, s, d_rs_status, d_info, d_au);
    VIT_HIP_ON_DEVICE(h->device);
    if (dabplus_launch_au(a, (hipStream_t)stream) != 0) return fail(VIT_HIP_ERR_RUNTIME, "dabplus au launch failed");
    return VIT_HIP_OK;
}

}  // extern "C"
