// vit_marker.hip -- frame synchronisation of the C ABI: vit_hip_marker_search (the distance of a sync marker to every bit position of
// decoded, bit-packed rows, summed per phase of the frame period, and the phase and polarity no other beats).  It works on the
// caller's bytes alone and reads the handle only for its device.  The kernels of kernels_marker.hpp are launched only here.  Host-side
// logic only: argument checking and launches.
#include "vit_internal.hpp"
#include "kernels_marker.hpp"

using namespace vit;

namespace {

// argument rule (include/vit_hip.h): everything the host can know without reading device memory
const char* marker_invalid(const uint8_t* d_bytes, size_t stride, size_t rows, size_t n_bits, uint64_t marker, unsigned m,
                           const uint64_t* d_history, unsigned hb, size_t P, size_t phase0, unsigned flags, const uint32_t* d_distance,
                           const uint32_t* d_count, const vit_hip_marker_lock* d_lock) {
    const bool accumulate = flags & VIT_HIP_MARKER_ACCUMULATE;
    if (flags & ~VIT_HIP_MARKER_ACCUMULATE) return "unknown flag bits";
    if (!d_bytes || !d_distance) return "NULL buffer";
    if (accumulate && d_lock && !d_count) return "a lock over accumulated totals needs d_count";
    if (m < 1 || m > 64) return "marker_bits must be 1 .. 64";
    if (m < 64 && (marker >> m) != 0) return "marker has bits above marker_bits";
    if (hb > 63) return "history_bits must be 0 .. 63";
    if (hb > 0 && !d_history) return "d_history is NULL with history_bits > 0";
    if (n_bits >= 0x100000000ull - 64) return "n_bits must be below 2^32 - 64";
    if (n_bits + hb < m) return "n_bits + history_bits must be at least marker_bits";
    if (P == 0 || P >= 0x80000000ull) return "period_bits must be 1 .. 2^31 - 1";
    if (phase0 >= P) return "phase0 must be below period_bits";
    if (stride != 0 && stride < (n_bits + 7) / 8) return "bytes_row_stride is below ceil(n_bits / 8)";
    if (rows > 0x7FFFFFFFu) return "more than 2^31 - 1 rows";
    if (!accumulate && (uint64_t)m * ((n_bits + hb + P - 1) / P) >= 0x100000000ull) return "marker_bits * ceil((n_bits + history_bits) / period_bits) must be below 2^32";
    return nullptr;
}

}  // namespace

extern "C" {

int vit_hip_marker_search(vit_hip_handle h, const uint8_t* d_bytes, size_t bytes_row_stride, size_t rows, size_t n_bits, uint64_t marker,
                          unsigned marker_bits, const uint64_t* d_history, unsigned history_bits, size_t period_bits, size_t phase0,
                          unsigned flags, uint32_t* d_distance, uint32_t* d_count, vit_hip_marker_lock* d_lock, vit_hip_stream_t stream) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    if (const char* why = marker_invalid(d_bytes, bytes_row_stride, rows, n_bits, marker, marker_bits, d_history, history_bits, period_bits,
                                         phase0, flags, d_distance, d_count, d_lock))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (rows == 0) return VIT_HIP_OK;
    const uint32_t P = (uint32_t)period_bits;
    const MarkerSearchArgs a = marker_search_args(d_bytes, bytes_row_stride, rows, n_bits, marker, marker_bits, d_history, history_bits, P,
                                                  phase0, d_distance, d_count);

    VIT_HIP_ON_DEVICE(h->device);
    hipStream_t st = (hipStream_t)stream;
    // the call overwrites its outputs: the search adds into zeroed totals
    if (!(flags & VIT_HIP_MARKER_ACCUMULATE) && marker_launch_zero(d_distance, d_count, (uint64_t)rows * P, st) != 0)
        return fail(VIT_HIP_ERR_RUNTIME, "marker zero launch failed");
    if (marker_launch_search(a, st) != 0) return fail(VIT_HIP_ERR_RUNTIME, "marker search launch failed");
    if (d_lock) {
        MarkerPickArgs p{};
        p.distance = d_distance; p.count = d_count; p.lock = d_lock;
        p.P = P; p.m = marker_bits; p.base = a.base; p.count_full = a.count_full; p.count_rem = a.count_rem;
        if (marker_launch_pick(p, rows, st) != 0) return fail(VIT_HIP_ERR_RUNTIME, "marker pick launch failed");
    }
    return VIT_HIP_OK;
}

}  // extern "C"
