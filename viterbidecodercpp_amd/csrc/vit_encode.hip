// vit_encode.hip -- the encoder on the caller's bytes and the re-encoded channel symbol error count (kernels_enc.hpp):
// vit_hip_encode_batch, vit_hip_channel_errors_batch.  Both read the handle (K, R, polynomials, high / low) and write only caller
// buffers; they enqueue on `stream` and nothing else.
#include "vit_internal.hpp"
#include "kernels_enc.hpp"

using namespace vit;

namespace {

// the argument rule both calls share (include/vit_hip.h); fills everything of `a` but the pointers.  0: launch, 1: no work
int enc_prepare(vit_hip_handle h, const void* d_symbols, size_t symbol_frame_stride, const uint8_t* d_bytes, size_t bytes_frame_stride,
                size_t frames, size_t L, unsigned flags, const uint32_t* d_start_state, size_t chunks_per_block_max, EncArgs& a,
                unsigned& blocks) {
    if (!h) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL handle");
    if (!h->linear) return fail(VIT_HIP_ERR_UNSUPPORTED, "the branch table is not that of a convolutional code (no polynomials)");
    if (frames == 0) return 1;
    if (!d_symbols || !d_bytes) return fail(VIT_HIP_ERR_INVALID_ARG, "NULL buffer");
    if (L == 0) return fail(VIT_HIP_ERR_INVALID_ARG, "L is 0");
    if (flags & ~(VIT_HIP_ENCODE_TAIL | VIT_HIP_ENCODE_TAIL_BITING)) return fail(VIT_HIP_ERR_INVALID_ARG, "unknown flag bits");
    const bool tail = flags & VIT_HIP_ENCODE_TAIL, tail_biting = flags & VIT_HIP_ENCODE_TAIL_BITING;
    if (tail && tail_biting) return fail(VIT_HIP_ERR_INVALID_ARG, "VIT_HIP_ENCODE_TAIL and VIT_HIP_ENCODE_TAIL_BITING exclude each other");
    if (tail_biting && L < (size_t)h->K) return fail(VIT_HIP_ERR_INVALID_ARG, "tail-biting frames need L >= K");
    if (tail_biting && d_start_state) return fail(VIT_HIP_ERR_INVALID_ARG, "a tail-biting frame takes its start state from its own last K-1 bits: d_start_state must be NULL");
    const size_t K = (size_t)h->K, R = (size_t)h->R;
    if (L >= 0x100000000ull) return fail(VIT_HIP_ERR_INVALID_ARG, "steps * R must be below 2^32");
    const size_t steps = L + (tail ? K - 1 : 0);
    if (steps * R >= 0x100000000ull) return fail(VIT_HIP_ERR_INVALID_ARG, "steps * R must be below 2^32");
    const size_t nbytes = (L + 7) / 8;
    if (symbol_frame_stride != 0 && symbol_frame_stride < steps * R) return fail(VIT_HIP_ERR_INVALID_ARG, "symbol_frame_stride is below steps * R");
    if (bytes_frame_stride != 0 && bytes_frame_stride < nbytes) return fail(VIT_HIP_ERR_INVALID_ARG, "bytes_frame_stride is below ceil(L/8)");
    if (h->soft_bytes == 2 && misaligned(d_symbols, 2)) return fail(VIT_HIP_ERR_INVALID_ARG, "int16 symbols must be 2-byte aligned");
    if (R > 8) return fail(VIT_HIP_ERR_UNSUPPORTED, "R > 8");
    const size_t nchunks = (steps + 7) / 8;
    if (frames > 0xFFFFFFFFull || frames > 0xFFFFFFFFFFFFFFFFull / nchunks) return fail(VIT_HIP_ERR_INVALID_ARG, "batch too large for one launch");
    a = EncArgs{};
    a.bytes = d_bytes;
    a.start = d_start_state;
    a.sym_stride = symbol_frame_stride ? symbol_frame_stride : steps * R;
    a.byte_stride = bytes_frame_stride ? bytes_frame_stride : nbytes;
    a.total_chunks = (uint64_t)frames * nchunks;
    a.L = (uint32_t)L; a.steps = (uint32_t)steps; a.nchunks = (uint32_t)nchunks;
    a.K = (uint32_t)K; a.tail_biting = tail_biting ? 1u : 0u;
    // long frames: a workgroup sums 8 chunks per thread before it touches the frame's counters (at least 8 such workgroups per frame)
    a.chunks_per_thread = nchunks >= 8 * 256 * chunks_per_block_max ? (uint32_t)chunks_per_block_max : 1u;
    for (size_t i = 0; i < R; ++i) a.G[i] = h->G[i] & ((1u << K) - 1u);
    a.high = h->high; a.low = h->low;
    const uint64_t tile = 256ull * a.chunks_per_thread, nblocks = (a.total_chunks + tile - 1) / tile;
    if (nblocks > 0x7FFFFFFFull) return fail(VIT_HIP_ERR_INVALID_ARG, "batch too large for one launch");
    blocks = (unsigned)nblocks;
    return 0;
}

}  // namespace

// vit_hip_channel_errors_batch, and the same count into counters the caller has zeroed on `stream` itself (zero_counters = false)
int vit::channel_errors_impl(vit_hip_handle h, const void* d_symbols, size_t symbol_frame_stride, const uint8_t* d_bytes,
                             size_t bytes_frame_stride, size_t frames, size_t L, unsigned flags, const uint32_t* d_start_state,
                             uint32_t* d_errors, uint32_t* d_compared, bool zero_counters, vit_hip_stream_t stream) {
    EncArgs a;
    unsigned blocks = 0;
    if (h && frames != 0 && !d_errors) return fail(VIT_HIP_ERR_INVALID_ARG, "d_errors is NULL");
    const int pre = enc_prepare(h, d_symbols, symbol_frame_stride, d_bytes, bytes_frame_stride, frames, L, flags, d_start_state, 8, a, blocks);
    if (pre != 0) return pre < 0 ? pre : VIT_HIP_OK;
    a.symbols = const_cast<void*>(d_symbols);
    a.errors = d_errors;
    a.compared = d_compared;
    VIT_HIP_ON_DEVICE(h->device);
    // the call overwrites its outputs: the kernel adds into zeroed counters
    if (zero_counters) {
        VIT_HIP_CHECK(hipMemsetAsync(d_errors, 0, frames * sizeof(uint32_t), (hipStream_t)stream));
        if (d_compared) VIT_HIP_CHECK(hipMemsetAsync(d_compared, 0, frames * sizeof(uint32_t), (hipStream_t)stream));
    }
    const int rc = with_rate(h->R, -1, [&](auto r) {
        if (h->soft_bytes == 2) hipLaunchKernelGGL((channel_errors_kernel<int16_t, r()>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((channel_errors_kernel<int8_t, r()>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    });
    if (rc != 0) return fail(VIT_HIP_ERR_RUNTIME, "channel error kernel launch failed");
    return VIT_HIP_OK;
}

extern "C" {

int vit_hip_encode_batch(vit_hip_handle h, const uint8_t* d_bytes, size_t bytes_frame_stride, size_t frames, size_t L, unsigned flags,
                         const uint32_t* d_start_state, void* d_symbols_out, size_t symbol_frame_stride, uint32_t* d_end_state_out,
                         vit_hip_stream_t stream) {
    EncArgs a;
    unsigned blocks = 0;
    const int pre = enc_prepare(h, d_symbols_out, symbol_frame_stride, d_bytes, bytes_frame_stride, frames, L, flags, d_start_state, 1, a, blocks);
    if (pre != 0) return pre < 0 ? pre : VIT_HIP_OK;
    a.symbols = d_symbols_out;
    a.end_state = d_end_state_out;
    VIT_HIP_ON_DEVICE(h->device);
    const int rc = with_rate(h->R, -1, [&](auto r) {
        if (h->soft_bytes == 2) hipLaunchKernelGGL((encode_kernel<int16_t, r()>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((encode_kernel<int8_t, r()>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    });
    if (rc != 0) return fail(VIT_HIP_ERR_RUNTIME, "encode kernel launch failed");
    return VIT_HIP_OK;
}

int vit_hip_channel_errors_batch(vit_hip_handle h, const void* d_symbols, size_t symbol_frame_stride, const uint8_t* d_bytes,
                                 size_t bytes_frame_stride, size_t frames, size_t L, unsigned flags, const uint32_t* d_start_state,
                                 uint32_t* d_errors, uint32_t* d_compared, vit_hip_stream_t stream) {
    return channel_errors_impl(h, d_symbols, symbol_frame_stride, d_bytes, bytes_frame_stride, frames, L, flags, d_start_state, d_errors,
                               d_compared, true, stream);
}

}  // extern "C"
