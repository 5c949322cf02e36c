// vit_dvbt.hip -- the front of the DVB-T route of the C ABI: vit_hip_dvbt_deinterleave_batch, the inner de-interleaver (symbol
// interleaver, bit interleaver, demultiplexer) fused with depuncturing, writing the [steps][2] symbols vit_hip_decode_stream(s) reads.
// Everything behind the decode is the DVB-S outer chain (vit_marker.hip, vit_frames.hip, vit_dvb.hip, vit_rs.hip).  It works on the
// caller's buffers alone and reads the handle for its device, its symbol width and its rate.  The kernel of kernels_dvbt.hpp is launched
// only here.  Host-side logic only: the argument rule (kernels_dvbt.hpp, so that it runs without a device), a handful of constants and
// the launch.
// Out of scope: hierarchical modes, the DVB-H in-depth interleaver, OFDM demodulation, pilots, TPS decoding and demapping, DVB-T2, a
// transmitter on the card.
#include "vit_internal.hpp"
#include "kernels_dvbt.hpp"

using namespace vit;

extern "C" {

int vit_hip_dvbt_deinterleave_batch(vit_hip_handle h, const void* d_in, size_t in_row_stride, size_t rows, size_t n_sym, unsigned mode,
                                    unsigned v, unsigned rate, unsigned parity, const uint32_t* d_parity_in, uint32_t* d_parity_out,
                                    void* d_symbols_out, size_t out_row_stride, vit_hip_stream_t stream) {
    if (const char* why = dvbt_invalid(h != nullptr, h ? h->R : 0, h ? (size_t)h->soft_bytes : 1, d_in, in_row_stride, rows, n_sym, mode, v, rate,
                                       d_parity_in, d_parity_out, d_symbols_out, out_row_stride))
        return fail(VIT_HIP_ERR_INVALID_ARG, why);
    if (rows == 0 || n_sym == 0) return VIT_HIP_OK;
    const DvbtArgs a = dvbt_args(d_in, in_row_stride, rows, n_sym, mode, v, rate, parity, d_parity_in, d_parity_out, d_symbols_out, out_row_stride);
    VIT_HIP_ON_DEVICE(h->device);
    if (dvbt_launch(a, (size_t)h->soft_bytes, (hipStream_t)stream) != 0) return fail(VIT_HIP_ERR_RUNTIME, "DVB-T de-interleave launch failed");
    return VIT_HIP_OK;
}

}  // extern "C"
