// vit_internal.hpp -- what the translation units of the C ABI share: the decoder handle, the error path, and the few entry points
// one route calls in another.  Each kernel is launched from exactly ONE unit (there is no -fgpu-rdc: a kernel referenced from two
// units would be emitted twice):
//   vit_hip.hip      handle, plans, batched update / chainback / decode / export / depuncture / reset
//                    (kernels_lds.hpp, kernels_lds2.hpp; the register plan through reg_plan.hpp / reg_inst.hip)
//   vit_windows.hip  tail-biting, one long stream, many lockstep streams: side passes around the plans' update / chainback, which it
//                    calls as declared below (kernels_tb.hpp, kernels_stream.hpp)
//   vit_pipeline.hip vit_hip_pipeline_* and its schedule rules (no kernel of its own)
//   vit_host.hip     the single-decoder host route and the frame route (kernels_one.hpp)
//   vit_host_wide.hip  that header's kernels for K = 8, 9 and their launchers, which vit_host.hip calls: beside it for the build's sake
//   vit_tools.hip    synth, bit-error count, shader clock, kernel listing, precompile, RCCL table broadcast (kernels_synth.hpp)
//   vit_encode.hip   the encoder on the caller's bytes and the re-encoded channel symbol error count (kernels_enc.hpp)
//   vit_sync.hip     node synchronisation: the streams of a set of alignment hypotheses and their ranking, around the C ABI's own
//                    vit_hip_decode_streams and the body of vit_hip_channel_errors_batch, declared below (kernels_sync.hpp)
//   vit_marker.hip   frame synchronisation: the sync marker's distance per phase of the frame period, on the caller's bytes
//                    (kernels_marker.hpp)
//   vit_frames.hip   frame extraction: the frames of the caller's bytes cut at that lock, byte-aligned, with the carry between calls
//                    (kernels_frames.hpp)
//   vit_rs.hip       Reed-Solomon decoding of those frames' interleaved codewords: the code object with its tables (rs_tables.hpp)
//                    and the decode (kernels_rs.hpp)
//   vit_dvb.hip      the DVB-S stages on either side of it: the convolutional de-interleaver and the energy-dispersal removal
//                    (kernels_dvb.hpp)
//   vit_crc.hip      the frame check behind them: the CRC of a bit range of every frame and its syndrome (kernels_crc.hpp)
//   vit_lte.hip      the front of the LTE control-channel route: descrambling and rate de-matching into the symbols the tail-biting
//                    decode reads (kernels_lte.hpp)
//   vit_dab.hip      the DAB receive chain around the decode: time de-interleaver fused with depuncturing in front, energy-dispersal
//                    removal behind (kernels_dab.hpp)
//   vit_dabplus.hip  DAB+ audio superframes behind it: Fire-code superframe sync, the access-unit table and its CRCs
//                    (kernels_dabplus.hpp, which takes the device functions of kernels_crc.hpp without its kernel)
//   vit_wifi.hip     the IEEE 802.11a/g OFDM data path: de-interleaver fused with depuncturing in front of the decode, the SIGNAL
//                    parser, descrambling and the FCS behind it (kernels_wifi.hpp, which takes those device functions likewise)
//   vit_dvbt.hip     the front of the DVB-T route: the inner de-interleaver (symbol, bit, demultiplexer) fused with depuncturing in front
//                    of the stream decode (kernels_dvbt.hpp); behind the decode DVB-T is the DVB-S chain of vit_dvb.hip
//   vit_is95.hip     the IS-95A forward traffic channel around the K = 9 decode: descrambling, block de-interleaver and the combining of
//                    the repetitions under the four rate hypotheses in front, the blind rate decision behind (kernels_is95.hpp)
//   vit_gsm.hip      GSM channel decoding around the K = 5 decode: the block and diagonal burst de-interleavers in front, the Fire code
//                    of the control channels and the TCH/FS frame behind (kernels_gsm.hpp)
// arg_rules.hpp states what every unit's argument rule is worded in: overlap, extent, misaligned.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <type_traits>
#include <vector>

#include "../../include/vit_hip.h"
#include "../../include/vit_hip_experiments.h"
#include "arg_rules.hpp"
#include "reg_plan.hpp"

#pragma GCC visibility push(hidden)

struct vit_hip_decoder {
    int K = 0, R = 0, soft_bytes = 0, error_bytes = 0, device = 0;
    int N = 0, H = 0, W = 0, shift = 0;
    int plan = VIT_HIP_PLAN_LDS;
    int high = 0, low = 0;
    bool linear = false;
    uint32_t G[16] = {0};
    uint32_t cfg_raw[4] = {0, 0, 0, 0};
    vit::DevConfig cfg{};
    std::vector<uint16_t> pattern;  // [H] host copy
    uint16_t* d_pattern = nullptr;
    vit::RegCode reg_code{};        // PLAN_REG description (valid when reg_ok)
    bool reg_ok = false;
    bool lds2_ok = false;
    std::string reg_origin;         // path of the code object a run-time / install-time compiled PLAN_REG was loaded from
    // host-route scratch
    hipStream_t stream = nullptr;
    void* d_scratch = nullptr;
    size_t scratch_bytes = 0;
    void* h_stage = nullptr;        // pinned host staging: one H2D and one D2H per host-route call
    size_t stage_bytes = 0;
    // frame route (vit_hip_update_host_lazy / vit_hip_chainback_host_lazy / vit_hip_fetch_decisions_host)
    uint64_t* d_rows = nullptr;     // decision rows of the handle's ONE host-route frame, [row][W], kept on the device
    size_t rows_cap = 0;            // rows allocated
    void* h_map = nullptr;          // pinned AND host-mapped: [64 B control | 192 B | metrics | symbols | decoded bytes]
    size_t map_bytes = 0;
    uint32_t seq = 0;               // the value the next frame kernel stores into the control word when it is done
    bool spec_valid = false;        // the decoded bytes in h_map are those of chainback(spec_bits, spec_end) over the rows in d_rows
    size_t spec_bits = 0, spec_end = 0, spec_off = 0;
    int host_route = VIT_HIP_HOST_ROUTE_AUTO;   // vit_hip_set_host_route: AUTO, or the LDS plan on one frame at any K
};

namespace vit {

// what vit_hip_last_error returns: one string per thread, whichever unit failed
inline std::string& last_error() { thread_local std::string e; return e; }
inline int fail(int code, const std::string& msg) {
    last_error() = msg;
    return code;
}

#define VIT_HIP_CHECK(expr)                                                                                  \
    do {                                                                                                     \
        hipError_t _e = (expr);                                                                              \
        if (_e != hipSuccess)                                                                                \
            return vit::fail(VIT_HIP_ERR_RUNTIME, std::string(#expr) + ": " + hipGetErrorString(_e));        \
    } while (0)

// entry points that allocate on the host: no exception crosses the ABI
#define VIT_HIP_NOTHROW(stmt)                                                                       \
    try {                                                                                           \
        stmt;                                                                                       \
    } catch (const std::exception& e) {                                                             \
        try { vit::last_error() = std::string("host exception: ") + e.what(); } catch (...) {}      \
        return VIT_HIP_ERR_RUNTIME;                                                                 \
    } catch (...) {                                                                                 \
        return VIT_HIP_ERR_RUNTIME;                                                                 \
    }

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = (prev == dev) || (hipSetDevice(dev) == hipSuccess);
        if (prev == dev) prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// the rest of the calling function runs with `dev` current; the device the caller had comes back when it returns
#define VIT_HIP_ON_DEVICE(dev) vit::DeviceGuard guard(dev); if (!guard.ok) return vit::fail(VIT_HIP_ERR_RUNTIME, "hipSetDevice failed")

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// a code rate known at run time as a template argument: f(std::integral_constant<int, R>{}) for R = 1..8, `bad` for any other
template <class F>
int with_rate(int R, int bad, F&& f) {
#define VIT_RATE_CASE(r) case r: return f(std::integral_constant<int, r>{});
    switch (R) {
        VIT_RATE_CASE(1) VIT_RATE_CASE(2) VIT_RATE_CASE(3) VIT_RATE_CASE(4) VIT_RATE_CASE(5) VIT_RATE_CASE(6) VIT_RATE_CASE(7) VIT_RATE_CASE(8)
        default: return bad;
    }
#undef VIT_RATE_CASE
}

// the table blob of vit_hip_pack_blob / vit_hip_create_from_blob / vit_hip_broadcast_table
constexpr uint32_t BLOB_MAGIC = 0x56495442u;  // "VITB"
struct BlobHeader {
    uint32_t magic;
    int32_t K, R, soft_bytes, error_bytes;
};

inline void kernel_resources_to_abi(const kd::KernelResources& r, unsigned dyn_lds_bytes, vit_hip_kernel_resources* out) {
    memset(out, 0, sizeof(*out));
    out->vgpr_alloc = r.vgpr_alloc; out->accum_offset = r.accum_offset; out->lds_static_bytes = r.lds_static_bytes;
    out->lds_dynamic_bytes = dyn_lds_bytes; out->scratch_bytes = r.scratch_bytes;
}

// ---- defined in vit_hip.hip, called from the other routes ----
// reset + update (d_metrics_in == null, first_step == 0) or resumed update: one body behind both entry points
int update_batch_impl(vit_hip_handle h, const void* d_symbols, size_t sym_stride, size_t frames, size_t first_step, size_t n_steps,
                      size_t L, void* d_workspace, size_t workspace_bytes, const void* d_metrics_in, void* d_metrics_out,
                      uint64_t* d_renorm_sum, const uint32_t* d_start_state, vit_hip_stream_t stream, bool overlapped_chunks = false);
// alt_kernel: the code's other chainback kernel (K = 7: the LDS-ring body, K = 9: the cooperative one); ignored by codes with one
int chainback_batch_impl(vit_hip_handle h, const void* d_workspace, size_t frames, size_t L, uint8_t* d_bytes_out,
                         const uint32_t* d_end_state, vit_hip_stream_t stream, unsigned wave_priority, bool alt_kernel = false);
// the LDS plan on caller-chosen rows (the host routes run it on one frame); decisions in the reference layout [F][rows][W]
int lds_update(vit_hip_handle h, const void* d_symbols, size_t sym_stride, size_t frames, size_t n_steps, size_t rows,
               uint32_t row0, uint64_t* d_decisions, void* d_metrics, bool reset, uint64_t* d_renorm, const uint32_t* d_start,
               hipStream_t st);
int lds_chainback(vit_hip_handle h, const uint64_t* d_decisions, size_t frames, size_t L, uint8_t* d_out,
                  const uint32_t* d_end, hipStream_t st);
// PLAN_LDS2: does the chainback kernel fit beside the update waves of this handle's code (kernels_lds2.hpp)?
bool lds2_chainback_fits(vit_hip_handle h);

// ---- defined in vit_encode.hip ----
// the body of vit_hip_channel_errors_batch.  zero_counters = false: the kernel adds into d_errors / d_compared as they are -- a caller
// that zeroes them in a kernel of its own on `stream` (the synchronisation search) enqueues no memset
int channel_errors_impl(vit_hip_handle h, const void* d_symbols, size_t symbol_frame_stride, const uint8_t* d_bytes,
                        size_t bytes_frame_stride, size_t frames, size_t L, unsigned flags, const uint32_t* d_start_state,
                        uint32_t* d_errors, uint32_t* d_compared, bool zero_counters, vit_hip_stream_t stream);

}  // namespace vit

#pragma GCC visibility pop
